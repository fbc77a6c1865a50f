// The span decimation SSBDemod::feed and ChannelAnalyzer::processOneSample share: m_sum += s[j] in float, a group closes on the
// sample whose pre-increment m_undersampleCount has its low bits clear (ssb_first_close / ssb_closes, ssb_scan.hpp), the sum
// goes back to 0.  Groups are independent once the counter is known; the open group's partial sum and the counter carry.
#pragma once
#include <hip/hip_runtime.h>
#include "ssb_scan.hpp"

namespace sdrx {

// the sum of group q of a feed: the decim samples up to i0 + q * decim in their order, on top of the carried partial sum where
// the group was open when the feed began
__device__ __forceinline__ float2 span_group_sum(const float2* __restrict__ s, float2 open_sum, int i0, int decim, int q)
{
    const int last = i0 + q * decim, first = last - decim + 1;
    float2 acc = make_float2(0.0f, 0.0f);
    if (first < 0) acc = open_sum;
    for (int j = max(first, 0); j <= last; j++) { const float2 v = s[j]; acc.x += v.x; acc.y += v.y; }
    return acc;
}

// the open group after a feed of n samples of which ncl closed a group: what was carried if nothing closed, then the samples
// after the last close (fewer than decim)
__device__ __forceinline__ float2 span_open_sum(const float2* __restrict__ s, float2 open_sum, int i0, int decim, int ncl, int n)
{
    float2 acc = ncl > 0 ? make_float2(0.0f, 0.0f) : open_sum;
    for (int j = ncl > 0 ? i0 + (ncl - 1) * decim + 1 : 0; j < n; j++) { const float2 v = s[j]; acc.x += v.x; acc.y += v.y; }
    return acc;
}

} // namespace sdrx
