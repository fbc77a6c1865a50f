// Rounded prefix sum along time, acc += term, for 16 channels per wave: the one loop of the demodulator banks that is
// serial in time (am_kernels.hpp: moving-average total and AGC sum; nfm_kernels.hpp: moving-average total).
// The wave loads each channel's 64 terms with one coalesced 512-byte instruction into LDS (row pitch 65 doubles: the 16
// chain lanes fall into 16 different bank pairs), lane c then walks row c -- LDS read, one double add, LDS write of its
// result -- and the rows go back out coalesced.  (A lane reading its own channel's terms straight from memory touches 64
// different lines per instruction: measured 8.4 ms per launch for 256 channels x 48 000 terms)
#pragma once
#include <hip/hip_runtime.h>

namespace sdrx {

constexpr int PS_CH = 16, PS_T = 64;

// One wave of 64.  Lane q < PS_CH owns row q and calls row(term, out, n_mine, acc): the row's terms, where the sums go, their
// number and the carried sum; a row past the last channel (`chain` false) names any valid pointers and leaves n_mine = 0.
// Returns the row's sum after its last term.
template <class Row>
__device__ __forceinline__ double psum_rows(int lane, bool chain, Row row)
{
    __shared__ double tile[PS_CH][PS_T + 1];
    __shared__ const double* st[PS_CH];
    __shared__ double* so[PS_CH];
    __shared__ int sn[PS_CH];
    double acc = 0.0;
    int n_mine = 0;
    if (lane < PS_CH) {
        const double* term;
        double* out;
        row(term, out, n_mine, acc);
        st[lane] = term; so[lane] = out; sn[lane] = n_mine;
    }
    __syncthreads();
    int n_max = 0;
    for (int q = 0; q < PS_CH; q++) n_max = max(n_max, sn[q]);
    for (int i = 0; i < n_max; i += PS_T) {
        // unconditional loads with the index clamped into the channel's terms, so that all sixteen are in flight together;
        // what lies past a channel's end is never added and never stored
        double v[PS_CH];
#pragma unroll
        for (int q = 0; q < PS_CH; q++) v[q] = st[q][min(i + lane, max(sn[q] - 1, 0))];
#pragma unroll
        for (int q = 0; q < PS_CH; q++) tile[q][lane] = v[q];
        __syncthreads();
        if (chain) {
            const int m = min(PS_T, n_mine - i);
            if (m == PS_T) {
#pragma unroll 16
                for (int k = 0; k < PS_T; k++) { acc += tile[lane][k]; tile[lane][k] = acc; }
            } else {
                for (int k = 0; k < m; k++) { acc += tile[lane][k]; tile[lane][k] = acc; }
            }
        }
        __syncthreads();
        for (int q = 0; q < PS_CH; q++)
            if (i + lane < sn[q]) so[q][i + lane] = tile[q][lane];
        __syncthreads();
    }
    return acc;
}

// What a psum kernel is (one wave of 64 per PS_CH channels, grid = the channel count rounded up): for channel c, row_of(c) names
// the terms, where the sums go, their number, the carried sum, and where the sum after the last term goes.  am_psum_kernel
// spells this out instead; am_kernels.hpp says why.
struct PsumRow { const double* term; double* out; int n; double sum; double* next; };
template <class RowOf>
__device__ __forceinline__ void psum_channels(int n_ch, RowOf row_of)
{
    const int lane = threadIdx.x, c = blockIdx.x * PS_CH + lane;
    const bool chain = lane < PS_CH && c < n_ch;
    const double acc = psum_rows(lane, chain, [&](const double*& term, double*& out, int& n_mine, double& sum) {
        // rows past the last channel: its pointers, no terms.  The count and the carried sum are loaded for those rows too (valid
        // memory, the index is clamped) and dropped; the row is named again below for `next` alone
        const PsumRow r = row_of(min(c, n_ch - 1));
        term = r.term; out = r.out;
        if (chain) { n_mine = r.n; sum = r.sum; }
    });
    if (chain) *row_of(c).next = acc;
}

} // namespace sdrx
