// Workgroup plumbing the demodulator-bank kernels share (am_, nfm_, ssb_, udpsrc_ and wfm_kernels.hpp): the recurrences
// themselves are the *_scan.hpp files'; this is what carries them across a workgroup of 256 lanes = 4 waves of 64.
// Force-inlined templates only, like psum_rows (demod_psum.hpp); DESIGN.md 4.15.
//
// 1. wg_scan, wg_scan_incl, wg_total: scan of an associative map over the workgroup.  Every lane brings the composition of its
//    own consecutive samples; wg_scan gives back the composition of everything in front of the lane (wg_scan_incl: up to and
//    including the lane), wg_total the whole workgroup's (the same in every lane).  The wave-inclusive scan runs by __shfl_up (wg_wave_scan); the four wave totals go through a 4-slot LDS array
//    the caller owns.  The map type comes with an ops struct: Map, identity(), compose(f, g) = first f then g, shfl_up(m, o)
//    (WfmClampOps in wfm_scan.hpp, SsbPairOps in ssb_scan.hpp, UdpSqOps in udpsrc_scan.hpp, WgCount / WgCount2 here).
//
//    Barrier contract.  wg_scan and wg_scan_incl hold exactly one __syncthreads(), between the write of the slots and the reads of
//    them, so every call sits in workgroup-uniform control flow.  wg_total has none: it reads the slots the last wg_scan filled, at
//    the place the caller chooses (where it keeps the fewest registers live).  A slot array may be given to wg_scan again only
//    after one more barrier that every wave passes after its last read of it:
//      - am_gate_kernel, nfm_gate_kernel and udp_gate_kernel run a map scan and a count scan per trip, take their totals after
//        the trip's stores and so close every trip with one barrier of their own;
//      - magagc_trip (ssb_scan.hpp) runs three scans in a row on three slot arrays, takes each total right after its scan, and has no
//        barrier of its own: between those reads and the next trip's write of the same array lie the barriers of the two
//        other scans;
//      - a kernel that scans once (wfm_demod_kernel) needs nothing more.
// 2. WgCount, WgCount2: the scan for plain int sums -- the prefix count of flags that is the compaction index, and its total, which
//    the caller adds to its running count.  WgCount2 counts two flags under the one barrier.  The callers take wg_scan_incl and
//    subtract the lane's own count.
// 3. wg_level_reduce / wg_level_gather: sum (double) and peak over 256 lanes in the fixed tree order st = 128, 64 .. 1 (the sums are
//    compared bit for bit downstream), result in sums[0] / peaks[0] for lane 0.  The peak is float (AM, NFM) or double (SSB).
#pragma once
#include <hip/hip_runtime.h>

namespace sdrx {

template <class Ops>
__device__ __forceinline__ typename Ops::Map wg_wave_scan(const Ops& op, typename Ops::Map m, int lane)     // inclusive, in lane order
{
    for (int o = 1; o < 64; o *= 2) {
        const typename Ops::Map t = op.shfl_up(m, o);
        if (lane >= o) m = op.compose(t, m);
    }
    return m;
}

// the waves in front of wave w, from a lane's wave-inclusive value: the slot write, THE barrier, the slot reads
template <class Ops>
__device__ __forceinline__ typename Ops::Map wg_waves_before(const Ops& op, typename Ops::Map incl, int lane, int w, typename Ops::Map* slot)
{
    if (lane == 63) slot[w] = incl;
    __syncthreads();
    typename Ops::Map pre = op.identity();
    for (int q = 0; q < w; q++) pre = op.compose(pre, slot[q]);
    return pre;
}
// lane = tid & 63, w = tid >> 6; slot: __shared__ Map[4] of the caller (see the barrier contract above)
template <class Ops>
__device__ __forceinline__ typename Ops::Map wg_scan(const Ops& op, typename Ops::Map m, int lane, int w, typename Ops::Map* slot)
{
    using Map = typename Ops::Map;
    const Map incl = wg_wave_scan(op, m, lane);
    const Map pre = wg_waves_before(op, incl, lane, w, slot);
    Map ex = op.shfl_up(incl, 1);
    if (lane == 0) ex = op.identity();
    return op.compose(pre, ex);
}
// everything up to AND including this lane: for maps with an inverse the caller takes its own part off again (a count: minus the
// lane's own), which saves wg_scan's last shuffle
template <class Ops>
__device__ __forceinline__ typename Ops::Map wg_scan_incl(const Ops& op, typename Ops::Map m, int lane, int w, typename Ops::Map* slot)
{
    const typename Ops::Map incl = wg_wave_scan(op, m, lane);
    return op.compose(wg_waves_before(op, incl, lane, w, slot), incl);
}
// the whole workgroup's map, from the slots a wg_scan filled; the same in every lane
template <class Ops>
__device__ __forceinline__ typename Ops::Map wg_total(const Ops& op, const typename Ops::Map* slot)
{
    typename Ops::Map all = slot[0];
    for (int q = 1; q < 4; q++) all = op.compose(all, slot[q]);
    return all;
}

struct WgCount {
    using Map = int;
    __device__ __forceinline__ int identity() const { return 0; }
    __device__ __forceinline__ int compose(int f, int g) const { return f + g; }
    __device__ __forceinline__ int shfl_up(int m, int o) const { return __shfl_up(m, o, 64); }
};
struct WgCount2 {
    using Map = int2;
    __device__ __forceinline__ int2 identity() const { return make_int2(0, 0); }
    __device__ __forceinline__ int2 compose(int2 f, int2 g) const { return make_int2(f.x + g.x, f.y + g.y); }
    __device__ __forceinline__ int2 shfl_up(int2 m, int o) const { return make_int2(__shfl_up(m.x, o, 64), __shfl_up(m.y, o, 64)); }
};

__device__ __forceinline__ float wg_peak(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double wg_peak(double a, double b) { return fmax(a, b); }

// sums, peaks: __shared__ [256] of the caller.  Ends with a barrier; lane 0 then reads sums[0] and peaks[0].
template <class P>
__device__ __forceinline__ void wg_level_reduce(double* sums, P* peaks, int tid, double sum, P peak)
{
    sums[tid] = sum; peaks[tid] = peak;
    __syncthreads();
    for (int st = 128; st; st >>= 1) {
        if (tid < st) { sums[tid] += sums[tid + st]; peaks[tid] = wg_peak(peaks[tid], peaks[tid + st]); }
        __syncthreads();
    }
}
// the same over nblk partials of a level kernel, lane tid taking every 256th in order
template <class P>
__device__ __forceinline__ void wg_level_gather(double* sums, P* peaks, int tid, int nblk, const double* blk_sum, const P* blk_peak)
{
    double ps = 0.0; P pk = 0;
    for (int j = tid; j < nblk; j += 256) { ps += blk_sum[j]; pk = wg_peak(pk, blk_peak[j]); }
    wg_level_reduce(sums, peaks, tid, ps, pk);
}

} // namespace sdrx
