// The front the two broadcast-FM banks share (wfm_kernels.hpp, bfm_kernels.hpp), as device functions: block cut and pending
// samples, NCO mix on load, the two g_fft of fftfilt::runFilt, the block reduction of the level sums and counter maps, the scan of
// the squelch counter per block and across blocks, the resampler schedule, the real polyphase FIR and the carry.  The kernels
// that call them are thin: a translation unit defines its own, so nothing here is a __global__.
//
// Per feed and channel the stream is [pending raw samples (< 512, carried) | new samples]; it is cut into 512-sample
// blocks, the remainder is carried raw (with the NCO phase at its start) to the next feed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gfft_kernel.hpp"
#include "wfm_scan.hpp"
#include "demod_wg.hpp"
#include "dsp_device.hpp"

namespace sdrx {

constexpr int WFM_FFT = 1024, WFM_H = WFM_FFT / 2;
constexpr int WFM_NCO_N = 4096;
constexpr int WFM_HIST = 128;           // demodulated samples kept in front of a feed's: the resampler's window (>= taps per phase)

struct WfmChan {                        // device resident: config + carried state of one channel
    // --- config
    int nco_inc;                        // NCO::setFreq: (int)((freq * 4096) / rate)
    float step;                         // m_interpolatorDistance = (Real) inRate / (Real) audioRate
    int ntaps, taps_off;                // taps per phase; float offset into the taps table: [phase][ntaps]
    int filt_off;                       // complex offset into the filter table (WFM_FFT entries per channel)
    float fm_scaling;                   // 1.0f / m_fmExcursion
    float squelch_level;                // (Real) pow(10.0, squelch / 10.0)
    float cap_f, open_f;                // rfBandwidth / 10, rfBandwidth / 20 (float, compared against the int counter)
    int cap;                            // wfm_counter_cap(cap_f): where the counter saturates
    float volume;
    int mute;
    int dy_q, dy_S;                     // dyadic step: Q = 1 << dy_q, S = step * Q (dy_q < 0: not dyadic)
    // --- state
    int nco_phase;                      // phase before the first pending sample
    int pending;                        // raw samples waiting for a full block
    int sq_state, sq_open;              // m_squelchState, m_squelchOpen
    float prev_arg;                     // m_prevArg
    float distance;                     // m_interpolatorDistanceRemain
    double magsq_sum, magsq_peak;
    long long magsq_count;
    // --- per feed
    int n_in, n_blocks, n_dem, n_out;
    int dy_active, dy_mode, dy_pre, dy_cnt, dy_kb, dy_P0;   // closed-form schedule of this feed (backend_kernels.hpp 1b)
};

struct WfmBufs {                        // per channel device pointers (per feed capacity ensured by the host)
    const uint32_t* in;                 // n_in packed Samples
    const uint32_t* pend;               // WFM_H packed Samples: the pending ones
    uint32_t* pend_next;
    float2* head;                       // n_blocks * 512
    float2* tail;                       // (1 + n_blocks) * 512; slot 0 = ovlbuf carried from the previous feed
    float* arg;                         // atan2_approximation2 of every filtered sample
    uint8_t* flag;                      // magsq >= m_squelchLevel
    WfmClamp* blk_map;                  // per block: composed counter map of its 512 samples
    double* blk_sum; float* blk_peak;   // per block: sum / max of magsq
    int* blk_state;                     // per block: counter before its first sample
    int* blk_first;                     // per block: index of its first open sample (-1: none); its prevArg comes from an earlier block
    int* blk_last;                      // per block: index of its last open sample (-1: none)
    float* dem;                         // [WFM_HIST carried | 512 * n_blocks] demodulated samples
    uint2* sched;                       // per audio sample: {index of the completing input, bits(distance)}
    int16_t* audio;
    long n_in;
};

// ---- 1. per channel: block count, and the resampler schedule's closed form where the step is dyadic (240000/48000 = 5,
// 120000/48000 = 2.5 ...).  Same derivation as be_sched_dyadic_prep_kernel; the distance starts at `step`, which is on the
// 1/Q grid, and every operation keeps it there.
__device__ __forceinline__ void wfm_prep_body(WfmChan& s, const WfmBufs& b)
{
    const long n_new = b.n_in;
    s.n_in = (int)n_new;
    s.n_blocks = (int)((s.pending + n_new) / WFM_H);
    s.n_dem = s.n_blocks * WFM_H;
    s.n_out = 0;
    s.dy_active = 0;
    if (s.dy_q < 0) return;
    const int q = s.dy_q;
    const long Q = 1L << q, S = s.dy_S;
    const float d0 = s.distance;
    long D = (long)(d0 * (float)Q);                         // exact when d0 is on the grid
    if ((float)D / (float)Q != d0 || D > (1L << 40) || D < -(1L << 40)) return;
    const long n_in = s.n_dem;
    uint2* p = b.sched;
    long k = -1; int pre = 0;
    bool ended = false;
    while (D < Q && S != Q) {                               // start-up: one input per emission until the distance passes 1
        if (k + 1 >= n_in) { ended = true; break; }
        k += 1; D -= Q;
        *p++ = make_uint2((uint32_t)k, __float_as_uint((float)D / (float)Q)); pre++;
        D += S;
    }
    long cnt = 0, kb = 0, P0 = 0; int mode = 0;
    if (!ended) {
        if (D < Q) {                                        // S == Q and d < 1: one input per emission for ever, constant distance
            mode = 1; kb = k + 1; P0 = D - Q;
            cnt = n_in - 1 - k; if (cnt < 0) cnt = 0;
            k += cnt;
        } else {
            const long m0 = D >> q;
            P0 = D & (Q - 1); kb = k + m0;
            if (kb <= n_in - 1) {
                const long R = n_in - 1 - kb;
                const long J = (R * Q + Q - 1 - P0) / S;
                cnt = J + 1;
                k = kb + ((P0 + J * S) >> q);
                D = ((P0 + J * S) & (Q - 1)) + S;
            }
        }
    }
    D -= (n_in - 1 - k) * Q;                                // inputs consumed without an emission: each `-= 1.0` exact
    s.dy_active = 1; s.dy_mode = mode; s.dy_pre = pre; s.dy_cnt = (int)cnt; s.dy_kb = (int)kb; s.dy_P0 = (int)P0;
    s.distance = (float)D / (float)Q;
    s.n_out = pre + (int)cnt;
}

__device__ __forceinline__ void wfm_sched_fill_body(const WfmChan& s, const WfmBufs& b)
{
    if (!s.dy_active) return;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.dy_cnt) return;
    const int q = s.dy_q;
    const long Q = 1L << q, t = (long)s.dy_P0 + j * (long)s.dy_S;
    const float inv = 1.0f / (float)Q;                      // a power of two: the product below is the exact quotient
    const uint32_t k = s.dy_mode ? (uint32_t)(s.dy_kb + j) : (uint32_t)(s.dy_kb + (t >> q));
    const float d = s.dy_mode ? (float)s.dy_P0 * inv : (float)(t & (Q - 1)) * inv;
    b.sched[s.dy_pre + j] = make_uint2(k, __float_as_uint(d));
}

// the float recurrence itself for the other steps (250000/48000, 384000/44100 ...), emission by emission: while d >= 1 the
// reference's `d -= 1.0` is exact, so the next emission happens m = max(1, floor(d)) inputs later with d - m
__device__ __forceinline__ void wfm_sched_walk_body(WfmChan& s, const WfmBufs& b)
{
    if (s.dy_active) return;
    const int n = s.n_dem;
    const float step = s.step;
    uint2* __restrict__ p = b.sched;
    float d = s.distance;
    int k = -1, cnt = 0;
    for (;;) {
        const float m = fmaxf(floorf(d), 1.0f);
        const int kn = k + (int)m;
        if (kn >= n) break;
        k = kn; d -= m;
        p[cnt++] = make_uint2((uint32_t)k, __float_as_uint(d));
        d += step;
    }
    s.distance = d - (float)(n - 1 - k);
    s.n_out = cnt;
}

__device__ __forceinline__ uint32_t wfm_stream_sample(const WfmBufs& b, int pending, long j)
{
    return j < pending ? b.pend[j] : b.in[j - pending];
}

// ---- 2. one workgroup per (block, channel): NCO mix on load, zero-padded forward g_fft, filter over all 1024 bins,
// inverse g_fft; writes the head and tail halves (fftfilt::runFilt).  SCALED: the samples are divided by SDR_RX_SCALEF in front of
// the mix (BFMDemod::feed, bfm_kernels.hpp); WFMDemod mixes the integers as they are
template <bool SCALED>
__device__ __forceinline__ void wfm_fft_body(const WfmChan& s, const WfmBufs& b, const float2* __restrict__ filters,
                                             const float* __restrict__ utbl, const float* __restrict__ nco_tbl)
{
    constexpr int N = WFM_FFT, NT = N / 8, H = WFM_H;
    __shared__ float2 xa[N], ya[N];
    __shared__ float us[N / 4 + 1];
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= s.n_blocks) return;
    const int pending = s.pending;
    const uint32_t ph0 = (uint32_t)s.nco_phase, inc = (uint32_t)s.nco_inc & (WFM_NCO_N - 1);
    for (int i = tid; i <= N / 4; i += NT) us[i] = utbl[i];
    for (int i = tid; i < H; i += NT) {
        const long j = (long)blk * H + i;
        const uint32_t v = wfm_stream_sample(b, pending, j);
        // phase after nextPhase() for stream sample j: (phase0 + (j + 1) * inc) mod 4096, on the residues
        const uint32_t p = (ph0 + ((uint32_t)(j + 1) & (WFM_NCO_N - 1)) * inc) & (WFM_NCO_N - 1);
        const float o_r = nco_tbl[p], o_i = -nco_tbl[(p + WFM_NCO_N / 4) & (WFM_NCO_N - 1)];
        float a = (float)(int16_t)(v & 0xffffu), q = (float)(int16_t)(v >> 16);
        if (SCALED) { a = a / 32768.0f; q = q / 32768.0f; }
        float2 m; m.x = a * o_r - q * o_i; m.y = a * o_i + q * o_r;         // std::complex<float> operator*=
        xa[i] = m; xa[H + i] = make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    gfft<N, false>(ya, xa, us, tid);
    const float2* filt = filters + s.filt_off;
    for (int i = tid; i < N; i += NT) xa[i] = c_mul(ya[i], filt[i]);
    __syncthreads();
    gfft<N, true>(ya, xa, us, tid);
    for (int i = tid; i < H; i += NT) {
        b.head[(long)blk * H + i] = ya[i];
        b.tail[(long)(blk + 1) * H + i] = ya[H + i];
    }
}

// raw samples that did not fill a block: carried to the next feed (double-buffered).  The last reader of `in`.
__device__ __forceinline__ void wfm_pend_body(const WfmChan& s, const WfmBufs& b)
{
    const int i = threadIdx.x;
    const long total = (long)s.pending + s.n_in;
    const long j = (long)s.n_blocks * WFM_H + i;
    b.pend_next[i] = j < total ? wfm_stream_sample(b, s.pending, j) : 0u;
}

// a block's composed counter map, magsq sum and peak from two consecutive samples per lane (maps, sums, peaks: __shared__ [256])
__device__ __forceinline__ void wfm_block_reduce(const WfmBufs& b, int blk, int tid, int cap, bool f0, bool f1, float mag0, float mag1,
                                                 WfmClamp* maps, double* sums, float* peaks)
{
    maps[tid] = wfm_compose(wfm_step(f0, cap), wfm_step(f1, cap));
    sums[tid] = (double)mag0 + (double)mag1;
    peaks[tid] = fmaxf(mag0, mag1);
    __syncthreads();
    for (int st = 1; st < 256; st *= 2) {                   // neighbours first: keeps the order of the (non-commutative) maps
        if ((tid & (2 * st - 1)) == 0) {
            maps[tid] = wfm_compose(maps[tid], maps[tid + st]);
            sums[tid] += sums[tid + st];
            peaks[tid] = fmaxf(peaks[tid], peaks[tid + st]);
        }
        __syncthreads();
    }
    if (tid == 0) { b.blk_map[blk] = maps[0]; b.blk_sum[blk] = sums[0]; b.blk_peak[blk] = peaks[0]; }
}

__device__ __forceinline__ int wfm_wave_max_scan(int v, int lane)           // inclusive
{
    for (int o = 1; o < 64; o *= 2) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v = wfm_last_open(t, v);
    }
    return v;
}

// ---- 4. one wave per channel: scan of the block maps -> the counter in front of every block; level accumulators
__device__ __forceinline__ void wfm_blockscan_body(WfmChan& s, const WfmBufs& b)
{
    const int lane = threadIdx.x;
    const int nb = s.n_blocks, cap = s.cap;
    int carry = s.sq_state;
    double sum = 0.0; float peak = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int blk = b0 + lane;
        const bool in = blk < nb;
        const WfmClamp m = wg_wave_scan(WfmClampOps{cap}, in ? b.blk_map[blk] : wfm_identity(cap), lane);
        const int after = wfm_apply(m, carry);
        int before = __shfl_up(after, 1, 64);
        if (lane == 0) before = carry;
        if (in) { b.blk_state[blk] = before; sum += b.blk_sum[blk]; peak = fmaxf(peak, b.blk_peak[blk]); }
        carry = __shfl(after, 63, 64);
    }
    for (int o = 32; o; o >>= 1) { sum += __shfl_xor(sum, o, 64); peak = fmaxf(peak, __shfl_xor(peak, o, 64)); }
    if (lane == 0 && nb > 0) {
        s.magsq_sum += sum;
        if ((double)peak > s.magsq_peak) s.magsq_peak = (double)peak;
        s.magsq_count += (long long)nb * WFM_H;
        s.sq_state = carry;
        s.sq_open = (float)carry > s.open_f ? 1 : 0;
    }
}

__device__ __forceinline__ float wfm_discri(float cur, float prev, float fm_scaling)   // phaseDiscriminatorDelta
{
    float dev = (float)((double)(cur - prev) / 3.14159265358979323846);
    if (dev < -1.0f) dev += 2.0f; else if (dev > 1.0f) dev -= 2.0f;
    return dev * fm_scaling;
}

// the counter after a lane's two samples (scan of the step maps from the block's start state) -> their open flags.  Holds
// wg_scan's one barrier; wmap: __shared__ [4]
__device__ __forceinline__ void wfm_open_pair(const WfmChan& s, int blk_state, uchar2 f2, int lane, int w, WfmClamp* wmap, bool* open0, bool* open1)
{
    const int cap = s.cap;
    const WfmClamp m0 = wfm_step(f2.x != 0, cap), m1 = wfm_step(f2.y != 0, cap);
    const int before = wfm_apply(wg_scan(WfmClampOps{cap}, wfm_compose(m0, m1), lane, w, wmap), blk_state);
    const int st0 = wfm_apply(m0, before), st1 = wfm_apply(m1, st0);
    const bool live = !s.mute;
    *open0 = live && (float)st0 > s.open_f; *open1 = live && (float)st1 > s.open_f;             // m_squelchOpen && !m_audioMute
}

// ---- 7. real polyphase FIR, one lane per audio sample: taps summed newest-first like the ring walk (mul and add separate,
// in order; the reference's iAcc of the zero imaginary part does not touch rAcc)
__device__ __forceinline__ const float* wfm_fir_taps(const WfmChan& s, uint2 e, const float* __restrict__ taps)
{
    int ph = (int)floorf(__uint_as_float(e.y) * 16.0f);     // Interpolator::decimate's phase (interpolator.h:33)
    if (ph < 0) ph = 0;
    return taps + s.taps_off + ph * s.ntaps;
}
__device__ __forceinline__ float wfm_fir_acc(const float* __restrict__ t, int nt, const float* __restrict__ x)
{
    float acc = 0.0f;
#pragma unroll 8
    for (int i = 0; i < nt; i++) acc += t[i] * x[-i];
    return acc;
}

// ---- 8. carry: ovlbuf, the resampler window, NCO phase, pending count (one workgroup per channel, after everything else)
__device__ __forceinline__ void wfm_carry_body(WfmChan& s, const WfmBufs& b)
{
    const int tid = threadIdx.x;
    const int nb = s.n_blocks, n_dem = s.n_dem;
    if (nb > 0) b.tail[tid] = b.tail[(long)nb * WFM_H + tid];
    float keep = 0.0f;
    if (tid < WFM_HIST) keep = b.dem[n_dem + tid];          // the last WFM_HIST of [carried | new]
    __syncthreads();
    if (tid < WFM_HIST) b.dem[tid] = keep;
    if (tid == 0) {
        const long adv = ((long)nb * WFM_H) % WFM_NCO_N * ((long)s.nco_inc % WFM_NCO_N);
        long p = ((long)s.nco_phase + adv) % WFM_NCO_N;
        if (p < 0) p += WFM_NCO_N;
        s.nco_phase = (int)p;
        s.pending = (int)((long)s.pending + s.n_in - (long)nb * WFM_H);
    }
}

} // namespace sdrx
