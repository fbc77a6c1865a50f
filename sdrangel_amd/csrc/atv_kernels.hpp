// ATV demodulator bank kernels: ATVDemod::feed behind the NCO mix and ATVDemod::demod (plugins/channelrx/demodatv/atvdemod.cpp:
// 167-444, atvdemod.h:498-744).  The front (the NCO mix, or none at offset 0) is the channel back-end's in bypass; these kernels
// start from its output, the mixed sample c unscaled as the reference holds it.
//     the "decimator": its step is <= 1 and its distance never reaches 1, so every input emits at phase 0: the 72-tap
//                  phase-0 row of create(24, tvRate, ..) as a FIR at the input rate, doInterpolate's order              atv_fir_kernel
//     the FFT filter: runAsym on blocks of 1024 of the stream (2048-point g_fft, filter / filterOpp), head and tail     atv_filt_kernel
//     per sample:  the sample demod() reads: the filtered stream 1023 samples late behind 1023 zeros (m_DSBFilterBuffer's
//                  slot index - 1, refilled every 1024th call), or ci; FM1 / FM2: the normalised (I, Q) and the stencil
//                  over the 2 / 6 normalised samples before it, the deviation scaling; FM3: phaseDiscriminatorDelta of the
//                  UNFILTERED ci + 0.5; AM: sqrt(magSq) / SDR_RX_SCALEF; and for FM, where nothing of it hangs on the
//                  line, the inversion, the clamp, the scope Sample and the grey level                                  atv_video_kernel
//                  the same four for AM behind its normalisation by the line before; the running sum, processClassic /
//                  processHSkip, pixels into the channel's image, a snapshot at each of the first frames_cap renders    atv_walk_kernel
//                  the filter's pending input, overlap and last block, FM3's last argument, the stream position        atv_carry_kernel
// Every output is bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  atv_scan.hpp has the per-sample step, shared with the host check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "atv_scan.hpp"
#include "wave_walk.hpp"
#include "gfft_kernel.hpp"                  // gfft<N>, c_mul, atan2_approx2

namespace sdrx {

constexpr int ATV_WALK_WAVES = 4;           // channels per workgroup of the walk, one wave each
constexpr int ATV_HIST = 6;                 // m_fltBufferI / Q
constexpr int ATV_FFT = 2048;               // 2 * m_ssbFftLen
constexpr int ATV_BLK = ATV_FFT / 2;        // samples per runAsym block, and m_DSBFilterBuffer's length
constexpr int ATV_TAPS_MAX = 128;           // taps per phase the FIR's carried input covers (create(24, .., 3.0) has 72)

struct AtvChan {                            // device resident: config + carried state of one channel
    // --- config
    AtvDesign d;
    int frames_cap;
    int img_bytes;                          // rows * cols rounded up to whole words: a snapshot's pitch
    unsigned char* img;                     // the screen: rows * cols grey levels, carried from feed to feed
    int decim, filt;                        // m_blndecimatorEnable, m_blnFFTFiltering
    int ntaps;                              // taps of the phase-0 row
    float fm_scaling;                       // FM3: 1.0f / m_fmDeviation
    const float* taps;                      // the phase-0 row
    const float2* filters;                  // [filter 2048 | filterOpp 2048]
    const float* utbl;                      // g_fft's cosine table for 2048
    float2* pend;                           // ATV_BLK: the inputs of the block that is not full yet (fftfilt's data[0 .. inptr))
    float2* ovl;                            // ATV_BLK: ovlbuf
    float2* fbuf;                           // ATV_BLK: m_DSBFilterBuffer, the last block runAsym returned
    // --- state
    AtvState s;
    float2 hist[ATV_HIST];                  // (m_fltBufferI[k], m_fltBufferQ[k]): a copy for the state getter
    long long g;                            // demod() calls since creation or reset
    float prev_arg;                         // m_objPhaseDiscri's m_prevArg
    // --- per feed
    int n;                                  // demodulated samples = inputs
    int n_events;                           // renderImage calls
    int n_scope;                            // Samples of the scope buffer: n, or 0 without a scope
};

struct AtvBufs {                            // per channel device pointers (per feed capacity ensured by the host)
    const float2* x;                        // the front's output of this feed: the mixed samples
    const int* n_ptr;                       // its count (device side)
    const float2* nh; float2* nh_next;      // the last 6 normalised samples, newest first
    const float2* xh; float2* xh_next;      // the last ATV_TAPS_MAX mixed samples, oldest first: the FIR's ring
    float2* ci;                             // per sample: the FIR's output (decimator channels)
    float2* head; float2* tail;             // per block of the feed: runAsym's two halves; tail is shifted by one block, slot 0 = ovl
    float* raw;                             // per sample: FM's fltVal, inverted and clamped, or AM's value before its normalisation
    unsigned char* grey;                    // per sample, FM only: the grey level
    int16_t* scope;                         // per sample: the scope Sample's real part
    int* events;                            // per render: the index of its sample within the feed
    unsigned char* snaps;                   // frames_cap snapshots of img_bytes
};

// the mixed sample j of the feed, j >= -ATV_TAPS_MAX
__device__ __forceinline__ float2 atv_mixed_at(const AtvBufs& b, long j) { return j < 0 ? b.xh[ATV_TAPS_MAX + j] : b.x[j]; }

// ---- 0a. the "decimator": sum of taps[t] * c[i - t], newest first, multiply and add apart (doInterpolate, interpolator.h:182-195)
__global__ __launch_bounds__(256)
void atv_fir_kernel(AtvChan* __restrict__ ch, const AtvBufs* __restrict__ bufs)
{
    __shared__ float tp[ATV_TAPS_MAX];
    __shared__ float2 win[256 + ATV_TAPS_MAX];
    const int c = blockIdx.y, tid = threadIdx.x;
    const AtvChan& q = ch[c];
    if (!q.decim) return;                                   // uniform
    const AtvBufs b = bufs[c];
    const int n = *b.n_ptr, nt = q.ntaps;
    const long i0 = (long)blockIdx.x * 256, i = i0 + tid;
    if (blockIdx.x == 0 && tid < ATV_TAPS_MAX) b.xh_next[tid] = atv_mixed_at(b, (long)n - ATV_TAPS_MAX + tid);
    if (i0 >= n) return;                                    // uniform
    if (tid < nt) tp[tid] = q.taps[tid];
    for (int k = tid; k < 256 + ATV_TAPS_MAX; k += 256) {   // win[k] is sample i0 - ATV_TAPS_MAX + k
        const long j = i0 - ATV_TAPS_MAX + k;
        win[k] = j < n ? atv_mixed_at(b, j) : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    if (i >= n) return;
    const float2* x = win + ATV_TAPS_MAX + tid;
    float ra = 0.0f, ia = 0.0f;
    for (int t = 0; t < nt; t++) {
        const float2 v = x[-t];
        ra += tp[t] * v.x;
        ia += tp[t] * v.y;
    }
    b.ci[i] = make_float2(ra, ia);
}

// what demod() is called with: the decimator's output, or the mixed sample
__device__ __forceinline__ float2 atv_ci_at(const AtvChan& q, const AtvBufs& b, long i) { return q.decim ? b.ci[i] : b.x[i]; }

// ---- 0b. the FFT filter: block `blk` of the feed is the stream's block g / 1024 + blk; its inputs lie in pend (before the feed)
// and in ci.  runAsym usb (fftfilt.cpp:361-402): data[0] *= filter[0], the upper side through filter, the lower through
// filterOpp, bin N / 2 left alone.
__global__ __launch_bounds__(ATV_FFT / 8)
void atv_filt_kernel(AtvChan* __restrict__ ch, const AtvBufs* __restrict__ bufs)
{
    constexpr int N = ATV_FFT, NT = N / 8, H = N / 2;
    __shared__ float2 xa[N], ya[N];
    __shared__ float us[N / 4 + 1];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const AtvChan& q = ch[c];
    if (!q.filt) return;                                    // uniform
    const AtvBufs b = bufs[c];
    const int n = *b.n_ptr;
    const long long g = q.g;
    const int fill = (int)(g & (H - 1));                    // inputs already in pend
    const int nb = (int)((fill + (long long)n) / H);
    if (blk >= nb) return;                                  // uniform
    for (int i = tid; i <= N / 4; i += NT) us[i] = q.utbl[i];
    for (int i = tid; i < H; i += NT) {
        const long j = (long)blk * H + i - fill;            // index within the feed
        xa[i] = j < 0 ? q.pend[fill + j] : atv_ci_at(q, b, j);
        xa[H + i] = make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    gfft<N, false>(ya, xa, us, tid);
    const float2* filt = q.filters;
    for (int i = tid; i < H; i += NT) {
        float2 lo = ya[i], hi = ya[H + i];
        if (i == 0) lo = c_mul(lo, filt[0]);
        else { lo = c_mul(lo, filt[i]); hi = c_mul(hi, filt[N + H + i]); }
        xa[i] = lo; xa[H + i] = hi;
    }
    __syncthreads();
    gfft<N, true>(ya, xa, us, tid);
    for (int i = tid; i < H; i += NT) {
        b.head[(long)blk * H + i] = ya[i];
        b.tail[(long)(blk + 1) * H + i] = ya[H + i];
    }
}

// the sample demod() reads as fltI, fltQ for feed index i >= 0: with the filter on, slot index - 1 of m_DSBFilterBuffer, which
// holds zeros until the 1024th call and then the block that ended 0 .. 1023 calls ago
__device__ __forceinline__ float2 atv_src_at(const AtvChan& q, const AtvBufs& b, long i)
{
    if (!q.filt) return atv_ci_at(q, b, i);
    const long long g = q.g + i;
    if (g < ATV_BLK - 1) return make_float2(0.0f, 0.0f);
    const long long f = g - (ATV_BLK - 1);                  // index into the filtered stream
    const long long done = q.g >> 10;                       // blocks returned before this feed
    const long long blk = f >> 10;
    const int k = (int)(f & (ATV_BLK - 1));
    if (blk < done) return q.fbuf[k];                       // then blk == done - 1
    const long o = (long)(blk - done) * ATV_BLK + k;
    const float2 t = (blk == done) ? q.ovl[k] : b.tail[o], h = b.head[o];
    return make_float2(t.x + h.x, t.y + h.y);               // output[i] = ovlbuf[i] + data[i]
}

// the normalised sample j of the feed, j >= -6: the carried ones before 0
__device__ __forceinline__ AtvNorm atv_norm_at(const AtvChan& q, const AtvBufs& b, long j)
{
    if (j < 0) { const float2 h = b.nh[-j - 1]; AtvNorm n; n.i = h.x; n.q = h.y; return n; }
    const float2 v = atv_src_at(q, b, j);
    return atv_normalise(v.x, v.y);
}

// FM's sample behind the discriminator: nothing of it hangs on the walk's state, so the inversion, the clamp, the grey level's
// division and the scope Sample are done here, per sample, and the walk keeps the running sum and the state machine
__device__ __forceinline__ void atv_fm_finish(const AtvDesign& d, const AtvBufs& b, long i, float r)
{
    AtvState unused;                                        // atv_level reads the state for AM alone
    const float v = atv_level(d, unused, r);
    b.raw[i] = v;
    b.grey[i] = (unsigned char)atv_grey(d, v);
    if (d.scope) b.scope[i] = atv_scope_sample(v);
}

// ---- 1. per sample: the discriminators.  FM1 / FM2 stage a workgroup's normalised samples and the 6 before them in LDS.
__global__ __launch_bounds__(256)
void atv_video_kernel(AtvChan* __restrict__ ch, const AtvBufs* __restrict__ bufs)
{
    __shared__ AtvNorm nrm[256 + ATV_HIST];
    const int c = blockIdx.y, tid = threadIdx.x;
    const AtvBufs b = bufs[c];
    const int n = *b.n_ptr;
    const AtvChan& q = ch[c];
    const AtvDesign d = q.d;
    const int mod = d.modulation;
    const float dev = d.fm_deviation;
    if (blockIdx.x == 0 && tid == 0) ch[c].n = n;
    const long i0 = (long)blockIdx.x * 256, i = i0 + tid;
    if (i0 >= n && blockIdx.x != 0) return;                 // uniform
    const bool fm12 = mod == ATV_FM1 || mod == ATV_FM2;
    if (fm12) {
        if (i < n) nrm[ATV_HIST + tid] = atv_norm_at(q, b, i);
        if (tid < ATV_HIST) nrm[tid] = atv_norm_at(q, b, i0 - ATV_HIST + tid);
        __syncthreads();
        if (i < n) {
            const AtvNorm* p = nrm + ATV_HIST + tid;        // p[-k - 1] is m_fltBuffer[k]
            const float v = mod == ATV_FM1 ? atv_fm1(p[0], p[-1], p[-2]) : atv_fm2(p[0], p[-2], p[-3], p[-4], p[-6]);
            atv_fm_finish(d, b, i, atv_fm_deviation(v, dev));
        }
        // the buffers of the next feed: FM1 moves [0] and [1] only, the rest stays 0
        if (blockIdx.x == 0 && tid < ATV_HIST) {
            const AtvNorm h = atv_norm_at(q, b, (long)n - 1 - tid);
            const float2 v = (mod == ATV_FM1 && tid >= 2) ? make_float2(0.0f, 0.0f) : make_float2(h.i, h.q);
            b.nh_next[tid] = v;
            ch[c].hist[tid] = v;
        }
        return;
    }
    if (blockIdx.x == 0 && tid < ATV_HIST) b.nh_next[tid] = make_float2(0.0f, 0.0f);
    if (i >= n) return;
    if (mod == ATV_FM3) {
        // phaseDiscriminatorDelta(c, ..) (phasediscri.h:61-78) on the sample demod() was called with, filter or not
        const float2 v = atv_ci_at(q, b, i);
        const float cur = atan2_approx2(v.y, v.x);
        float prev = q.prev_arg;
        if (i > 0) { const float2 pv = atv_ci_at(q, b, i - 1); prev = atan2_approx2(pv.y, pv.x); }
        float fm = (float)((double)(cur - prev) / 3.14159265358979323846);
        if (fm < -1.0f) fm += 2.0f; else if (fm > 1.0f) fm -= 2.0f;
        atv_fm_finish(d, b, i, fm * q.fm_scaling + 0.5f);
    } else {
        const float2 v = atv_src_at(q, b, i);
        b.raw[i] = atv_am_raw(v.x, v.y);
    }
}

// the walk's byte and word streams as global memory by name (wave_walk.hpp): a generic store would count on the LDS / scalar-memory
// counter, and every step would wait for the pixel of the step before
typedef __attribute__((address_space(1))) unsigned char walk_global_u8;
typedef __attribute__((address_space(1))) int walk_global_i32;

// what atv_step calls: every lane of the wave holds the same values, lane 0 stores the pixels, the wave copies a snapshot
struct AtvWalkOut {
    unsigned char* img; unsigned char* snaps; int* events;
    int cols, lane, frames_cap, img_bytes;
    int n_events, idx;
    int16_t sample;
    __device__ __forceinline__ void hit(int) {}
    __device__ __forceinline__ void scope(int16_t v) { sample = v; }
    __device__ __forceinline__ void pixel(int row, int col, int grey)
    {
        if (lane == 0) ((walk_global_u8*)img)[(size_t)row * (size_t)cols + (size_t)col] = (unsigned char)grey;
    }
    __device__ __forceinline__ void render()
    {
        if (n_events < frames_cap) {
            __threadfence();                                // lane 0's pixels are in memory before any lane reads them
            const unsigned int* src = reinterpret_cast<const unsigned int*>(img);
            unsigned int* dst = reinterpret_cast<unsigned int*>(snaps + (size_t)n_events * (size_t)img_bytes);
            for (int w = lane; w < img_bytes / 4; w += 64) dst[w] = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();                                // ... and the copy has read them before the next pixel lands
        }
        if (lane == 0) ((walk_global_i32*)events)[n_events] = idx;
        n_events++;
    }
};

// A stretch of a line at a time (FM under processClassic): `cnt` samples from column s.col_index on among which no line ends and
// the half-frame branch stays shut, lane k taking sample k.  What is not sequential goes to the lanes: the pixel of column
// col + k, `v < top` and `v > black` as two ballots from which every lane counts its m_intSynchroPoints (the set bits of the first
// since the last set bit of the second, or since the stretch began plus the carried count) and so the detections; the last
// detection gives m_intAvgColIndex and m_intSampleIndex in closed form.  m_fltAmpLineAverage stays a serial chain of float adds in
// sample order, every lane keeping its prefix; past three quarters of the line the prefixes are held against the vsync level, and
// only if none is at or under it (no vsync fires: the flag is just cleared) does the stretch stand.  Returns false, with the
// state untouched, where it does not: the caller then walks the stretch sample by sample.  Pixels stored before that are the ones
// the walk stores again.
__device__ __forceinline__ bool atv_fast_stretch(const AtvDesign& d, AtvState& s, float v, int grey, int cnt, int lane, unsigned char* img)
{
    const unsigned long long live = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
    const bool in = lane < cnt;
    const bool lt = in && v < d.level_top, gt = in && !lt && v > d.level_black;
    const unsigned long long LT = __ballot(lt), GT = __ballot(gt);
    const unsigned long long upto = lane >= 63 ? ~0ull : ((2ull << lane) - 1ull);       // bits 0 .. lane
    const unsigned long long R = GT & upto;
    int p;
    if (R) {
        const int r = 63 - __clzll((long long)R);
        const unsigned long long after = r >= 63 ? 0ull : ~((2ull << r) - 1ull);
        p = __popcll(LT & upto & after);
    } else {
        p = (int)((unsigned)s.synchro_points + (unsigned)__popcll(LT & upto));
    }
    const unsigned long long D = __ballot(in && p == d.spt);
    // the running sum, in sample order
    float a = s.amp_line_average, mine = 0.0f;
    for (int j = 0; j < cnt; j++) {
        a = atv_x86_nan(a + walk_lane_value(v, j));
        if (lane == j) mine = a;
    }
    const int sync_time = (3 * d.spl) / 4;
    const bool watched = d.vsync && s.line_index < d.n_lines;
    const bool region = in && watched && s.col_index + lane + 1 >= sync_time;
    const float level = 0.5f * ((float)sync_time) * d.level_black;
    if (__ballot(region && mine <= level)) return false;
    // pixels
    const int pc = s.col_index + lane - d.sp_hsync + d.spt + 4;
    if (in && pc >= 0 && pc < d.cols && s.screen_row >= 0) ((walk_global_u8*)img)[(size_t)s.screen_row * (size_t)d.cols + (size_t)pc] = (unsigned char)grey;
    // the state behind the stretch
    if (D) {
        const int jl = 63 - __clzll((long long)D);
        const unsigned long long below = D & ((1ull << jl) - 1ull);
        const int si = below ? jl - (63 - __clzll((long long)below)) - 1 : (int)((unsigned)s.sample_index + (unsigned)jl);
        const int col_at = s.col_index + jl;
        s.avg_col_index = si - col_at - (col_at < d.spl / 2 ? 150 : 0);
        s.sample_index = cnt - 1 - jl;
    } else {
        s.sample_index = (int)((unsigned)s.sample_index + (unsigned)cnt);
    }
    s.synchro_points = __builtin_amdgcn_readlane(p, cnt - 1);
    s.synchro_detected = (int)((D >> (cnt - 1)) & 1ull);
    if (__ballot(region)) s.vsynchro_detected = 0;
    s.amp_line_average = a;
    s.col_index += cnt;
    (void)live;
    return true;
}

// ---- 2. the sync / screen walk, one wave per channel: 64 samples are staged one per lane and each step takes its value from
// its lane's register, so the step's values and branches are the wave's.  FM runs atv_sync on the video kernel's value and grey;
// AM, whose value hangs on the extrema of the line before, runs the whole atv_step.
__global__ __launch_bounds__(64 * ATV_WALK_WAVES)
void atv_walk_kernel(AtvChan* __restrict__ ch, const AtvBufs* __restrict__ bufs, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * ATV_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    AtvChan& q = ch[c];
    const AtvBufs b = bufs[c];
    const int n = q.n;
    const AtvDesign d = q.d;
    AtvState s = q.s;
    AtvWalkOut out;
    out.img = q.img; out.snaps = b.snaps; out.events = b.events;
    out.cols = d.cols; out.lane = lane; out.frames_cap = q.frames_cap; out.img_bytes = q.img_bytes;
    out.n_events = 0; out.idx = 0; out.sample = 0;
    const bool am = d.modulation == ATV_AM;
    float next = lane < n ? walk_global_load(b.raw + lane) : 0.0f;
    const walk_global_u8* greys = (const walk_global_u8*)b.grey;
    int next_g = (!am && lane < n) ? (int)greys[lane] : 0;
    for (int base = 0; base < n; base += 64) {
        const float cur = next;
        const int cur_g = next_g;
        if (base + 64 + lane < n) {
            next = walk_global_load(b.raw + base + 64 + lane);
            if (!am) next_g = (int)greys[base + 64 + lane];
        }
        const int cnt = min(64, n - base);
        if (am) {
            int16_t mine = 0;
            for (int j = 0; j < cnt; j++) {
                out.idx = base + j;
                atv_step(d, s, walk_lane_value(cur, j), out);
                if (lane == j) mine = out.sample;
            }
            if (d.scope && base + lane < n) b.scope[base + lane] = mine;
        } else {
            int j = 0;
            while (j < cnt) {
                // how far from here no line ends: up to the column at which processClassic starts a new line
                const int room = (d.hsync ? d.spl + d.spt : d.spl) - s.col_index;
                const bool shut = (d.vsync && s.line_index < d.n_lines) || s.line_index < d.n_lines / 2;      // the half-frame branch
                int span = min(cnt - j, room);
                if (!d.hskip && shut && span >= 8) {
                    const float fv = __shfl(cur, j + lane);
                    const int fg = __shfl(cur_g, j + lane);
                    if (atv_fast_stretch(d, s, fv, fg, span, lane, out.img)) { j += span; continue; }
                } else {
                    span = 1;
                }
                for (const int end = j + span; j < end; j++) {
                    out.idx = base + j;
                    atv_sync(d, s, walk_lane_value(cur, j), __builtin_amdgcn_readlane(cur_g, j), out);
                }
            }
        }
    }
    if (lane == 0) { q.s = s; q.n_events = out.n_events; q.n_scope = d.scope ? n : 0; }
}


// ---- 3. carry, one workgroup per channel behind everything else: what the next feed's kernels read of this one
__global__ __launch_bounds__(256)
void atv_carry_kernel(AtvChan* __restrict__ ch, const AtvBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    AtvChan& q = ch[c];
    const AtvBufs b = bufs[c];
    const int n = q.n;
    const long long g = q.g;
    if (q.filt) {
        const int fill = (int)(g & (ATV_BLK - 1));
        const int nb = (int)((fill + (long long)n) / ATV_BLK);
        const int left = (int)((fill + (long long)n) - (long long)nb * ATV_BLK);       // inputs of the block that is not full yet
        float2 keep[ATV_BLK / 256], last[ATV_BLK / 256], ov[ATV_BLK / 256];
        for (int r = 0; r < ATV_BLK / 256; r++) {
            const int k = r * 256 + tid;
            const long j = (long)nb * ATV_BLK + k - fill;   // index within the feed
            keep[r] = k < left ? (j < 0 ? q.pend[fill + j] : atv_ci_at(q, b, j)) : make_float2(0.0f, 0.0f);
            if (nb > 0) {
                const long o = (long)(nb - 1) * ATV_BLK + k;
                const float2 t = nb == 1 ? q.ovl[k] : b.tail[o], h = b.head[o];
                last[r] = make_float2(t.x + h.x, t.y + h.y);
                ov[r] = b.tail[(long)nb * ATV_BLK + k];
            }
        }
        __syncthreads();                                    // every read of pend and ovl is done
        for (int r = 0; r < ATV_BLK / 256; r++) {
            const int k = r * 256 + tid;
            if (k < left) q.pend[k] = keep[r];
            if (nb > 0) { q.fbuf[k] = last[r]; q.ovl[k] = ov[r]; }
        }
    }
    if (tid == 0) {
        if (q.d.modulation == ATV_FM3 && n > 0) { const float2 v = atv_ci_at(q, b, (long)n - 1); q.prev_arg = atan2_approx2(v.y, v.x); }
        q.g = g + n;
    }
}

} // namespace sdrx
