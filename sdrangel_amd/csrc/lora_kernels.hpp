// LoRa demodulator bank kernels: LoRaDemod::feed behind the front (plugins/channelrx/demodlora/lorademod.cpp:191-288, sfft of
// sdrbase/dsp/fftfilt.cpp:406-457).  The front (NCO, Interpolator::decimate) is the channel back-end's; these kernels start
// from its complex resampler output `ci` at the bandwidth rate, unscaled: the division by SDR_RX_SCALEF, a power of two, is
// exact and commutes with the front, so it is applied where ci is loaded (as am_kernels.hpp does).
//     per output g:  a = chirp[m_angle(g)];  va = ci * a, vb = ci * conj(a);  z = v - k2 * v[128 outputs ago]      lora_dechirp_kernel
//                    bins[0 .. 126] = (bins + z) * vrot, both filters; every 64th: detect()'s fetch; m_bin; Sample  lora_walk_kernel
//                    the last 128 (va, vb) and the stream count for the next feed                                   lora_carry_kernel
// Samples are bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  lora_scan.hpp has the fetch step and why the walk is no scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lora_scan.hpp"
#include "wave_walk.hpp"

namespace sdrx {

constexpr int LORA_WALK_WAVES = 4;          // channels per workgroup of the walk, one wave each

struct LoraChan {                           // device resident: config + carried state of one channel
    // --- state
    long long count;                        // m_count as 64 bits: decimator outputs since creation or reset
    int bin;                                // m_bin
    // --- per feed
    int n;                                  // decimator outputs = Samples
    int n_lines;                            // lines dumpRaw ended
    // --- state the walk alone reads and writes
    float2 bins[4][64];                     // lane l: loraFilter's bins l and l + 64, negaFilter's bins l and l + 64
    float mov[4 * LORA_LEN];
    LoraSynch sy;
};

struct LoraBufs {                           // per channel device pointers (per feed capacity ensured by the host)
    const float2* ci;                       // the front's output of this feed
    const int* n_ptr;                       // its count (device side)
    const float4* vhist; float4* vhist_next;    // the last 128 (va, vb): the two delay lines
    float2* za; float2* zb;                 // per output: the two filters' z
    unsigned int* samples;                  // per output: Sample {re, im} as two int16
    char* text;                             // LORA_TEXT characters per line of the feed
    int max_lines;                          // ... for this many lines (lora_lines_bound of the arena's capacity)
};

struct LoraTables {                         // the same for every channel: design products of the constructor
    const float2* chirp;                    // [256] (float) cos(2 pi a / 256), (float) -sin(2 pi a / 256)
    const float2* vrot;                     // [128] sfft's vrot
    const unsigned int* sample;             // [128] Sample(cos(2 pi b / 128) * 100, sin(..) * 100)
    float k2;                               // sfft's k2
};

// (va, vb) of feed index j >= 0 whose stream index is g0 + j.  std::complex<float> products as (ac - bd, ad + bc): no infinity or
// NaN can arise (|ci| <= 1 after the scaling, K1 < 1 bounds the bins), so the __mulsc3 fallback of the reference is never taken.
__device__ __forceinline__ float4 lora_v(const LoraBufs& b, const float2* __restrict__ chirp, long long g0, long j)
{
    const float2 v = b.ci[j];
    const float re = v.x / 32768.0f, im = v.y / 32768.0f;      // SDR_RX_SCALEF
    const float2 a = chirp[lora_angle(g0 + j)];
    const float nay = -a.y;
    return make_float4(re * a.x - im * a.y, re * a.y + im * a.x, re * a.x - im * nay, re * nay + im * a.x);
}
// the same for j >= -128: the carried ones
__device__ __forceinline__ float4 lora_v_at(const LoraBufs& b, const float2* __restrict__ chirp, long long g0, long j)
{
    return j < 0 ? b.vhist[LORA_LEN + j] : lora_v(b, chirp, g0, j);
}

// ---- 1. per output: dechirp, and z against the output 128 earlier
__global__ __launch_bounds__(256)
void lora_dechirp_kernel(LoraChan* __restrict__ ch, const LoraBufs* __restrict__ bufs, LoraTables t)
{
    const int c = blockIdx.y, tid = threadIdx.x;
    const LoraBufs b = bufs[c];
    const int n = *b.n_ptr;
    if (blockIdx.x == 0 && tid == 0) ch[c].n = n;
    const long i = (long)blockIdx.x * 256 + tid;
    if (i >= n) return;
    const long long g0 = ch[c].count;
    const float4 v = lora_v(b, t.chirp, g0, i), d = lora_v_at(b, t.chirp, g0, i - LORA_LEN);
    b.za[i] = make_float2(v.x - t.k2 * d.x, v.y - t.k2 * d.y);
    b.zb[i] = make_float2(v.z - t.k2 * d.z, v.w - t.k2 * d.w);
}

// bins = (bins + z) * vrot
__device__ __forceinline__ void lora_bin_step(float2& bin, float zx, float zy, float2 v)
{
    const float tx = bin.x + zx, ty = bin.y + zy;
    bin = make_float2(tx * v.x - ty * v.y, tx * v.y + ty * v.x);
}

// the first strict maximum over the wave's 128 values (lane l holds values l and l + 64), starting from 0.0f: the largest
// value, and among equal ones the lowest index.  All values are >= 0, so "none above 0" is index 0 as well.
__device__ __forceinline__ void lora_first_max(float v0, float v1, int lane, float* peak, int* index)
{
    float val = v1 > v0 ? v1 : v0;
    int idx = v1 > v0 ? lane + 64 : lane;
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(val, off);
        const int oi = __shfl_xor(idx, off);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
    *peak = walk_lane_value(val, 0);
    *index = __builtin_amdgcn_readfirstlane(idx);
}

// ---- 2. the serial walk, one wave per channel: lane l keeps bins l and l + 64 of both filters in registers (bin 127 never
// moves: its vrot is zero here and its magnitude is forced to 0), 64 outputs' z are staged one per lane and each step takes
// its value from its lane's register.  A fetch falls on stream counts that are multiples of 64, wherever the feed began.
__global__ __launch_bounds__(64 * LORA_WALK_WAVES)
void lora_walk_kernel(LoraChan* __restrict__ ch, const LoraBufs* __restrict__ bufs, LoraTables t, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * LORA_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    LoraChan& s = ch[c];
    const LoraBufs b = bufs[c];
    const int n = s.n;
    if (n <= 0) { if (lane == 0) s.n_lines = 0; return; }
    float2 a0 = s.bins[0][lane], a1 = s.bins[1][lane], b0 = s.bins[2][lane], b1 = s.bins[3][lane];
    const float2 v0 = t.vrot[lane], v1 = lane < 63 ? t.vrot[lane + 64] : make_float2(0.0f, 0.0f);
    long long count = s.count;
    int bin = s.bin, result = s.sy.result, n_lines = 0;
    float* __restrict__ mov = s.mov;
    const float2 zero = make_float2(0.0f, 0.0f);
    float2 next_a = lane < n ? walk_global_load(b.za + lane) : zero, next_b = lane < n ? walk_global_load(b.zb + lane) : zero;
    for (int base = 0; base < n; base += 64) {
        const float2 cur_a = next_a, cur_b = next_b;
        if (base + 64 + lane < n) { next_a = walk_global_load(b.za + base + 64 + lane); next_b = walk_global_load(b.zb + base + 64 + lane); }
        const int cnt = min(64, n - base);
        int mine = 0;
        for (int j = 0; j < cnt; j++) {
            const float zax = walk_lane_value(cur_a.x, j), zay = walk_lane_value(cur_a.y, j);
            const float zbx = walk_lane_value(cur_b.x, j), zby = walk_lane_value(cur_b.y, j);
            lora_bin_step(a0, zax, zay, v0); lora_bin_step(a1, zax, zay, v1);
            lora_bin_step(b0, zbx, zby, v0); lora_bin_step(b1, zbx, zby, v1);
            count++;
            if (lora_is_fetch(count)) {                     // the wave's branch: count is uniform
                const bool top = lane == 63;                // bin 127: fetch never writes mag[127] / rev[127], which are 0 here
                const float m0 = a0.x * a0.x + a0.y * a0.y, m1 = top ? 0.0f : a1.x * a1.x + a1.y * a1.y;
                const float r0 = b0.x * b0.x + b0.y * b0.y, r1 = top ? 0.0f : b1.x * b1.x + b1.y * b1.y;
                const float t0 = mov[lane] + mov[LORA_LEN + lane] + mov[2 * LORA_LEN + lane] + mov[3 * LORA_LEN + lane] + m0;
                const float t1 = mov[64 + lane] + mov[LORA_LEN + 64 + lane] + mov[2 * LORA_LEN + 64 + lane] + mov[3 * LORA_LEN + 64 + lane] + m1;
                const int mp = lora_movpoint(count) * LORA_LEN;
                mov[mp + lane] = m0; mov[mp + 64 + lane] = m1;      // each lane reads and writes its own two columns only
                float peak, negpeak; int res, negres;
                lora_first_max(r0, r1, lane, &negpeak, &negres);
                lora_first_max(t0, t1, lane, &peak, &res);
                const int p = (res - 1 + LORA_LEN) & (LORA_LEN - 1), q = (res + 1) & (LORA_LEN - 1);
                const float mag_p = p < 64 ? walk_lane_value(m0, p & 63) : walk_lane_value(m1, p & 63);
                const float mag_q = q < 64 ? walk_lane_value(m0, q & 63) : walk_lane_value(m1, q & 63);
                int r = 0;
                if (lane == 0) r = lora_fetch_step(s.sy, mag_p, mag_q, peak, negpeak, (short)res, b.text, &n_lines, b.max_lines);
                result = __builtin_amdgcn_readfirstlane(r);
            }
            bin = (bin + result) & (LORA_LEN - 1);
            if (lane == j) mine = bin;
        }
        if (base + lane < n) walk_global_store(b.samples + base + lane, t.sample[mine]);
    }
    s.bins[0][lane] = a0; s.bins[1][lane] = a1; s.bins[2][lane] = b0; s.bins[3][lane] = b1;
    if (lane == 0) { s.bin = bin; s.n_lines = n_lines; }
}

// ---- 3. carry: the delay lines of the next feed (double-buffered: this feed's are still being read) and the stream count
__global__ __launch_bounds__(LORA_LEN)
void lora_carry_kernel(LoraChan* __restrict__ ch, const LoraBufs* __restrict__ bufs, LoraTables t)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    LoraChan& s = ch[c];
    const LoraBufs b = bufs[c];
    const int n = s.n;
    const long long g0 = s.count;
    b.vhist_next[tid] = lora_v_at(b, t.chirp, g0, (long)n - LORA_LEN + tid);
    __syncthreads();                                        // every lane has read count
    if (tid == 0) s.count = g0 + n;
}

} // namespace sdrx
