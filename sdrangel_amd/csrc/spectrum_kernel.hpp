// Device code of sdrx_spectrum_* (sdrx_spectrum.hip): SpectrumVis::feed (sdrgui/dsp/spectrumvis.cpp:70-250) for every frame
// a feed completes, bit for bit in the transform, the power and the averaging.
//
// The reference keeps a 4096-entry complex buffer B.  With ov = N*pct/100, R = N - ov and S = R - ov, frame k of a feed
// transforms B[0, N) where
//   B[ov, R)  fresh samples:   frame 0 takes the pending fill [ov, fill0) from B and input [0, R - fill0) at [fill0, R);
//                              frame k >= 1 takes input (R - fill0) + (k-1)*S + [0, S)
//   elsewhere stale entries:   after each frame std::copy(B+R, B+4096, B) moves entry q+R to q (q < 4096-R) and leaves
//                              [4096-R, 4096) alone, so a stale position p at frame k holds B0[p + t*R] with
//                              t = min(k, ceil((4096 - R - p) / R)) (t = 0 when p >= 4096 - R); a fresh entry is never
//                              moved into a stale position of a later frame of the same feed (it would have to come from >= R).
// B0 is the device copy of B at the start of the feed, pending fill included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrx_spec {

constexpr int BUF = 4096;          // MAX_FFT_SIZE (spectrumvis.cpp:6)
constexpr int NT = 256;            // threads per workgroup
constexpr int MIN_LDS_CPLX = 1024; // frames per workgroup = max(1, 1024 / N)

struct Geom {
    int n, log2n, ov, r, s;        // N, log2 N, overlap, refill size R, fresh samples per frame S = R - ov
    int fill0;                     // B fill at the start of the feed (ov <= fill0 < R)
    int nst, last_radix;           // kissfft stages: nst - 1 radix-4 stages, then radix 4 or 2
    int fpb;                       // frames per workgroup
    int frames;                    // frames this feed completes
    int stale_zero;                // every stale position of B0 holds zero (fresh object): no B0 reads for them
    float scalef;
};

struct Post {                      // power -> output (spectrumvis.cpp:107-145)
    int linear, positive_only;
    float mult, ofs, powdiv;       // m_mult, m_ofs, m_powFFTDiv
};

__device__ __forceinline__ float2 scaled(uint32_t v, float scalef)
{
    // Complex(begin->real() / m_scalef, begin->imag() / m_scalef)
    return make_float2((float)(int16_t)(v & 0xffffu) / scalef, (float)(int16_t)(v >> 16) / scalef);
}

// B'_k[p]: what frame k transforms at position p (before the window)
__device__ __forceinline__ float2 frame_value(const Geom& g, const uint32_t* __restrict__ in, const float2* __restrict__ b0,
                                              long k, int p, bool stale_reads)
{
    if (p >= g.ov && p < g.r) {
        if (k == 0) return p < g.fill0 ? b0[p] : scaled(in[p - g.fill0], g.scalef);
        return scaled(in[(long)(g.r - g.fill0) + (k - 1) * g.s + (p - g.ov)], g.scalef);
    }
    if (!stale_reads) return make_float2(0.f, 0.f);
    int q = p;
    const int lim = BUF - g.r;
    if (k > 0 && q < lim) {
        long t = (lim - q + g.r - 1) / g.r;
        if (t > k) t = k;
        q += (int)t * g.r;
    }
    return b0[q];
}

// kissfft's C_MUL (kissfft.h), strict operation order
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ float log2_as_float(float v)
{
    // glibc's log2f, evaluated in double and rounded once (DESIGN.md "Spectrum sink" gives the measured agreement)
    return (float)::log2((double)v);
}

__device__ __forceinline__ float post_value(const Post& o, float v)
{
    return o.linear ? v / o.powdiv : o.mult * log2_as_float(v) + o.ofs;
}

// out index of bin b: fft-shift, or both halves of the pair with positiveOnly (only bins < N/2 are emitted then)
__device__ __forceinline__ void store_bin(float* __restrict__ frame, int n, int b, bool positive_only, float val)
{
    if (positive_only) {
        if (b < n / 2) { frame[2 * b] = val; frame[2 * b + 1] = val; }
    } else {
        frame[(b + n / 2) & (n - 1)] = val;
    }
}

// One workgroup transforms g.fpb frames (fpb * N <= 4096 complex values of LDS).  raw != 0: writes |X|^2 in bin order
// (the averaging kernel finishes it), else the emitted frame (fft-shifted, linear or dB) to out + k*N.
__global__ __launch_bounds__(NT)
void spectrum_fft_kernel(const uint32_t* __restrict__ in, const float2* __restrict__ b0, const float* __restrict__ win,
                         const float2* __restrict__ tw, float* __restrict__ out, Geom g, Post o, int raw)
{
    extern __shared__ float2 lds[];
    const int tid = threadIdx.x;
    const int n = g.n, total = g.fpb * n;
    const long k0 = (long)blockIdx.x * g.fpb;
    const bool stale_reads = !g.stale_zero;

    // 1. load, scale, window (FFTWindow::apply: (re*w, im*w)), scatter to kissfft's leaf order (mixed-radix digit reversal:
    //    the digit of stage s of the input index is the stage's sub-DFT, whose outputs sit at q_s * m_s)
    for (int idx = tid; idx < total; idx += NT) {
        const int lf = idx >> g.log2n, p = idx & (n - 1);
        const long k = k0 + lf;
        if (k >= g.frames) break;
        float2 x = frame_value(g, in, b0, k, p, stale_reads);
        const float w = win[p];
        x.x = x.x * w; x.y = x.y * w;
        int dst = 0, rest = p, m = n;
        for (int s = 0; s < g.nst; s++) {
            const int lr = (s == g.nst - 1 && g.last_radix == 2) ? 1 : 2;
            m >>= lr;
            dst += (rest & ((1 << lr) - 1)) * m;
            rest >>= lr;
        }
        lds[lf * n + dst] = x;
    }
    __syncthreads();

    // 2. butterflies, innermost stage first (kf_work recombines after its recursive calls).  Stage s: radix p, m = N / 4^s / p,
    //    fstride = 4^s; every (group, k) butterfly touches its own p entries, so the lanes of a stage are independent.
    //    All sizes are powers of two: indices come from shifts and masks.
    int fstride = 1 << (2 * (g.nst - 1));
    for (int s = g.nst - 1; s >= 0; s--, fstride >>= 2) {
        const int radix = (s == g.nst - 1) ? g.last_radix : 4;
        const int lr = radix == 4 ? 2 : 1;
        const int log2m = g.log2n - 2 * s - lr;              // m = N / (fstride * radix)
        const int m = 1 << log2m;
        const int log2pf = g.log2n - lr;                     // butterflies per frame = N / radix
        for (int u = tid; u < (g.fpb << log2pf); u += NT) {
            const int lf = u >> log2pf, w = u & ((1 << log2pf) - 1);
            const int grp = w >> log2m, k = w & (m - 1);
            float2* F = lds + lf * n + ((grp * radix) << log2m);
            if (radix == 4) {               // kf_bfly4, forward (negative_if_inverse = 1)
                const float2 s0 = cmul(F[k + m], tw[k * fstride]);
                const float2 s1 = cmul(F[k + 2 * m], tw[k * fstride * 2]);
                const float2 s2 = cmul(F[k + 3 * m], tw[k * fstride * 3]);
                float2 f0 = F[k];
                const float2 s5 = make_float2(f0.x - s1.x, f0.y - s1.y);
                f0.x = f0.x + s1.x; f0.y = f0.y + s1.y;
                const float2 s3 = make_float2(s0.x + s2.x, s0.y + s2.y);
                float2 s4 = make_float2(s0.x - s2.x, s0.y - s2.y);
                s4 = make_float2(s4.y, -s4.x);
                F[k + 2 * m] = make_float2(f0.x - s3.x, f0.y - s3.y);
                F[k] = make_float2(f0.x + s3.x, f0.y + s3.y);
                F[k + m] = make_float2(s5.x + s4.x, s5.y + s4.y);
                F[k + 3 * m] = make_float2(s5.x - s4.x, s5.y - s4.y);
            } else {                        // kf_bfly2
                const float2 t = cmul(F[m + k], tw[k * fstride]);
                const float2 f0 = F[k];
                F[m + k] = make_float2(f0.x - t.x, f0.y - t.y);
                F[k] = make_float2(f0.x + t.x, f0.y + t.y);
            }
        }
        __syncthreads();
    }

    // 3. v = re*re + im*im, then the emitted value or the raw power
    for (int idx = tid; idx < total; idx += NT) {
        const int lf = idx >> g.log2n, b = idx & (n - 1);
        const long k = k0 + lf;
        if (k >= g.frames) break;
        const float2 c = lds[idx];
        const float v = c.x * c.x + c.y * c.y;
        float* frame = out + k * n;
        if (raw) frame[b] = v;
        else store_bin(frame, n, b, o.positive_only != 0, post_value(o, v));
    }
}

// MovingAverage2D<double> / FixedAverage2D<double> over the raw powers of one feed (util/movingaverage2d.h,
// util/fixedaverage2d.h; spectrumvis.cpp:147-245).  One lane per bin walks the frames in order, as the reference does.
struct Avg {
    int mode;                      // 1 moving, 2 fixed (depth / size > 1)
    unsigned depth;                // averageNb
    unsigned idx0;                 // m_avgIndex at the start of the feed
    int frames;
};

__global__ __launch_bounds__(NT)
void spectrum_avg_kernel(const float* __restrict__ raw, double* __restrict__ data, double* __restrict__ sum,
                         float* __restrict__ out, int n, Avg a, Post o)
{
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= n) return;
    const bool used = !o.positive_only || b < n / 2;
    double acc = sum[b];
    unsigned idx = a.idx0;
    long e = 0;
    for (int f = 0; f < a.frames; f++) {
        const float v = raw[(long)f * n + b];
        if (a.mode == 1) {
            if (used) {
                double* slot = data + (long)idx * n + b;
                const double first = *slot;
                acc += ((double)v - first);
                *slot = (double)v;
                const float avg = (float)(acc / (double)a.depth);
                store_bin(out + (long)f * n, n, b, o.positive_only != 0, post_value(o, avg));
            }
            idx = idx == a.depth - 1 ? 0 : idx + 1;
        } else {
            if (used) acc += (double)v;
            if (idx == a.depth - 1) {
                if (used) {
                    // the linear branch emits the frame's own v / N^2, not the average (spectrumvis.cpp:216,229)
                    const float val = o.linear ? v / o.powdiv : o.mult * log2_as_float((float)(acc / (double)a.depth)) + o.ofs;
                    store_bin(out + e * n, n, b, o.positive_only != 0, val);
                }
                acc = 0.0;
                idx = 0;
                e++;
            } else {
                idx++;
            }
        }
    }
    sum[b] = acc;
}

// B after the feed: F frames (each followed by the shift), then the trailing partial samples at [fill_F, fill_F + rem)
__global__ __launch_bounds__(NT)
void spectrum_buf_kernel(const uint32_t* __restrict__ in, const float2* __restrict__ b0, float2* __restrict__ b1, Geom g, long consumed, int fill_f, int rem)
{
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= BUF) return;
    float2 x;
    if (g.frames == 0) {
        x = b0[p];
    } else {
        const int q = p < BUF - g.r ? p + g.r : p;
        x = frame_value(g, in, b0, g.frames - 1, q, true);
    }
    if (p >= fill_f && p < fill_f + rem) x = scaled(in[consumed + (p - fill_f)], g.scalef);
    b1[p] = x;
}

} // namespace sdrx_spec
