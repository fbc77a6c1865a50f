// g_fft (sdrbase/dsp/gfft.h) on a block held in LDS, the filter-design kernel built on it and the discriminator's
// atan2 approximation: shared by the channel back-end (backend_kernels.hpp) and the WFM demodulator (wfm_kernels.hpp).
// Float path rules as in backend_kernels.hpp: reference operand order, -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrx {

// ---- g_fft network on a 1024-point block held in LDS.
// John Green's FFT as the reference runs it for N = 1024 (gfft.h: ffts1 :1189-1224, iffts1 :2238-2275):
// bit-reversed load fused with one radix-2 stage (bitrevR2 :185-317; scbitrevR2 :1231-1363 scales by 1/N),
// then three radix-8 passes (bfstages :843-1158 / ibfstages :1889-2209) with D = 2, 16, 128.  The reference's
// in-place index choreography does not change values; the arithmetic FORMS do.  With multiplier m = (mr, mi):
//     PLUS (a,b,m): r = (a.r + b.r*mr) - b.i*mi ;  i = (a.i + b.r*mi) + b.i*mr      (= a + b*m)
//     MINUS(a,b,m): r = (a.r - b.r*mr) + b.i*mi ;  i = (a.i - b.r*mi) - b.i*mr      (= a - b*m)
//     and the partner of every butterfly is formed as 2*a - result.
// Forward multipliers are conj(w), i*conj(w); inverse ones their conjugates (IEEE negation is exact, so a
// sign flip of mi reproduces the reference's explicit +/- variants bit for bit).  Twiddles come from the
// quarter-wave float cosine table of fftCosInit (:141-150); w0 crosses pi/2 at u = D/2 and is mirrored.
__device__ __forceinline__ float2 c_plus(float2 a, float2 b, float mr, float mi)  { float2 t; t.x = (a.x + b.x * mr) - b.y * mi; t.y = (a.y + b.x * mi) + b.y * mr; return t; }
__device__ __forceinline__ float2 c_minus(float2 a, float2 b, float mr, float mi) { float2 t; t.x = (a.x - b.x * mr) + b.y * mi; t.y = (a.y - b.x * mi) - b.y * mr; return t; }
__device__ __forceinline__ float2 c_two_minus(float2 a, float2 t)                 { float2 f; f.x = a.x * 2.0f - t.x; f.y = a.y * 2.0f - t.y; return f; }
__device__ __forceinline__ float2 c_mul(float2 a, float2 b) { float2 t; t.x = a.x * b.x - a.y * b.y; t.y = a.x * b.y + a.y * b.x; return t; }

// y: LDS work array (N float2); x: LDS input copy (N float2); u: cosine table (N/4+1 floats); N/8 threads.
// N = 1024: stage list R2(bitrev) + 3 x radix-8 (D = 2, 16, 128);  N = 2048: R2(bitrev) + bfR2 (:531-635 /
// ibfR2 :1577-1681: twiddles 1 and -/+i) + 3 x radix-8 (D = 4, 32, 256);  N = 512: R2(bitrev) + bfR4 (:637-841 / ibfR4
// :1683-1887, NDiffU = 2: per 8 points the even ones take twiddles 1 and -/+i, the odd ones -/+i and w1 = cos(pi/4) in the
// `a - b*w1 ...; partner = 2*a - result` form) + 2 x radix-8 (D = 8, 64);  N = 8192 (fftcorr): R2(bitrev) + 4 x radix-8
// (D = 2, 16, 128, 1024), the stages ffts1 reaches through fftrecurs (:1161-1177), whose blocking reorders the passes of
// separate sub-transforms and no arithmetic.  inverse: first stage scaled by 1/N, multipliers conjugated.
template<int N, bool INVERSE>
__device__ __forceinline__ void gfft(float2* __restrict__ y, const float2* __restrict__ x, const float* __restrict__ u, int tid)
{
    constexpr int NT = N / 8;
    constexpr int M = N == 512 ? 9 : (N == 1024 ? 10 : (N == 2048 ? 11 : 13));
    static_assert(N == 512 || N == 1024 || N == 2048 || N == 8192, "fftfilt lengths of the demods and of UDPSrc; fftcorr's 8192");
    const float scale = (float)(1.0 / N);
    for (int j = tid; j < N / 2; j += NT) {
        const unsigned r = __brev((unsigned)(2 * j)) >> (32 - M);
        const float2 a = x[r], b = x[r + N / 2];
        float2 s, d; s.x = a.x + b.x; s.y = a.y + b.y; d.x = a.x - b.x; d.y = a.y - b.y;
        if (INVERSE) { s.x = scale * s.x; s.y = scale * s.y; d.x = scale * d.x; d.y = scale * d.y; }
        y[2 * j] = s; y[2 * j + 1] = d;
    }
    __syncthreads();
    constexpr int D0 = N == 512 ? 8 : (N == 2048 ? 4 : 2);
    if constexpr (N == 2048) {
        for (int k = 4 * tid; k < N; k += 4 * NT) {
            const float2 a = y[k], b = y[k + 2], c = y[k + 1], d = y[k + 3];
            float2 t;
            t.x = a.x + b.x; t.y = a.y + b.y; y[k] = t;
            t.x = a.x - b.x; t.y = a.y - b.y; y[k + 2] = t;
            if (!INVERSE) { t.x = c.x + d.y; t.y = c.y - d.x; y[k + 1] = t; t.x = c.x - d.y; t.y = c.y + d.x; y[k + 3] = t; }
            else          { t.x = c.x - d.y; t.y = c.y + d.x; y[k + 1] = t; t.x = c.x + d.y; t.y = c.y - d.x; y[k + 3] = t; }
        }
        __syncthreads();
    }
    if constexpr (N == 512) {
        const float w1 = (float)(1.0 / 1.414213562373095048801688724209698078569);       // FFT_TYPE w1r = 1.0 / FFT_ROOT2
        for (int k = 8 * tid; k < N; k += 8 * NT) {
            // even points: twiddles 1, then 1 and -/+i
            const float2 a0 = y[k], a1 = y[k + 2], a2 = y[k + 4], a3 = y[k + 6];
            float2 e5, e0, e6, e3, t;
            e5.x = a0.x - a1.x; e5.y = a0.y - a1.y; e0.x = a0.x + a1.x; e0.y = a0.y + a1.y;
            e6.x = a2.x + a3.x; e6.y = a2.y + a3.y; e3.x = a2.x - a3.x; e3.y = a2.y - a3.y;
            t.x = e0.x + e6.x; t.y = e0.y + e6.y; y[k] = t;
            t.x = e0.x - e6.x; t.y = e0.y - e6.y; y[k + 4] = t;
            if (!INVERSE) { t.x = e5.x + e3.y; t.y = e5.y - e3.x; y[k + 2] = t; t.x = e5.x - e3.y; t.y = e5.y + e3.x; y[k + 6] = t; }
            else          { t.x = e5.x - e3.y; t.y = e5.y + e3.x; y[k + 2] = t; t.x = e5.x + e3.y; t.y = e5.y - e3.x; y[k + 6] = t; }
            // odd points: twiddles -/+i, then w1 and i*w1
            const float2 b0 = y[k + 1], b1 = y[k + 3], b2 = y[k + 5], b3 = y[k + 7];
            float2 o7, o2, o4, t1, o5, o6;
            if (!INVERSE) {
                o7.x = b2.x - b3.y; o7.y = b2.y + b3.x; o2.x = b2.x + b3.y; o2.y = b2.y - b3.x;
                o4.x = b0.x + b1.y; o4.y = b0.y - b1.x; t1.x = b0.x - b1.y; t1.y = b0.y + b1.x;
                o5.x = t1.x - o7.x * w1 + o7.y * w1; o5.y = t1.y - o7.x * w1 - o7.y * w1;
                o6.x = o4.x - o2.x * w1 - o2.y * w1; o6.y = o4.y + o2.x * w1 - o2.y * w1;
            } else {
                o7.x = b2.x + b3.y; o7.y = b2.y - b3.x; o2.x = b2.x - b3.y; o2.y = b2.y + b3.x;
                o4.x = b0.x - b1.y; o4.y = b0.y + b1.x; t1.x = b0.x + b1.y; t1.y = b0.y - b1.x;
                o5.x = t1.x - o7.x * w1 - o7.y * w1; o5.y = t1.y + o7.x * w1 - o7.y * w1;
                o6.x = o4.x - o2.x * w1 + o2.y * w1; o6.y = o4.y - o2.x * w1 - o2.y * w1;
            }
            y[k + 3] = o5; y[k + 7] = c_two_minus(t1, o5);
            y[k + 5] = o6; y[k + 1] = c_two_minus(o4, o6);
        }
        __syncthreads();
    }
    const float sg = INVERSE ? 1.0f : -1.0f;
#pragma unroll
    for (int D = D0; D < N; D *= 8) {
        const int uinc = N / 8 / D;
        const int uu = tid % D, g = tid / D;                           // N/8 butterflies per pass
        const int i2 = uu * uinc, i1 = 2 * i2;
        int i0 = 4 * i2; float w0r;
        if (uu < D / 2) w0r = u[i0]; else { i0 = N / 2 - i0; w0r = -u[i0]; }
        const float w0i = u[N / 4 - i0];
        const float w1r = u[i1], w1i = u[N / 4 - i1];
        const float w2r = u[i2], w2i = u[N / 4 - i2];
        const float w3r = u[i2 + N / 8], w3i = u[N / 4 - i2 - N / 8];
        float2* p = y + g * 8 * D + uu;
        float2 f0 = p[0], f1 = p[D], f2 = p[2 * D], f3 = p[3 * D], f4 = p[4 * D], f5 = p[5 * D], f6 = p[6 * D], f7 = p[7 * D];
        float2 t0, t1;
        t0 = c_plus(f0, f1, w0r, sg * w0i);  f1 = c_two_minus(f0, t0);
        t1 = c_minus(f2, f3, w0r, sg * w0i); f2 = c_two_minus(f2, t1);
        f0 = c_plus(t0, f2, w1r, sg * w1i);  f2 = c_two_minus(t0, f0);
        f3 = c_plus(f1, t1, w1i, -sg * w1r); f1 = c_two_minus(f1, f3);
        t0 = c_plus(f4, f5, w0r, sg * w0i);  f5 = c_two_minus(f4, t0);
        t1 = c_minus(f6, f7, w0r, sg * w0i); f6 = c_two_minus(f6, t1);
        f4 = c_plus(t0, f6, w1r, sg * w1i);  f6 = c_two_minus(t0, f4);
        f7 = c_plus(f5, t1, w1i, -sg * w1r); f5 = c_two_minus(f5, f7);
        t0 = c_minus(f0, f4, w2r, sg * w2i); f0 = c_two_minus(f0, t0);
        t1 = c_minus(f1, f5, w3r, sg * w3i); f1 = c_two_minus(f1, t1);
        const float2 n4 = c_minus(f2, f6, w2i, -sg * w2r); f6 = c_two_minus(f2, n4);
        const float2 n5 = c_minus(f3, f7, w3i, -sg * w3r); f7 = c_two_minus(f3, n5);
        p[0] = f0; p[D] = f1; p[2 * D] = n4; p[3 * D] = n5; p[4 * D] = t0; p[5 * D] = t1; p[6 * D] = f6; p[7 * D] = f7;
        __syncthreads();
    }
}

// phasediscri.h:172-197
__device__ __forceinline__ float atan2_approx2(float y, float x)
{
    const float PI_F = 3.14159265f, PIBY2_F = 1.5707963f;
    if (x == 0.0f) { if (y > 0.0f) return PIBY2_F; if (y == 0.0f) return 0.0f; return -PIBY2_F; }
    float at;
    const float z = y / x;
    if (fabsf(z) < 1.0f) {
        at = z / (1.0f + 0.28f * z * z);
        if (x < 0.0f) { if (y < 0.0f) return at - PI_F; return at + PI_F; }
    } else {
        at = PIBY2_F - z / (z * z + 0.28f);
        if (y < 0.0f) return at - PI_F;
    }
    return at;
}

// single forward FFT of one block (filter design: fft->ComplexFFT(filter), fftfilt.cpp:131,158)
template<int N>
__global__ __launch_bounds__(N / 8)
void be_fft_design_kernel(float2* __restrict__ data, const float* __restrict__ utbl)
{
    constexpr int NT = N / 8;
    __shared__ float2 xa[N], ya[N];
    __shared__ float us[N / 4 + 1];
    const int tid = threadIdx.x;
    for (int i = tid; i <= N / 4; i += NT) us[i] = utbl[i];
    for (int i = tid; i < N; i += NT) xa[i] = data[i];
    __syncthreads();
    gfft<N, false>(ya, xa, us, tid);
    for (int i = tid; i < N; i += NT) data[i] = ya[i];
}

} // namespace sdrx
