// UDPSrc bank, formats FormatLSB, FormatUSB, FormatLSBMono and FormatUSBMono (udpsrc.cpp:179-242): ci *= agcFactor, then
// UDPFilter->runSSB(ci, &sideband, usb) with the one fftfilt(0, 6250 / 48000, 512) every UDPSrc has, 256 payload elements per
// completed block.  These kernels run behind udp_gate_kernel (the per-sample open flags in aidx, the AGC factor in gterm)
// only when a handle has such a channel; udpsrc_ssb_sched.hpp has the index arithmetic, DESIGN.md 4.14 the kernel table.
// Float rules as in backend_kernels.hpp: reference operand order, -ffp-contract=off.
#pragma once
#include "udpsrc_kernels.hpp"
#include "gfft_kernel.hpp"

namespace sdrx {

constexpr int UDP_SSB_WAVES = 4;                            // blocks per workgroup of udp_ssb_fft_kernel, one wave each

// ci *= agcFactor: std::complex<float>::operator*=(float), the double factor narrowed once, two float products
__device__ __forceinline__ float2 udp_ssb_scaled(const UdpChan& s, const UdpBufs& b, int k)
{
    float2 v = b.ci[k];
    if (s.agc) { const float f = (float)b.gterm[k]; v.x *= f; v.y *= f; }
    return v;
}
// sample `q` of the feed as runSSB saw it (q < 0: carried from earlier feeds, already scaled)
__device__ __forceinline__ float2 udp_ssb_input(const UdpChan& s, const UdpBufs& b, int pend, int q)
{
    return q < 0 ? b.pend[pend + q] : udp_ssb_scaled(s, b, q);
}

// ---- S1. one block per wave: the 256 scaled samples zero-padded to 512, forward g_fft, runSSB's bin rule, inverse g_fft; the
// two halves go to head / tail as in be_fft_kernel.  A 512-point transform has N / 8 = 64 butterflies per pass, one wave;
// the waves of a group share the cosine table and nothing else, and all of them run every pass (gfft's barriers are the
// workgroup's), a wave without a block on zeros.
__global__ __launch_bounds__(64 * UDP_SSB_WAVES)
void udp_ssb_fft_kernel(const UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs, const float2* __restrict__ filt,
                        const float* __restrict__ utbl)
{
    constexpr int N = UDP_SSB_FLEN, H = UDP_SSB_H;
    __shared__ float2 xa[UDP_SSB_WAVES][N], ya[UDP_SSB_WAVES][N];
    __shared__ float us[N / 4 + 1];
    const int c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const UdpChan& s = ch[c];
    if (!s.ssb || (int)blockIdx.x * UDP_SSB_WAVES >= s.nb) return;
    const UdpBufs& b = bufs[c];
    const int blk = (int)blockIdx.x * UDP_SSB_WAVES + w, pend = s.s_pend;
    const bool live = blk < s.nb, usb = udp_fmt_ssb_usb(s.fmt);
    float2* x = xa[w];
    float2* y = ya[w];
    for (int i = threadIdx.x; i <= N / 4; i += 64 * UDP_SSB_WAVES) us[i] = utbl[i];
    for (int j = lane; j < H; j += 64) {
        x[j] = live ? udp_ssb_input(s, b, pend, udp_ssb_source(pend, blk, j)) : make_float2(0.0f, 0.0f);
        x[H + j] = make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    gfft<N, false>(y, x, us, lane);
    for (int i = lane; i < H; i += 64) {
        float2 lo = y[i], hi = y[H + i];
        if (i == 0) lo = c_mul(lo, filt[0]);                // data[0] * filter[0]; bin 256 is left as it is
        else if (usb) { lo = c_mul(lo, filt[i]); hi = make_float2(0.0f, 0.0f); }
        else { lo = make_float2(0.0f, 0.0f); hi = c_mul(hi, filt[H + i]); }
        x[i] = lo; x[H + i] = hi;
    }
    __syncthreads();
    gfft<N, true>(y, x, us, lane);
    if (!live) return;
    for (int i = lane; i < H; i += 64) {
        b.head[(size_t)blk * H + i] = y[i];
        b.tail[(size_t)blk * H + i] = y[H + i];
    }
}

// ---- S2. the payload.  Workgroup x writes block x (output[i] = ovlbuf[i] + data[i], all 256 elements under the squelch flag
// of the block's completing sample) and, for format 4, the raw elements of samples 256 x .. 256 x + 255.  Every lane stores
// whole dwords: a {int16, int16} element, or two int16 of a mono block.
__global__ __launch_bounds__(256)
void udp_ssb_out_kernel(const UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    constexpr int H = UDP_SSB_H;
    const int c = blockIdx.y, tid = threadIdx.x, x = blockIdx.x;
    const UdpChan& s = ch[c];
    if (!s.ssb) return;
    const UdpBufs& b = bufs[c];
    const int fmt = s.fmt, pend = s.s_pend, n = s.n;
    const float gain = s.gain;
    if (x < s.nb) {
        const bool open = b.aidx[udp_ssb_completing(pend, x)] >= 0;        // m_squelchOpen when runSSB returned the block
        const long pos = udp_ssb_block_pos(fmt, pend, x);
        auto sideband = [&](int i) {
            const float2 o = x == 0 ? b.ovl[i] : b.tail[(size_t)(x - 1) * H + i], h = b.head[(size_t)x * H + i];
            float2 r; r.x = o.x + h.x; r.y = o.y + h.y;
            return r;
        };
        if (!udp_fmt_ssb_mono(fmt)) {
            const float2 v = sideband(tid);
            const int l = open ? udp_q16d((double)(v.x * gain)) : 0, r = open ? udp_q16d((double)(v.y * gain)) : 0;
            static_cast<short2*>(b.out)[pos + tid] = make_short2((short)l, (short)r);
        } else if (tid < H / 2) {
            int q[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const float2 v = sideband(2 * tid + k);
                q[k] = open ? udp_q16d((double)(v.x + v.y) * 0.7 * (double)gain) : 0;
            }
            static_cast<short2*>(b.out)[pos / 2 + tid] = make_short2((short)q[0], (short)q[1]);
        }
    }
    if (fmt == UDP_LSB) {                                   // the unchained ladder's raw I/Q branch, on the scaled ci
        const long k = (long)x * 256 + tid;
        if (k < n) {
            const float2 v = udp_ssb_scaled(s, b, (int)k);
            int re = 0, im = 0;
            if (b.aidx[k] >= 0) { re = udp_q16f(v.x * gain); im = udp_q16f(v.y * gain); }
            static_cast<short2*>(b.out)[udp_ssb_raw_pos(pend, (int)k)] = make_short2((short)re, (short)im);
        }
    }
}

// ---- S3. carry: the samples behind the last full block, ovlbuf, inptr and the counts
__global__ __launch_bounds__(UDP_SSB_H)
void udp_ssb_carry_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    constexpr int H = UDP_SSB_H;
    const int c = blockIdx.x, i = threadIdx.x;
    UdpChan& s = ch[c];
    if (!s.ssb) return;
    const UdpBufs& b = bufs[c];
    const int n = s.n, pend = s.s_pend, nb = s.nb, n_pay = s.n_pay, left = udp_ssb_left(pend, n);
    b.pend_next[i] = i < left ? udp_ssb_input(s, b, pend, udp_ssb_carried_source(pend, n, i)) : make_float2(0.0f, 0.0f);
    b.ovl_next[i] = nb > 0 ? b.tail[(size_t)(nb - 1) * H + i] : b.ovl[i];
    __syncthreads();                                        // every lane has read s_pend
    if (i == 0) { s.s_pend = left; s.s_blocks += nb; s.total_pay += n_pay; }
}

} // namespace sdrx
