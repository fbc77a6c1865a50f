// ChannelAnalyzer bank kernels: what ChannelAnalyzer::processOneSample and feedOneSample do with the filter's output
// (plugins/channelrx/chanalyzer/chanalyzer.cpp:128-182, chanalyzer.h:250-287; what m_pll, m_fll and InputPLL add is chana_pll_kernels.hpp's).  The front (NCOF, the optional
// Interpolator, fftfilt runSSB / runDSB / runFilt) is the channel back-end's (backend_kernels.hpp); these kernels start from
// its stream `s`, which arrives in blocks of 512 (SSB) or 1024 samples.
//     m_sum += s[j];  every (1 << span_log2)-th sample: m_sum /= decim, m_magsq, feedOneSample(m_sum), m_sum = 0
//     InputSignal:    Sample(re, im), or (im, re) for m_ssb & !m_usb
//     InputAutoCorr:  a = m_corr->run(m_sum / (SDR_RX_SCALEF / 768.0f), 0), fftcorr(8192) (sdrbase/dsp/fftcorr.cpp): call t
//                     returns P_b[t mod 4096], b = t / 4096, P_0 = 0, P_b = InverseComplexFFT(A .* conj(A)) with A the
//                     ComplexFFT of the b-th run of 4096 inputs padded with zeros to 8192
// Bit-identical to the strict-IEEE scalar reference build: reference operand order, -ffp-contract=off.  Nothing here is serial
// along time: groups are independent (span_group.hpp), a completed block of 4096 inputs is one workgroup's work, and output t
// only has to know which block it reads.  DESIGN.md 4.16 has the kernel table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "span_group.hpp"
#include "gfft_kernel.hpp"
#include "dsp_device.hpp"
#include "pll_math.hpp"

namespace sdrx {

constexpr int CHANA_CORR_N = 8192;                      // m_corr = new fftcorr(8 * ssbFftLen)
constexpr int CHANA_CORR_H = CHANA_CORR_N / 2;          // inputs per block = lags kept
constexpr int CHANA_CORR_LDS = 2 * CHANA_CORR_N * (int)sizeof(float2) + (CHANA_CORR_N / 4 + 1) * (int)sizeof(float);

struct ChanaChan {                      // device resident: config + carried state of one channel
    // --- config
    int decim;                          // 1 << span_log2
    int swap_iq;                        // m_ssb & !m_usb: the Sample is (im, re)
    int corr;                           // input_type == InputAutoCorr
    int osc_out;                        // input_type == InputPLL: the Sample is the oscillator
    PllCfg pk;                          // m_pll / m_fll, m_pllPskOrder and what the configuration sequence left in both loops
    // --- state
    unsigned usc;                       // m_undersampleCount; only its low bits matter
    float2 open_sum;                    // m_sum of the open group
    double magsq;                       // m_magsq
    int fill;                           // fftcorr: calls so far modulo 4096 = inputs waiting in the open block
    PllState ps;                        // PhaseLockComplex and FreqLockComplex
    // --- per feed
    int n, n_out;                       // filtered samples; Samples
};

struct ChanaBufs {                      // per channel device pointers (per feed capacity ensured by the host)
    const float2* s;                    // the front's filtered output of this feed
    const int* n_ptr;                   // its count (device side)
    const float2* part; float2* part_next;      // fftcorr: the open block's inputs (4096 slots)
    const float2* p; float2* p_next;            // fftcorr: lags 0 .. 4095 of the last completed block's product
    int16_t* out;                       // re, im pairs of this feed's Samples, 4-byte aligned
    float2* g;                          // fftcorr: this feed's inputs, one per closed group
    float2* pblk;                       // fftcorr: lags 0 .. 4095 of every block this feed completed
    float2* avg;                        // PLL / FLL / InputPLL: m_sum of every closed group, for the stages behind the group kernel
    float2* osc;                        // PLL / FLL: the oscillator (cos, sin) of every step
};

// the channel's Samples come from chana_post_kernel (chana_pll_kernels.hpp), not from the group kernel
__device__ __forceinline__ bool chana_has_post(const ChanaChan& s) { return s.pk.mode != PLL_OFF || s.osc_out; }

// input number idx of fftcorr counted from the start of the block that was open when the feed began
__device__ __forceinline__ float2 chana_corr_in(const ChanaBufs& b, int fill, long idx) { return idx < fill ? b.part[idx] : b.g[idx - fill]; }

// ---- 1. per closed group: the average, m_magsq, and either the Sample or fftcorr's input.  Thread q of the channel's grid
// owns group q (there are never more groups than samples).
__global__ __launch_bounds__(256)
void chana_group_kernel(ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs)
{
    const int c = blockIdx.y, tid = threadIdx.x;
    const ChanaBufs b = bufs[c];
    const int n = *b.n_ptr;
    ChanaChan& s = ch[c];
    const int decim = s.decim;
    const int i0 = ssb_first_close(s.usc, decim), ncl = ssb_closes(n, i0, decim);
    if (blockIdx.x == 0 && tid == 0) { s.n = n; s.n_out = ncl; }
    const long i = (long)blockIdx.x * 256 + tid;
    if (i >= ncl) return;
    const float2 acc = span_group_sum(b.s, s.open_sum, i0, decim, (int)i);
    const float avgr = acc.x / (float)decim, avgi = acc.y / (float)decim;         // m_sum /= decim
    const float re = avgr / 32768.0f, im = avgi / 32768.0f;                       // SDR_RX_SCALEF
    if (i == ncl - 1) s.magsq = (double)(re * re + im * im);
    if (chana_has_post(s)) { b.avg[i] = make_float2(avgr, avgi); return; }
    if (s.corr) {
        const float k = 32768.0f / 768.0f;                                        // s / (SDR_RX_SCALEF / 768.0f)
        b.g[i] = make_float2(avgr / k, avgi / k);
    } else {
        const int o_re = sdrx_to_q16(s.swap_iq ? avgi : avgr), o_im = sdrx_to_q16(s.swap_iq ? avgr : avgi);
        reinterpret_cast<short2*>(b.out)[i] = make_short2((short)o_re, (short)o_im);
    }
}

// ---- 2. fftcorr::run's transform, one workgroup per (block completed in this feed, channel): the block's 4096 inputs padded
// with zeros, the forward g_fft, a * conj(a) in std::complex<float>'s operand order, the inverse g_fft, lags 0 .. 4095 out
// (the others are never read: outptr goes back to 0 every 4096 calls).  Two 64 KB arrays and the quarter-wave cosine table
// in LDS; 1024 threads, one radix-8 butterfly each per pass.
__global__ __launch_bounds__(CHANA_CORR_N / 8)
void chana_corr_kernel(const ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs, const float* __restrict__ utbl)
{
    constexpr int N = CHANA_CORR_N, H = CHANA_CORR_H, NT = N / 8;
    __shared__ float2 xa[N], ya[N];
    __shared__ float us[N / 4 + 1];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const ChanaChan& s = ch[c];
    if (!s.corr) return;
    const int fill = s.fill;
    if (blk >= (fill + s.n_out) / H) return;
    const ChanaBufs b = bufs[c];
    for (int i = tid; i <= N / 4; i += NT) us[i] = utbl[i];
    for (int i = tid; i < H; i += NT) { xa[i] = chana_corr_in(b, fill, (long)blk * H + i); xa[H + i] = make_float2(0.0f, 0.0f); }
    __syncthreads();
    gfft<N, false>(ya, xa, us, tid);
    for (int i = tid; i < N; i += NT) { const float2 a = ya[i]; xa[i] = c_mul(a, make_float2(a.x, -a.y)); }
    __syncthreads();
    gfft<N, true>(ya, xa, us, tid);
    for (int i = tid; i < H; i += NT) b.pblk[(long)blk * H + i] = ya[i];
}

// ---- 3. fftcorr's outputs: call q of the feed (counted from the start of the open block, the first being fill + 1) returns
// entry q mod 4096 of the product of the last block completed by then
__global__ __launch_bounds__(256)
void chana_emit_kernel(const ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const ChanaChan& s = ch[c];
    if (!s.corr) return;
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= s.n_out) return;
    const ChanaBufs& b = bufs[c];
    const long q = (long)s.fill + o + 1;
    const long rel = q / CHANA_CORR_H; const int pos = (int)(q % CHANA_CORR_H);
    const float2 a = rel == 0 ? b.p[pos] : b.pblk[(rel - 1) * CHANA_CORR_H + pos];
    const int o_re = sdrx_to_q16(s.swap_iq ? a.y : a.x), o_im = sdrx_to_q16(s.swap_iq ? a.x : a.y);
    reinterpret_cast<short2*>(b.out)[o] = make_short2((short)o_re, (short)o_im);
}

// ---- 4. carry: the counter and the open group's partial sum; fftcorr's open block and last product into the next feed's set
// (double-buffered: this feed's are still being read)
__global__ __launch_bounds__(256)
void chana_carry_kernel(ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    ChanaChan& s = ch[c];
    const ChanaBufs b = bufs[c];
    const int n = s.n, ncl = s.n_out, fill = s.fill;
    const int nb = (fill + ncl) / CHANA_CORR_H, left = (fill + ncl) % CHANA_CORR_H;
    if (s.corr) {
        for (int i = tid; i < CHANA_CORR_H; i += 256) {
            b.p_next[i] = nb > 0 ? b.pblk[(long)(nb - 1) * CHANA_CORR_H + i] : b.p[i];
            if (i < left) b.part_next[i] = chana_corr_in(b, fill, (long)nb * CHANA_CORR_H + i);
        }
    }
    __syncthreads();                                        // every thread has read s.fill
    if (tid == 0) {
        s.open_sum = span_open_sum(b.s, s.open_sum, ssb_first_close(s.usc, s.decim), s.decim, ncl, n);
        s.usc += (unsigned)n;
        if (s.corr) s.fill = left;
    }
}

} // namespace sdrx
