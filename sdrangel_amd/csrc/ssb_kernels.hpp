// SSB / DSB demodulator bank kernels: the tail of SSBDemod::feed (plugins/channelrx/demodssb/ssbdemod.cpp:181-250).  The
// front (NCO, Interpolator::decimate, fftfilt runSSB / runDSB) is the channel back-end's (backend_kernels.hpp); these kernels
// start from its sideband stream `s` at the audio rate, which arrives in blocks of 512 (DSB: 1024) samples.
//     m_sum += s[j]; every decim-th sample: avg, m_magsq, level sums, one spectrum Sample
//     agcVal = m_agcActive ? m_agc.feedAndGetValue(s[j]) : 10.0;  x = m_squelchDelayLine.readBack(hn);  write(s[j] * agcVal)
//     muted: {0, 0};  else z = x * m_agc.getStepValue(): mono (qint16)((z.re + z.im) * 0.7 * volume), or binaural
// Audio and spectrum are bit-identical to the strict-IEEE scalar reference build: every float and double expression keeps
// the reference's operand order and the file is compiled with -ffp-contract=off.  ssb_scan.hpp has the cut of the
// recurrences; DESIGN.md 4.13 the kernel table.  The only loop that is serial along time is psum_rows' (demod_psum.hpp): a
// load, one double add, a store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssb_scan.hpp"
#include "span_group.hpp"
#include "demod_psum.hpp"
#include "demod_wg.hpp"
#include "dsp_device.hpp"

namespace sdrx {

struct SsbChan {                        // device resident: config + carried state of one channel
    // --- config
    int hn;                             // m_agcNbSamples = m_stepDownDelay = the moving average's length; L = hn / 2
    int D;                              // ssb_delay(hn)
    int gate;                           // m_agc.setGate: (rate / 1000) * agc_threshold_gate
    int decim;                          // 1 << (span_log2 - 1)
    int agc, thr_enable, clamping;      // m_agcActive, m_thresholdEnable, m_clamping
    int mute, binaural, flip, swap_iq;  // swap_iq: !m_dsb & !m_usb, the spectrum Sample is (avgi, avgr)
    float volume;                       // m_volume / 4.0
    double threshold, step_delta;       // powerFromdB(dB) * 32768^2; 1.0 / L
    // --- state
    int g, count, U, Dn;                // m_gateCounter, m_count, m_stepUpCounter, m_stepDownCounter
    unsigned usc;                       // m_undersampleCount
    float2 open_sum;                    // m_sum of the open spectrum group
    double total;                       // MovingAverage::m_sum
    double u0;                          // m_u0
    double magsq, magsq_sum, magsq_peak;
    long long magsq_count;
    int audio_active;                   // m_audioActive
    // --- per feed
    int n, n_spec;                      // sideband samples; spectrum Samples
    double total_next;                  // written by ssb_psum_kernel, committed by ssb_carry_kernel
};

struct SsbBufs {                        // per channel device pointers (per feed capacity ensured by the host)
    const float2* s;                    // the front's sideband output of this feed
    const int* n_ptr;                   // its count (device side)
    const float* phist; float* phist_next;        // last hn powers
    const float2* whist; float2* whist_next;      // last D + 1 delay-line writes
    float* pw;                          // per sample: re * re + im * im
    double* dterm; double* tot;         // moving-average terms and sums
    float2* w;                          // per sample: what the delay line was given
    float* sv;                          // per sample: getStepValue() after it
    int16_t* audio;                     // l, r pairs, 4-byte aligned
    int16_t* spec;                      // re, im pairs of the spectrum Samples, 4-byte aligned
    double* blk_sum; double* blk_peak;  // per 256 spectrum groups
};

// ---- 1. per sample: power and the moving-average term; per closed spectrum group: average, m_magsq, the Sample; per 256
// groups the level partials.  Thread q of the channel's grid owns sample q and group q (there are never more groups than samples).
__global__ __launch_bounds__(256)
void ssb_level_kernel(SsbChan* __restrict__ ch, const SsbBufs* __restrict__ bufs)
{
    __shared__ double sums[256];
    __shared__ double peaks[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const SsbBufs b = bufs[c];
    const int n = *b.n_ptr;
    SsbChan& s = ch[c];
    const int decim = s.decim, hn = s.hn;
    const int i0 = ssb_first_close(s.usc, decim), ncl = ssb_closes(n, i0, decim);
    if (blockIdx.x == 0 && tid == 0) { s.n = n; s.n_spec = ncl; }
    const long i = (long)blockIdx.x * 256 + tid;
    if ((long)blockIdx.x * 256 >= n) return;
    if (i < n && s.agc) {
        const float2 v = b.s[i];
        const float p = v.x * v.x + v.y * v.y;
        float old = b.phist[min(i, (long)hn - 1)];
        if (i >= hn) { const float2 o = b.s[i - hn]; old = o.x * o.x + o.y * o.y; }
        b.pw[i] = p;
        b.dterm[i] = (double)p - (double)old;
    }
    double m = 0.0;
    if (i < ncl) {
        const float2 acc = span_group_sum(b.s, s.open_sum, i0, decim, (int)i);
        const float avgr = acc.x / (float)decim, avgi = acc.y / (float)decim;
        m = (double)(avgr * avgr + avgi * avgi) / (32768.0 * 32768.0);
        const int re = sdrx_to_q16(s.swap_iq ? avgi : avgr), im = sdrx_to_q16(s.swap_iq ? avgr : avgi);
        reinterpret_cast<short2*>(b.spec)[i] = make_short2((short)re, (short)im);
        if (i == ncl - 1) s.magsq = m;
    }
    wg_level_reduce(sums, peaks, tid, m, m);
    if (tid == 0) { b.blk_sum[blockIdx.x] = sums[0]; b.blk_peak[blockIdx.x] = peaks[0]; }
}

// ---- 2. the moving-average sum after every sample: one wave per 16 channels (psum_rows); channels with the AGC off have no terms
__global__ __launch_bounds__(64)
void ssb_psum_kernel(SsbChan* __restrict__ ch, const SsbBufs* __restrict__ bufs, int n_ch)
{
    psum_channels(n_ch, [&](int c) { return PsumRow{bufs[c].dterm, bufs[c].tot, ch[c].agc ? ch[c].n : 0, ch[c].total, &ch[c].total_next}; });
}

// ---- 3. one workgroup per channel, 1024 samples per trip, four consecutive samples per lane: the gate counter, m_count and the
// step pair (magagc_trip, ssb_scan.hpp), m_u0, the factor, the delay-line write and getStepValue() per sample; then the level
// accumulators
__global__ __launch_bounds__(256)
void ssb_gate_kernel(SsbChan* __restrict__ ch, const SsbBufs* __restrict__ bufs)
{
    __shared__ MagAgcSlots slots;
    __shared__ double sums[256];
    __shared__ double peaks[256];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SsbChan& s = ch[c];
    const SsbBufs b = bufs[c];
    const int n = s.n, hn = s.hn, L = hn / 2, gate = s.gate;
    const double thr = s.threshold, sd = s.step_delta;
    const bool clamping = s.clamping != 0;
    SsbCounters st; st.g = s.g; st.count = s.count; st.ud.U = s.U; st.ud.D = s.Dn;
    if (!s.agc || !s.thr_enable) {
        // no counter moves: agcVal is 10.0 or m_u0, getStepValue() is what the carried pair gives
        const float svc = ssb_step_value(ssb_up(st.count, hn), st.ud, sd);
        for (int i = tid; i < n; i += 256) {
            const float2 v = b.s[i];
            float a = 10.0f;
            if (s.agc) {
                const double u0 = ssb_u0((double)b.pw[i], b.tot[i], hn, clamping);
                a = (float)u0;
                if (i == n - 1) s.u0 = u0;
            }
            b.w[i] = make_float2(v.x * a, v.y * a);
            b.sv[i] = svc;
        }
    } else {
        for (int base = 0; base < n; base += 1024)
            magagc_trip(st, slots, base + tid * 4, n, lane, w, gate, hn, L, thr,
                [&](int i) { return (double)b.pw[i]; },
                [&](int i, bool up, SsbUD was, SsbUD ud, double magsq) {
                    const double u0 = ssb_u0(magsq, b.tot[i], hn, clamping);
                    const float a = (float)ssb_agc_value(up, was, ud, L, sd, u0);
                    const float2 v = b.s[i];
                    b.w[i] = make_float2(v.x * a, v.y * a);
                    b.sv[i] = ssb_step_value(up, ud, sd);
                    if (i == n - 1) s.u0 = u0;
                });
    }
    // level accumulators: the 256-group partials of ssb_level_kernel, in a fixed order
    const int ncl = s.n_spec;
    wg_level_gather(sums, peaks, tid, (ncl + 255) / 256, b.blk_sum, b.blk_peak);
    if (tid == 0) {
        s.g = st.g; s.count = st.count; s.U = st.ud.U; s.Dn = st.ud.D;
        if (ncl > 0) {
            s.magsq_sum += sums[0];
            if (peaks[0] > s.magsq_peak) s.magsq_peak = peaks[0];
            s.magsq_count += ncl;
        }
    }
}

// what the delay line holds for stream index j of this feed (j < 0: the carried history of D + 1 writes)
__device__ __forceinline__ float2 ssb_w_at(const SsbBufs& b, int D, long j) { return am_stream_at(b.whist, D + 1, (const float2*)b.w, j); }

// ---- 4. per sample: the delayed sample times the step value, volume, conversion to the l, r pair
__global__ __launch_bounds__(256)
void ssb_out_kernel(SsbChan* __restrict__ ch, const SsbBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    SsbChan& s = ch[c];
    const int n = s.n;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SsbBufs& b = bufs[c];
    const float2 x = ssb_w_at(b, s.D, i - 1 - s.D);
    if (i == n - 1) s.audio_active = x.x != 0.0f ? 1 : 0;
    int l = 0, r = 0;
    if (!s.mute) {
        const float sv = b.sv[i], vol = s.volume;
        const float zr = x.x * sv, zi = x.y * sv;
        if (s.binaural) {
            const int a = sdrx_to_q16(zr * vol), q = sdrx_to_q16(zi * vol);
            if (s.flip) { r = q; l = a; } else { r = a; l = q; }
        } else {
            const float demod = (float)((double)(zr + zi) * 0.7);
            l = r = sdrx_to_q16(demod * vol);
        }
    }
    reinterpret_cast<short2*>(b.audio)[i] = make_short2((short)l, (short)r);
}

// ---- 5. carry: the histories of the next feed (double-buffered: this feed's are still being read), the moving-average sum,
// the spectrum counter and the open group's partial sum
__global__ __launch_bounds__(256)
void ssb_carry_kernel(SsbChan* __restrict__ ch, const SsbBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    SsbChan& s = ch[c];
    const SsbBufs b = bufs[c];
    const int n = s.n, K = s.D + 1;
    if (s.agc) for (int i = tid; i < s.hn; i += 256) b.phist_next[i] = am_hist_next(b.phist, s.hn, (const float*)b.pw, n, i);
    for (int i = tid; i < K; i += 256) b.whist_next[i] = am_hist_next(b.whist, K, (const float2*)b.w, n, i);
    if (tid == 0) {
        s.total = s.total_next;
        s.open_sum = span_open_sum(b.s, s.open_sum, ssb_first_close(s.usc, s.decim), s.decim, s.n_spec, n);
        s.usc += (unsigned)n;
    }
}

} // namespace sdrx
