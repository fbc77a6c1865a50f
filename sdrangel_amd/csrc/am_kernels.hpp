// AM demodulator bank kernels: the tail of AMDemod::feed, AMDemod::processOneSample in envelope mode
// (plugins/channelrx/demodam/amdemod.cpp:152-276).  The front (NCO, Interpolator::decimate) is the channel back-end's
// (backend_kernels.hpp); these kernels start from its complex resampler output `ci` at the audio rate.
//     magsq = re*re + im*im;  m_movingAverage(magsq);  level sums;  m_squelchDelayLine.write(magsq);  squelch counter
//     open: demod = sqrt(readBack(rate / 20)); m_volumeAGC.feed(demod); demod = (demod - agc) / agc;
//           [m_bandpass.filter(demod) / 301.0f];  attack;  (qint16)(demod * smootherstep(attack) * (rate / 24) * volume)
// Audio is bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  am_scan.hpp has the cut of the recurrences; DESIGN.md 4.10 the
// kernel table.  The only loops that are serial along time are am_psum_kernel's: loads, one double add per sample, stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "am_scan.hpp"
#include "am_sync_scan.hpp"
#include "demod_psum.hpp"
#include "demod_wg.hpp"
#include "dsp_device.hpp"

namespace sdrx {

struct AmChan {                         // device resident: config + carried state of one channel
    // --- config
    int rate;                           // m_audioSampleRate
    int D, H;                           // rate / 20: readBack delay and opening count; rate / 10: counter cap and AGC length
    float level;                        // m_squelchLevel = (Real) pow(10.0, squelch / 10.0)
    float volume;
    float att;                          // 0.05f * rate
    float gain;                         // (float)(rate / 24)
    int mute, bandpass;
    int bp_off;                         // float offset into the Bandpass tap table (151 per channel)
    // --- state
    int count, sq_open;                 // m_squelchCount, m_squelchOpen
    double total;                       // MovingAverageUtil::m_total
    double agc_sum;                     // MovingAverage<double>::m_sum of m_volumeAGC
    double magsq;                       // m_magsq
    double magsq_sum, magsq_peak;
    long long magsq_count;
    // --- per feed
    int n, n_act, n_fed;                // audio samples; open and unmuted ones; AGC feeds
    double total_next, agc_sum_next;    // written by am_psum_kernel, committed by am_carry_kernel
    // --- synchronous AM (am_sync_kernels.hpp), behind everything the envelope kernels read
    int sync;                           // AMS_OFF: envelope; AMS_DSB / AMS_USB / AMS_LSB: m_pll with that m_syncAMOperation
    int s_B, s_hn;                      // filter block (flen / 2); m_syncAMAGC's history, rate / 4
    int pf_off;                         // float offset of the 51 folded m_pllFilt taps in the tap table
    int filt_off;                       // float2 offset of the channel's frequency-domain filter
    PllCfg pk;                          // m_pll's configuration
    PllState ps;                        // ... and state
    int s_pend;                         // open samples in the filter's open block (fftfilt::inptr)
    long long s_open;                   // open samples since creation
    double s_total;                     // m_syncAMAGC's MovingAverage::m_sum
    int s_nb;                           // per feed: blocks the filter completed
    double s_total_next;                // written by am_sync_psum_kernel, committed by am_sync_carry_kernel
};

struct AmBufs {                         // per channel device pointers (per feed capacity ensured by the host)
    const float2* ci;                   // the front's output of this feed
    const int* n_ptr;                   // its count (device side)
    const float* mhist; float* mhist_next;       // last 16 magsq
    const float* rhist; float* rhist_next;       // last D roots
    const double* vhist; double* vhist_next;     // last H fed values
    const float* dhist; float* dhist_next;       // last 300 open demods
    float* msq; float* root;            // per sample
    double* dterm; double* tot;         // moving-average terms and totals
    int* cnt; int* aidx; int* fcnt;     // counter after the sample; index in the open sequence (-1: closed); fed count through it
    double* vnew; double* uterm; double* agc;    // per fed sample: value, AGC term, AGC sum after it
    float* dem;                         // per open sample: (r - g) / g
    int16_t* audio;
    double* blk_sum; float* blk_peak;   // per 256 samples
    // --- synchronous AM: carried (null in an envelope channel) ...
    const float2* xhist; float2* xhist_next;     // last 100 open (re, im): m_pllFilt's ring
    const float2* pend; float2* pend_next;       // the open block's inputs so far
    const float2* ovl; float2* ovl_next;         // fftfilt::ovlbuf
    const float* phist; float* phist_next;       // last s_hn magsq of the filter's outputs
    const float* zhist; float* zhist_next;       // last s_B zsum: what m_syncAMBuff still holds
    // ... and per feed
    float2* xc; float2* pf; float2* osc;         // per open sample: (re, im), m_pllFilt's output, (m_yRe, m_yIm) after feed()
    float2* head; float2* tail;                  // per filter output: the two halves of its block's inverse transform
    float* pw; double* sterm; double* stot;      // per filter output: magsq, moving-average term and sum
};

// ---- 1. per sample: magsq, its root, the moving-average term; per 256 samples the level partials
__global__ __launch_bounds__(256)
void am_level_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const AmBufs b = bufs[c];
    const int n = *b.n_ptr;
    if (blockIdx.x == 0 && tid == 0) ch[c].n = n;
    const long i = (long)blockIdx.x * 256 + tid;
    if ((long)blockIdx.x * 256 >= n) return;
    auto power = [&](long j) -> float {
        const float2 v = b.ci[j];
        const float re = v.x / 32768.0f, im = v.y / 32768.0f;      // SDR_RX_SCALEF
        return re * re + im * im;
    };
    float m = 0.0f;
    if (i < n) {
        m = power(i);
        const float old = i >= AM_MA ? power(i - AM_MA) : b.mhist[i];
        b.msq[i] = m;
        b.root[i] = sqrtf(m);                           // the correctly rounded expansion (IEEE sqrt is the build default)
        b.dterm[i] = am_ma_term(m, old);
    }
    wg_level_reduce(sums, peaks, tid, (double)m, m);
    if (tid == 0) { b.blk_sum[blockIdx.x] = sums[0]; b.blk_peak[blockIdx.x] = peaks[0]; }
}

// ---- 2. rounded prefix sum along time: acc += term.  which = 0: moving-average total; 1: AGC sum over the fed samples.
// One wave per 16 channels, 64 terms per channel and trip: psum_rows (demod_psum.hpp).
constexpr int AM_PS_CH = PS_CH;
__global__ __launch_bounds__(64)
void am_psum_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, int n_ch, int which)
{
    // psum_rows called directly, not through psum_channels as in the other families: with the wrapper this kernel ran 3 % longer
    // (2.13 against 2.07 ms per launch) and the AM feed 1.8 % over the parent's slowest run, though its loop kept its instructions (experiments/README.md)
    const int lane = threadIdx.x, c = blockIdx.x * AM_PS_CH + lane;
    const bool chain = lane < AM_PS_CH && c < n_ch;
    const double acc = psum_rows(lane, chain, [&](const double*& term, double*& out, int& n_mine, double& sum) {
        const int cc = min(c, n_ch - 1);                    // rows past the last channel: its pointers, no terms
        const AmChan& s = ch[cc];
        const AmBufs& b = bufs[cc];
        term = which ? b.uterm : b.dterm;
        out = which ? b.agc : b.tot;
        if (chain) { n_mine = which ? s.n_fed : s.n; sum = which ? s.agc_sum : s.total; }
    });
    if (chain) { if (which) ch[c].agc_sum_next = acc; else ch[c].total_next = acc; }
}

// ---- 3. one workgroup per channel, 1024 samples per trip: the squelch counter as a scan of clamp maps, open and fed
// flags, their prefix counts (the compaction indices), the fed values, then the AGC terms; level accumulators
__global__ __launch_bounds__(256)
void am_gate_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    __shared__ WfmClamp wmap[4];
    __shared__ int2 wcnt[4];                                // open, fed
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    AmChan& s = ch[c];
    const AmBufs b = bufs[c];
    const int n = s.n, cap = s.H, D = s.D, rate = s.rate;
    const float level = s.level;
    const bool mute = s.mute != 0;
    const WfmClampOps sq{cap};
    int carry = s.count, nact = 0, nfed = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i0 = base + tid * 4;
        bool up[4];
        WfmClamp m = sq.identity();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            up[k] = false;
            if (i0 + k < n) { up[k] = am_up(b.tot[i0 + k], level); m = wfm_compose(m, wfm_step(up[k], cap)); }
        }
        int st = wfm_apply(wg_scan(sq, m, lane, w, wmap), carry);
        int stv[4]; bool act[4], fed[4]; float rr[4];
        int a_loc = 0, f_loc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            act[k] = fed[k] = false; stv[k] = st; rr[k] = 0.0f;
            if (i0 + k < n) {
                st = wfm_apply(wfm_step(up[k], cap), st);
                stv[k] = st;
                const bool open = am_open(st, rate);
                act[k] = open && !mute;
                rr[k] = am_stream_at(b.rhist, D, b.root, (long)(i0 + k) - D);
                fed[k] = am_fed(open, mute, rr[k]);
                a_loc += act[k]; f_loc += fed[k];
            }
        }
        const int2 incl = wg_scan_incl(WgCount2{}, make_int2(a_loc, f_loc), lane, w, wcnt);
        int a_ex = nact + incl.x - a_loc, f_ex = nfed + incl.y - f_loc;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                b.cnt[i0 + k] = stv[k];
                b.aidx[i0 + k] = act[k] ? a_ex++ : -1;
                if (fed[k]) b.vnew[f_ex++] = (double)rr[k];
                b.fcnt[i0 + k] = f_ex;
            }
        }
        carry = wfm_apply(wg_total(sq, wmap), carry);
        const int2 all = wg_total(WgCount2{}, wcnt);
        nact += all.x; nfed += all.y;
        __syncthreads();                                    // wmap / wcnt are rewritten by the next trip
    }
    // level accumulators: the 256-sample partials of am_level_kernel, in a fixed order
    // (its barriers also: every vnew of this feed is written)
    wg_level_gather(sums, peaks, tid, (n + 255) / 256, b.blk_sum, b.blk_peak);
    const int H = s.H;
    for (int j = tid; j < nfed; j += 256) b.uterm[j] = am_agc_term(b.vnew[j], am_stream_at(b.vhist, H, (const double*)b.vnew, (long)j - H));
    if (tid == 0) {
        s.n_act = nact; s.n_fed = nfed;
        if (n > 0) {
            s.count = carry;
            s.sq_open = am_open(carry, rate) ? 1 : 0;
            s.magsq = b.tot[n - 1] / (double)AM_MA;
            s.magsq_sum += sums[0];
            if ((double)peaks[0] > s.magsq_peak) s.magsq_peak = (double)peaks[0];
            s.magsq_count += n;
        }
    }
}

// ---- 4. per open sample: the AGC value at its fed count and the normalised envelope, into the compacted sequence
__global__ __launch_bounds__(256)
void am_demod_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const AmChan& s = ch[c];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const AmBufs& b = bufs[c];
    const int a = b.aidx[i];
    if (a < 0) return;
    const float r = am_stream_at(b.rhist, s.D, (const float*)b.root, i - s.D);   // sqrt(readBack(rate / 20)) after the write
    const int f = b.fcnt[i];
    const double sum = f > 0 ? b.agc[f - 1] : s.agc_sum;
    const float avg = (float)(sum / (double)s.H);                                // SimpleAGC::getValue, m_clip = 0
    const float g = avg > 0.0f ? avg : 0.0f;
    b.dem[a] = (r - g) / g;
}

__device__ __forceinline__ float am_smootherstep(float x)                   // util/stepfunctions.h:23-36
{
    if (x == 1.0f) return 1.0f; else if (x == 0.0f) return 0.0f;
    const double x3 = x * x * x, x4 = x * x3, x5 = x * x4;
    return (float)(6.0 * x5 - 15.0 * x4 + 10.0 * x3);
}

// ---- 5. per sample: the Bandpass over the compacted sequence (one lane per open sample, taps from LDS), attack,
// conversion; closed or muted samples are 0
__global__ __launch_bounds__(256)
void am_out_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, const float* __restrict__ bp_taps)
{
    __shared__ float taps[AM_BP_H + 1];
    const int c = blockIdx.y;
    const AmChan& s = ch[c];
    if ((long)blockIdx.x * 256 >= s.n) return;
    if (s.bandpass) {
        for (int k = threadIdx.x; k <= AM_BP_H; k += 256) taps[k] = bp_taps[s.bp_off + k];
        __syncthreads();
    }
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const AmBufs& b = bufs[c];
    const int a = b.aidx[i];
    int q = 0;
    if (a >= 0) {
        float demod = b.dem[a];
        if (s.bandpass) {
            const float* __restrict__ hist = b.dhist;
            const float* __restrict__ cur = b.dem;
            demod = am_bandpass(taps, [&](int k) { return am_stream_at(hist, AM_BP_HIST, cur, (long)a - k); });
            demod /= 301.0f;
        }
        const float attack = ((float)b.cnt[i] - s.att) / s.att;
        q = sdrx_to_q16(demod * am_smootherstep(attack) * s.gain * s.volume);
    }
    b.audio[i] = (int16_t)q;
}

// ---- 6. carry: the histories of the next feed (double-buffered: this feed's are still being read), the two sums
__global__ __launch_bounds__(256)
void am_carry_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    AmChan& s = ch[c];
    const AmBufs b = bufs[c];
    const int n = s.n;
    if (tid < AM_MA) b.mhist_next[tid] = am_hist_next(b.mhist, AM_MA, (const float*)b.msq, n, tid);
    for (int i = tid; i < s.D; i += 256) b.rhist_next[i] = am_hist_next(b.rhist, s.D, (const float*)b.root, n, i);
    for (int i = tid; i < s.H; i += 256) b.vhist_next[i] = am_hist_next(b.vhist, s.H, (const double*)b.vnew, s.n_fed, i);
    for (int i = tid; i < AM_BP_HIST; i += 256) b.dhist_next[i] = am_hist_next(b.dhist, AM_BP_HIST, (const float*)b.dem, s.n_act, i);
    if (tid == 0) { s.total = s.total_next; s.agc_sum = s.agc_sum_next; }
}

} // namespace sdrx
