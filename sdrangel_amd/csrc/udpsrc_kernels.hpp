// UDPSrc bank kernels: the tail of UDPSrc::feed (plugins/channelrx/udpsrc/udpsrc.cpp:150-310) for the formats IQ16, IQ24,
// NFM, NFMMono, AMMono, AMNoDCMono and AMBPFMono, with MagAGC for the three AM formats when m_agc is on.  The front (NCO, Interpolator::decimate) is the channel
// back-end's (backend_kernels.hpp); these kernels start from its complex resampler output `ci` at the output rate.
//     inMagSq = |ci|^2;  m_inMovingAverage.feed(inMagSq / 2^30);  m_inMagsq = average();  spectrum Sample(ci)
//     agcFactor = m_agc.feedAndGetValue(ci) (AM formats with m_agc on: every sample, open or not), else 1.0
//     calculateSquelch(m_inMagsq);  the format's payload sample, 0 while the squelch is closed
// Payloads are bit-identical to the strict-IEEE scalar reference build; for NFM / NFMMono that holds where the reference's libm
// has the fdlibm atan2f that udp_atan2f restates (udpsrc_scan.hpp).  Every float and double expression keeps the reference's
// operand order and the file is compiled with -ffp-contract=off.  udpsrc_scan.hpp has the cut of the recurrences; DESIGN.md 4.14 the
// kernel table.  The only loop that is serial along time is psum_rows' (demod_psum.hpp).  A channel's format is uniform over a
// block (blockIdx.y is the channel), so the format branches diverge per block, not per lane.
// The SSB formats LSB, USB, LSBMono and USBMono (4 .. 7) share kernels 1 .. 3 and 6 with the others; their filter, payload and
// carry are udpsrc_ssb_kernels.hpp's, which run between udp_out_kernel and udp_carry_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "udpsrc_scan.hpp"
#include "udpsrc_ssb_sched.hpp"
#include "demod_psum.hpp"
#include "demod_wg.hpp"

namespace sdrx {

struct UdpChan {                        // device resident: config + carried state of one channel
    // --- config
    int fmt;                            // UDPSrcSettings::SampleFormat
    int gate, top;                      // m_squelchGate; the chain's last position (udp_sq_top with the effective release)
    int sq_enabled;
    int w_in, w_am;                     // entries of m_inMovingAverage / m_amMovingAverage
    int xk;                             // carried entries of the compacted stream: w_am (format 9), 300 (format 10), else 1
    int bp_off;                         // float offset into the Bandpass tap table (151 per channel)
    double level;                       // m_squelch = powerFromdB(squelch_db)
    float gain;
    float fm_scaling;                   // output_sample_rate / (2.0f * fm_deviation)
    int agc;                            // m_agc and an AM format: MagAGC is fed
    int a_hn, a_L, a_sdd, a_gate;       // its history length, step length, step-down delay and gate, in samples
    double a_thr;                       // m_threshold = powerFromdB(squelch_db) * 2^23
    // --- state
    int a_g, a_count, a_U, a_D;         // m_gateCounter, m_count, m_stepUpCounter, m_stepDownCounter
    double agc_sum, agc_sum_next;       // the AGC history's m_sum (next: written by udp_agcpsum_kernel)
    int pos;                            // squelch position (udp_sq_pos)
    float m1r, m1i;                     // PhaseDiscriminators::m_m1Sample: the last OPEN sample
    double in_sum, am_sum;              // MovingAverage<double>::m_sum of the two averages
    long long total;                    // output samples since creation or reset
    // --- per feed
    int n, n_act;                       // output samples; open ones
    double in_sum_next, am_sum_next;    // written by the psum kernels, committed by udp_carry_kernel
    // --- formats 4 .. 7 (udpsrc_ssb_kernels.hpp); all zero for the other formats but n_pay
    int ssb;                            // config: an SSB format
    int s_pend;                         // state: fftfilt::inptr
    long long s_blocks;                 // state: blocks completed since creation or reset
    long long total_pay;                // state: payload elements since creation or reset
    int nb, n_pay;                      // per feed: blocks completed; payload elements (= n for the other formats)
};

struct UdpBufs {                        // per channel device pointers (per feed capacity ensured by the host)
    const float2* ci;                   // the front's output of this feed
    const int* n_ptr;                   // its count (device side)
    const double* mhist; double* mhist_next;     // last w_in input powers
    const double* xhist; double* xhist_next;     // last xk elements of the compacted stream
    const double* ghist; double* ghist_next;     // last a_hn raw powers (AGC on)
    double* gterm; double* gtot;        // AGC history: terms and sums; udp_agc_kernel leaves the factor per sample in gterm
    double* dterm; double* tot;         // input average: terms and sums; reused for m_amMovingAverage's once the gate kernel is done
    int* aidx;                          // index in the open sequence (-1: closed)
    int* blk_a;                         // per 256 samples: open samples of this feed before them
    double* x;                          // per open sample: sqrt(inMagSq) (formats 9, 10) or the float2 ci (formats 2, 3)
    int16_t* spec;                      // Sample {re, im} per output sample
    void* out;                          // payload samples
    // formats 4 .. 7, null for the others: the scaled samples waiting for a full block and fftfilt::ovlbuf (256 each, carried),
    // the two halves of every block's inverse FFT
    const float2* pend; float2* pend_next;
    const float2* ovl; float2* ovl_next;
    float2* head; float2* tail;
};

constexpr int UDP_OUT_WIN = 256 + AM_BP_HIST;              // Bandpass inputs one block of udp_out_kernel can touch

__device__ __forceinline__ bool udp_fmt_nfm(int fmt) { return fmt == UDP_NFM || fmt == UDP_NFM_MONO; }
__device__ __forceinline__ bool udp_fmt_amx(int fmt) { return fmt == UDP_AM_NODC_MONO || fmt == UDP_AM_BPF_MONO; }
__device__ __forceinline__ double udp_power_at(const UdpBufs& b, int w, long j)      // input power of stream index j (j < 0: carried)
{
    if (j < 0) return b.mhist[w + j];
    const float2 v = b.ci[j];
    return udp_in_power(v.x * v.x + v.y * v.y);
}

__device__ __forceinline__ double udp_raw_at(const UdpBufs& b, int hn, long j)        // m_magsq of stream index j (j < 0: carried)
{
    if (j < 0) return b.ghist[hn + j];
    const float2 v = b.ci[j];
    return (double)(v.x * v.x + v.y * v.y);
}

// ---- 1. per sample: the input power's moving-average term and the spectrum Sample
__global__ __launch_bounds__(256)
void udp_level_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    const int c = blockIdx.y, tid = threadIdx.x;
    const UdpBufs b = bufs[c];
    const int n = *b.n_ptr;
    if (blockIdx.x == 0 && tid == 0) {
        ch[c].n = n;
        const int nb = ch[c].ssb ? udp_ssb_blocks(ch[c].s_pend, n) : 0;
        ch[c].nb = nb;
        ch[c].n_pay = ch[c].ssb ? (int)udp_ssb_payload_count(ch[c].fmt, ch[c].s_pend, n) : n;
    }
    const long i = (long)blockIdx.x * 256 + tid;
    if (i >= n) return;
    const int w = ch[c].w_in;
    const float2 v = b.ci[i];
    b.dterm[i] = udp_ma_term(udp_in_power(v.x * v.x + v.y * v.y), udp_power_at(b, w, i - w));
    reinterpret_cast<short2*>(b.spec)[i] = make_short2((short)udp_q16f(v.x), (short)udp_q16f(v.y));
    if (ch[c].agc) b.gterm[i] = (double)(v.x * v.x + v.y * v.y) - udp_raw_at(b, ch[c].a_hn, i - ch[c].a_hn);
}

// ---- 2. m_inMovingAverage's sum after every sample: one wave per 16 channels (psum_rows)
__global__ __launch_bounds__(64)
void udp_psum_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs, int n_ch)
{
    psum_channels(n_ch, [&](int c) { return PsumRow{bufs[c].dterm, bufs[c].tot, ch[c].n, ch[c].in_sum, &ch[c].in_sum_next}; });
}

// ---- 2a. AGC on: the history's sum after every sample (psum_rows); the other channels have no terms
__global__ __launch_bounds__(64)
void udp_agcpsum_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs, int n_ch)
{
    psum_channels(n_ch, [&](int c) { return PsumRow{bufs[c].gterm, bufs[c].gtot, ch[c].agc ? ch[c].n : 0, ch[c].agc_sum, &ch[c].agc_sum_next}; });
}

// ---- 2b. AGC on: one workgroup per channel, 1024 samples per trip, four consecutive samples per lane: the gate counter, m_count
// (capped at the step-down delay) and the step pair (magagc_trip, ssb_scan.hpp), then m_u0 and the factor feedAndGetValue
// returns, left in gterm
__global__ __launch_bounds__(256)
void udp_agc_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    __shared__ MagAgcSlots slots;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    UdpChan& s = ch[c];
    if (!s.agc) return;
    const UdpBufs b = bufs[c];
    const int n = s.n, hn = s.a_hn, L = s.a_L, sdd = s.a_sdd, gate = s.a_gate;
    const double thr = s.a_thr, sd = 1.0 / (double)L;
    SsbCounters st; st.g = s.a_g; st.count = s.a_count; st.ud.U = s.a_U; st.ud.D = s.a_D;
    for (int base = 0; base < n; base += 1024)
        magagc_trip(st, slots, base + tid * 4, n, lane, w, gate, sdd, L, thr,
            [&](int i) { const float2 v = b.ci[i]; return (double)(v.x * v.x + v.y * v.y); },
            [&](int i, bool up, SsbUD was, SsbUD ud, double magsq) {
                const double u0 = udp_agc_u0(magsq, b.gtot[i], hn);
                b.gterm[i] = ssb_agc_value(up, was, ud, L, sd, u0);
            });
    if (tid == 0) { s.a_g = st.g; s.a_count = st.count; s.a_U = st.ud.U; s.a_D = st.ud.D; }
}

// ---- 3. one workgroup per channel, 1024 samples per trip: the squelch as a scan of chain maps, the open flags and their
// prefix count (the compaction index), the compacted stream of the formats that advance on open samples only
__global__ __launch_bounds__(256)
void udp_gate_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    __shared__ UdpSq wmap[4];
    __shared__ int wact[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    UdpChan& s = ch[c];
    const UdpBufs b = bufs[c];
    const int n = s.n, G = s.gate, top = s.top, win = s.w_in, fmt = s.fmt;
    const bool enabled = s.sq_enabled != 0, nfm = udp_fmt_nfm(fmt), amx = udp_fmt_amx(fmt);
    const double level = s.level;
    const UdpSqOps sq{top};
    int carry = s.pos, nact = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i0 = base + tid * 4;
        bool up[4];
        UdpSq m = sq.identity();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            up[k] = false;
            if (i0 + k < n) {
                up[k] = udp_above(b.tot[i0 + k], win, enabled, level);
                m = udp_sq_compose(m, udp_sq_map(up[k], G, top), top);
            }
        }
        int st = udp_sq_apply(wg_scan(sq, m, lane, w, wmap), carry);
        bool act[4];
        int a_loc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            act[k] = false;
            if (i0 + k < n) {
                st = udp_sq_step(st, up[k], G, top);
                act[k] = udp_sq_open(st, G);
                a_loc += act[k];
            }
        }
        int a_ex = nact + wg_scan_incl(WgCount{}, a_loc, lane, w, wact) - a_loc;
        if (lane == 0 && i0 < n) b.blk_a[i0 >> 8] = a_ex;   // i0 is a multiple of 256 here
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                b.aidx[i0 + k] = act[k] ? a_ex : -1;
                if (act[k]) {
                    if (nfm) reinterpret_cast<float2*>(b.x)[a_ex] = b.ci[i0 + k];
                    else if (amx) { const float2 v = b.ci[i0 + k]; b.x[a_ex] = __builtin_sqrt((double)(v.x * v.x + v.y * v.y)); }
                    a_ex++;
                }
            }
        }
        carry = udp_sq_apply(wg_total(sq, wmap), carry);
        nact += wg_total(WgCount{}, wact);
        __syncthreads();                                    // wmap / wact are rewritten by the next trip
    }
    if (tid == 0) {
        s.n_act = nact;
        s.pos = carry;
    }
}

// ---- 4a. format 9: m_amMovingAverage's terms over the compacted stream (the input average's buffers are free by now)
__global__ __launch_bounds__(256)
void udp_amterm_kernel(const UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const UdpChan& s = ch[c];
    if (s.fmt != UDP_AM_NODC_MONO) return;
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= s.n_act) return;
    const UdpBufs& b = bufs[c];
    b.dterm[a] = udp_ma_term(b.x[a], am_stream_at(b.xhist, s.xk, (const double*)b.x, a - s.w_am));
}

// ---- 4b. format 9: its sum after every open sample (psum_rows); the other formats have no terms
__global__ __launch_bounds__(64)
void udp_ampsum_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs, int n_ch)
{
    psum_channels(n_ch, [&](int c) {
        return PsumRow{bufs[c].dterm, bufs[c].tot, ch[c].fmt == UDP_AM_NODC_MONO ? ch[c].n_act : 0, ch[c].am_sum, &ch[c].am_sum_next};
    });
}

// ---- 5. per sample: the format's payload sample; closed samples are 0.  The open samples of a block are consecutive in the
// compacted sequence: for format 10 their 256 + 300 inputs and the taps are staged in LDS once, lane p then reads [p - k],
// neighbours in neighbouring bank pairs.
__global__ __launch_bounds__(256)
void udp_out_kernel(const UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs, const float* __restrict__ bp_taps)
{
    __shared__ float taps[AM_BP_H + 1];
    __shared__ double win[UDP_OUT_WIN];
    const int c = blockIdx.y, tid = threadIdx.x;
    const UdpChan& s = ch[c];
    if ((long)blockIdx.x * 256 >= s.n) return;
    const UdpBufs& b = bufs[c];
    const long i = (long)blockIdx.x * 256 + tid;
    const int fmt = s.fmt;
    if (udp_fmt_ssb(fmt)) return;                           // udp_ssb_out_kernel writes these payloads
    const int a = i < s.n ? b.aidx[i] : -1;
    const float gain = s.gain;
    const double factor = s.agc && i < s.n ? b.gterm[i] : 1.0;     // agcFactor
    if (fmt == UDP_AM_BPF_MONO) {
        int q = 0;
        if (__syncthreads_count(a >= 0) != 0) {
            const int a0 = b.blk_a[blockIdx.x], n_act = s.n_act;
            for (int k = tid; k <= AM_BP_H; k += 256) taps[k] = bp_taps[s.bp_off + k];
            for (int j = tid; j < UDP_OUT_WIN; j += 256) {
                const long idx = (long)a0 - AM_BP_HIST + j;
                win[j] = idx < n_act ? am_stream_at(b.xhist, AM_BP_HIST, (const double*)b.x, idx) : 0.0;
            }
            __syncthreads();
            if (a >= 0) {
                const int p = a - a0 + AM_BP_HIST;
                double demodf = udp_bandpass(taps, [&](int k) { return win[p - k]; });
                demodf /= 301.0;
                q = udp_q16f((float)(demodf * factor * (double)gain));
            }
        }
        if (i < s.n) static_cast<int16_t*>(b.out)[i] = (int16_t)q;
        return;
    }
    if (i >= s.n) return;
    const float2 v = b.ci[i];
    if (fmt == UDP_IQ16 || fmt == UDP_IQ24) {
        int re = 0, im = 0;
        if (a >= 0) { re = udp_q16f(v.x * gain); im = udp_q16f(v.y * gain); }
        if (fmt == UDP_IQ16) static_cast<short2*>(b.out)[i] = make_short2((short)re, (short)im);
        else static_cast<int2*>(b.out)[i] = make_int2(re * 256, im * 256);
    } else if (fmt == UDP_NFM || fmt == UDP_NFM_MONO) {
        float d = 0.0f;
        if (a >= 0) {
            float2 m1; if (a == 0) { m1.x = s.m1r; m1.y = s.m1i; } else m1 = reinterpret_cast<const float2*>(b.x)[a - 1];
            const float dr = m1.x * v.x - (-m1.y) * v.y, di = m1.x * v.y + (-m1.y) * v.x;    // conj(m_m1Sample) * ci
            const float ang = udp_atan2f(di, dr);                                            // std::arg = atan2f, the host libm's bits (udpsrc_scan.hpp)
            d = (float)(((double)ang / 3.14159265358979323846) * (double)s.fm_scaling) * gain;
        }
        const int q = udp_q16d((double)d * 32768.0);
        if (fmt == UDP_NFM) static_cast<short2*>(b.out)[i] = make_short2((short)q, (short)q);
        else static_cast<int16_t*>(b.out)[i] = (int16_t)q;
    } else {
        float amp = 0.0f;
        if (a >= 0) {
            const double root = __builtin_sqrt((double)(v.x * v.x + v.y * v.y));
            if (fmt == UDP_AM_MONO) amp = (float)(root * factor * (double)gain);
            else amp = (float)((root - b.tot[a] / (double)s.w_am) * factor * (double)gain);      // UDP_AM_NODC_MONO
        }
        static_cast<int16_t*>(b.out)[i] = (int16_t)udp_q16f(amp);
    }
}

// ---- 6. carry: the histories of the next feed (double-buffered: this feed's are still being read), m_m1Sample, the sums
__global__ __launch_bounds__(256)
void udp_carry_kernel(UdpChan* __restrict__ ch, const UdpBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    UdpChan& s = ch[c];
    const UdpBufs b = bufs[c];
    const int n = s.n, w = s.w_in, xk = s.xk, n_act = s.n_act;
    for (int i = tid; i < w; i += 256) b.mhist_next[i] = udp_power_at(b, w, (long)n - w + i);
    if (udp_fmt_amx(s.fmt))
        for (int i = tid; i < xk; i += 256) b.xhist_next[i] = am_hist_next(b.xhist, xk, (const double*)b.x, n_act, i);
    if (s.agc)
        for (int i = tid; i < s.a_hn; i += 256) b.ghist_next[i] = udp_raw_at(b, s.a_hn, (long)n - s.a_hn + i);
    if (tid == 0) {
        s.in_sum = s.in_sum_next;
        if (s.agc) s.agc_sum = s.agc_sum_next;
        if (s.fmt == UDP_AM_NODC_MONO) s.am_sum = s.am_sum_next;
        if (udp_fmt_nfm(s.fmt) && n_act > 0) { const float2 v = reinterpret_cast<const float2*>(b.x)[n_act - 1]; s.m1r = v.x; s.m1i = v.y; }
        s.total += n;
    }
}

} // namespace sdrx
