// Broadcast-FM stereo demodulator bank kernels: BFMDemod::feed (plugins/channelrx/demodbfm/bfmdemod.cpp:116-281), m_rdsActive clear
//     Complex c(re / SDR_RX_SCALEF, im / SDR_RX_SCALEF); c *= m_nco.nextIQ();        NCO            sdrbase/dsp/nco.cpp:30-64
//     rf_out = m_rfFilter->runFilt(c, &rf);                                           fftfilt 1024   fftfilt.cpp:261-282 (g_fft)
//     for each rf[i]: msq, level sums, squelch counter, gated phaseDiscriminator                    phasediscri.h:50-55
//                     m_pilotPLL.process(demod, m_pilotPLLSamples)                                   phaselock.cpp:253-367
//                     m_interpolatorStereo.decimate(s), m_interpolator.decimate(Complex(demod, 0))   interpolator.h:23-36,182-195
//                     m_deemphasisFilterX / Y.process, (qint16)(deemph * (1 << 12) * volume)         filterrc.cpp:44-56
// Audio, sink stream and state are bit-identical to the strict-IEEE scalar reference build: every float expression keeps the
// reference's operand order and the file is compiled with -ffp-contract=off.  DESIGN.md 4.17 has the kernel cut and what bounds
// each kernel.
//
// The front is WFM's (wfm_kernels.hpp): the block cut, pending samples, the NCO mix on load (here on scaled samples), the two
// g_fft, overlap-add, the level sums, the clamp-map scan of the squelch counter and the resampler schedule are its device
// functions, run on the WfmChan / WfmBufs a BFM channel embeds.  What differs starts at the level kernel: msq is not divided
// by the scale squared, the filtered sample itself is kept (the discriminator multiplies by the conjugate of the last OPEN
// sample), and behind the discriminator come the pilot walk, the two resamplers and the de-emphasis walk.
#pragma once
#include "fm_front.hpp"
#include "wave_walk.hpp"
#include "bfm_pll.hpp"
#include "bfm_rds.hpp"

namespace sdrx {

constexpr int BFM_WALK_WAVES = 4;       // channels per workgroup of the two walks, one wave each

struct BfmChan {                        // device resident: config + carried state of one channel
    WfmChan w;                          // the front's; w.fm_scaling = (Real) in_rate / m_fmExcursion, w.mute = 0, w.prev_arg unused
    // --- config
    int stereo, lsb, show_pilot;        // m_audioStereo, m_lsbStereo, m_showPilot
    BfmPllCfg pk;                       // m_pilotPLL.configure(19000.0 / in_rate, 50.0 / in_rate, 0.01)
    float rc_b0, rc_a1;                 // both LowPassFilterRC: configure(50.0 * audio_rate * 1.0e-6)
    // --- state
    float2 m1;                          // m_phaseDiscri.m_m1Sample: the last open sample
    BfmPllState ps;
    float y1x, y1y;                     // m_deemphasisFilterX / Y.m_y1
    // --- per feed
    int last_open;                      // index of the feed's last open sample (-1: none)
    int n_sink;                         // Samples of the sink stream
};

struct BfmBufs {                        // per channel device pointers (per feed capacity ensured by the host)
    WfmBufs w;                          // arg, blk_first and audio are not used here
    float2* rf;                         // the filtered samples
    uint8_t* opn;                       // squelch open at the sample
    int* blk_prev;                      // per block: index in the feed of the last open sample in front of it (-1: none)
    float2* psc;                        // (m_psin, m_pcos) of every step of the pilot loop
    float2* st;                         // [WFM_HIST carried | 512 * n_blocks] input of m_interpolatorStereo
    float2* mix;                        // per audio sample: (ci.real(), sampleStereo)
    uint32_t* sink;                     // packed Samples of m_sampleBuffer
    short2* pairs;                      // l, r
};

// RDS (m_rdsActive): a second pair of tables next to BfmChan / BfmBufs, which a handle without RDS never allocates
constexpr int RDS_PHASES = 4;           // m_interpolatorRDS.create(4, in_rate, 600.0)
constexpr int RDS_XV_FRONT = 4;         // m_xv values kept in front of a feed's (three are read)

struct BfmRdsChan {
    // --- config
    int active;                         // m_rdsActive
    int ntaps, taps_off;                // taps per phase (18); float offset into the RDS taps table: [phase][ntaps]
    float step;                         // m_interpolatorRDSDistance = (Real) in_rate / 250000.0
    // --- state
    float distance;                     // m_interpolatorRDSDistanceRemain
    float mix_phase;                    // m_pilotPLLSamples[3]: m_phase at the entry of the last pilot step
    RdsDemodState d;
    RdsDecoderState k;
    unsigned long long unsure;          // samples whose r the cosine's enclosure does not pin (rds_mix.hpp), since the last reset of it
    // --- per feed
    int n_rds, n_bits, n_groups, pad_;
};

struct BfmRdsBufs {                     // per channel device pointers (all null for a channel without RDS)
    float* ph;                          // per filtered sample of a stereo channel: m_phase as its pilot step found it
    float* rin;                         // [WFM_HIST carried | 512 * n_blocks] r.real(): the input of m_interpolatorRDS
    uint2* sched;                       // per RDS sample: {index of the completing input, bits(distance)}
    float* xv;                          // [RDS_XV_FRONT carried | n_rds] m_xv[0][2] of every RDS sample
    float* bb;                          // m_parms.subcarr_bb[0] of every RDS sample
    uint8_t* bits;                      // the bits RDSDemod::process returned
    uint16_t* groups;                   // four blocks per group RDSDecoder::frameSync completed
};

__device__ __forceinline__ uint32_t bfm_sink_sample(float v)                // Sample(v * SDR_RX_SCALEF, 0.0)
{
    return (uint32_t)sdrx_to_q16(v * 32768.0f) & 0xffffu;
}

// ---- 1. the front, WFM's device functions on the embedded structures
__global__ void bfm_prep_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_ch) wfm_prep_body(ch[c].w, bufs[c].w);
}
__global__ void __launch_bounds__(256) bfm_sched_fill_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    wfm_sched_fill_body(ch[blockIdx.y].w, bufs[blockIdx.y].w);
}
__global__ void bfm_sched_walk_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_ch) wfm_sched_walk_body(ch[c].w, bufs[c].w);
}
__global__ __launch_bounds__(WFM_FFT / 8)
void bfm_fft_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, const float2* __restrict__ filters,
                    const float* __restrict__ utbl, const float* __restrict__ nco_tbl)
{
    wfm_fft_body<true>(ch[blockIdx.y].w, bufs[blockIdx.y].w, filters, utbl, nco_tbl);
}
__global__ __launch_bounds__(WFM_H)
void bfm_pend_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    wfm_pend_body(ch[blockIdx.x].w, bufs[blockIdx.x].w);
}

// ---- 2. overlap-add, the filtered sample, msq = re*re + im*im (float, then double: no division by the scale), squelch flag;
// per block the composed counter map, the msq sum and peak.  256 threads, two consecutive samples each.
__global__ __launch_bounds__(256)
void bfm_level_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    __shared__ WfmClamp maps[256];
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const WfmChan& s = ch[c].w;
    if (blk >= s.n_blocks) return;
    const BfmBufs& b = bufs[c];
    const long j0 = (long)blk * WFM_H + 2 * tid;
    const float4 o = *reinterpret_cast<const float4*>(b.w.tail + j0), h = *reinterpret_cast<const float4*>(b.w.head + j0);
    float4 r;                                               // output[i] = ovlbuf[i] + data[i] (tail slots are shifted by one block)
    r.x = o.x + h.x; r.y = o.y + h.y; r.z = o.z + h.z; r.w = o.w + h.w;
    *reinterpret_cast<float4*>(b.rf + j0) = r;
    const float level = s.squelch_level;
    const float msq0 = r.x * r.x + r.y * r.y, msq1 = r.z * r.z + r.w * r.w;
    const bool f0 = msq0 >= level, f1 = msq1 >= level;     // double against Real: both are floats' values
    *reinterpret_cast<uchar2*>(b.w.flag + j0) = make_uchar2(f0 ? 1 : 0, f1 ? 1 : 0);
    wfm_block_reduce(b.w, blk, tid, s.cap, f0, f1, msq0, msq1, maps, sums, peaks);
}

__global__ __launch_bounds__(64)
void bfm_blockscan_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    wfm_blockscan_body(ch[blockIdx.x].w, bufs[blockIdx.x].w);
}

// ---- 3. the gated discriminator.  (a) per (block, channel): the open flag of every sample and the block's last open sample
__global__ __launch_bounds__(256)
void bfm_open_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    __shared__ WfmClamp wmap[4];
    __shared__ int wlast[4];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const WfmChan& s = ch[c].w;
    if (blk >= s.n_blocks) return;
    const BfmBufs& b = bufs[c];
    const long j0 = (long)blk * WFM_H + 2 * tid;
    const uchar2 f2 = *reinterpret_cast<const uchar2*>(b.w.flag + j0);
    bool open0, open1;
    wfm_open_pair(s, b.w.blk_state[blk], f2, lane, w, wmap, &open0, &open1);
    *reinterpret_cast<uchar2*>(b.opn + j0) = make_uchar2(open0 ? 1 : 0, open1 ? 1 : 0);
    int last = open1 ? 2 * tid + 1 : (open0 ? 2 * tid : -1);
    for (int o = 32; o; o >>= 1) last = wfm_last_open(last, __shfl_xor(last, o, 64));
    if (lane == 0) wlast[w] = last;
    __syncthreads();
    if (tid == 0) b.w.blk_last[blk] = wfm_last_open(wfm_last_open(wlast[0], wlast[1]), wfm_last_open(wlast[2], wlast[3]));
}

// (b) one wave per channel: the last open sample in front of every block, and the feed's last (m_m1Sample of the next feed)
__global__ __launch_bounds__(64)
void bfm_lastopen_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    BfmChan& s = ch[c];
    const BfmBufs& b = bufs[c];
    const int nb = s.w.n_blocks;
    int carry = -1;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int blk = b0 + lane;
        const bool in = blk < nb;
        const int last = in ? b.w.blk_last[blk] : -1;
        const int incl = wfm_wave_max_scan(last >= 0 ? blk * WFM_H + last : -1, lane);
        int ex = __shfl_up(incl, 1, 64);
        if (lane == 0) ex = -1;
        if (in) b.blk_prev[blk] = wfm_last_open(carry, ex);
        carry = wfm_last_open(carry, __shfl(incl, 63, 64));
    }
    if (lane == 0) s.last_open = carry;
}

__device__ __forceinline__ float bfm_discri(float2 m1, float2 x, float fm_scaling)      // phaseDiscriminator
{
    // std::conj(m_m1Sample) * sample
    const float cj = -m1.y;
    const float dr = m1.x * x.x - cj * x.y, di = m1.x * x.y + cj * x.x;
    return (float)(((double)udp_atan2f(di, dr) / 3.14159265358979323846) * (double)fm_scaling);
}

// (c) per (block, channel): last-open scan inside the block, the predecessor's VALUE from the filtered samples (of this block,
// of an earlier block through blk_prev, or the carried m_m1Sample), demod, and the sink stream's Sample when m_showPilot is clear
__global__ __launch_bounds__(256)
void bfm_discri_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    __shared__ int wmax[4];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const BfmChan& s = ch[c];
    if (blk >= s.w.n_blocks) return;
    const BfmBufs& b = bufs[c];
    const long j0 = (long)blk * WFM_H + 2 * tid;
    const uchar2 o2 = *reinterpret_cast<const uchar2*>(b.opn + j0);
    const bool open0 = o2.x != 0, open1 = o2.y != 0;
    const int base = blk * WFM_H;
    const int mine = open1 ? base + 2 * tid + 1 : (open0 ? base + 2 * tid : -1);
    const int mincl = wfm_wave_max_scan(mine, lane);
    if (lane == 63) wmax[w] = mincl;
    __syncthreads();
    int prev0 = __shfl_up(mincl, 1, 64);
    if (lane == 0) prev0 = -1;
    for (int q = 0; q < w; q++) prev0 = wfm_last_open(prev0, wmax[q]);
    prev0 = wfm_last_open(prev0, b.blk_prev[blk]);
    const float4 x = *reinterpret_cast<const float4*>(b.rf + j0);
    const float fm = s.w.fm_scaling;
    float d0 = 0.0f, d1 = 0.0f;
    if (open0) d0 = bfm_discri(prev0 >= 0 ? b.rf[prev0] : s.m1, make_float2(x.x, x.y), fm);
    if (open1) d1 = bfm_discri(open0 ? make_float2(x.x, x.y) : (prev0 >= 0 ? b.rf[prev0] : s.m1), make_float2(x.z, x.w), fm);
    *reinterpret_cast<float2*>(b.w.dem + WFM_HIST + j0) = make_float2(d0, d1);
    if (!s.show_pilot) *reinterpret_cast<uint2*>(b.sink + j0) = make_uint2(bfm_sink_sample(d0), bfm_sink_sample(d1));
}

// ---- 4. the pilot walk, one wave per stereo channel (wave_walk.hpp): demod is staged 64 steps ahead, one per lane; every lane
// takes step j's input from lane j's register and runs the same step, lane j keeps (m_psin, m_pcos) of step j, and the 64 go out
// in one store.  The loop's state stays in registers from the first step of a feed to its last.  The loop runs on every
// filtered sample, closed squelch included (demod = 0).
__global__ __launch_bounds__(64 * BFM_WALK_WAVES)
void bfm_walk_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * BFM_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    BfmChan& s = ch[c];
    if (!s.stereo) return;
    const int n = s.w.n_dem;
    if (n <= 0) return;
    const BfmPllCfg k = s.pk;
    BfmPllState st = s.ps;
    const float* __restrict__ dem = bufs[c].w.dem + WFM_HIST;
    float2* __restrict__ psc = bufs[c].psc;
    float next = lane < n ? walk_global_load(dem + lane) : 0.0f;
    for (int base = 0; base < n; base += 64) {
        const float cur = next;
        if (base + 64 + lane < n) next = walk_global_load(dem + base + 64 + lane);
        const int cnt = min(64, n - base);
        float2 mine = make_float2(0.0f, 0.0f);
        for (int j = 0; j < cnt; j++) {
            float sn, cs;
            bfm_pll_step(k, st, walk_lane_value(cur, j), &sn, &cs, (BfmPllProbe*)nullptr);
            if (lane == j) mine = make_float2(sn, cs);
        }
        if (base + lane < n) walk_global_store(psc + base + lane, mine);
    }
    if (lane == 0) s.ps = st;
}

// The same walk for a handle with RDS on in a stereo channel: those channels also keep m_phase as every step finds it (what
// processPhase stores into m_pilotPLLSamples[3], phaselock.h:179) for the 57 kHz mixer.  A kernel of its own, not a template
// flag on the one above: with the body shared through an inlined function the compiler scheduled the RDS-off walk differently
// and it ran 3.4 % slower, so the walk of a handle without RDS stays the source it was, line for line.
__global__ __launch_bounds__(64 * BFM_WALK_WAVES)
void bfm_walk_rds_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, int n_ch,
                         const BfmRdsChan* __restrict__ rds, const BfmRdsBufs* __restrict__ rbufs)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * BFM_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    BfmChan& s = ch[c];
    if (!s.stereo) return;
    const int n = s.w.n_dem;
    if (n <= 0) return;
    const BfmPllCfg k = s.pk;
    BfmPllState st = s.ps;
    const float* __restrict__ dem = bufs[c].w.dem + WFM_HIST;
    float2* __restrict__ psc = bufs[c].psc;
    unsigned int* __restrict__ ph = rds[c].active ? reinterpret_cast<unsigned int*>(rbufs[c].ph) : nullptr;
    float next = lane < n ? walk_global_load(dem + lane) : 0.0f;
    for (int base = 0; base < n; base += 64) {
        const float cur = next;
        if (base + 64 + lane < n) next = walk_global_load(dem + base + 64 + lane);
        const int cnt = min(64, n - base);
        float2 mine = make_float2(0.0f, 0.0f);
        float entry = 0.0f;
        for (int j = 0; j < cnt; j++) {
            float sn, cs;
            if (lane == j) entry = st.phase;
            bfm_pll_step(k, st, walk_lane_value(cur, j), &sn, &cs, (BfmPllProbe*)nullptr);
            if (lane == j) mine = make_float2(sn, cs);
        }
        if (base + lane < n) {
            walk_global_store(psc + base + lane, mine);
            if (ph) walk_global_store(ph + base + lane, (unsigned int)__float_as_int(entry));
        }
    }
    if (lane == 0) s.ps = st;
}

// ---- 5. per filtered sample of a stereo channel: m_pilotPLLSamples[1], [2] -> the input of m_interpolatorStereo, and the sink
// stream's Sample when m_showPilot is set
__global__ __launch_bounds__(256)
void bfm_post_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const BfmChan& s = ch[c];
    if (!s.stereo) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= s.w.n_dem) return;
    const BfmBufs& b = bufs[c];
    const float2 p = b.psc[j];
    const float demod = b.w.dem[WFM_HIST + j];
    const float p1 = bfm_pilot_sin2(p.x, p.y);
    float2 v;
    if (s.lsb) { v.x = demod * p1; v.y = demod * bfm_pilot_cos2(p.y); }
    else { v.x = (float)((double)demod * 1.17 * (double)p1); v.y = 0.0f; }
    b.st[WFM_HIST + j] = v;
    if (s.show_pilot) b.sink[j] = bfm_sink_sample(p1);
}

// ---- 6. the two polyphase FIRs, one lane per audio sample from the one schedule (both distances run through the same
// arithmetic from the same start): the mono sum on demod, real accumulator only; the stereo difference on s, real and
// imaginary accumulators, mul and add separate, newest first
__global__ __launch_bounds__(256)
void bfm_fir_kernel(const BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, const float* __restrict__ taps)
{
    const int c = blockIdx.y;
    const BfmChan& s = ch[c];
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= s.w.n_out) return;
    const BfmBufs& b = bufs[c];
    const uint2 e = b.w.sched[o];
    const float* __restrict__ t = wfm_fir_taps(s.w, e, taps);
    const int nt = s.w.ntaps;
    const float ci = wfm_fir_acc(t, nt, b.w.dem + WFM_HIST + (int)e.x);
    float ss = 0.0f;                                        // sampleStereo
    if (s.stereo) {
        const float2* __restrict__ x = b.st + WFM_HIST + (int)e.x;
        float ra = 0.0f, ia = 0.0f;
        if (s.lsb) {
#pragma unroll 8
            for (int i = 0; i < nt; i++) { ra += t[i] * x[-i].x; ia += t[i] * x[-i].y; }
            ss = ra + ia;
        } else {
#pragma unroll 8
            for (int i = 0; i < nt; i++) ra += t[i] * x[-i].x;
            ss = ra;
        }
    }
    b.mix[o] = make_float2(ci, ss);
}

// ---- 7. de-emphasis and conversion, one wave per channel, staged like the pilot walk: the two filters' inputs of 64 audio
// samples one per lane, every lane steps both recurrences, lane j keeps step j's pair and converts it
__global__ __launch_bounds__(64 * BFM_WALK_WAVES)
void bfm_deemph_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * BFM_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    BfmChan& s = ch[c];
    const int n = s.w.n_out;
    if (n <= 0) return;
    const bool stereo = s.stereo != 0;
    const float b0 = s.rc_b0, a1 = s.rc_a1, volume = s.w.volume;
    float yx = s.y1x, yy = s.y1y;
    const float2* __restrict__ mix = bufs[c].mix;
    unsigned int* __restrict__ out = reinterpret_cast<unsigned int*>(bufs[c].pairs);
    float2 next = lane < n ? walk_global_load(mix + lane) : make_float2(0.0f, 0.0f);
    for (int base = 0; base < n; base += 64) {
        const float2 cur = next;
        if (base + 64 + lane < n) next = walk_global_load(mix + base + 64 + lane);
        const float xin = stereo ? cur.x + cur.y : cur.x, yin = cur.x - cur.y;
        const int cnt = min(64, n - base);
        float mx = 0.0f, my = 0.0f;
        for (int j = 0; j < cnt; j++) {
            const float ox = bfm_rc_step(walk_lane_value(xin, j), b0, a1, &yx);
            float oy = 0.0f;
            if (stereo) oy = bfm_rc_step(walk_lane_value(yin, j), b0, a1, &yy);
            if (lane == j) { mx = ox; my = oy; }
        }
        if (base + lane < n) {
            const unsigned int l = (unsigned int)sdrx_to_q16(mx * (float)(1 << 12) * volume) & 0xffffu;
            const unsigned int r = stereo ? (unsigned int)sdrx_to_q16(my * (float)(1 << 12) * volume) & 0xffffu : l;
            walk_global_store(out + base + lane, l | (r << 16));
        }
    }
    if (lane == 0) { s.y1x = yx; s.y1y = yy; }
}

// ---- 7a. RDS, per channel with m_rdsActive (bfmdemod.cpp:169-187).  The schedule of m_interpolatorRDS: wfm_sched_walk_body's
// recurrence on the RDS distance.  With in_rate < 250000 the distance goes negative and stays there; d - 1.0 then rounds, as the
// reference's does (one float operation either way), every input emits, and the FIR clamps the negative phase to 0.
__global__ void bfm_rds_sched_kernel(const BfmChan* __restrict__ ch, BfmRdsChan* __restrict__ rds, const BfmRdsBufs* __restrict__ rbufs, int n_ch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_ch) return;
    BfmRdsChan& r = rds[c];
    if (!r.active) return;
    const int n = ch[c].w.n_dem;
    const float step = r.step;
    uint2* __restrict__ p = rbufs[c].sched;
    float d = r.distance;
    int k = -1, cnt = 0;
    for (;;) {
        const float m = fmaxf(floorf(d), 1.0f);
        const int kn = k + (int)m;
        if (kn >= n) break;
        k = kn; d -= m;
        p[cnt++] = make_uint2((uint32_t)k, __float_as_uint(d));
        d += step;
    }
    r.distance = d - (float)(n - 1 - k);
    r.n_rds = cnt;
}

// the mixer, per filtered sample: stereo channels through rds_mix with the phase the PREVIOUS sample's pilot step found (the
// carried one for a feed's first sample); mono channels never write m_pilotPLLSamples[3], cos(0.0) = 1 and r = demod * 2.0
__global__ __launch_bounds__(256)
void bfm_rds_mix_kernel(const BfmChan* __restrict__ ch, BfmRdsChan* __restrict__ rds, const BfmBufs* __restrict__ bufs,
                        const BfmRdsBufs* __restrict__ rbufs)
{
    const int c = blockIdx.y;
    BfmRdsChan& r = rds[c];
    if (!r.active) return;
    const BfmChan& s = ch[c];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= s.w.n_dem) return;
    const BfmRdsBufs& rb = rbufs[c];
    const float demod = bufs[c].w.dem[WFM_HIST + j];
    float v;
    if (s.stereo) {
        const float phase = j ? rb.ph[j - 1] : r.mix_phase;
        bool unsure;
        v = rds_mix(demod, phase, &unsure);
        if (unsure) atomicAdd(&r.unsure, 1ull);
    } else {
        v = demod + demod;
    }
    rb.rin[WFM_HIST + j] = v;
}

// m_interpolatorRDS's FIR on the real part (interpolator.h:183-194, real accumulator, taps in that order, mul and add
// separate), one lane per RDS sample, and the sample's m_xv[0][2] = input / 4.491730007e+03
__global__ __launch_bounds__(256)
void bfm_rds_fir_kernel(const BfmRdsChan* __restrict__ rds, const BfmRdsBufs* __restrict__ rbufs, const float* __restrict__ taps)
{
    const int c = blockIdx.y;
    const BfmRdsChan& r = rds[c];
    if (!r.active) return;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= r.n_rds) return;
    const BfmRdsBufs& rb = rbufs[c];
    const uint2 e = rb.sched[o];
    int ph = (int)floorf(__uint_as_float(e.y) * (float)RDS_PHASES);
    if (ph < 0) ph = 0;                                     // doInterpolate's clamp
    const float* __restrict__ t = taps + r.taps_off + ph * r.ntaps;
    rb.xv[RDS_XV_FRONT + o] = rds_xv(wfm_fir_acc(t, r.ntaps, rb.rin + WFM_HIST + (int)e.x));
}

// RDSDemod::process and RDSDecoder::frameSync, one wave per channel staged like the pilot walk: lane j holds the FIR half of
// the filter for step j (three m_xv values, read with the carried front), every lane runs the same step, lane j keeps step j's
// subcarr_bb.  Bits and groups leave from lane 0 as they come.  The state stays in registers for the feed.
__global__ __launch_bounds__(64 * BFM_WALK_WAVES)
void bfm_rds_walk_kernel(BfmRdsChan* __restrict__ rds, const BfmRdsBufs* __restrict__ rbufs, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * BFM_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    BfmRdsChan& r = rds[c];
    if (!r.active) return;
    const int n = r.n_rds;
    int n_bits = 0, n_groups = 0;
    if (n > 0) {
        RdsDemodState d = r.d;
        RdsDecoderState k = r.k;
        const float* __restrict__ xv = rbufs[c].xv + RDS_XV_FRONT;
        unsigned int* __restrict__ bb = reinterpret_cast<unsigned int*>(rbufs[c].bb);
        uint8_t* __restrict__ bits = rbufs[c].bits;
        uint16_t* __restrict__ groups = rbufs[c].groups;
        for (int base = 0; base < n; base += 64) {
            float fir = 0.0f;
            if (base + lane < n) {
                const float* x = xv + base + lane;
                fir = rds_fir_part(walk_global_load(x - 2), walk_global_load(x - 1), walk_global_load(x));
            }
            const int cnt = min(64, n - base);
            float mine = 0.0f;
            for (int j = 0; j < cnt; j++) {
                bool bit = false;
                const bool got = rds_demod_step(d, walk_lane_value(fir, j), &bit, (RdsProbe*)nullptr);
                if (lane == j) mine = d.yv[2];
                if (got) {
                    if (lane == 0) bits[n_bits] = bit ? 1 : 0;
                    n_bits++;
                    if (rds_frame_sync(k, bit, (RdsProbe*)nullptr)) {
                        if (lane < 4) groups[4 * n_groups + lane] = (uint16_t)(lane == 0 ? k.group0 : lane == 1 ? k.group1 : lane == 2 ? k.group2 : k.group3);
                        n_groups++;
                    }
                }
            }
            if (base + lane < n) walk_global_store(bb + base + lane, (unsigned int)__float_as_int(mine));
        }
        if (lane == 0) {
            const float* last = xv + n - 3;
            d.xv[0] = last[0]; d.xv[1] = last[1]; d.xv[2] = last[2];
            r.d = d; r.k = k;
        }
    }
    if (lane == 0) { r.n_bits = n_bits; r.n_groups = n_groups; }
}

// the RDS resampler's window, the m_xv front and the mixer's phase for the next feed (one workgroup per channel, after
// everything else of RDS)
__global__ __launch_bounds__(WFM_HIST)
void bfm_rds_carry_kernel(const BfmChan* __restrict__ ch, BfmRdsChan* __restrict__ rds, const BfmRdsBufs* __restrict__ rbufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    BfmRdsChan& r = rds[c];
    if (!r.active) return;
    const BfmRdsBufs& rb = rbufs[c];
    const int n_dem = ch[c].w.n_dem, n = r.n_rds;
    const float keep = rb.rin[n_dem + tid];                 // the last WFM_HIST of [carried | new]
    float kx = 0.0f;
    if (tid < RDS_XV_FRONT) kx = rb.xv[n + tid];
    __syncthreads();
    rb.rin[tid] = keep;
    if (tid < RDS_XV_FRONT) rb.xv[tid] = kx;
    if (tid == 0 && n_dem > 0 && ch[c].stereo) r.mix_phase = rb.ph[n_dem - 1];
}

// ---- 8. carry: the front's (ovlbuf, mono resampler window, NCO phase, pending count), the stereo resampler's window,
// m_m1Sample, the sink stream's length (one workgroup per channel, after everything else)
__global__ __launch_bounds__(WFM_H)
void bfm_carry_kernel(BfmChan* __restrict__ ch, const BfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    BfmChan& s = ch[c];
    const BfmBufs& b = bufs[c];
    const int n_dem = s.w.n_dem, nb = s.w.n_blocks;
    float2 keep = make_float2(0.0f, 0.0f);
    if (s.stereo && tid < WFM_HIST) keep = b.st[n_dem + tid];              // the last WFM_HIST of [carried | new]
    wfm_carry_body(s.w, b.w);                                               // holds a barrier
    if (s.stereo && tid < WFM_HIST) b.st[tid] = keep;
    if (tid == 0) {
        if (nb > 0 && s.last_open >= 0) s.m1 = b.rf[s.last_open];
        s.n_sink = (!s.show_pilot || s.stereo) ? n_dem : 0;
    }
}

} // namespace sdrx
