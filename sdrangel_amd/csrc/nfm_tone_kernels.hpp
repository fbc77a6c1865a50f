// NFM demodulator bank, the tone options.  The AF squelch (m_deltaSquelch, nfmdemod.cpp:179-206): nfm_af_walk_kernel, launched
// only by a handle that has such a channel.  CTCSS: the m_ctcssOn branch of NFMDemod::feed (nfmdemod.cpp:235-296) behind
// nfm_gate_kernel (and the walk) and in front of nfm_out_kernel.  nfm_tone_scan.hpp has the cut; DESIGN.md 4.12 the kernel table.  Launched
// only by a handle that has a CTCSS channel; a channel of such a handle without CTCSS leaves every kernel here at once.
//   nfm_af_walk_kernel      one lane per channel: the feed's samples in order through AFSquelch and the delay line with zeroBack
//   nfm_ct_pack_kernel      per sample: keeps nfm_gate_kernel's compaction (A: open and unmuted) and compacts the Lowpass inputs
//   nfm_ct_lowpass_kernel   per detector sample (one in eight of A): the 301-tap Lowpass over A, window and taps in LDS, 32 lanes a block
//   nfm_ct_detect_kernel    one workgroup per channel: detector samples compacted (C), Goertzel per (block, tone), the
//                           m_ctcssIndex stream as a last-writer scan, the compaction nfm_out_kernel then runs on (B: A that
//                           passes the tone test), the index changes, the carry
// Every float expression keeps the reference's operand order; the file is compiled with -ffp-contract=off.
#pragma once
#include "nfm_kernels.hpp"
#include "nfm_tone_scan.hpp"

namespace sdrx {

struct CtLastOps {
    using Map = int;
    __device__ __forceinline__ int identity() const { return -1; }
    __device__ __forceinline__ int compose(int f, int g) const { return ct_last_compose(f, g); }
    __device__ __forceinline__ int shfl_up(int m, int o) const { return __shfl_up(m, o, 64); }
};

constexpr int CT_GROUPS = 256 / CT_TONES;                  // detector blocks one trip of nfm_ct_detect_kernel runs

// ---- 0. the AF squelch (m_deltaSquelch): one lane per channel walks the feed's samples in order through the reference's
// containers (nfm_tone_scan.hpp) and leaves what nfm_gate_kernel leaves -- w, aidx, blk_a, x, n_act, count, sq_open -- so that
// everything behind it, CTCSS included, runs unchanged.  nfm_gate_kernel has run before it with the power squelch's `up`: its
// level accumulators stand (the 32-sample average runs in delta mode too), the rest is overwritten here.
template <class T> __device__ __forceinline__ T* af_set0(const T* a, T* b) { return const_cast<T*>(a) < b ? const_cast<T*>(a) : b; }

__global__ __launch_bounds__(64)
void nfm_af_walk_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_ch) return;
    NfmChan& s = ch[c];
    if (!s.af_on) return;
    const NfmBufs b = bufs[c];
    float* dl = af_set0(b.dl, b.dl_next);
    double* hist = af_set0(b.afh, b.afh_next);
    AfState a = s.af;
    AfDelay q = s.afq;
    const int n = s.n, gate = s.gate, cap = 2 * s.gate, N = s.af_n, Z = s.af_z;
    const double coef[2] = {s.af_coef[0], s.af_coef[1]}, thr = s.af_thr;
    const bool mute = s.mute != 0;
    int count = s.af_sq_count, nact = 0;
    for (int i = 0; i < n; i++) {
        const float wr = b.wraw[i];
        const bool up = af_sample(a, hist, dl, q, N, coef, thr, Z, wr, nullptr);
        b.w[i] = up ? wr : 0.0f;
        count = wfm_apply(wfm_step(up, cap), count);
        const bool act = nfm_open(count, gate) && !mute;
        if ((i & 255) == 0) b.blk_a[i >> 8] = nact;
        b.aidx[i] = act ? nact : -1;
        if (act) b.x[nact++] = dl[af_dl_read_slot(q, gate)];
    }
    s.af = a; s.afq = q; s.n_act = nact;
    if (n > 0) { s.af_sq_count = count; s.count = count; s.sq_open = nfm_open(count, gate) ? 1 : 0; }
}

// ---- 1. per sample: nfm_gate_kernel's aidx and x are about to be rebuilt for B; keep A's, and compact demod * comp over A
__global__ __launch_bounds__(256)
void nfm_ct_pack_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y, tid = threadIdx.x;
    NfmChan& s = ch[c];
    if (!s.ct_on) return;
    const int n = s.n;
    if (blockIdx.x == 0 && tid == 0) s.n_act_a = s.n_act;
    const long i = (long)blockIdx.x * 256 + tid;
    if (i >= n) return;
    const NfmBufs& b = bufs[c];
    const int a = b.aidx[i];
    b.aidx_a[i] = a;
    if (a >= 0) { b.xl[a] = b.wraw[i]; b.xa[a] = b.x[a]; }
}

// ---- 2. per detector sample: m_lowpass.filter over the open sequence.  As nfm_out_kernel: the open samples of a block are
// consecutive in A, their 256 + 300 inputs and the taps are staged in LDS once.  Whether a sample is the detector's depends on
// its position mod 8 alone, so each aligned group of eight lanes has one candidate: the block's up to 32 outputs are handed to
// the lower half of wave 0 through a list, and the other waves leave after the staging.  Neighbouring outputs are eight inputs
// apart; element idx of the window sits at idx + idx / 8, which puts them nine banks apart.
constexpr int CT_LP_WIN = NFM_OUT_WIN + NFM_OUT_WIN / 8 + 1;

__global__ __launch_bounds__(256)
void nfm_ct_lowpass_kernel(const NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs, const float* __restrict__ tab)
{
    __shared__ float taps[CT_LP_H + 1];
    __shared__ float win[CT_LP_WIN];
    __shared__ int plist[32], tlist[32];                    // per group of eight: the output's place in the window (-1: none), its lane
    const int c = blockIdx.y, tid = threadIdx.x;
    const NfmChan& s = ch[c];
    if (!s.ct_on || (long)blockIdx.x * 256 >= s.n) return;
    const NfmBufs& b = bufs[c];
    const long i0 = (long)blockIdx.x * 256, i = i0 + tid;
    const int a = i < s.n ? b.aidx[i] : -1;
    const bool cand = ct_detector_sample(s.sc, i), det = cand && a >= 0;
    if (__syncthreads_count(det) == 0) return;              // no detector sample in this block
    const int a0 = b.blk_a[blockIdx.x], n_act = s.n_act;
    if (cand) { plist[tid >> 3] = det ? a - a0 + CT_LP_HIST : -1; tlist[tid >> 3] = tid; }
    for (int k = tid; k <= CT_LP_H; k += 256) taps[k] = tab[s.bp_off + NFM_TAB_LP + k];
    for (int j = tid; j < NFM_OUT_WIN; j += 256) {
        const long idx = (long)a0 - CT_LP_HIST + j;
        win[j + (j >> 3)] = idx < n_act ? am_stream_at(b.lhist, CT_LP_HIST, (const float*)b.xl, idx) : 0.0f;
    }
    __syncthreads();
    if (tid >= 32) return;
    const int p = plist[tid];
    if (p < 0) return;
    // Lowpass::filter walks its ring as Bandpass::filter does
    b.ctl[i0 + tlist[tid]] = am_bandpass(taps, [&](int k) { const int q = p - k; return win[q + (q >> 3)]; });
}

// ---- 3. one workgroup per channel
__global__ __launch_bounds__(256)
void nfm_ct_detect_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs, const float* __restrict__ tab)
{
    __shared__ int slot[4];
    __shared__ int2 slot2[4];
    __shared__ float pw[CT_GROUPS][CT_TONES];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    NfmChan& s = ch[c];
    if (!s.ct_on) return;
    const NfmBufs b = bufs[c];
    const int n = s.n, N = s.ct_n, sc0 = s.sc, fill0 = s.ct_fill, sel = s.ct_sel, n_act_a = s.n_act_a;
    const bool mute = s.mute != 0;

    // (a) compaction C: the detector's inputs and where they sit; the events of closed samples
    int nd = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i0 = base + tid * 4;
        bool det[4];
        int loc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            det[k] = i0 + k < n && b.aidx_a[i0 + k] >= 0 && ct_detector_sample(sc0, i0 + k);
            loc += det[k];
        }
        int d = nd + wg_scan_incl(WgCount{}, loc, lane, w, slot) - loc;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                b.ev[i0 + k] = ct_closed_event(b.aidx_a[i0 + k] >= 0, mute);
                if (det[k]) { b.cs[d] = b.ctl[i0 + k]; b.cpos[d] = i0 + k; d++; }
            }
        }
        nd += wg_total(WgCount{}, slot);
        __syncthreads();                                    // slot is rewritten by the next trip; cs, cpos and ev are read below
    }

    // (b) Goertzel: 32 tones of 8 blocks per trip.  Block 0 goes on from the carried u0, u1; a block that ends in this feed
    // leaves its event at its last member's sample; the one that does not leaves u0, u1 and the fill
    const int tone = tid & (CT_TONES - 1), grp = tid / CT_TONES;
    const float coef = tab[s.bp_off + NFM_TAB_COEF + tone];
    const float cu0 = s.ct_u0[tone], cu1 = s.ct_u1[tone];
    const int nb = ct_blocks_touched(fill0, nd, N), nbc = ct_blocks_done(fill0, nd, N);
    __syncthreads();                                        // every lane has the carried state before one of them rewrites it
    for (int b0 = 0; b0 < nb; b0 += CT_GROUPS) {
        const int blk = b0 + grp;
        const bool done = blk < nbc;
        if (blk < nb) {
            float u0 = blk == 0 ? cu0 : 0.0f, u1 = blk == 0 ? cu1 : 0.0f;
            const long end = ct_block_end(fill0, blk, N), hi = end < nd ? end : (long)nd;
            for (long d = ct_block_first(fill0, blk, N); d < hi; d++) ct_feedback(b.cs[d], coef, u0, u1);
            if (done) {
                const float p = ct_power(coef, u0, u1);
                pw[grp][tone] = p;
                if (blk == nbc - 1) s.ct_power[tone] = p;
            } else {
                s.ct_u0[tone] = u0; s.ct_u1[tone] = u1;
            }
        }
        __syncthreads();
        if (done && tone == 0) {
            int mi;
            const bool detected = ct_evaluate(pw[grp], &mi);
            b.cblk[blk] = mi;
            // a tone is detected only with a power above 0 (the powers are sums of squares up to rounding): mi >= 0 then
            b.ev[b.cpos[ct_block_end(fill0, blk, N) - 1]] = detected ? mi + 1 : 0;
            if (blk == nbc - 1) s.ct_detected = detected ? 1 : 0;
        }
        __syncthreads();                                    // pw is rewritten by the next trip; ev is read below
    }
    if (nbc > 0 && (fill0 + nd) % N == 0 && tid < CT_TONES) { s.ct_u0[tid] = 0.0f; s.ct_u1[tid] = 0.0f; }     // feedForward's reset

    // (c) m_ctcssIndex after every sample, the samples that pass the tone test (B) and their Bandpass inputs, the changes
    int index = s.ct_index, n_b = 0, n_ev = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i0 = base + tid * 4;
        int e[4], a[4], m = -1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            e[k] = -1; a[k] = -1;
            if (i0 + k < n) { e[k] = b.ev[i0 + k]; a[k] = b.aidx_a[i0 + k]; }
            m = ct_last_compose(m, e[k]);
        }
        int cur = ct_last_apply(wg_scan(CtLastOps{}, m, lane, w, slot), index);
        bool pass[4], chg[4];
        int idx[4];
        int2 loc = make_int2(0, 0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            chg[k] = e[k] >= 0 && e[k] != cur;
            cur = ct_last_apply(e[k], cur);
            idx[k] = cur;
            pass[k] = a[k] >= 0 && !ct_mismatch(sel, cur);
            loc.x += pass[k]; loc.y += chg[k];
        }
        const int2 inc = wg_scan_incl(WgCount2{}, loc, lane, w, slot2);
        int b_ex = n_b + inc.x - loc.x, e_ex = n_ev + inc.y - loc.y;
        if (lane == 0 && i0 < n) b.blk_a[i0 >> 8] = b_ex;   // i0 is a multiple of 256 here
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                b.aidx[i0 + k] = pass[k] ? b_ex : -1;
                if (pass[k]) b.x[b_ex++] = b.xa[a[k]];
                if (chg[k]) { b.ev_at[e_ex] = i0 + k; b.ev_idx[e_ex] = idx[k]; e_ex++; }
            }
        }
        index = ct_last_apply(wg_total(CtLastOps{}, slot), index);
        const int2 tot = wg_total(WgCount2{}, slot2);
        n_b += tot.x; n_ev += tot.y;
        __syncthreads();                                    // slot / slot2 are rewritten by the next trip
    }

    // (d) carry
    for (int i = tid; i < CT_LP_HIST; i += 256) b.lhist_next[i] = am_hist_next(b.lhist, CT_LP_HIST, (const float*)b.xl, n_act_a, i);
    if (tid == 0) {
        s.n_act = n_b;
        s.n_ev = n_ev;
        s.ct_index = index;
        s.ct_changes += n_ev;
        s.ct_blocks += nbc;
        s.ct_fill = (fill0 + nd) % N;
        s.sc = ct_count_after(sc0, n);
        for (int k = nbc - 1; k >= 0; k--) if (b.cblk[k] >= 0) { s.ct_max_index = b.cblk[k]; break; }      // the last block that has a maximum
    }
}

} // namespace sdrx
