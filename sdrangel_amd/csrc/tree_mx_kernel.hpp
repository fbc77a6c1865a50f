// The bank's lean kernel: a pass whose every level runs on the matrix cores (the default plans, at most MX_MAX_LEVELS levels).
// Same skeleton and the same arithmetic as tree_kernel<true> (tree_kernel.hpp: root fill, array histories, hb_mfma.hpp tiles,
// packed int16 epilogue), without the dot2 engine and its node / sink table copies, and with the jobs lowered by chan_lower.cpp:
// one 8-dword descriptor per job, every LDS address a base plus a compile-time multiple of the level's pitch, so the lane adds its
// share once per base and the ds_read / ds_write immediate offsets do the rest.  The level index is a template parameter (it
// fixes the pitches), and so is the job's epilogue class: a wave's job pair runs a body with no branch it does not need.
// What is the same for every lane of a chunk is decided on the scalar side or at compile time: the array lengths are constants of
// the level, the root arms hang off one lowered base (TkLRoot), and a job whose 256 outputs lie inside the feed's range stores them
// without a per-lane compare.
// The 16-dword histories of the arrays (TkArray: slot -> head of the window, tail of the window -> slot, once per chunk) are not a
// walk of the whole workgroup at the head of a level, as in tree_kernel.hpp: the wave that writes an array's tail copies both ways
// itself, right behind its stores (hist below; chan_lower.cpp marks the jobs and names the slots).
// Bit for bit what tree_kernel<true> computes: the biased odd arms and their zero history, the wrap-negated alternating copies,
// the int16 stores, the sink ranges of ragged feeds are all the same code.
#pragma once
#include "hb_common.hpp"
#include "hb_mfma.hpp"
#include "tree_layout.hpp"
#include "chan_lower.hpp"

namespace sdrx {

__device__ __forceinline__ int mx_div_pow2_trunc(int v, int n)
{
    return (v + ((v >> 31) & ((1 << n) - 1))) >> n;     // s.m_real /= (1 << n) (downchannelizer.cpp:80)
}

__global__ __launch_bounds__(TK_THREADS, 4)
void tree_mx_kernel(const TkSubtree* __restrict__ subtrees, const TkArray* __restrict__ arrays, const TkStream* __restrict__ streams,
                    const TkSink* __restrict__ sinks, const TkLJob* __restrict__ ljobs, const TkLRoot* __restrict__ lroots)
{
    constexpr int C = TK_CHUNK, NT = TK_THREADS, LPT = C / 4 / NT;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];

    const TkStream sp = streams[blockIdx.y];
    const long first = sp.c_first + (long)blockIdx.x * sp.cps;
    if (first > sp.c_last) return;
    long last = first + sp.cps - 1; if (last > sp.c_last) last = sp.c_last;
    const TkSubtree& st = subtrees[sp.subtree];
    const int tid = threadIdx.x;

    for (int i = tid; i < st.lds_dwords; i += NT) lds[i] = 0;
    __syncthreads();
    // odd arms an MFMA level reads carry 0x0080 in every int16 (hb_mfma.hpp): so does their zero history
    for (int i = tid; i < st.n_arrays * 16; i += NT) {
        const TkArray a = arrays[st.array_base + (i >> 4)];
        if (a.bias) lds[a.store + (i & 15)] = HBM_BIAS2;
    }
    typedef HbMfmaTaps<48, false> Taps;
    Taps taps;
    const int lane = tid & 63, n16 = lane & 15, g4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    taps.init(lane);
    const uint32_t root_xm = st.root_xm;
    // pinned in registers, as in tree_kernel.hpp (the compiler re-loads them from the descriptor inside the loops otherwise)
    int n_levels = st.n_levels, store_base = st.store_base, root_base = lroots[sp.subtree].base, root_kinds = lroots[sp.subtree].kinds;
    asm volatile("" : "+s"(n_levels), "+s"(store_base), "+s"(root_base), "+s"(root_kinds));

    uint4 pre[LPT];
    auto fetch = [&](long chunk, const int tid) {
        const long c0 = chunk * C;
        if (c0 >= sp.t_old && c0 + C <= sp.t_new) {
            typedef uint32_t u4v __attribute__((ext_vector_type(4)));
            typedef const u4v __attribute__((address_space(1))) gq4;
            gq4* src = (gq4*)reinterpret_cast<const u4v*>(sp.in + (c0 - sp.t_old));
#pragma unroll
            for (int j = 0; j < LPT; j++) { const u4v v = src[j * NT + tid]; pre[j] = make_uint4(v[0], v[1], v[2], v[3]); }
            return;
        }
#pragma unroll
        for (int j = 0; j < LPT; j++) {
            const long p0 = chunk * C + 4 * (j * NT + tid);
            if (p0 >= sp.t_old && p0 + 4 <= sp.t_new) {
                pre[j] = *reinterpret_cast<const uint4*>(sp.in + (p0 - sp.t_old));
            } else {
                uint32_t v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const long p = p0 + e;
                    v[e] = p < sp.t_old ? sp.hist[p - (sp.t_old - sp.hist_len)] : (p < sp.t_new ? sp.in[p - sp.t_old] : 0u);
                }
                pre[j] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                       // vmcnt(0) only (tree_kernel.hpp)
    };
    fetch(first - st.warm, tid);
    __syncthreads();

    typedef int s8i __attribute__((ext_vector_type(8)));
    typedef int s16i __attribute__((ext_vector_type(16)));
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const v4i bias = { Taps::BIAS, Taps::BIAS, Taps::BIAS, Taps::BIAS };
    const char* ldsb = reinterpret_cast<const char*>(lds);
    char* ldsw = reinterpret_cast<char*>(lds);
    const int wl = 32 * n16 + 16 * g4, cl = 32 * n16 + 8 * g4, pl = 16 * n16 + 4 * g4;      // the lane's byte offsets
    constexpr uint32_t PLAIN = 0x00010001u, ALT = 0x0001ffffu;     // (+1, +1) / (-1, +1): the low half wraps like (FixReal) -x
    auto padd = [](uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, (us2)(__builtin_bit_cast(us2, a) + __builtin_bit_cast(us2, b))); };
    auto psub = [](uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, (us2)(__builtin_bit_cast(us2, a) - __builtin_bit_cast(us2, b))); };
    auto pmul = [](uint32_t a, uint32_t m) { return __builtin_bit_cast(uint32_t, (us2)(__builtin_bit_cast(us2, a) * __builtin_bit_cast(us2, m))); };

    // The histories of `n` arrays (4 .. 12) that lie back to back, P bytes each, the first at byte `head`, their slots from byte
    // `slot` on, made by the one wave that has just stored their last 16 dwords: the slots (the previous chunk's tails) go in front
    // of the windows, the new tails into the slots.  Lane = 16 * array + dword, four arrays per round, every further round an
    // immediate offset.  The LDS serves one wave's operations in order: the tails read are the ones just stored, a slot is read
    // before it is written, and neither needs a barrier.  Nobody else touches these heads before the barrier that ends the phase
    // (their readers run one level down), nor these slots at all.
    auto hist = [&](auto Pc, const int head, const int slot, const int n) {
        constexpr int P = decltype(Pc)::value;
        static_assert(9 * P < 65536, "ds_read / ds_write immediate offset");
        int ln = threadIdx.x & 63;
        asm volatile("" : "+v"(ln));                                   // opaque: no address of this leaves the branch it is in
        const int g = ln >> 4;
        char* w = ldsw + head + __mul24(g, P) + 4 * (ln & 15);
        char* s = ldsw + slot + 4 * ln;
        auto round = [&](auto Rc) {
            constexpr int R = decltype(Rc)::value;
            const uint32_t h = *reinterpret_cast<const uint32_t*>(s + 256 * R), t = *reinterpret_cast<const uint32_t*>(w + (4 * R + 1) * P - 64);
            *reinterpret_cast<uint32_t*>(w + 4 * R * P) = h;
            *reinterpret_cast<uint32_t*>(s + 256 * R) = t;
        };
        round(std::integral_constant<int, 0>{});
        if (n > 4) {
            if (g < n - 4) round(std::integral_constant<int, 1>{});
            if (n > 8 && g < n - 8) round(std::integral_constant<int, 2>{});
        }
    };

    for (long chunk = first - st.warm; chunk <= last; ++chunk) {
        // the thread index, opaque inside the chunk loop: the compiler would otherwise hoist every per-lane address of the root fill
        // and the boundary fetch out of the loop, and spill them
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        // ---- stream samples -> root arms (TkLRoot: E_I E_Q [O_I O_Q] [A_I A_Q], one pitch apart): one address per lane and
        // chunk, every store an immediate offset from it; one body per set of kinds.  A root is an inner node, so it has at least
        // one odd kind (chan_lower.cpp refuses a root with none): E+O, E+A or E+O+A.
        {
            char* p = ldsw + root_base + 4 * (HIST / 2 + tid);
            auto fill = [&](auto Kc) {
                constexpr int K = decltype(Kc)::value, P0 = mx_pitch(0), AT = (K & MX_ROOT_O) ? 4 * P0 : 2 * P0;
                static_assert(AT + P0 + 4 * (LPT - 1) * NT < 65536, "ds_write immediate offset");
#pragma unroll
                for (int j = 0; j < LPT; j++) {
                    const uint4 v = pre[j];
                    const uint32_t oI = __builtin_amdgcn_perm(v.w, v.y, 0x05040100u);
                    const uint32_t oQ = __builtin_amdgcn_perm(v.w, v.y, 0x07060302u);
                    char* pj = p + 4 * j * NT;
                    *reinterpret_cast<uint32_t*>(pj) = __builtin_amdgcn_perm(v.z, v.x, 0x05040100u);
                    *reinterpret_cast<uint32_t*>(pj + P0) = __builtin_amdgcn_perm(v.z, v.x, 0x07060302u);
                    if constexpr (K & MX_ROOT_O) {
                        *reinterpret_cast<uint32_t*>(pj + 2 * P0) = oI ^ root_xm; *reinterpret_cast<uint32_t*>(pj + 3 * P0) = oQ ^ root_xm;
                    }
                    if constexpr (K & MX_ROOT_A) {
                        *reinterpret_cast<uint32_t*>(pj + AT) = pmul(oI, ALT) ^ root_xm; *reinterpret_cast<uint32_t*>(pj + AT + P0) = pmul(oQ, ALT) ^ root_xm;
                    }
                }
            };
            if (root_kinds == (MX_ROOT_O | MX_ROOT_A)) fill(std::integral_constant<int, MX_ROOT_O | MX_ROOT_A>{});
            else if (root_kinds == MX_ROOT_O) fill(std::integral_constant<int, MX_ROOT_O>{});
            else fill(std::integral_constant<int, MX_ROOT_A>{});
        }
        // the root arms' histories: the last wave's last stores above are the 16 tail dwords of every arm
        static_assert(NT >= 64 && (LPT - 1) * NT + NT - 16 == C / 4 - 16, "the tail of a root arm is stored by the last 16 lanes of the fill");
        {
            // opaque: hoisted out of the chunk loop, the wave test and the array count become lane masks held across it (spills)
            int w = wv, kinds = root_kinds;
            asm volatile("" : "+s"(w), "+s"(kinds));
            if (w == NT / 64 - 1) hist(std::integral_constant<int, mx_pitch(0)>{}, root_base, 4 * store_base, mx_root_arrays(kinds));
        }
        if (chunk < last) fetch(chunk + 1, tid);
        __syncthreads();

        const bool live = chunk >= first;
        // the level records, opaque to the compiler inside the chunk loop: with the level index a template parameter it would hoist
        // all four records out of the loop, and hold them across it (spills)
        int lv0 = 0;
        asm volatile("" : "+s"(lv0), "+s"(n_levels));
        // ---- one level, L = its index in the pass (compile time: the pitches of what it reads and writes)
        auto level = [&](auto Lc) {
            constexpr int L = decltype(Lc)::value;
            constexpr int PI = mx_pitch(L), PO = mx_pitch(L + 1);
            const s16i rec = *(const s16i __attribute__((address_space(4)))*)reinterpret_cast<const int*>(&st.lv[L + lv0]);
            const int nout = rec[3], mjob_base = rec[9], n_mjobs = rec[10];
            const uint32_t xm = (uint32_t)rec[11];
            struct JobIn { v4i bI0, bI1, bQ0, bQ1; uint2 cI01, cQ01; uint32_t cI2, cQ2; };
            // the job's operands: two bases, everything else immediate offsets (the centre taps of a lower/upper parent come from
            // the OTHER component's even arm: E[1] feeds I)
            auto load = [&](const s8i d, JobIn& r, auto Cc) {
                const char* pb = ldsb + d[0] + wl;
                r.bI0 = *reinterpret_cast<const v4i*>(__builtin_assume_aligned(pb, 16));
                r.bI1 = *reinterpret_cast<const v4i*>(__builtin_assume_aligned(pb + 64, 16));
                r.bQ0 = *reinterpret_cast<const v4i*>(__builtin_assume_aligned(pb + PI, 16));
                r.bQ1 = *reinterpret_cast<const v4i*>(__builtin_assume_aligned(pb + PI + 64, 16));
                const char* pc = ldsb + d[1] + cl;
                const char *pI, *pQ;
                if constexpr (decltype(Cc)::value == MX_FAST) { pI = pc + PI; pQ = pc; }
                else { const bool lu = d[7] & MX_LU_BIT; pI = lu ? pc + PI : pc; pQ = lu ? pc : pc + PI; }
                r.cI01 = *reinterpret_cast<const uint2*>(__builtin_assume_aligned(pI, 8));
                r.cI2 = *reinterpret_cast<const uint32_t*>(pI + 8);
                r.cQ01 = *reinterpret_cast<const uint2*>(__builtin_assume_aligned(pQ, 8));
                r.cQ2 = *reinterpret_cast<const uint32_t*>(pQ + 8);
            };
            auto st32 = [&](char* p, int off, uint32_t v) { *reinterpret_cast<uint32_t*>(p + off) = v; };
            // a child's outputs: arms (flags f, see TkMOut) at its base, then its sink list (MX_SINK only)
            auto child = [&](auto Sk, const uint32_t eI, const uint32_t oI, const uint32_t eQ, const uint32_t oQ, const int base, const int f,
                             const int sink, const long job0) {
                constexpr bool SINK = decltype(Sk)::value;
                if (f) {
                    char* p = ldsw + base + pl;
                    const uint32_t m = (f & 2) ? PLAIN : ALT;
                    st32(p, 0, eI); st32(p, PO, eQ);
                    st32(p, 2 * PO, pmul(oI, m) ^ xm); st32(p, 3 * PO, pmul(oQ, m) ^ xm);
                    if (f == 7) { st32(p, 4 * PO, pmul(oI, ALT) ^ xm); st32(p, 5 * PO, pmul(oQ, ALT) ^ xm); }
                }
                if constexpr (SINK) {
                    if (live) {
                        typedef const s8i __attribute__((address_space(4))) cs8;
                        for (int si = sink; si >= 0; ) {
                            const s8i sr = *(cs8*)reinterpret_cast<const int*>(sinks + si);
                            const long ptr0 = ((long)sr[1] << 32) | (uint32_t)sr[0];
                            const long lo = ((long)sr[3] << 32) | (uint32_t)sr[2], hi = ((long)sr[5] << 32) | (uint32_t)sr[4];
                            const int shift = sr[6];
                            uint32_t w[4];
                            if (shift) {
                                w[0] = pack_iq(mx_div_pow2_trunc((int)(int16_t)eI, shift), mx_div_pow2_trunc((int)(int16_t)eQ, shift));
                                w[1] = pack_iq(mx_div_pow2_trunc((int)(int16_t)oI, shift), mx_div_pow2_trunc((int)(int16_t)oQ, shift));
                                w[2] = pack_iq(mx_div_pow2_trunc((int)eI >> 16, shift), mx_div_pow2_trunc((int)eQ >> 16, shift));
                                w[3] = pack_iq(mx_div_pow2_trunc((int)oI >> 16, shift), mx_div_pow2_trunc((int)oQ >> 16, shift));
                            } else {
                                w[0] = __builtin_amdgcn_perm(eQ, eI, 0x05040100u); w[1] = __builtin_amdgcn_perm(oQ, oI, 0x05040100u);
                                w[2] = __builtin_amdgcn_perm(eQ, eI, 0x07060302u); w[3] = __builtin_amdgcn_perm(oQ, oI, 0x07060302u);
                            }
                            typedef uint32_t __attribute__((address_space(1))) gu32;
                            typedef uint32_t u4a __attribute__((ext_vector_type(4), aligned(4)));
                            // The job's 256 outputs [job0, job0 + 256) against [lo, hi), on the scalar side: every job but those of
                            // a feed's first and last chunk lies wholly inside, and stores 16 bytes per lane at one scalar base
                            // plus the lane's 32-bit offset, no compare.  (The sign of both differences in one 32-bit register:
                            // there is no scalar 64-bit signed compare.)
                            int inside = (int)((uint64_t)((job0 - lo) | (hi - 256 - job0)) >> 32);
                            asm("" : "+s"(inside));
                            if (inside >= 0) {
                                typedef char __attribute__((address_space(1))) gchar;
                                gchar* row = (gchar*)(reinterpret_cast<uint32_t*>(ptr0) + job0);
                                *(u4a __attribute__((address_space(1)))*)(row + (uint32_t)(4 * pl)) = u4a{ w[0], w[1], w[2], w[3] };
                            } else {
                                const long abs0 = job0 + pl;
                                gu32* dst = (gu32*)(reinterpret_cast<uint32_t*>(ptr0) + abs0);
                                const long rel = abs0 - lo, span = hi - lo;
                                if (rel >= 0 && rel + 4 <= span) {
                                    *(u4a __attribute__((address_space(1)))*)dst = u4a{ w[0], w[1], w[2], w[3] };
                                } else if (rel > -4 && rel < span) {
#pragma unroll
                                    for (int i = 0; i < 4; i++) if (rel + i >= 0 && rel + i < span) dst[i] = w[i];
                                }
                            }
                            si = sr[7];
                        }
                    }
                }
            };
            // the epilogue of class CLS (chan_lower.hpp)
            auto finish = [&](auto Cc, const JobIn& r, const v4i SI, const v4i SQ, const s8i d) {
                constexpr int CLS = decltype(Cc)::value;
                // the low 16 bits of (a >> 11) and of (b >> 11) in one dword: the second shift is an SDWA write to WORD_1 that preserves
                // the rest (dst_unused:UNUSED_PRESERVE).  On gfx950 a VALU consumer of an SDWA dst_sel write needs one wait state, and the
                // compiler's hazard recognizer does not see inside inline asm: the s_nop 0 in the string carries it, whatever the
                // schedule.  The pack in plain C++ (two shifts and a v_bfi_b32, hazards owned by the compiler) needs one more live
                // register per pack and spilled 24 VGPRs to scratch here (experiments/README.md), so it was not kept.
                auto shpack = [](int a, int b) {
                    uint32_t v = (uint32_t)(a >> (HB_SHIFT - 1));
                    asm("v_ashrrev_i32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\ts_nop 0" : "+v"(v) : "s"(HB_SHIFT - 1), "v"(b));
                    return v;
                };
                const uint32_t sI02 = shpack(SI[0], SI[2]), sI13 = shpack(SI[1], SI[3]);
                const uint32_t sQ02 = shpack(SQ[0], SQ[2]), sQ13 = shpack(SQ[1], SQ[3]);
                const uint32_t cI02 = __builtin_amdgcn_perm(r.cI01.y, r.cI01.x, 0x07060302u), cI13 = __builtin_amdgcn_perm(r.cI2, r.cI01.y, 0x05040100u);
                const uint32_t cQ02 = __builtin_amdgcn_perm(r.cQ01.y, r.cQ01.x, 0x07060302u), cQ13 = __builtin_amdgcn_perm(r.cQ2, r.cQ01.y, 0x05040100u);
                const int meta = d[7], f0 = (meta >> 4) & 15, f1 = (meta >> 8) & 15;
                if constexpr (CLS == MX_FAST) {
                    // both children have even arms and one odd kind at 2 PO: eight stores, no branch
                    const uint32_t ma = (f0 & 2) ? PLAIN : ALT, mb = (f1 & 2) ? PLAIN : ALT;
                    auto st4 = [&](const int base, uint32_t eI, uint32_t eQ, uint32_t oI, uint32_t oQ, uint32_t m) {
                        char* p = ldsw + base + pl;
                        st32(p, 0, eI); st32(p, PO, eQ); st32(p, 2 * PO, pmul(oI, m) ^ xm); st32(p, 3 * PO, pmul(oQ, m) ^ xm);
                    };
                    st4(d[2], padd(sI02, cI02), psub(sQ02, cQ02), psub(sI13, cI13), padd(sQ13, cQ13), ma);
                    st4(d[3], psub(sI02, cI02), padd(sQ02, cQ02), padd(sI13, cI13), psub(sQ13, cQ13), mb);
                } else {
                    const std::integral_constant<bool, CLS == MX_SINK> Sk;
                    const long job0 = CLS == MX_SINK ? chunk * nout + d[6] : 0;       // first output of the job: wave-uniform
                    // child 0: the centre stage (every centre tap added), or the lower half: k even -> (+im, -re), k odd -> (-im, +re);
                    // child 1: the upper half, the negation (inthalfbandfiltereo.h:158-206, 357-405).  The sign that differs between
                    // centre and lower is one packed multiply.
                    const uint32_t sg = (meta & MX_LU_BIT) ? 0xffffffffu : PLAIN;
                    if (f0 | (d[4] >= 0)) {
                        const uint32_t nI13 = pmul(cI13, sg), nQ02 = pmul(cQ02, sg);
                        child(Sk, padd(sI02, cI02), padd(sI13, nI13), padd(sQ02, nQ02), padd(sQ13, cQ13), d[2], f0, d[4], job0);
                    }
                    if (f1 | (d[5] >= 0)) child(Sk, psub(sI02, cI02), padd(sI13, cI13), padd(sQ02, cQ02), psub(sQ13, cQ13), d[3], f1, d[5], job0);
                }
            };
            // two jobs of one class: both jobs' loads, then the MFMAs, then the epilogues (tree_kernel.hpp); or one job
            auto pair = [&](auto Cc, const s8i d0, const s8i d1) {
                JobIn r0, r1;
                __builtin_amdgcn_s_setprio(2);
                load(d0, r0, Cc); load(d1, r1, Cc);
                __builtin_amdgcn_sched_barrier(0);
                const v4i SI0 = taps.tile(r0.bI0, r0.bI1, bias), SQ0 = taps.tile(r0.bQ0, r0.bQ1, bias);
                const v4i SI1 = taps.tile(r1.bI0, r1.bI1, bias), SQ1 = taps.tile(r1.bQ0, r1.bQ1, bias);
                __builtin_amdgcn_s_setprio(0);
                finish(Cc, r0, SI0, SQ0, d0);
                finish(Cc, r1, SI1, SQ1, d1);
            };
            auto single = [&](auto Cc, const s8i d0) {
                JobIn r0;
                load(d0, r0, Cc);
                const v4i SI0 = taps.tile(r0.bI0, r0.bI1, bias), SQ0 = taps.tile(r0.bQ0, r0.bQ1, bias);
                finish(Cc, r0, SI0, SQ0, d0);
            };
            // a tail job (MX_TAIL_BIT) has just completed its children's arrays for this chunk: their histories, by this wave
            auto tail = [&](const s8i d) {
                const uint32_t meta = (uint32_t)d[7];
                if (meta & MX_TAIL_BIT)
                    hist(std::integral_constant<int, PO>{}, ((meta & 0xf0) ? d[2] : d[3]) + 256 - PO, 4 * store_base + 64 * (int)((meta >> MX_SLOT_SHIFT) & MX_SLOT_MASK),
                         (int)(meta >> MX_CNT_SHIFT));
            };
            typedef std::integral_constant<int, MX_FAST> KF;
            typedef std::integral_constant<int, MX_ARMS> KA;
            typedef std::integral_constant<int, MX_SINK> KS;
            const int per = (n_mjobs + NT / 64 - 1) / (NT / 64);
            const int t0 = wv * per, t1 = t0 + per < n_mjobs ? t0 + per : n_mjobs;
            typedef const s8i __attribute__((address_space(4))) cs8j;
            for (int tt = t0; tt < t1; ) {
                const s8i d0 = *(cs8j*)reinterpret_cast<const int*>(ljobs + mjob_base + tt);
                const int c0 = d0[7] & 15;
                if (tt + 1 < t1) {
                    const s8i d1 = *(cs8j*)reinterpret_cast<const int*>(ljobs + mjob_base + tt + 1);
                    if ((d1[7] & 15) == c0) {                                      // jobs are sorted by class: the common case
                        if (c0 == MX_FAST) pair(KF{}, d0, d1);
                        else if (c0 == MX_ARMS) pair(KA{}, d0, d1);
                        else pair(KS{}, d0, d1);
                        tail(d0); tail(d1);
                        tt += 2;
                        continue;
                    }
                }
                if (c0 == MX_FAST) single(KF{}, d0);
                else if (c0 == MX_ARMS) single(KA{}, d0);
                else single(KS{}, d0);
                tail(d0);
                tt += 1;
            }
            __syncthreads();
        };
        level(std::integral_constant<int, 0>{});
        if (n_levels > 1) level(std::integral_constant<int, 1>{});
        if (n_levels > 2) level(std::integral_constant<int, 2>{});
        if (n_levels > 3) level(std::integral_constant<int, 3>{});
    }
}

} // namespace sdrx
