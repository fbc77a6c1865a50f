// Half-band odd-arm FIR on the gfx950 matrix cores: v_mfma_i32_16x16x64_i8 on PACKED int16 polyphase arms.
//
// VERDICT round 2 ruled the matrix cores into the product path (the half-band FIR is a banded-Toeplitz contraction).
// This is the primitive both product kernels use (tree_kernel.hpp: DownChannelizer stages, inthalfbandfiltereo.h:792-830;
// decim_fast_kernel.hpp: Decimators stages whose input is int16, inthalfbandfiltereo.h:832-870).
//
// Exact integer arithmetic, no range contract on the data:
//   * the odd arm sits in LDS as packed int16 (the layout the dot2 kernels already use) with 0x0080 XORed into every
//     entry: byte 0 of an entry read as SIGNED is then (x & 255) - 128, byte 1 is x >> 8, so  x = 256 b1 + b0 + 128;
//   * every tap splits as h = 256 hh + hl with hl in [-128, 127] (|hh| <= 5: only the 8 central taps have hh != 0);
//   * sum_j h_j x_j = 65536 P1 + 256 P2 + P3 + 128 sum_j h_j  with  P1 = sum hh b1,  P2 = sum (hl b1 + hh b0),
//     P3 = sum hl b0  -- three int32 accumulators; |sum| < 2^31 for any int16 data (sum|h| + 2048 = 6850), and the
//     combination is plain modulo-2^32 arithmetic like the reference's qint32 accumulator.
//
// Mapping: a tile = 16 columns x 16 rows; column n = one block of 16 consecutive outputs of one arm, row m = output
// m of the block.  B[k][n] = the block's window, read straight from the packed arm: lane (n, g) loads ONE aligned
// ds_read_b128 per K-step = entries w = 32 s + 8 g .. + 7 (both bytes of each), window entry w = o[16 blk - T + w].
// A[m][k] = the tap that entry w carries for output m, j = m + T - w, as limbs at the byte positions of B -- a banded
// Toeplitz operand built once per wave (registers).  Two K-steps (64 entries) cover the 15 + T <= 47 entries a block
// needs.  The D layout (lane (n, g) holds outputs 4g .. 4g+3 of block n) hands each lane two even- and two odd-indexed
// outputs = one packed dword for each arm of the next stage.
// The k <-> (lane group, byte) assignment of the hardware does not matter: A and B use the same one.
//
// CTR (centre-mode decimator stages): entries 48..63 of the window carry no odd-arm tap (j < 0 for every output), so the lanes of
// groups g = 2, 3 load the EVEN arm into the second K-step instead -- slot c = 8 (g - 2) + 2 q + u holds e[16 blk + 16 + c], biased by
// 0x0080 like the odd arm -- and the operand puts the centre tap 2^11 = 256 * 8 + 0 (hh = 8, hl = 0) at c = m + 1; slot 0 (c = m + 1
// would be 16 for m = 15) is overwritten by the caller with e[16 blk + 32], output 15's centre sample, and carries its tap.  The bias
// gains 128 * 2^11 per output.  The limb bound still holds with the extra term: over the 32 odd taps and the centre tap, sum|hh| = 26 and
// sum|hl| = 1262, so |P1| <= 128 * 26, |P2| <= 128 * 1288 and |P3| <= 128 * 1262 (plus the bias, < 2^19) -- far inside int32 -- and
// the combination is the same modulo-2^32 arithmetic.
#pragma once
#include "hb_common.hpp"

namespace sdrx {

typedef int v4i __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int tap_lo8(int h) { int l = ((h % 256) + 256) % 256; return l >= 128 ? l - 256 : l; }
__host__ __device__ constexpr int tap_hi8(int h) { return (h - tap_lo8(h)) / 256; }

template<int ORDER> __host__ __device__ constexpr int hb_tap_sum()
{
    int s = 0;
    for (int j = 0; j < ORDER / 2; j++) s += hb_tap<ORDER>(j);
    return s;
}

// ALT: the odd arm is multiplied by (-1)^(index + 1) (the inf/sup rotations of the int32 flavour, folded into the taps;
// exact modulo 2^32).  The channelizer's int16 flavour stores explicitly wrap-negated copies instead and uses ALT = false.
template<int ORDER, bool ALT, bool CTR = false>
struct HbMfmaTaps {
    static constexpr int T = ORDER / 2;                 // taps of the odd-arm FIR; also the window's lead: entry w = o[16 blk - T + w]
    static constexpr bool P1_STEP2 = (ORDER == 64);     // order 48: the central taps only meet entries 9..31
    static constexpr int BIAS = ALT ? 0 : 128 * hb_tap_sum<ORDER>();   // alternating signs cancel (the taps are symmetric, T even)
    static_assert(T >= 15 && T <= 32, "the 64-lane tap table of init() holds j = -16 .. 47");
    static_assert(!CTR || (T == 32 && !ALT), "the centre tap takes window entries 48..63: order 64, plain taps");
    static constexpr int CBIAS = BIAS + (CTR ? 128 * (1 << (HB_SHIFT - 1)) : 0);   // accumulator start of a tile with the centre tap folded in
    v4i p1[2], p2[2], p3[2];

    // Every entry of the operand is ONE table value: lane (m, g), K-step s, entry 8 g + 2 q + u carries the tap j = (m - 8 g) + (T - 32 s - 2 q - u),
    // a per-lane base plus a compile-time offset.  The table (the tap's two limbs as 16 bits, zero outside 0 <= j < T) is built once, one
    // value per lane -- lane l holds j = l - 16, which covers every j any entry can ask for once j < -16 is clamped (those are zero) --
    // and the 16 entries are ds_bpermute reads of it (a select chain per ENTRY was 1250 instructions of prologue, half a sub-chunk's work,
    // in every workgroup of the short launches).
    __device__ __forceinline__ void init(int lane)
    {
        const int m = lane & 15, g = lane >> 4;
        const int jt = lane - 16;
        int h = 0;
#pragma unroll
        for (int t = 0; t < T; t++) if (t == jt) h = hb_tap<ORDER>(t);
        auto limbs = [](int hv) -> int {                                        // (hh & 255) << 8 | (hl & 255), h = 256 hh + hl, hl in [-128, 127]
            const int l = ((hv & 255) ^ 128) - 128;
            const int hh = (hv - l) >> 8;
            return (int)((((uint32_t)hh & 255u) << 8) | ((uint32_t)l & 255u));
        };
        const int tab = limbs(h), tabn = ALT ? limbs(-h) : tab;                  // ALT: entries with an even window index carry -h
        const int base = 4 * (m - 8 * g + 16);                                  // byte address of the lane that holds j = m - 8 g
#pragma unroll
        for (int s = 0; s < 2; s++) {
            uint32_t d1[4], d2[4], d3[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t x[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    int a = base + 4 * (T - 32 * s - 2 * q - u);
                    if (s == 1) a = a < 0 ? 0 : a;                              // j < -16: lane 0 holds a zero
                    x[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(a, u == 0 ? tabn : tab);   // window index parity = parity of u
                    if (CTR && s == 1 && g >= 2)                                // centre slot c = 8 (g - 2) + 2 q + u: tap 2^11 at c = (m + 1) mod 16
                        x[u] = (8 * (g - 2) + 2 * q + u) == ((m + 1) & 15) ? (uint32_t)(8 << 8) : 0u;
                }
                const uint32_t y = x[0] | (x[1] << 16);
                d3[q] = y & 0x00ff00ffu;                                        // hl
                d2[q] = __builtin_amdgcn_perm(y, y, 0x02030001u);               // hh | hl << 8
                d1[q] = y & 0xff00ff00u;                                        // hh << 8
            }
            p1[s] = v4i{ (int)d1[0], (int)d1[1], (int)d1[2], (int)d1[3] };
            p2[s] = v4i{ (int)d2[0], (int)d2[1], (int)d2[2], (int)d2[3] };
            p3[s] = v4i{ (int)d3[0], (int)d3[1], (int)d3[2], (int)d3[3] };
        }
    }

    // S[i] = sum_j h_j o[k - j] for the lane's four outputs k = 16 blk + 4 g + i; b0 / b1 = the two K-steps of the window
    __device__ __forceinline__ v4i tile(const v4i b0, const v4i b1, const v4i bias) const
    {
        const v4i z = { 0, 0, 0, 0 };
        v4i P3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p3[0], b0, bias, 0, 0, 0);
        v4i P2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p2[0], b0, z, 0, 0, 0);
        v4i P1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p1[0], b0, z, 0, 0, 0);
        P3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p3[1], b1, P3, 0, 0, 0);
        P2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p2[1], b1, P2, 0, 0, 0);
        if constexpr (P1_STEP2) P1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(p1[1], b1, P1, 0, 0, 0);
        // S = (P1 << 16) + (P2 << 8) + P3 as a Horner chain of two v_lshl_add_u32 (left alone the compiler makes it two shifts and
        // an add3: the combine is the largest VALU item of the stage)
        v4i S;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // (the empty asm only stops the re-association; an asm that READ the MFMA results itself would sit outside the
            // compiler's MFMA -> VALU hazard padding)
            uint32_t t = ((uint32_t)P1[i] << 8) + (uint32_t)P2[i];
            asm("" : "+v"(t));
            S[i] = (int)((t << 8) + (uint32_t)P3[i]);
        }
        return S;
    }
};

} // namespace sdrx
