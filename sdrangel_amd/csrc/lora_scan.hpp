// The part of LoRaDemod that is neither the front nor the two sliding FFTs (plugins/channelrx/demodlora/lorademod.cpp:94-252,
// lorabits.h): the stream-position arithmetic of the dechirp, and what happens at a fetch, every 64th decimator output, once the
// magnitudes and the two peaks are known -- finetune, the squelch, synch() and, when the squelch closes late enough, dumpRaw()
// with its whitening, de-interleaving and Hamming extraction.  Compiles for the host too (tests/lora_check.cpp), no HIP header
// needed.  On the device one lane of the walk's wave runs lora_fetch_step on the channel's LoraSynch in global memory.
//
// Why the sliding FFT itself is a walk and not a scan: bins' = (bins + z) * vrot is linear in bins, so n steps compose into
// bins * vrot^n + sum z_k vrot^(n-k), but that is another float expression than the reference's n rounded products, and the
// magnitudes feed strict comparisons.  The walk (lora_kernels.hpp) keeps the reference's order, step by step.
//
// Four places where the reference reads memory it never wrote, defined here as in tests/golden/lora_rec.cpp (include/sdrx.h):
// mov starts as zeros; mag[127] and rev[127] are 0; dumpRaw's text starts as zeros; the stream count is 64 bits wide.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LORA_HD __host__ __device__ __forceinline__
#else
#define LORA_HD inline
#endif

namespace sdrx {

constexpr int LORA_SPREAD = 256;            // SPREADFACTOR
constexpr int LORA_LEN = 128;               // LORA_SFFT_LEN
constexpr int LORA_DATA_BITS = 6;           // a fetch every 1 << 6 samples
constexpr float LORA_SQUELCH = 3.0f;        // LORA_SQUELCH, an int in the reference: negpeak * 3 converts it
constexpr int LORA_TEXT = 256;              // dumpRaw's text[256]: one slot per line
constexpr int LORA_LINE_FETCHES = 71;       // a dump needs m_time > 70: at most one line per 71 fetches

// m_angle after decimator output g (g = 0 is the first): m_chirp counts 1, 2, .. 255, 0, 1, .. and m_angle sums it mod 256.
// One whole period of m_chirp sums to 32640 = 128 mod 256, so with N = g + 1 = 256 q + r: angle = 128 q + r (r + 1) / 2 mod 256.
LORA_HD int lora_angle(long long g)
{
    const long long N = g + 1;
    const int q = (int)((N >> 8) & 1), r = (int)(N & 255);
    return (q * 128 + r * (r + 1) / 2) & (LORA_SPREAD - 1);
}

// 3 & (m_count >> 6) with the 64-bit count, m_count already incremented
LORA_HD int lora_movpoint(long long count) { return (int)((count >> LORA_DATA_BITS) & 3); }
LORA_HD bool lora_is_fetch(long long count) { return (count & ((1 << LORA_DATA_BITS) - 1)) == 0; }

// most lines a feed of n decimator outputs can end: a line needs 71 fetches since the last reset of m_time
LORA_HD long long lora_lines_bound(long long n) { return n / (LORA_LINE_FETCHES * 64) + 2; }

struct LoraSynch {                          // what detect's tail, synch and dumpRaw keep between fetches
    int time;                               // m_time
    int result;                             // m_result: the last value that was not negative
    short tune;                             // m_tune
    short pad;
    long long lines;                        // lines dumped since creation or reset
    short history[1024];
    short finetune[16];
};

LORA_HD short lora_to_gray(short num) { return (short)((num >> 1) ^ num); }

// prng6: the whitening sequence of the explicit mode, character - 48, as far as dumpRaw's 140 symbols reach
LORA_HD void lora_prng6(char* inout, int size)
{
    const unsigned char white[140] = {
        51, 31, 23, 23, 55, 7, 19, 29, 2, 13, 50, 5, 49, 15, 12, 48, 57, 11, 36, 2, 63, 54, 5, 58, 20, 17, 18, 13, 2, 20, 63, 33, 9, 59, 63,
        15, 56, 47, 34, 28, 33, 34, 4, 16, 42, 44, 48, 9, 58, 41, 44, 32, 40, 8, 9, 60, 24, 40, 8, 56, 47, 34, 45, 51, 47, 46, 16, 31, 18, 12,
        0, 48, 39, 0, 8, 57, 59, 15, 29, 55, 14, 52, 33, 42, 54, 3, 59, 62, 5, 26, 53, 5, 34, 13, 34, 4, 56, 43, 12, 32, 56, 9, 0, 24, 24, 56,
        9, 58, 11, 56, 10, 61, 35, 46, 15, 54, 10, 60, 33, 10, 23, 23, 11, 62, 37, 10, 50, 15, 39, 22, 37, 2, 0, 28, 54, 4, 16, 17, 15, 48 };
    const int n = size < 140 ? size : 140;
    for (int i = 0; i < n; i++) inout[i] = (char)(inout[i] ^ (char)white[i]);
}

// interleave6: whole blocks of six characters from inout[0] until `size` is covered -- the last block reads and writes up to
// five characters past inout[size - 1]
LORA_HD void lora_interleave6(char* inout, int size)
{
    for (int j = 0; j < size; j += 6) {
        char in[12];
        for (int i = 0; i < 6; i++) in[i] = in[i + 6] = inout[i + j];
        for (int i = 0; i < 6; i++) {
            short s = (short)((32 & in[2 + i]) | (16 & in[1 + i]) | (8 & in[3 + i]) | (4 & in[4 + i]) | (2 & in[5 + i]) | (1 & in[6 + i]));
            s = (short)((s << 3) | (s >> 3));
            s &= 63;
            s = (short)((s >> i) | (s << (6 - i)));
            inout[i + j] = (char)(s & 63);
        }
    }
}

// hamming6: the data bits of each block of six, and a 0 behind the last block
LORA_HD void lora_hamming6(char* c, int size)
{
    int i;
    for (i = 0; i < size; i++) {
        c[i] = (char)(((c[i] & 1) << 3) | ((c[i] & 2) << 0) | ((c[i] & 4) >> 0) | ((c[i] & 8) >> 3)); i++;
        c[i] = (char)(((c[i] & 1) << 2) | ((c[i] & 2) << 2) | ((c[i] & 4) >> 1) | ((c[i] & 8) >> 3)); i++;
        c[i] = (char)(((c[i] & 32) >> 2) | ((c[i] & 2) << 1) | ((c[i] & 4) >> 1) | ((c[i] & 8) >> 3)); i++;
        c[i] = (char)(((c[i] & 1) << 3) | ((c[i] & 2) << 1) | ((c[i] & 4) >> 1) | ((c[i] & 8) >> 3)); i++;
        c[i] = (char)(((c[i] & 1) << 3) | ((c[i] & 2) << 1) | ((c[i] & 4) >> 1) | ((c[i] & 16) >> 4)); i++;
        c[i] = (char)(((c[i] & 1) << 3) | ((c[i] & 2) << 1) | ((c[i] & 4) >> 2) | ((c[i] & 8) >> 2));
    }
    c[i] = 0;
}

// dumpRaw into one text slot of LORA_TEXT characters; the line is text + 1 up to the terminating 0.  Returns its length.
// `char` is signed in the reference's build: int8_t here.  text is zeroed first (the third definition above).
LORA_HD int lora_dump_raw(const LoraSynch& st, char* text)
{
    for (int i = 0; i < LORA_TEXT; i++) text[i] = 0;
    short max = (short)(st.time / 4 - 3);
    if (max > 140) max = 140;
    short j;
    for (j = 0; j < max; j++) {
        const short bin = (short)((st.history[(j + 1) * 4] + st.tune) & (LORA_LEN - 1));
        text[j] = (char)lora_to_gray((short)(bin >> 1));
    }
    lora_prng6(text, max);
    lora_interleave6(text, 6);
    lora_interleave6(text + 8, max);
    lora_hamming6(text, 6);
    lora_hamming6(text + 8, max);
    for (j = 0; j < max / 2; j++) {
        const int8_t v = (int8_t)(((int8_t)text[j * 2 + 1] << 4) | (0xf & (int8_t)text[j * 2 + 0]));
        text[j] = (v < 32 || v > 126) ? (char)0x5f : (char)v;
    }
    text[3] = text[2];
    text[2] = text[1];
    text[1] = text[0];
    text[j] = 0;
    return j - 1;
}

// synch(bin).  A dump goes to text_slots + LORA_TEXT * *n_lines and counts there; st.lines counts the stream's.  max_lines is
// how many slots there are: lora_lines_bound() of the feed at least, so the guard never holds a line back.
LORA_HD short lora_synch(LoraSynch& st, short bin, char* text_slots, int* n_lines, int max_lines)
{
    if (bin < 0) {
        if (st.time > 70 && *n_lines < max_lines) {
            lora_dump_raw(st, text_slots + (long long)LORA_TEXT * *n_lines);
            *n_lines += 1;
            st.lines += 1;
        }
        st.time = 0;
        return -1;
    }
    st.history[st.time] = bin;
    if (st.time > 12 && bin == st.history[st.time - 6] && bin == st.history[st.time - 12]) {
        st.tune = (short)(LORA_LEN - bin);
        short j = 0;
        for (short i = 0; i < 12; i++) j = (short)(j + st.finetune[15 & (st.time - i)]);
        if (j < 0) st.tune = (short)(st.tune + 1);
        st.tune &= (LORA_LEN - 1);
        st.time = 0;
        return -1;
    }
    st.time++;
    st.time &= 1023;
    if (st.time & 3) return -1;
    return (short)((bin + st.tune) & (LORA_LEN - 1));
}

// detect() from `finetune[..] = ..` on: mag_p and mag_q are mag[result - 1] and mag[result + 1] (mod 128), peak / result the
// first strict maximum of the five-term sums, negpeak that of rev[].  Returns m_result.
LORA_HD int lora_fetch_step(LoraSynch& st, float mag_p, float mag_q, float peak, float negpeak, short result, char* text_slots, int* n_lines, int max_lines)
{
    st.finetune[15 & st.time] = (mag_p > mag_q) ? -1 : 1;
    if (peak < negpeak * LORA_SQUELCH) result = -1;
    result = lora_synch(st, result, text_slots, n_lines, max_lines);
    if (result >= 0) st.result = result;
    return st.result;
}

// The loop of detect() over the 128 magnitudes, for the host (tests/lora_check.cpp): on the device the wave does it across lanes.
// mov is the 4 x 128 history, count the stream count already incremented.
inline int lora_fetch_host(LoraSynch& st, float* mov, long long count, const float* mag, const float* rev, char* text_slots, int* n_lines,
                           int max_lines, short* result_before_squelch = nullptr)
{
    const int movpoint = lora_movpoint(count);
    float peak = 0.0f, negpeak = 0.0f;
    short result = 0, negresult = 0;
    for (short i = 0; i < LORA_LEN; i++) {
        if (rev[i] > negpeak) { negpeak = rev[i]; negresult = i; }
        const float t = mov[i] + mov[LORA_LEN + i] + mov[2 * LORA_LEN + i] + mov[3 * LORA_LEN + i] + mag[i];
        if (t > peak) { peak = t; result = i; }
        mov[movpoint * LORA_LEN + i] = mag[i];
    }
    (void)negresult;
    if (result_before_squelch) *result_before_squelch = result;
    const int p = (result - 1 + LORA_LEN) & (LORA_LEN - 1), q = (result + 1) & (LORA_LEN - 1);
    return lora_fetch_step(st, mag[p], mag[q], peak, negpeak, result, text_slots, n_lines, max_lines);
}

} // namespace sdrx
