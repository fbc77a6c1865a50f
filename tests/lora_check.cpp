// Host check of sdrangel_amd/csrc/lora_scan.hpp (built with plain g++ by tests/test_lora_host.py): the fetch step of the LoRa bank
// -- the two first-strict-maximum picks, the mov sums, finetune, the squelch, synch() and dumpRaw() with the four lorabits
// functions -- against what the reference recorded per fetch (tests/golden/lora_rec.cpp's trace: mag[128], rev[128], the result
// before and after the squelch, m_time, m_tune, m_result).
//   lora_check replay <seed> <trace.bin> <text.bin>
//       the recorded magnitudes cut into random feeds (empty ones and one-fetch ones among them); the state is carried across
//       them as the device carries it, the text slots are a feed's own, sized by lora_lines_bound.  Every fetch must give the
//       recorded values and the feeds' lines together the recorded text.  Prints "ok <fetches> <lines> <feeds>" or the first mismatch.
//   lora_check angle
//       lora_angle against the running sums of m_chirp / m_angle over three periods; then lora_angle, lora_is_fetch and
//       lora_movpoint over 1024 consecutive counts around each of 2^31, 2^32, 2^33 and 2^40 against their values at the count
//       mod 512 and mod 256; prints "ok <steps> <large counts checked>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lora_scan.hpp"

using namespace sdrx;

static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

template <class T> static bool load(const char* path, std::vector<T>& v)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    const bool ok = v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

static int angle()
{
    int chirp = 0, ang = 0;
    const long long steps = 3 * 512 + 7;
    for (long long g = 0; g < steps; g++) {
        chirp = (chirp + 1) & (LORA_SPREAD - 1);
        ang = (ang + chirp) & (LORA_SPREAD - 1);
        if (lora_angle(g) != ang) { std::printf("angle mismatch at %lld: %d, want %d\n", g, lora_angle(g), ang); return 1; }
        // the period is 512 however far the stream has come
        if (lora_angle(g + (1ll << 40)) != ang) { std::printf("angle mismatch at %lld + 2^40\n", g); return 1; }
    }
    // the closed forms at large stream counts: 1024 consecutive counts around 2^31, 2^32, 2^33 and 2^40 against their values at
    // g mod 512 (m_angle's period) and c mod 256 (a fetch every 64, movpoint's period of 4 fetches)
    long long checked = 0;
    for (int e : { 31, 32, 33, 40 })
        for (long long v = (1ll << e) - 512; v < (1ll << e) + 512; v++, checked++) {
            if (lora_angle(v) != lora_angle(v & 511)) { std::printf("angle mismatch at %lld against %lld\n", v, v & 511); return 1; }
            if (lora_is_fetch(v) != lora_is_fetch(v & 255)) { std::printf("is_fetch mismatch at %lld\n", v); return 1; }
            if (lora_movpoint(v) != lora_movpoint(v & 255)) { std::printf("movpoint mismatch at %lld\n", v); return 1; }
        }
    std::printf("ok %lld %lld\n", steps, checked);
    return 0;
}

static int replay(uint64_t seed, const char* trace_path, const char* text_path)
{
    constexpr int W = 2 * LORA_LEN + 5;
    std::vector<float> tr;
    std::vector<char> want_text;
    if (!load(trace_path, tr) || !load(text_path, want_text) || tr.size() % W) { std::printf("cannot read the trace\n"); return 2; }
    const long fetches = (long)(tr.size() / W);
    g_s = seed;
    LoraSynch st;
    std::memset(&st, 0, sizeof st);
    std::vector<float> mov(4 * LORA_LEN, 0.0f);
    long long count = 0;
    std::string text;
    long done = 0, feeds = 0, lines = 0;
    while (done < fetches) {
        static const long pick[6] = { 0, 1, 1, 2, 3, 4 };
        const uint64_t r = rnd();
        long m = r % 3 == 0 ? pick[(r >> 8) % 6] : (long)((r >> 8) % 30);
        if (m > fetches - done) m = fetches - done;
        const int max_lines = (int)lora_lines_bound(64 * m);
        std::vector<char> slots((size_t)max_lines * LORA_TEXT, (char)0x7f);        // dumpRaw has to clear its slot itself
        int n_lines = 0;
        for (long i = 0; i < m; i++, done++) {
            const float* rec = &tr[(size_t)done * W];
            count += 64;
            short before = -2;
            const int res = lora_fetch_host(st, mov.data(), count, rec, rec + LORA_LEN, slots.data(), &n_lines, max_lines, &before);
            if (before != (short)rec[256] || st.time != (int)rec[258] || st.tune != (short)rec[259] || res != (int)rec[260]) {
                std::printf("fetch %ld: result %d time %d tune %d m_result %d, want %d %d %d %d\n", done, before, st.time, st.tune, res,
                            (int)rec[256], (int)rec[258], (int)rec[259], (int)rec[260]);
                return 1;
            }
        }
        for (int k = 0; k < n_lines; k++) { text += &slots[(size_t)k * LORA_TEXT + 1]; text += '\n'; }
        lines += n_lines;
        feeds++;
    }
    if (text != std::string(want_text.begin(), want_text.end()) || lines != st.lines) { std::printf("text mismatch: %s", text.c_str()); return 1; }
    std::printf("ok %ld %ld %ld\n", fetches, lines, feeds);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "angle")) return angle();
    if (argc == 5 && !std::strcmp(argv[1], "replay")) return replay(std::strtoull(argv[2], nullptr, 10), argv[3], argv[4]);
    std::fprintf(stderr, "usage: lora_check replay <seed> <trace.bin> <text.bin> | lora_check angle\n");
    return 2;
}
