// Host check of sdrangel_amd/csrc/udpsrc_ssb_sched.hpp: the closed forms the SSB kernels of the UDPSrc bank index with,
// against a literal loop -- a counter that takes one resampled sample at a time as fftfilt::runSSB does, writes 256 block
// elements into a payload list when it reaches 256 and, for format 4, one raw element behind them.  Random sequences of
// feeds, the pending count carried from one to the next.  Plain C++, its own main: tests/test_udpsrc_ssb_scan.py builds it
// twice, the second time with -fsanitize=address,undefined, and runs both directly.
//     udpsrc_ssb_scan_check <seed> <feeds>      prints "ok <checks>"
#include "udpsrc_ssb_sched.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrx;

namespace {

uint64_t state = 1;
uint64_t rnd()
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

long checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { std::printf("FAILED %s (line %d): fmt %d pending %d n %d\n", #cond, __LINE__, fmt, pending, n); return 1; } } while (0)

// what element `pos` of a feed's payload is: block b input-output index j, or raw sample k
struct Elem { int block, j, raw; };

// one feed, literally; `stream` numbers every resampled sample since the start, `held` are the stream numbers waiting in the filter
int feed(int fmt, int pending, int n, std::vector<long>& held, long& stream)
{
    std::vector<Elem> payload;
    std::vector<std::vector<long>> inputs;                  // per block of this feed: the stream numbers it was made of
    std::vector<int> completing, through((size_t)n, 0);
    int inptr = pending, blocks = 0;
    for (int k = 0; k < n; k++) {
        held.push_back(stream++);
        if (++inptr == UDP_SSB_H) {
            inptr = 0;
            inputs.push_back(held); held.clear();
            completing.push_back(k);
            for (int j = 0; j < UDP_SSB_H; j++) payload.push_back(Elem{blocks, j, -1});
            blocks++;
        }
        through[(size_t)k] = blocks;
        if (fmt == UDP_LSB) payload.push_back(Elem{-1, -1, k});
    }
    const long first = stream - n;                          // stream number of this feed's sample 0
    CHECK(udp_ssb_blocks(pending, n) == blocks);
    CHECK(udp_ssb_left(pending, n) == inptr);
    CHECK(udp_ssb_payload_count(fmt, pending, n) == (long)payload.size());
    CHECK((long)payload.size() <= udp_ssb_payload_bound(n));
    CHECK(blocks <= (n + 255) / 256);                       // the grid of 256-sample tiles covers the blocks
    for (int b = 0; b < blocks; b++) {
        const int kb = udp_ssb_completing(pending, b);
        CHECK(kb == completing[(size_t)b] && kb >= 0 && kb < n);
        const long at = udp_ssb_block_pos(fmt, pending, b);
        CHECK(at >= 0 && at + UDP_SSB_H <= (long)payload.size());
        CHECK((at & 1) == 0 || !udp_fmt_ssb_mono(fmt));     // a mono block starts on a dword
        for (int j = 0; j < UDP_SSB_H; j++) {
            CHECK(payload[(size_t)(at + j)].block == b && payload[(size_t)(at + j)].j == j);
            const int q = udp_ssb_source(pending, b, j);
            CHECK(q < n && q >= -pending);
            CHECK(first + q == inputs[(size_t)b][(size_t)j]);      // q < 0: carried sample pending + q, whose stream number is first + q
        }
        if (fmt == UDP_LSB) CHECK(udp_ssb_raw_pos(pending, kb) == at + UDP_SSB_H);      // right in front of its completing sample's raw element
    }
    for (int k = 0; k < n; k++) {
        CHECK(udp_ssb_blocks_through(pending, k) == through[(size_t)k]);
        if (fmt == UDP_LSB) {
            const long at = udp_ssb_raw_pos(pending, k);
            CHECK(at >= 0 && at < (long)payload.size() && payload[(size_t)at].raw == k);
        }
    }
    CHECK((int)held.size() == inptr);
    for (int i = 0; i < inptr; i++) {
        const int q = udp_ssb_carried_source(pending, n, i);
        CHECK(q < n && q >= -pending && first + q == held[(size_t)i]);
    }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: udpsrc_ssb_scan_check seed feeds\n"); return 2; }
    state = (uint64_t)std::strtoull(argv[1], nullptr, 10);
    const int feeds = std::atoi(argv[2]);
    static const int lens[] = { 0, 1, 2, 255, 256, 257, 511, 512, 513, 768 };
    for (int fmt = UDP_LSB; fmt <= UDP_USB_MONO; fmt++) {
        // every pending count against the edge lengths, then random walks
        for (int pending = 0; pending < UDP_SSB_H; pending++)
            for (int n : lens) {
                std::vector<long> held; long stream = 0;
                for (int i = 0; i < pending; i++) held.push_back(stream++);
                if (feed(fmt, pending, n, held, stream)) return 1;
            }
        std::vector<long> held; long stream = 0;
        int pending = 0;
        for (int f = 0; f < feeds; f++) {
            const uint64_t r = rnd();
            const int n = (r & 3) == 0 ? lens[(r >> 8) % 10] : (int)((r >> 8) % ((r & 4) ? 300 : 5000));
            if (feed(fmt, pending, n, held, stream)) return 1;
            pending = udp_ssb_left(pending, n);
        }
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
