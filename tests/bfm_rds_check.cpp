// Host build of sdrangel_amd/csrc/bfm_rds.hpp, the header the device walk runs, for tests/test_bfm_rds_host.py.
//   bfm_rds_check framesync bits.bin out.bin   a fresh decoder on the bytes of bits.bin; per step 10 bytes, as the recorder
//                                              (tests/golden/bfm_rds_rec.cpp): group_ready, synced(), the group as 4 uint16
//   bfm_rds_check demod cr.bin out.bin         a fresh RDSDemod + RDSDecoder on the floats of cr.bin (what RDSDemod::process is
//                                              given); out.bin: int64 n, subcarr_bb of each; int64 bits, one byte each; int64
//                                              groups, 4 uint16 each; the report (4 float bits, synced); 40 state words: the
//                                              recorder's without distance_remain, mix_phase and n_rds
// Both print the probe's branch counts as "name=count" pairs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "bfm_rds.hpp"

using namespace sdrx;

static uint32_t fb(float v) { uint32_t i; std::memcpy(&i, &v, 4); return i; }

static void print_probe(const RdsProbe& p)
{
    const char* names[] = { "zero_cross", "corr_minus", "corr_plus", "dump", "biphase_err", "biphase_bit", "biphase_skip", "frame_flip", "report",
                            "fs_nosync", "fs_presync_set", "fs_presync_drop", "fs_enter_sync", "fs_wait", "fs_c_good", "fs_cprime_good", "fs_c_bad",
                            "fs_good", "fs_bad", "fs_group_start", "fs_group_abort", "fs_group_ready", "fs_lost_sync", "fs_still_sync" };
    const long* v = &p.zero_cross;
    for (size_t i = 0; i < sizeof names / sizeof names[0]; i++) std::printf("%s=%ld ", names[i], v[i]);
    std::printf("\n");
}

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> b;
    FILE* f = std::fopen(path, "rb");
    if (!f) return b;
    int c;
    while ((c = std::fgetc(f)) != EOF) b.push_back((uint8_t)c);
    std::fclose(f);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: bfm_rds_check framesync|demod in.bin out.bin\n"); return 2; }
    const std::vector<uint8_t> in = slurp(argv[2]);
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) { std::perror("open"); return 2; }
    RdsProbe pr;
    std::memset(&pr, 0, sizeof pr);
    RdsDecoderState k;
    rds_decoder_fresh(&k);
    if (!std::strcmp(argv[1], "framesync")) {
        for (size_t i = 0; i < in.size(); i++) {
            const uint8_t ready = rds_frame_sync(k, in[i] != 0, &pr) ? 1 : 0, synced = (uint8_t)k.sync;
            const uint16_t g[4] = { (uint16_t)k.group0, (uint16_t)k.group1, (uint16_t)k.group2, (uint16_t)k.group3 };
            std::fwrite(&ready, 1, 1, out); std::fwrite(&synced, 1, 1, out); std::fwrite(g, 2, 4, out);
        }
    } else if (!std::strcmp(argv[1], "demod")) {
        const int64_t n = (int64_t)(in.size() / 4);
        RdsDemodState d;
        rds_demod_fresh(&d);
        std::vector<float> bb((size_t)n);
        std::vector<uint8_t> bits;
        std::vector<uint16_t> groups;
        for (int64_t i = 0; i < n; i++) {
            float x;
            std::memcpy(&x, &in[(size_t)i * 4], 4);
            d.xv[0] = d.xv[1]; d.xv[1] = d.xv[2]; d.xv[2] = rds_xv(x);
            bool bit = false;
            const bool got = rds_demod_step(d, rds_fir_part(d.xv[0], d.xv[1], d.xv[2]), &bit, &pr);
            bb[(size_t)i] = d.yv[2];
            if (got) {
                bits.push_back(bit ? 1 : 0);
                if (rds_frame_sync(k, bit, &pr)) { groups.push_back((uint16_t)k.group0); groups.push_back((uint16_t)k.group1); groups.push_back((uint16_t)k.group2); groups.push_back((uint16_t)k.group3); }
            }
        }
        const int64_t nb = (int64_t)bits.size(), ng = (int64_t)(groups.size() / 4);
        std::fwrite(&n, 8, 1, out); if (n) std::fwrite(bb.data(), 4, (size_t)n, out);
        std::fwrite(&nb, 8, 1, out); if (nb) std::fwrite(bits.data(), 1, (size_t)nb, out);
        std::fwrite(&ng, 8, 1, out); if (ng) std::fwrite(groups.data(), 2, groups.size(), out);
        const uint32_t rep[5] = { fb(d.rep_acc), fb(d.rep_qua), fb(d.rep_fclk), fb(k.qua), (uint32_t)k.sync };
        std::fwrite(rep, 4, 5, out);
        auto db = [](double v) { uint64_t i; std::memcpy(&i, &v, 8); return i; };
        const uint64_t st[] = {
            db(d.subcarr_phi), db(d.clock_offset), db(d.clock_phi), db(d.prev_clock_phi), db(d.d_cphi),
            fb(d.xv[0]), fb(d.xv[1]), fb(d.xv[2]), fb(d.yv[0]), fb(d.yv[1]), fb(d.yv[2]),
            fb(d.prev_bb), fb(d.acc), fb(d.prev_acc), fb(d.lo_clock), fb(d.prev_lo_clock),
            (uint64_t)(int64_t)d.numsamples, (uint64_t)(int64_t)d.counter, (uint64_t)(int64_t)d.reading_frame,
            (uint64_t)(int64_t)d.tot_errs0, (uint64_t)(int64_t)d.tot_errs1, (uint64_t)(int64_t)d.dbit,
            k.reg, k.lastseenOffsetCounter, k.bitCounter, k.blockBitCounter, k.wrongBlocksCounter, k.blocksCounter, k.groupGoodBlocksCounter,
            k.group0, k.group1, k.group2, k.group3, (uint64_t)k.sync, (uint64_t)k.presync, (uint64_t)k.lastseenOffset, (uint64_t)k.blockNumber,
            (uint64_t)k.groupAssemblyStarted, (uint64_t)k.goodBlock, fb(k.qua) };
        std::fwrite(st, 8, sizeof st / sizeof st[0], out);
    } else return 2;
    std::fclose(out);
    print_probe(pr);
    return 0;
}
