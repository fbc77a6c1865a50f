// The serial part of RDS for the host and the device: RDSDemod::process with biphase and the feedback half of
// filter_lp_2400_iq (plugins/channelrx/demodbfm/rdsdemod.cpp:73-197, types in rdsdemod.h:50-76) and RDSDecoder::frameSync with
// calc_syndrome (rdsdecoder.cpp:50-261), one step each in the reference's operand order and float / double promotions.
// Compiles for the host too (tests/bfm_rds_check.cpp), no HIP header needed.  The struct members carry the reference's names.
#pragma once
#include <stdint.h>
#include "rds_mix.hpp"

namespace sdrx {

struct RdsDemodState {                  // RDSDemod::m_parms, m_xv[0], m_yv[0], m_report
    double subcarr_phi, clock_offset, clock_phi, prev_clock_phi, d_cphi;
    float xv[3], yv[3];
    float prev_bb, acc, prev_acc, lo_clock, prev_lo_clock;
    int numsamples, counter, reading_frame, tot_errs0, tot_errs1, dbit;
    float rep_acc, rep_qua, rep_fclk;
    int pad_;
};

struct RdsDecoderState {                // every member of RDSDecoder
    uint64_t reg, lastseenOffsetCounter, bitCounter;
    uint32_t blockBitCounter, wrongBlocksCounter, blocksCounter, groupGoodBlocksCounter;
    uint32_t group0, group1, group2, group3;
    int sync;                           // NO_SYNC = 0, SYNC = 1
    int presync, lastseenOffset, blockNumber, groupAssemblyStarted, goodBlock;
    float qua;
    int pad_;
};

struct RdsProbe {                       // the branches the steps went through
    long zero_cross, corr_minus, corr_plus, dump, biphase_err, biphase_bit, biphase_skip, frame_flip, report;
    long fs_nosync, fs_presync_set, fs_presync_drop, fs_enter_sync, fs_wait, fs_c_good, fs_cprime_good, fs_c_bad, fs_good, fs_bad,
         fs_group_start, fs_group_abort, fs_group_ready, fs_lost_sync, fs_still_sync;
};

AM_HD void rds_demod_fresh(RdsDemodState* s) { *s = RdsDemodState(); }
AM_HD void rds_decoder_fresh(RdsDecoderState* d) { *d = RdsDecoderState(); d->sync = 1; }

AM_HD int rds_sign(float a) { return a >= 0 ? 1 : 0; }

// filter_lp_2400_iq: what does not feed back, from three consecutive m_xv values (a float expression)
AM_HD float rds_xv(float input) { return (float)((double)input / 4.491730007e+03); }
AM_HD float rds_fir_part(float xv0, float xv1, float xv2) { return (xv0 + xv2) + 2 * xv1; }

// RDSDemod::biphase
template <class Probe>
AM_HD bool rds_biphase(RdsDemodState& s, float acc, bool* bit, float d_cphi, Probe* pr)
{
    bool ret = false;
    const int odd = s.counter % 2;
    if (rds_sign(acc) != rds_sign(s.prev_acc)) {
        if (odd) s.tot_errs1++; else s.tot_errs0++;
        if (pr) pr->biphase_err++;
    }
    if (odd == s.reading_frame) {
        const int b = rds_sign(s.acc + s.prev_acc);
        *bit = (b ^ s.dbit) != 0;
        s.dbit = b;
        ret = true;
        if (pr) pr->biphase_bit++;
    } else if (pr) pr->biphase_skip++;
    if (s.counter == 0) {
        const int cur = s.reading_frame ? s.tot_errs1 : s.tot_errs0, other = s.reading_frame ? s.tot_errs0 : s.tot_errs1;
        if (other < cur) { s.reading_frame = 1 - s.reading_frame; if (pr) pr->frame_flip++; }
        const int diff = s.tot_errs0 - s.tot_errs1;
        s.rep_qua = (float)((1.0 * (double)(diff < 0 ? -diff : diff) / (double)(s.tot_errs0 + s.tot_errs1)) * 100.0);
        s.rep_acc = acc;
        s.rep_fclk = (float)(((double)d_cphi / (2 * 3.14159265358979323846)) * 250000.0);
        s.tot_errs0 = 0; s.tot_errs1 = 0;
        if (pr) pr->report++;
    }
    s.prev_acc = acc;
    s.counter = (s.counter + 1) % 800;
    return ret;
}

// RDSDemod::process behind the FIR half of the filter: fir = rds_fir_part of the sample's m_xv.  The caller keeps s.xv.
template <class Probe>
AM_HD bool rds_demod_step(RdsDemodState& s, float fir, bool* bit, Probe* pr)
{
    const double pi = 3.14159265358979323846, pi_2 = 1.57079632679489661923;
    s.yv[0] = s.yv[1]; s.yv[1] = s.yv[2];
    s.yv[2] = (float)(((double)fir + (-0.9582451124 * (double)s.yv[0])) + (1.9573545869 * (double)s.yv[1]));
    const float bb = s.yv[2];                                // m_parms.subcarr_bb[0]
    s.subcarr_phi += (2 * pi * 1187.5) / 250000.0;          // (2 * M_PI * m_fsc) / (Real) m_srate
    s.clock_phi = s.subcarr_phi + s.clock_offset;
    if (rds_sign(s.prev_bb) != rds_sign(bb)) {
        s.d_cphi = rds_fmod(s.clock_phi, pi);
        if (s.d_cphi >= pi_2) { s.d_cphi -= pi; if (pr) pr->corr_minus++; } else if (pr) pr->corr_plus++;
        s.clock_offset -= 0.005 * s.d_cphi;
        if (pr) pr->zero_cross++;
    }
    s.clock_phi = rds_fmod(s.clock_phi, 2 * pi);
    s.lo_clock = s.clock_phi < pi ? 1.0f : -1.0f;
    bool ret = false;
    if (s.numsamples % 8 == 0) {
        s.acc += bb * s.lo_clock;
        if (rds_sign(s.lo_clock) != rds_sign(s.prev_lo_clock)) {
            ret = rds_biphase(s, s.acc, bit, (float)(s.clock_phi - s.prev_clock_phi), pr);
            s.acc = 0;
            if (pr) pr->dump++;
        }
        s.prev_lo_clock = s.lo_clock;
    }
    s.numsamples++;
    s.prev_bb = bb;
    s.prev_clock_phi = s.clock_phi;
    return ret;
}

// RDSDecoder::calc_syndrome (Annex B of the standard)
AM_HD uint32_t rds_syndrome(uint64_t message, int mlen)
{
    uint64_t reg = 0;
    const uint64_t poly = 0x5B9;
    const int plen = 10;
    for (int i = mlen; i > 0; i--) {
        reg = (reg << 1) | ((message >> (i - 1)) & 0x01);
        if (reg & (1 << plen)) reg = reg ^ poly;
    }
    for (int i = plen; i > 0; i--) {
        reg = reg << 1;
        if (reg & (1 << plen)) reg = reg ^ poly;
    }
    return (uint32_t)(reg & ((1 << plen) - 1));
}

AM_HD uint32_t rds_offset_pos(int j) { return j == 4 ? 2u : (uint32_t)j; }                 // {0, 1, 2, 3, 2}
AM_HD uint32_t rds_offset_word(int j) { return j == 0 ? 252u : j == 1 ? 408u : j == 2 ? 360u : j == 3 ? 436u : 848u; }
AM_HD uint32_t rds_syndrome_of(int j) { return j == 0 ? 383u : j == 1 ? 14u : j == 2 ? 303u : j == 3 ? 663u : 748u; }

// RDSDecoder::frameSync; true: a group is ready in group0 .. group3
template <class Probe>
AM_HD bool rds_frame_sync(RdsDecoderState& d, bool bit, Probe* pr)
{
    bool group_ready = false;
    d.reg = (d.reg << 1) | (bit ? 1u : 0u);
    if (d.sync == 0) {
        const uint32_t reg_syndrome = rds_syndrome(d.reg, 26);
        if (pr) pr->fs_nosync++;
        for (int j = 0; j < 5; j++) {
            if (reg_syndrome != rds_syndrome_of(j)) continue;
            if (!d.presync) {
                d.lastseenOffset = j;
                d.lastseenOffsetCounter = d.bitCounter;
                d.presync = 1;
                if (pr) pr->fs_presync_set++;
            } else {
                const uint64_t bit_distance = d.bitCounter - d.lastseenOffsetCounter;
                const uint32_t pl = rds_offset_pos(d.lastseenOffset), pj = rds_offset_pos(j);
                const uint64_t block_distance = pl >= pj ? pj + 4 - pl : pj - pl;
                if (block_distance * 26 != bit_distance) { d.presync = 0; if (pr) pr->fs_presync_drop++; }
                else {                                      // enter_sync(j)
                    d.wrongBlocksCounter = 0; d.blocksCounter = 0; d.blockBitCounter = 0;
                    d.blockNumber = (j + 1) % 4;
                    d.groupAssemblyStarted = 0;
                    d.sync = 1;
                    if (pr) pr->fs_enter_sync++;
                }
            }
            break;
        }
    } else if (d.blockBitCounter < 25) {
        d.blockBitCounter++;
        if (pr) pr->fs_wait++;
    } else {
        d.goodBlock = 0;
        const uint32_t dataword = (uint32_t)((d.reg >> 10) & 0xffff);
        const uint32_t calc = rds_syndrome(dataword, 16);
        const uint32_t checkword = (uint32_t)(d.reg & 0x3ff);
        if (d.blockNumber == 2) {
            if ((checkword ^ rds_offset_word(2)) == calc) { d.goodBlock = 1; if (pr) pr->fs_c_good++; }
            else if ((checkword ^ rds_offset_word(4)) == calc) { d.goodBlock = 1; if (pr) pr->fs_cprime_good++; }
            else { d.wrongBlocksCounter++; if (pr) pr->fs_c_bad++; }
        } else {
            if ((checkword ^ rds_offset_word(d.blockNumber)) == calc) { d.goodBlock = 1; if (pr) pr->fs_good++; }
            else { d.wrongBlocksCounter++; if (pr) pr->fs_bad++; }
        }
        if (d.blockNumber == 0 && d.goodBlock) {
            d.groupAssemblyStarted = 1;
            d.groupGoodBlocksCounter = 1;
            if (pr) pr->fs_group_start++;
        }
        if (d.groupAssemblyStarted) {
            if (!d.goodBlock) { d.groupAssemblyStarted = 0; if (pr) pr->fs_group_abort++; }
            else {
                if (d.blockNumber == 0) d.group0 = dataword;
                else if (d.blockNumber == 1) d.group1 = dataword;
                else if (d.blockNumber == 2) d.group2 = dataword;
                else d.group3 = dataword;
                d.groupGoodBlocksCounter++;
            }
            if (d.groupGoodBlocksCounter == 5) { group_ready = true; if (pr) pr->fs_group_ready++; }
        }
        d.blockBitCounter = 0;
        d.blockNumber = (d.blockNumber + 1) % 4;
        d.blocksCounter++;
        if (d.blocksCounter == 50) {
            if (d.wrongBlocksCounter > 35) { d.presync = 0; d.sync = 0; if (pr) pr->fs_lost_sync++; }    // enter_no_sync()
            else if (pr) pr->fs_still_sync++;
            d.qua = (float)(2.0 * (50 - d.wrongBlocksCounter));
            d.blocksCounter = 0;
            d.wrongBlocksCounter = 0;
        }
    }
    d.bitCounter++;
    return group_ready;
}

} // namespace sdrx
