// The host build of the pilot loop's step (sdrangel_amd/csrc/bfm_pll.hpp: bfm_pll_step, bfm_pilot_sin2 / cos2, bfm_rc_step) against
// a plain transcription of PhaseLock::process(const Real&, Real*) with process_phasor (sdrbase/dsp/phaselock.cpp:253-367) that
// calls the host libm's sinf / cosf, walked side by side over seeded input streams and the specials; built by
// tests/test_bfm_pll_math.py with plain g++ (no ROCm include path, -fno-builtin).
//
//   bfm_pll_check tone|noise|special seed n in_rate  ->  "ok <steps> <steps whose state or outputs differ> <probe counts x 8>"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bfm_pll.hpp"

using namespace sdrx;

namespace {

uint64_t g_s;
uint64_t next64() { g_s += 0x9E3779B97F4A7C15ull; uint64_t z = g_s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
float unit() { return (float)((double)(next64() >> 11) / 9007199254740992.0 * 2.0 - 1.0); }

#undef M_PI
#define M_PI 3.14159265358979323846
typedef float Real;

struct Plain {                              // the class's members
    Real m_phase, m_psin, m_pcos, m_minfreq, m_maxfreq, m_phasor_b0, m_phasor_a1, m_phasor_a2, m_phasor_i1, m_phasor_i2, m_phasor_q1, m_phasor_q2;
    Real m_loopfilter_b0, m_loopfilter_b1, m_loopfilter_x1, m_freq, m_minsignal, m_pilot_level;
    int m_lock_delay, m_lock_cnt, m_pilot_periods;
    void process(const Real& sample_in, Real* samples_out)
    {
        m_psin = sinf(m_phase);
        m_pcos = cosf(m_phase);
        samples_out[0] = m_psin;
        samples_out[1] = 2.0 * m_psin * m_pcos;
        samples_out[2] = (2.0 * m_pcos * m_pcos) - 1.0;
        samples_out[3] = m_phase;
        Real phasor_i = m_psin * sample_in;
        Real phasor_q = m_pcos * sample_in;
        phasor_i = m_phasor_b0 * phasor_i - m_phasor_a1 * m_phasor_i1 - m_phasor_a2 * m_phasor_i2;
        phasor_q = m_phasor_b0 * phasor_q - m_phasor_a1 * m_phasor_q1 - m_phasor_a2 * m_phasor_q2;
        m_phasor_i2 = m_phasor_i1; m_phasor_i1 = phasor_i;
        m_phasor_q2 = m_phasor_q1; m_phasor_q1 = phasor_q;
        Real phase_err;
        if (phasor_i > std::abs(phasor_q)) phase_err = phasor_q / phasor_i;
        else if (phasor_q > 0) phase_err = 1;
        else phase_err = -1;
        m_pilot_level = phasor_i;
        m_freq += m_loopfilter_b0 * phase_err + m_loopfilter_b1 * m_loopfilter_x1;
        m_loopfilter_x1 = phase_err;
        m_freq = std::max(m_minfreq, std::min(m_maxfreq, m_freq));
        m_phase += m_freq;
        if (m_phase > 2.0 * M_PI) {
            m_phase -= 2.0 * M_PI;
            m_pilot_periods++;
            if (m_pilot_periods == 19000) m_pilot_periods = 0;
        }
        if (2 * m_pilot_level > m_minsignal) { if (m_lock_cnt < m_lock_delay) m_lock_cnt += 1; }
        else m_lock_cnt = 0;
        if (m_lock_cnt < m_lock_delay) m_pilot_periods = 0;
    }
};

bool same(float a, float b) { return pll_bits(a) == pll_bits(b) || (a != a && b != b); }

} // namespace

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: bfm_pll_check tone|noise|special seed n in_rate\n"); return 2; }
    const char* set = argv[1];
    g_s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[2]) * 0x2545F4914F6CDD1Dull;
    const long n = std::atol(argv[3]);
    const int rate = std::atoi(argv[4]);
    BfmPllCfg k; BfmPllState s;
    bfm_pll_design(19000.0 / rate, 50.0 / rate, 0.01, &k, &s);
    Plain p;
    std::memset(&p, 0, sizeof p);
    p.m_minfreq = k.minfreq; p.m_maxfreq = k.maxfreq; p.m_phasor_b0 = k.b0; p.m_phasor_a1 = k.a1; p.m_phasor_a2 = k.a2;
    p.m_loopfilter_b0 = k.lf_b0; p.m_loopfilter_b1 = k.lf_b1; p.m_minsignal = k.minsignal; p.m_lock_delay = k.lock_delay; p.m_freq = s.freq;
    if (!std::strcmp(set, "special")) k.lock_delay = p.m_lock_delay = 40;       // so that the short stretches below reach it
    BfmPllProbe pr = {};
    const float specials[] = { 0.0f, -0.0f, 1.0e-45f, -1.0e-45f, 1.0e-38f, 3.0e38f, -3.0e38f, 1.0f, -1.0f, 0.02f };   // finite: demod is
    long differ = 0;
    float y1a = 0, y1b = 0, rb0, ra1;
    bfm_rc_design((double)(50.0f * 48000.0f) * 1.0e-6, &rb0, &ra1);
    for (long i = 0; i < n; i++) {
        float x;
        if (!std::strcmp(set, "tone")) {                    // a pilot a little off the loop's centre, its level and offset drawn per stretch
            static float amp = 0.02f, off = 0.0f;
            if (i % 20000 == 0) { amp = 0.001f + 0.05f * std::fabs(unit()); off = 300.0f * unit(); }
            x = amp * (float)std::sin(2.0 * M_PI * (19000.0 + off) * (double)i / rate) + 0.002f * unit();
        } else if (!std::strcmp(set, "noise")) x = unit() * ((i / 5000) % 3 == 2 ? 0.0f : 0.3f);
        else x = (i / 50) % 2 ? specials[(i / 100) % (sizeof specials / sizeof *specials)] : 0.05f * (float)std::sin(2.0 * M_PI * 19000.0 * (double)i / rate);
        float sn, cs, out[4];
        bfm_pll_step(k, s, x, &sn, &cs, &pr);
        p.process(x, out);
        const float ra = bfm_rc_step(out[1] * x, rb0, ra1, &y1a);
        y1b = (out[1] * x * rb0) - (y1b * ra1);
        const bool eq = same(sn, out[0]) && same(bfm_pilot_sin2(sn, cs), out[1]) && same(bfm_pilot_cos2(cs), out[2]) && same(s.phase, p.m_phase) &&
                        same(s.freq, p.m_freq) && same(s.i1, p.m_phasor_i1) && same(s.i2, p.m_phasor_i2) && same(s.q1, p.m_phasor_q1) &&
                        same(s.q2, p.m_phasor_q2) && same(s.x1, p.m_loopfilter_x1) && same(s.level, p.m_pilot_level) && s.lock_cnt == p.m_lock_cnt &&
                        s.periods == p.m_pilot_periods && same(ra, y1b);
        if (!eq) {
            differ++;
            // one loop has left the other's path: put them together again, so that every later step is compared on its own
            s.phase = p.m_phase; s.freq = p.m_freq; s.i1 = p.m_phasor_i1; s.i2 = p.m_phasor_i2; s.q1 = p.m_phasor_q1; s.q2 = p.m_phasor_q2;
            s.x1 = p.m_loopfilter_x1; s.level = p.m_pilot_level; s.lock_cnt = p.m_lock_cnt; s.periods = p.m_pilot_periods; y1a = y1b;
        }
    }
    std::printf("ok %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", n, differ, pr.ratio, pr.plus, pr.minus, pr.clamp_lo, pr.clamp_hi, pr.wrap, pr.lock_up, pr.lock_reset);
    return 0;
}
