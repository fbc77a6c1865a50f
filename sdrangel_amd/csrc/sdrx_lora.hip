// libsdrx.so: sdrx_lora_* -- N LoRa demodulators (LoRaDemod::feed, plugins/channelrx/demodlora/lorademod.cpp:94-288) on one
// device: int16 I/Q at the channelizer's output rate in; the Samples of m_sampleBuffer and the lines dumpRaw prints out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream, started one distance step in
// as LoRaDemod starts it and designed from the double m_Bandwidth / 1.9; the tail's kernels are in lora_kernels.hpp.  Host
// side: the design products of the constructor and of sfft's (fftfilt.cpp:411-427), the two layouts and the launches; the rest
// is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "lora_kernels.hpp"
#include "demod_bank.hpp"
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace sdrx;

namespace {

// m_sampleDistanceRemain = (Real) m_sampleRate / m_Bandwidth, a float quotient (m_Bandwidth is a Real): where the distance
// starts and what it steps by
float distance_step(const sdrx_lora_cfg& k) { return (float)k.in_rate / (float)k.bandwidth; }

} // namespace

struct LoraFamily : DemodDefaults {
    using Handle = sdrx_lora;
    using Cfg = sdrx_lora_cfg;
    using Chan = LoraChan;
    using Bufs = LoraBufs;
    static constexpr const char* name = "sdrx_lora";
    static constexpr const float2* LoraBufs::* input = &LoraBufs::ci;

    static int validate(int32_t n_ch, const sdrx_lora_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_lora_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++)
            if (cfg[c].in_rate <= 0 || cfg[c].bandwidth <= 0 || cfg[c].bandwidth > cfg[c].in_rate) {
                set_error("sdrx_lora_create: bad channel configuration (need 1 <= bandwidth <= in_rate; the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
        return SDRX_OK;
    }

    static void design(int, const sdrx_lora_cfg& k, sdrx_backend_cfg& f, LoraChan&, float*)
    {
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.bandwidth;     // the step itself goes in through backend_start_at
        f.interp_cutoff = (float)cutoff(k, f);              // for inspection only: the taps come from the double (cutoff())
        f.taps_per_phase = 4.5f;
        // everything else starts at 0: the constructor's values, the bins and delay lines of a fresh sfft, and mov (sdrx.h)
    }

    // m_interpolator.create(16, m_sampleRate, m_Bandwidth / 1.9): a float divided by a double
    static double cutoff(const sdrx_lora_cfg& k, const sdrx_backend_cfg&) { return (double)(float)k.bandwidth / 1.9; }

    static int front_made(sdrx_backend_t* front, int n_ch, const sdrx_lora_cfg* cfg)
    {
        for (int c = 0; c < n_ch; c++) {
            int rc = backend_start_at(front, c, distance_step(cfg[c]), distance_step(cfg[c])); if (rc) return rc;
        }
        return SDRX_OK;
    }

    // one history set: the last 128 (va, vb), zeros in a fresh one (sfft clears its delay line)
    static void hist(HistCarver& k, const LoraChan&, LoraBufs& u) { k.pair(u.vhist, u.vhist_next, (size_t)LORA_LEN); }

    static void work(Carver& k, size_t n, const LoraChan&, LoraBufs& u)
    {
        u.za = k.take<float2>(n); u.zb = k.take<float2>(n);
        u.samples = k.take<unsigned int>(n);
        u.max_lines = (int)lora_lines_bound((long long)n);
        u.text = k.take<char>((size_t)u.max_lines * LORA_TEXT);
    }

    static int64_t outputs_bound(const sdrx_lora_cfg& k, int64_t n_in) { return demod_outputs_bound(k.in_rate / k.bandwidth, n_in); }

    static int launch(DemodBank<LoraFamily>& b, unsigned nc, unsigned gx);
};

// the handle: the bank and the tables every channel shares
struct sdrx_lora : DemodBank<LoraFamily> {
    float* d_tab = nullptr;                 // [chirp 512 | vrot 256 | sample 128 (as bits)]
    std::vector<float> chirp, vrot;
    std::vector<uint32_t> sample;
    float k2 = 1.0f;
    LoraTables tables() const
    {
        return LoraTables{ reinterpret_cast<const float2*>(d_tab), reinterpret_cast<const float2*>(d_tab + 2 * LORA_SPREAD),
                           reinterpret_cast<const unsigned int*>(d_tab + 2 * LORA_SPREAD + 2 * LORA_LEN), k2 };
    }
};
using Bank = DemodBank<LoraFamily>;

int LoraFamily::launch(DemodBank<LoraFamily>& bank, unsigned nc, unsigned gx)
{
    sdrx_lora& b = static_cast<sdrx_lora&>(bank);
    const LoraTables t = b.tables();
    hipLaunchKernelGGL(lora_dechirp_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, t);
    SDRX_HIP(hipGetLastError());
    const unsigned gw = (nc + LORA_WALK_WAVES - 1) / LORA_WALK_WAVES;
    hipLaunchKernelGGL(lora_walk_kernel, dim3(gw), dim3(64 * LORA_WALK_WAVES), 0, b.core.stream, b.d_chan, b.d_bufs, t, b.n_ch);
    SDRX_HIP(hipGetLastError());
    b.core.note_launch("lora_walk_kernel", (int)gw, 64 * LORA_WALK_WAVES, 0);
    hipLaunchKernelGGL(lora_carry_kernel, dim3(nc), dim3(LORA_LEN), 0, b.core.stream, b.d_chan, b.d_bufs, t);
    SDRX_HIP(hipGetLastError());
    return SDRX_OK;
}

// the tables of the constructor and of feed(): the dechirp (lorademod.cpp:272), sfft's vrot and k2 (fftfilt.cpp:419-426) and the
// Samples of m_bin (lorademod.cpp:276-277), every expression with the reference's widths
static int lora_design_tables(sdrx_lora* b)
{
    b->chirp.resize(2 * LORA_SPREAD); b->vrot.resize(2 * LORA_LEN); b->sample.resize(LORA_LEN);
    for (int a = 0; a < LORA_SPREAD; a++) {
        b->chirp[(size_t)(2 * a)] = (float)std::cos(M_PI * 2 * a / LORA_SPREAD);
        b->chirp[(size_t)(2 * a + 1)] = (float)-std::sin(M_PI * 2 * a / LORA_SPREAD);
    }
    const double K1 = 0.99999;
    double phi = 0.0;
    const double tau = 2.0 * M_PI / LORA_LEN;
    float k2 = 1.0;
    for (int i = 0; i < LORA_LEN; i++) {
        b->vrot[(size_t)(2 * i)] = (float)(K1 * std::cos(phi));
        b->vrot[(size_t)(2 * i + 1)] = (float)(K1 * std::sin(phi));
        phi += tau;
        k2 = (float)(k2 * K1);
    }
    b->k2 = k2;
    for (int m = 0; m < LORA_LEN; m++) {
        const float re = (float)std::cos(M_PI * 2 * m / LORA_LEN), im = (float)std::sin(M_PI * 2 * m / LORA_LEN);      // Complex nangle
        const int16_t sr = (int16_t)(re * 100), si = (int16_t)(im * 100);                                               // Sample(FixReal, FixReal)
        b->sample[(size_t)m] = (uint32_t)(uint16_t)sr | ((uint32_t)(uint16_t)si << 16);
    }
    std::vector<float> all(b->chirp);
    all.insert(all.end(), b->vrot.begin(), b->vrot.end());
    all.resize(all.size() + LORA_LEN);
    std::memcpy(&all[2 * LORA_SPREAD + 2 * LORA_LEN], b->sample.data(), LORA_LEN * 4);
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_tab), all.size() * 4));
    SDRX_HIP(hipMemcpy(b->d_tab, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    return SDRX_OK;
}

static int lora_destroy(sdrx_lora* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    if (b->d_tab) (void)hipFree(b->d_tab);
    return Bank::destroy(b);
}

extern "C" {

int sdrx_lora_create(sdrx_lora_t** out, int device, int32_t n_ch, const sdrx_lora_cfg* cfg)
{
    int rc = Bank::create(out, device, n_ch, cfg); if (rc) return rc;
    rc = lora_design_tables(*out);
    if (rc) { lora_destroy(*out); *out = nullptr; }
    return rc;
}
int sdrx_lora_destroy(sdrx_lora_t* b) { return lora_destroy(b); }
int sdrx_lora_reset(sdrx_lora_t* b) { return Bank::reset(b); }
int sdrx_lora_feed_dev(sdrx_lora_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_lora_feed_bank(sdrx_lora_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_lora_feed(sdrx_lora_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }

int64_t sdrx_lora_read(sdrx_lora_t* b, int32_t c, int16_t* samples_iq, int64_t cap)
{
    return Bank::read(b, "read", c, reinterpret_cast<unsigned int*>(samples_iq), cap, &LoraBufs::samples, &LoraChan::n, 4);
}
int sdrx_lora_last_dev(sdrx_lora_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n)
{
    return Bank::last_dev(b, "last_dev", c, reinterpret_cast<const unsigned int**>(d_samples_iq), n, &LoraBufs::samples, &LoraChan::n);
}

int64_t sdrx_lora_read_text(sdrx_lora_t* b, int32_t c, char* buf, int64_t cap)
{
    if (cap < 0 || (cap > 0 && !buf)) return Bank::fail("read_text", ": bad argument");
    LoraChan s;
    int rc = Bank::fetch(b, "read_text", c, &s); if (rc) return rc;
    if (s.n_lines <= 0) return 0;
    std::vector<char> slots((size_t)s.n_lines * LORA_TEXT);
    SDRX_HIP(hipMemcpy(slots.data(), b->h_bufs[c].text, slots.size(), hipMemcpyDeviceToHost));
    std::string text;
    for (int i = 0; i < s.n_lines; i++) {
        const char* line = &slots[(size_t)i * LORA_TEXT + 1];                   // printf("%s\n", &text[1])
        text.append(line, strnlen(line, LORA_TEXT - 1));
        text.push_back('\n');
    }
    if ((int64_t)text.size() > cap) return Bank::fail("read_text", ": the buffer is too small for the lines of the last feed");
    std::memcpy(buf, text.data(), text.size());
    return (int64_t)text.size();
}

int sdrx_lora_state(sdrx_lora_t* b, int32_t c, sdrx_lora_state_t* out)
{
    if (!out) return Bank::fail("state", ": bad argument");
    LoraChan s;
    int rc = Bank::fetch(b, "state", c, &s); if (rc) return rc;
    out->tune = s.sy.tune; out->time = s.sy.time; out->result = s.sy.result; out->bin = s.bin;
    out->count = s.count; out->lines = s.sy.lines;
    return SDRX_OK;
}

int sdrx_lora_get_design(sdrx_lora_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, int32_t* nco_inc,
                         float* vrot_iq, float* k2, float* chirp_iq, int16_t* sample_iq)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, nullptr, nco_inc); if (rc) return rc;
    if (vrot_iq) std::memcpy(vrot_iq, b->vrot.data(), b->vrot.size() * 4);
    if (k2) *k2 = b->k2;
    if (chirp_iq) std::memcpy(chirp_iq, b->chirp.data(), b->chirp.size() * 4);
    if (sample_iq) std::memcpy(sample_iq, b->sample.data(), b->sample.size() * 4);
    return SDRX_OK;
}

int sdrx_lora_sync(sdrx_lora_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_lora_set_stream(sdrx_lora_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_lora_get_stream(sdrx_lora_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_lora_set_timing(sdrx_lora_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_lora_get_timing(sdrx_lora_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_lora_last_launch(const sdrx_lora_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
