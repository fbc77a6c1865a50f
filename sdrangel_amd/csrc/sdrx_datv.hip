// libsdrx.so: sdrx_datv_* -- the sample-rate half of N DATV receivers (DATVDemod::feed, plugins/channelrx/demoddatv/datvdemod.cpp:
// 767-863, down to p_symbols) on one device: int16 I/Q at the channelizer's output rate in; soft symbols, constellation points,
// measurements and the receiver's state out.  The front is a channel back-end in bypass that the handle owns and launches on its
// own stream: the NCO mix and fftfilt::runFilt on 1024 points (filter mode 1), which hands over 512 filtered samples per 512
// inputs and keeps a partial block.  The tail is one kernel, datv_walk_kernel (datv_kernels.hpp); the per-symbol and per-chunk
// step is datv_scan.hpp's, the design datv_design.hpp's.  Host side: validate, the tables (one trig16 per handle, one
// constellation table per distinct (modulation, fec, hard_metric)), the two layouts and the launch; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "datv_kernels.hpp"
#include "datv_design.hpp"
#include "demod_bank.hpp"
#include <cstddef>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

using namespace sdrx;

namespace {

DatvCfgView view_of(const sdrx_datv_cfg& k)
{
    return DatvCfgView{ k.msps, k.sample_rate, k.centre_frequency, k.rf_bandwidth, k.symbol_rate, k.modulation, k.fec, k.standard, k.sampler,
                        k.rolloff, k.excursion, k.hard_metric, k.viterbi, k.allow_drift, k.notch_filters, k.finfo };
}

} // namespace

struct DatvFamily : DemodDefaults {
    using Handle = sdrx_datv;
    using Cfg = sdrx_datv_cfg;
    using Chan = DatvChan;
    using Bufs = DatvBufs;
    static constexpr const char* name = "sdrx_datv";
    static constexpr const float2* DatvBufs::* input = &DatvBufs::y;
    // a feed's symbols: at most one per sample of the stream it walks, the held ones and the front's partial block included
    static constexpr int work_extra = DATV_HOLD + 512;

    static int validate(int32_t n_ch, const sdrx_datv_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_datv_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            DatvDesign d;
            const char* text = datv_design(view_of(cfg[c]), d);
            if (text) { set_error("sdrx_datv_create: channel " + std::to_string(c) + ": " + text); return SDRX_EINVAL; }
        }
        return SDRX_OK;
    }

    static void design(int, const sdrx_datv_cfg& k, sdrx_backend_cfg& f, DatvChan& s, float*)
    {
        f.in_rate = k.msps; f.nco_freq = -k.centre_frequency; f.out_rate = k.msps;      // bypass: one filter input per sample
        f.interp_cutoff = k.msps / 2.2f; f.taps_per_phase = 4.5f;                       // a design the bypass never runs
        f.filt_mode = 1;
        // fltLowCut = -((float) intRFBandwidth / 2.0) / (float) intMsps and its mirror: doubles stored as floats
        f.f1 = (float)(-((float)k.rf_bandwidth / 2.0) / (float)k.msps);
        f.f2 = (float)(((float)k.rf_bandwidth / 2.0) / (float)k.msps);
        (void)datv_design(view_of(k), s.d);
        datv_fresh(s.d, s.s);
    }

    static int front_made(sdrx_backend_t* front, int n_ch, const sdrx_datv_cfg*)
    {
        for (int c = 0; c < n_ch; c++) { int rc = backend_set_front(front, c, 1, 0); if (rc) return rc; }
        return SDRX_OK;
    }

    static void hist(HistCarver& k, const DatvChan&, DatvBufs& u) { k.pair(u.held, u.held_next, (size_t)DATV_HOLD); }

    static void work(Carver& k, size_t n, const DatvChan&, DatvBufs& u)
    {
        u.cost = k.take<int16_t>(n);
        u.symbol = k.take<uint8_t>(n);
        u.pts = k.take<float2>(n / DATV_CHUNK + 2);
        u.meas = k.take<DatvMeas>(3 * (n / DATV_CHUNK + 2));
    }

    static int64_t outputs_bound(const sdrx_datv_cfg&, int64_t n_in) { return n_in; }

    static int launch(DemodBank<DatvFamily>& b, unsigned nc, unsigned gx);
};

// the handle: the bank and the design's tables
struct sdrx_datv : DemodBank<DatvFamily> {
    float* d_trig = nullptr;
    char* d_tab = nullptr;                  // per distinct constellation: lut 65536 * 8 | symbols 512; then per channel its coefficients
    std::vector<float> trig;
    std::vector<DatvCstln> cstln;
    std::vector<int> cstln_of;              // channel -> index into cstln
    std::vector<std::vector<float>> coeffs;
};
using Bank = DemodBank<DatvFamily>;
constexpr size_t TAB_CSTLN = 65536 * sizeof(DatvLutEntry) + 512;

int DatvFamily::launch(DemodBank<DatvFamily>& bank, unsigned nc, unsigned)
{
    sdrx_datv& b = static_cast<sdrx_datv&>(bank);
    hipLaunchKernelGGL(datv_walk_kernel, dim3(nc), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
    SDRX_HIP(hipGetLastError());
    b.core.note_launch("datv_walk_kernel", (int)nc, 64, (int)((DATV_NCOEFFS_MAX + DATV_WIN + 256) * sizeof(float2)));
    return SDRX_OK;
}

static int datv_destroy(sdrx_datv* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    if (b->d_trig) (void)hipFree(b->d_trig);
    if (b->d_tab) (void)hipFree(b->d_tab);
    return Bank::destroy(b);
}

// the tables go up once; the channels' pointers go up with the fresh state
static int datv_make_tables(sdrx_datv* b)
{
    SDRX_HIP(hipSetDevice(b->core.device));
    const int n_ch = b->n_ch;
    datv_trig_table(b->trig);
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_trig), b->trig.size() * 4));
    SDRX_HIP(hipMemcpy(b->d_trig, b->trig.data(), b->trig.size() * 4, hipMemcpyHostToDevice));
    std::map<std::tuple<int, int, int>, int> seen;
    b->cstln_of.assign((size_t)n_ch, 0); b->coeffs.assign((size_t)n_ch, {});
    size_t coeff_bytes = 0;
    for (int c = 0; c < n_ch; c++) {
        const sdrx_datv_cfg& k = b->cfg[(size_t)c];
        // the radii hang on the code rate for 16APSK and 32APSK only
        const int fec_key = (k.modulation == DATV_APSK16 || k.modulation == DATV_APSK32) ? k.fec : 0;
        const auto key = std::make_tuple(k.modulation, fec_key, k.hard_metric != 0);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int)b->cstln.size()).first;
            b->cstln.emplace_back();
            datv_constellation(k.modulation, k.fec, k.hard_metric != 0, b->cstln.back());
        }
        b->cstln_of[(size_t)c] = it->second;
        const DatvDesign& d = b->h_chan[(size_t)c].d;
        if (d.sampler == DATV_SAMP_RRC) datv_rrc_coeffs(view_of(k), d, b->coeffs[(size_t)c]);
        coeff_bytes += Carver::al(b->coeffs[(size_t)c].size() * 4);
    }
    const size_t cstln_bytes = b->cstln.size() * TAB_CSTLN;
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_tab), cstln_bytes + coeff_bytes + 256));
    for (size_t i = 0; i < b->cstln.size(); i++) {
        char* base = b->d_tab + i * TAB_CSTLN;
        SDRX_HIP(hipMemcpy(base, b->cstln[i].lut.data(), 65536 * sizeof(DatvLutEntry), hipMemcpyHostToDevice));
        SDRX_HIP(hipMemcpy(base + 65536 * sizeof(DatvLutEntry), b->cstln[i].symbols, 512, hipMemcpyHostToDevice));
    }
    size_t off = cstln_bytes;
    for (int c = 0; c < n_ch; c++) {
        DatvChan& s = b->h_chan[(size_t)c];
        char* base = b->d_tab + (size_t)b->cstln_of[(size_t)c] * TAB_CSTLN;
        s.trig = reinterpret_cast<const float2*>(b->d_trig);
        s.lut = reinterpret_cast<const DatvLutEntry*>(base);
        s.symbols = reinterpret_cast<const signed char*>(base + 65536 * sizeof(DatvLutEntry));
        s.coeffs = reinterpret_cast<const float*>(b->d_tab + off);
        const std::vector<float>& co = b->coeffs[(size_t)c];
        if (!co.empty()) SDRX_HIP(hipMemcpy(b->d_tab + off, co.data(), co.size() * 4, hipMemcpyHostToDevice));
        off += Carver::al(co.size() * 4);
    }
    return Bank::upload_fresh_state(b);
}

extern "C" {

int sdrx_datv_create(sdrx_datv_t** out, int device, int32_t n_ch, const sdrx_datv_cfg* cfg)
{
    int rc = Bank::create(out, device, n_ch, cfg); if (rc) return rc;
    rc = datv_make_tables(*out);
    if (rc) { datv_destroy(*out); *out = nullptr; }
    return rc;
}
int sdrx_datv_destroy(sdrx_datv_t* b) { return datv_destroy(b); }
int sdrx_datv_reset(sdrx_datv_t* b) { return Bank::reset(b); }
int sdrx_datv_feed_dev(sdrx_datv_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_datv_feed_bank(sdrx_datv_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_datv_feed(sdrx_datv_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }

int64_t sdrx_datv_read(sdrx_datv_t* b, int32_t c, int16_t* cost, uint8_t* symbol, int64_t cap)
{
    if (cap < 0) return Bank::fail("read", ": bad argument");
    int64_t n = 0;
    if (cost || !symbol) { n = Bank::read(b, "read", c, cost, cost ? cap : 0, &DatvBufs::cost, &DatvChan::n_sym, 2); if (n < 0) return n; }
    if (symbol) n = Bank::read(b, "read", c, symbol, cap, &DatvBufs::symbol, &DatvChan::n_sym, 1);
    return n;
}
int64_t sdrx_datv_read_points(sdrx_datv_t* b, int32_t c, float* iq, int64_t cap)
{
    return Bank::read(b, "read_points", c, reinterpret_cast<float2*>(iq), cap, &DatvBufs::pts, &DatvChan::n_pts, 8);
}
int64_t sdrx_datv_read_meas(sdrx_datv_t* b, int32_t c, sdrx_datv_meas_t* out, int64_t cap)
{
    if (cap < 0 || (cap > 0 && !out)) return Bank::fail("read_meas", ": bad argument");
    DatvChan s;
    int rc = Bank::fetch(b, "read_meas", c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n_meas, cap);
    if (n == 0) return 0;
    std::vector<DatvMeas> m((size_t)n);
    SDRX_HIP(hipMemcpy(m.data(), b->h_bufs[c].meas, (size_t)n * sizeof(DatvMeas), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {
        const DatvMeas& v = m[(size_t)i];
        out[i].freq = v.freq_tap; out[i].ss = datv_meas_ss(v); out[i].mer = datv_meas_mer(v);
        out[i].est_insp = v.est_insp; out[i].est_sp = v.est_sp; out[i].est_ep = v.est_ep;
    }
    return n;
}
int sdrx_datv_last_dev(sdrx_datv_t* b, int32_t c, const int16_t** d_cost, const uint8_t** d_symbol, int64_t* n)
{
    if (!n) return Bank::fail("last_dev", ": bad argument");
    const int16_t* pc = nullptr;
    int rc = Bank::last_dev(b, "last_dev", c, &pc, n, &DatvBufs::cost, &DatvChan::n_sym); if (rc) return rc;
    if (d_cost) *d_cost = pc;
    if (d_symbol) *d_symbol = *n > 0 ? b->h_bufs[c].symbol : nullptr;
    return SDRX_OK;
}
int sdrx_datv_points_last_dev(sdrx_datv_t* b, int32_t c, const float** d_iq, int64_t* n)
{
    const float2* p = nullptr;
    int rc = Bank::last_dev(b, "points_last_dev", c, &p, n, &DatvBufs::pts, &DatvChan::n_pts); if (rc) return rc;
    if (d_iq) *d_iq = reinterpret_cast<const float*>(p);
    return SDRX_OK;
}
int sdrx_datv_meas_last_dev(sdrx_datv_t* b, int32_t c, const float** d_meas, int64_t* n)
{
    const DatvMeas* p = nullptr;
    int rc = Bank::last_dev(b, "meas_last_dev", c, &p, n, &DatvBufs::meas, &DatvChan::n_meas); if (rc) return rc;
    if (d_meas) *d_meas = reinterpret_cast<const float*>(p);
    return SDRX_OK;
}

int sdrx_datv_state(sdrx_datv_t* b, int32_t c, sdrx_datv_state_t* out)
{
    if (!out) return Bank::fail("state", ": bad argument");
    DatvChan q;
    int rc = Bank::fetch(b, "state", c, &q); if (rc) return rc;
    const DatvState& s = q.s;
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    std::memset(out, 0, sizeof *out);
    out->mu = bits(s.mu); out->phase = bits(s.phase); out->freqw = bits(s.freqw); out->agc_gain = bits(s.agc_gain);
    out->est_insp = bits(s.est_insp); out->est_sp = bits(s.est_sp); out->est_ep = bits(s.est_ep);
    out->meas_count = s.meas_count; out->update_freq_phase = s.update_freq_phase;
    for (int k = 0; k < 3; k++) {
        out->hist_p[k][0] = bits(s.hist[k].pr); out->hist_p[k][1] = bits(s.hist[k].pi);
        out->hist_c[k][0] = bits(s.hist[k].cr); out->hist_c[k][1] = bits(s.hist[k].ci);
    }
    out->held = s.held; out->chunks = s.chunks; out->n_in = s.n_in; out->n_symbols = s.n_symbols;
    return SDRX_OK;
}

int sdrx_datv_get_design(sdrx_datv_t* b, int32_t c, sdrx_datv_design_t* out)
{
    if (!out || !Bank::in_range(b, c)) return Bank::fail("get_design", ": bad argument");
    const DatvDesign& d = b->h_chan[(size_t)c].d;
    out->omega = d.omega; out->min_omega = d.min_omega; out->max_omega = d.max_omega; out->min_freqw = d.min_freqw; out->max_freqw = d.max_freqw;
    out->freq_beta = d.freq_beta; out->meas_decimation = (int32_t)d.meas_decimation;
    out->rrc_steps = d.sampler == DATV_SAMP_RRC ? d.subsampling : 0; out->ncoeffs = d.ncoeffs; out->readahead = d.readahead; out->nsymbols = d.nsymbols;
    return sdrx_backend_get_design(b->front, c, nullptr, nullptr, 0, nullptr, &out->nco_inc);
}

int sdrx_datv_get_tables(sdrx_datv_t* b, int32_t c, float* coeffs, int32_t coeffs_cap, float* trig_iq, void* lut, int8_t* symbols)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_tables", ": bad argument");
    const std::vector<float>& co = b->coeffs[(size_t)c];
    if (coeffs && coeffs_cap > 0 && !co.empty()) std::memcpy(coeffs, co.data(), std::min<size_t>(co.size(), (size_t)coeffs_cap) * 4);
    if (trig_iq) std::memcpy(trig_iq, b->trig.data(), b->trig.size() * 4);
    const DatvCstln& k = b->cstln[(size_t)b->cstln_of[(size_t)c]];
    if (lut) std::memcpy(lut, k.lut.data(), 65536 * sizeof(DatvLutEntry));
    if (symbols) std::memcpy(symbols, k.symbols, 512);
    return (int)co.size();
}

int sdrx_datv_sync(sdrx_datv_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_datv_set_stream(sdrx_datv_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_datv_get_stream(sdrx_datv_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_datv_set_timing(sdrx_datv_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_datv_get_timing(sdrx_datv_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_datv_last_launch(const sdrx_datv_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
