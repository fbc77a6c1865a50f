/* Strict-IEEE C restatement of NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:140-332) with m_ctcssOn and
 * m_deltaSquelch (AFSquelch, sdrbase/dsp/afsquelch.cpp, with its MovingAverage<double> pair; DoubleBufferFIFO::zeroBack): tests/nfm_oracle.c's loop, whose containers and derivations are taken as they are (the file is included), with
 * m_sampleCount, the Lowpass (sdrbase/dsp/lowpass.h), the CTCSSDetector (sdrbase/dsp/ctcssdetector.cpp) and m_ctcssIndex in the
 * reference's statement order.  The checker of sdrx_nfm_create_ex: tests build it like tests/nfm_oracle.c and call it through
 * ctypes; the product never links it.
 * The detector's u0, u1 and power start at 0 (the reference allocates them with new Real[] and never resets them; include/sdrx.h
 * states the ruling).
 *
 *   nfmto_create(<nfmo_create's arguments>, ctcss_on, ctcss_index, delta_squelch)
 *   nfmto_af(h, &af_open, sums[2], &count)   m_afSquelchOpen, the two MovingAverage sums, AFSquelch::m_squelchCount
 *   nfmto_af_probe(h, out[6])             AF block ends, maxPower == 0 returns, second evaluates, zeroing events, reads that
 *                                         returned a zeroed copy, reads whose other copy an event had cleared
 *   nfmto_feed(h, iq, n, audio, cap)      as nfmo_feed; the index changes of this feed are kept for nfmto_events
 *   nfmto_events(h, at, index, cap)       audio sample position in the last feed and new m_ctcssIndex of every change; returns their count
 *   nfmto_ctcss(h, &index, &n_changes)
 *   nfmto_powers(h, power[32], &detected, &max_index, &n_blocks)   of the last completed block
 *   nfmto_design(h, &N, &rate, coef[32], lowpass[151])
 *   nfmto_af_design(h, &N, tones[2], coef[2], &threshold)   AFSquelch as the constructor's setCoefficients leaves it
 *   nfmto_probe(h, out[6])                see the enum below
 *   nfmto_base(h)                         the nfmo inside, for nfmo_levels, nfmo_squelch_open, nfmo_squelch_count, nfmo_probe, nfmo_design
 */
#include "nfm_oracle.c"

#define CT_TONES 32
#define LP_TAPS 301

#define AF_AVG 600                                       /* m_nbAvg: the warm-up count */
/* the histories keep the constructor's 128 entries: setCoefficients' m_movingAverages.resize(m_nTones, ...) finds the vector
 * at that size already and changes nothing */
#define AF_MA 128
#define AF_ATTACK 200
enum { A_BLOCK_ENDS, A_MAX_ZERO, A_SECOND_EVAL, A_ZERO_EVENTS, A_ZEROED_READS, A_OTHER_COPY, A_N };

void nfmto_af_design(void* p, int* N, double* tones, double* coef, double* threshold);

enum { T_BLOCKS, T_DETECTIONS, T_CHG_BLOCK, T_CHG_CLOSE, T_MISMATCH, T_DET_SAMPLES, T_N };

static const float TONE_SET[CT_TONES] = {67.0f, 71.9f, 74.4f, 77.0f, 79.7f, 82.5f, 85.4f, 88.5f, 91.5f, 94.8f, 97.4f, 100.0f, 103.5f,
                                         107.2f, 110.9f, 114.8f, 118.8f, 123.0f, 127.3f, 131.8f, 136.5f, 141.3f, 146.2f, 151.4f, 156.7f,
                                         162.2f, 167.9f, 173.8f, 179.9f, 186.2f, 192.8f, 203.5f};

typedef struct {
    nfmo* b;
    int ctcss_on, selected, index, sample_count;
    /* Lowpass */
    float lp_taps[LP_TAPS / 2 + 1], lp_samples[LP_TAPS]; int lp_ptr;
    /* CTCSSDetector */
    int N, rate, processed, max_index, detected;
    float max_power, coef[CT_TONES], u0[CT_TONES], u1[CT_TONES], power[CT_TONES], last_power[CT_TONES];
    long n_changes, n_blocks, probe[T_N];
    long* ev_at; int* ev_idx; long n_ev, ev_cap;
    /* AFSquelch */
    int delta, af_N, af_processed, af_avg_processed, af_count, af_is_open, af_open, af_z;
    double af_coef[2], af_thr, af_u0[2], af_u1[2], af_power[2];
    double ma_hist[2][AF_MA], ma_sum[2]; unsigned ma_idx[2];
    unsigned char* dl_zeroed;                                /* per slot of the doubled array: cleared by zeroBack since its write */
    long aprobe[A_N];
} nfmto;

/* MovingAverage<double>::feed */
static void ma_feed(nfmto* h, int j, double value)
{
    double* oldest = &h->ma_hist[j][h->ma_idx[j]];
    h->ma_sum[j] += value - *oldest;
    *oldest = value;
    if (h->ma_idx[j] < AF_MA - 1) h->ma_idx[j]++; else h->ma_idx[j] = 0;
}

static int af_evaluate(nfmto* h)
{
    double maxPower = 0.0, minPower;
    int minIndex = 0, maxIndex = 0, j;
    for (j = 0; j < 2; j++) if (h->ma_sum[j] > maxPower) { maxPower = h->ma_sum[j]; maxIndex = j; }
    if (maxPower == 0.0) { h->aprobe[A_MAX_ZERO]++; return h->af_is_open; }
    minPower = maxPower;
    for (j = 0; j < 2; j++) if (h->ma_sum[j] < minPower) { minPower = h->ma_sum[j]; minIndex = j; }
    if ((minPower / maxPower < h->af_thr) && (minIndex > maxIndex)) { if (h->af_count < AF_ATTACK + 0) h->af_count++; }
    else { if (h->af_count > AF_ATTACK) h->af_count--; else h->af_count = 0; }
    h->af_is_open = (h->af_count >= AF_ATTACK);
    return h->af_is_open;
}

static int af_analyze(nfmto* h, double sample)
{
    int j;
    for (j = 0; j < 2; j++) {
        const double t = h->af_u0[j];
        h->af_u0[j] = sample + (h->af_coef[j] * h->af_u0[j]) - h->af_u1[j];
        h->af_u1[j] = t;
    }
    if (h->af_processed < h->af_N) { h->af_processed++; return 0; }
    for (j = 0; j < 2; j++) {
        h->af_power[j] = (h->af_u0[j] * h->af_u0[j]) + (h->af_u1[j] * h->af_u1[j]) - (h->af_coef[j] * h->af_u0[j] * h->af_u1[j]);
        ma_feed(h, j, h->af_power[j]);
        h->af_u0[j] = 0.0; h->af_u1[j] = 0.0;
    }
    h->aprobe[A_BLOCK_ENDS]++;
    af_evaluate(h);
    h->af_processed = 0;
    if (h->af_avg_processed < AF_AVG) { h->af_avg_processed++; return 0; }
    return 1;
}

/* DoubleBufferFIFO::zeroBack */
static void dl_zero_back(nfmto* t, int delay)
{
    nfmo* h = t->b;
    if (delay > h->dl_size) delay = h->dl_size;
    for (int i = 0; i < delay; i++) { h->dl[h->dl_cur + h->dl_size - i] = 0; t->dl_zeroed[h->dl_cur + h->dl_size - i] = 1; }
}

static void lowpass_create(nfmto* h, int nTaps, double sampleRate, double cutoff)
{
    const double wc = 2.0 * PI_D * cutoff, Wc = wc / sampleRate;
    const int nt = nTaps / 2 + 1;
    int i;
    for (i = 0; i < nt; i++) {
        if (i == (nTaps - 1) / 2) h->lp_taps[i] = (float)(Wc / PI_D);
        else h->lp_taps[i] = (float)(sin(((double)i - ((double)nTaps - 1.0) / 2.0) * Wc) / (((double)i - ((double)nTaps - 1.0) / 2.0) * PI_D));
    }
    for (i = 0; i < nt; i++)
        h->lp_taps[i] = (float)(h->lp_taps[i] * (0.54 + 0.46 * cos((2.0 * PI_D * ((double)i - ((double)nTaps - 1.0) / 2.0)) / (double)nTaps)));
    float sum = 0;
    for (i = 0; i < nt - 1; i++) sum += h->lp_taps[i] * 2;
    sum += h->lp_taps[i];
    for (i = 0; i < nt; i++) h->lp_taps[i] /= sum;
    memset(h->lp_samples, 0, sizeof h->lp_samples);
    h->lp_ptr = 0;
}

static float lowpass_filter(nfmto* h, float sample)
{
    float acc = 0;
    int a = h->lp_ptr, b = a - 1, i;
    const int size = LP_TAPS, n_taps = LP_TAPS / 2;
    h->lp_samples[h->lp_ptr] = sample;
    while (b < 0) b += size;
    for (i = 0; i < n_taps; i++) {
        acc += (h->lp_samples[a] + h->lp_samples[b]) * h->lp_taps[i];
        a++; while (a >= size) a -= size;
        b--; while (b < 0) b += size;
    }
    acc += h->lp_samples[a] * h->lp_taps[i];
    h->lp_ptr++; while (h->lp_ptr >= size) h->lp_ptr -= size;
    return acc;
}

/* CTCSSDetector::analyze */
static int detector_analyze(nfmto* h, float in)
{
    int j;
    for (j = 0; j < CT_TONES; j++) {                         /* feedback */
        const float t = h->u0[j];
        h->u0[j] = in + (h->coef[j] * h->u0[j]) - h->u1[j];
        h->u1[j] = t;
    }
    h->processed += 1;
    if (h->processed != h->N) return 0;
    for (j = 0; j < CT_TONES; j++) h->power[j] = 0.0f;       /* feedForward */
    for (j = 0; j < CT_TONES; j++) {
        h->power[j] = (h->u0[j] * h->u0[j]) + (h->u1[j] * h->u1[j]) - (h->coef[j] * h->u0[j] * h->u1[j]);
        h->u0[j] = h->u1[j] = 0.0f;
    }
    float sumPower = 0.0f;                                   /* evaluatePower */
    const float aboveAvg = 2.0f;
    h->max_power = 0.0f;
    for (j = 0; j < CT_TONES; j++) {
        sumPower += h->power[j];
        if (h->power[j] > h->max_power) { h->max_power = h->power[j]; h->max_index = j; }
    }
    h->detected = h->max_power > (sumPower / CT_TONES) + aboveAvg;
    h->processed = 0;
    memcpy(h->last_power, h->power, sizeof h->power);
    h->n_blocks++; h->probe[T_BLOCKS]++;
    if (h->detected) h->probe[T_DETECTIONS]++;
    return 1;
}

static void set_index(nfmto* h, int v, long pos, int why)
{
    if (v == h->index) return;
    h->index = v; h->n_changes++; h->probe[why]++;
    if (h->n_ev == h->ev_cap) {
        h->ev_cap = h->ev_cap ? 2 * h->ev_cap : 64;
        h->ev_at = (long*)realloc(h->ev_at, sizeof(long) * (size_t)h->ev_cap);
        h->ev_idx = (int*)realloc(h->ev_idx, sizeof(int) * (size_t)h->ev_cap);
    }
    h->ev_at[h->n_ev] = pos; h->ev_idx[h->n_ev] = v; h->n_ev++;
}

void* nfmto_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float af_bw, int fm_deviation, float volume, float squelch,
                   int squelch_gate, int mute, int ctcss_on, int ctcss_index, int delta_squelch)
{
    nfmto* h = (nfmto*)calloc(1, sizeof(nfmto));
    h->b = (nfmo*)nfmo_create(in_rate, nco_freq, audio_rate, rf_bw, af_bw, fm_deviation, volume, squelch, squelch_gate, mute);
    h->ctcss_on = ctcss_on; h->selected = ctcss_index;
    /* m_ctcssDetector.setCoefficients(m_audioSampleRate / 16, m_audioSampleRate / 8.0f), m_audioSampleRate a uint32_t */
    h->N = (int)((uint32_t)audio_rate / 16u);
    h->rate = (int)((float)(uint32_t)audio_rate / 8.0f);
    for (int j = 0; j < CT_TONES; j++) h->coef[j] = (float)(2.0 * cos((2.0 * PI_D * TONE_SET[j]) / (double)h->rate));
    lowpass_create(h, LP_TAPS, (double)audio_rate, 250.0);
    /* m_afSquelch.setCoefficients(rate / 2000, 600, rate, 200, 0, {1000, 6000}); applySettings with m_deltaSquelch:
     * m_squelchLevel = (-m_squelch) / 1000.0 (a Real), setThreshold(m_squelchLevel), reset() */
    h->delta = delta_squelch;
    int afn; double tones[2], thr;
    nfmto_af_design(h, &afn, tones, h->af_coef, &thr);
    h->af_N = afn; h->af_thr = thr;
    h->af_z = (int)((unsigned)audio_rate / 10u);
    if (delta_squelch) { h->b->level = (float)((double)(-squelch) / 1000.0); h->af_thr = (double)h->b->level; }
    h->dl_zeroed = (unsigned char*)calloc((size_t)(2 * h->b->dl_size), 1);
    return h;
}

void nfmto_destroy(void* p)
{
    nfmto* h = (nfmto*)p;
    if (!h) return;
    nfmo_destroy(h->b);
    free(h->ev_at); free(h->ev_idx); free(h->dl_zeroed); free(h);
}

static int16_t tone_process_one(nfmto* t, float ci_re, float ci_im, long pos)
{
    nfmo* h = t->b;
    const float fltI = ci_re, fltQ = ci_im;
    const double magsqRaw = (double)(fltI * fltI + fltQ * fltQ);
    const float curArg = atan2_approximation2(fltQ, fltI);
    if (fltI == 0.0f && fltQ == 0.0f) h->probe[P_ZERO_CI]++;
    float fmDev = (float)((double)(curArg - h->prev_arg) / PI_D);
    h->prev_arg = curArg;
    if (fmDev < -1.0f) fmDev += 2.0f; else if (fmDev > 1.0f) fmDev -= 2.0f;
    const float demod = fmDev * h->fm_scaling;

    const float magsq = (float)(magsqRaw / (32768.0 * 32768.0));
    if (h->ma_num < MA_N) { h->ma_samples[h->ma_num++] = magsq; h->ma_total += magsq; }
    else {
        float* oldest = &h->ma_samples[h->ma_index];
        h->ma_total += magsq - *oldest;
        *oldest = magsq;
        h->ma_index = (h->ma_index + 1) % MA_N;
    }
    h->magsq_sum += magsq;
    if (magsq > h->magsq_peak) h->magsq_peak = magsq;
    h->magsq_count++;
    t->sample_count++;

    const int below = (float)(h->ma_total / MA_N) < h->level;
    if (h->last_below >= 0 && below != h->last_below) h->probe[P_BELOW_CHANGES]++;
    h->last_below = below;
    int up = !below;
    if (t->delta) {
        if (af_analyze(t, (double)(demod * h->comp))) {
            t->aprobe[A_SECOND_EVAL]++;
            t->af_open = af_evaluate(t);
            if (!t->af_open) { dl_zero_back(t, t->af_z); t->aprobe[A_ZERO_EVENTS]++; }
        }
        up = t->af_open;
    }
    const float w = up ? demod * h->comp : 0.0f;
    h->dl[h->dl_write] = w; h->dl[h->dl_write + h->dl_size] = w;
    t->dl_zeroed[h->dl_write] = 0; t->dl_zeroed[h->dl_write + h->dl_size] = 0;
    h->dl_cur = h->dl_write;
    if (h->dl_write < h->dl_size - 1) h->dl_write++; else h->dl_write = 0;
    if (!up) { if (h->sq_count > 0) h->sq_count--; }
    else { if (h->sq_count < 2 * h->gate) h->sq_count++; }
    if (h->sq_count == 0) h->probe[P_COUNT_ZERO]++;
    if (h->sq_count == 2 * h->gate) h->probe[P_COUNT_CAP]++;

    const int open = h->sq_count > h->gate;
    if (open != h->sq_open) h->probe[P_TRANSITIONS]++;
    h->sq_open = open;
    int16_t sample;
    if (h->mute) sample = 0;
    else if (open) {
        h->probe[P_OPEN]++;
        if (t->ctcss_on) {
            float ctcss_sample = lowpass_filter(t, demod * h->comp);
            if ((t->sample_count & 7) == 7) {
                t->probe[T_DET_SAMPLES]++;
                if (detector_analyze(t, ctcss_sample)) {
                    if (t->detected) set_index(t, t->max_index + 1, pos, T_CHG_BLOCK);
                    else set_index(t, 0, pos, T_CHG_BLOCK);
                }
            }
        }
        if (t->ctcss_on && t->selected && t->selected != t->index) {
            sample = 0;
            t->probe[T_MISMATCH]++;
        } else {
            int delay = h->gate;
            if (delay > h->dl_size) { delay = h->dl_size; h->probe[P_CLAMPED_READS]++; }
            const int slot = h->dl_cur + h->dl_size - delay;
            if (t->dl_zeroed[slot]) t->aprobe[A_ZEROED_READS]++;
            else if (t->dl_zeroed[slot >= h->dl_size ? slot - h->dl_size : slot + h->dl_size]) t->aprobe[A_OTHER_COPY]++;
            sample = to_q16(bandpass_filter(h, h->dl[slot]) * h->volume);
        }
    } else {
        set_index(t, 0, pos, T_CHG_CLOSE);
        sample = 0;
    }
    if (h->have_last && abs((int)sample - (int)h->last_sample) > 40000) h->probe[P_WRAPS]++;
    h->last_sample = sample; h->have_last = 1;
    return sample;
}

long nfmto_feed(void* p, const int16_t* iq, long n, int16_t* audio, long cap)
{
    nfmto* t = (nfmto*)p;
    nfmo* h = t->b;
    t->n_ev = 0;
    if (n > h->ci_cap) { free(h->ci); h->ci_cap = n + 1024; h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); }
    const long k = n > 0 ? (long)sdro_backend_feed(h->front, iq, n, h->ci) : 0;
    for (long i = 0; i < k && i < cap; i++) audio[i] = tone_process_one(t, h->ci[2 * i], h->ci[2 * i + 1], i);
    return k;
}

long nfmto_events(void* p, long* at, int* index, long cap)
{
    nfmto* t = (nfmto*)p;
    for (long i = 0; i < t->n_ev && i < cap; i++) { at[i] = t->ev_at[i]; index[i] = t->ev_idx[i]; }
    return t->n_ev;
}
void nfmto_ctcss(void* p, int* index, long* n_changes) { nfmto* t = (nfmto*)p; *index = t->index; *n_changes = t->n_changes; }
void nfmto_powers(void* p, float* power, int* detected, int* max_index, long* n_blocks)
{
    nfmto* t = (nfmto*)p;
    memcpy(power, t->last_power, sizeof t->last_power);
    *detected = t->detected; *max_index = t->max_index; *n_blocks = t->n_blocks;
}
void nfmto_design(void* p, int* N, int* rate, float* coef, float* lowpass)
{
    nfmto* t = (nfmto*)p;
    *N = t->N; *rate = t->rate;
    memcpy(coef, t->coef, sizeof t->coef); memcpy(lowpass, t->lp_taps, sizeof t->lp_taps);
}
/* AFSquelch::setCoefficients(m_audioSampleRate / 2000, 600, m_audioSampleRate, 200, 0, {1000.0, 6000.0}) (afsquelch.cpp:77-118):
 * unsigned rate, every tone capped at 0.4 * rate, the threshold left at 0.0 (only applySettings with m_deltaSquelch sets one) */
void nfmto_af_design(void* p, int* N, double* tones, double* coef, double* threshold)
{
    const unsigned rate = (unsigned)((nfmto*)p)->b->rate;
    const double in[2] = {1000.0, 6000.0};
    *N = (int)(rate / 2000u);
    for (int j = 0; j < 2; j++) {
        tones[j] = in[j] < ((double)rate) * 0.4 ? in[j] : ((double)rate) * 0.4;
        coef[j] = 2.0 * cos((2.0 * PI_D * tones[j]) / (double)rate);
    }
    *threshold = ((nfmto*)p)->delta ? ((nfmto*)p)->af_thr : 0.0;
}
void nfmto_af(void* p, int* af_open, double* sums, int* count)
{
    nfmto* t = (nfmto*)p;
    *af_open = t->af_open; sums[0] = t->ma_sum[0]; sums[1] = t->ma_sum[1]; *count = t->af_count;
}
void nfmto_af_probe(void* p, long* out) { memcpy(out, ((nfmto*)p)->aprobe, sizeof(long) * A_N); }
float nfmto_level(void* p) { return ((nfmto*)p)->b->level; }
void nfmto_probe(void* p, long* out) { memcpy(out, ((nfmto*)p)->probe, sizeof(long) * T_N); }
void* nfmto_base(void* p) { return ((nfmto*)p)->b; }
