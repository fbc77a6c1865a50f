// Host-side design shared by the channel back-end and the WFM demodulator, exactly as the reference does it at configure
// time: Interpolator::create (interpolator.cpp:21-129) and the tap tables channels share, the NCO and g_fft cosine tables,
// the search for a dyadic resampling step, and the fsinc / blackman helpers of fftfilt (fftfilt.h:52-64) with the impulse
// responses built from them.  Plain C++ up to the last part, which a HIP compiler sees: table uploads, the filter's FFT.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace sdrx {

const double PI_D = 3.14159265358979323846;

// Interpolator::createPolyphaseLowPass + reorder + per-phase normalisation
inline void design_interp(int phase_steps, double sample_rate, double cutoff, double tpp, std::vector<float>& poly, int* ntaps_per_phase)
{
    double gain = 1.0;
    const double fs = phase_steps * sample_rate;
    int ntaps = (int)(tpp * phase_steps);
    if ((ntaps % 2) != 0) ntaps++;
    ntaps *= phase_steps;
    std::vector<float> taps((size_t)ntaps, 0.0f), window((size_t)ntaps);
    for (int n = 0; n < ntaps; n++) window[(size_t)n] = (float)(0.54 - 0.46 * std::cos((2 * PI_D * n) / (ntaps - 1)));
    const int M = (ntaps - 1) / 2;
    const double fwT0 = 2 * PI_D * cutoff / fs;
    for (int n = -M; n <= M; n++) {
        if (n == 0) taps[(size_t)(n + M)] = (float)(fwT0 / PI_D * window[(size_t)(n + M)]);
        else taps[(size_t)(n + M)] = (float)(std::sin(n * fwT0) / (n * PI_D) * window[(size_t)(n + M)]);
    }
    double mx = taps[(size_t)M];
    for (int n = 1; n <= M; n++) mx += 2.0 * taps[(size_t)(n + M)];
    gain /= mx;
    for (int i = 0; i < ntaps; i++) taps[(size_t)i] = (float)(taps[(size_t)i] * gain);
    const int nt = ntaps / phase_steps;
    poly.assign((size_t)ntaps, 0.0f);
    for (int ph = 0; ph < phase_steps; ph++)
        for (int i = 0; i < nt; i++) poly[(size_t)(ph * nt + i)] = taps[(size_t)(i * phase_steps + ph)];
    for (int ph = 0; ph < phase_steps; ph++) {
        float sum = 0;
        for (int i = 0; i < nt; i++) sum += poly[(size_t)(ph * nt + i)];
        for (int i = 0; i < nt; i++) poly[(size_t)(ph * nt + i)] /= sum;
    }
    *ntaps_per_phase = nt;
}

// channels with the same Interpolator::create(16, rate, cutoff, taps per phase) arguments share one tap table; add() is
// called once per channel, in channel order
struct InterpTables {
    std::vector<double> args;             // per channel: rate, cutoff, taps per phase
    std::vector<float> all;               // the tables back to back
    std::vector<int> off, ntaps;          // per channel: float offset into `all`, taps per phase
    void add(double rate, double cutoff, double tpp, int phase_steps = 16)   // one phase count per table set
    {
        size_t p = 0;
        while (p < off.size() && !(args[3 * p] == rate && args[3 * p + 1] == cutoff && args[3 * p + 2] == tpp)) p++;
        if (p < off.size()) { off.push_back(off[p]); ntaps.push_back(ntaps[p]); }
        else {
            std::vector<float> poly; int nt = 0;
            design_interp(phase_steps, rate, cutoff, tpp, poly, &nt);
            off.push_back((int)all.size()); ntaps.push_back(nt);
            all.insert(all.end(), poly.begin(), poly.end());
        }
        args.insert(args.end(), { rate, cutoff, tpp });
    }
};

// NCO::initTable (nco.cpp:30-39)
inline std::vector<float> design_nco_table(int n)
{
    std::vector<float> t((size_t)n);
    for (int i = 0; i < n; i++) t[(size_t)i] = (float)std::cos((2.0 * PI_D * i) / n);
    return t;
}

// g_fft::fftCosInit for an n-point transform (gfft.h:141-150): n / 4 + 1 entries
inline std::vector<float> design_gfft_table(int n)
{
    std::vector<float> utbl((size_t)n / 4 + 1);
    utbl[0] = 1.0f;
    for (int i = 1; i < n / 4; i++) utbl[(size_t)i] = (float)std::cos((2.0 * 3.141592653589793238462643383279502884197 * (float)i) / (float)n);
    utbl[(size_t)n / 4] = 0.0f;
    return utbl;
}

// Where step * 2^q is an integer below 2^20 for some q <= 10, the resampler's schedule has a closed form with Q = 1 << q
// and S = step * Q.  *q is -1 where there is none, where step < 1, and everywhere while the variable `serial_env` is set.
inline void design_dyadic_step(float step, const char* serial_env, int* q_out, int* S_out)
{
    *q_out = -1; *S_out = 0;
    if (!(step >= 1.0f) || std::getenv(serial_env)) return;
    for (int q = 0; q <= 10; q++) {
        const float v = step * (float)(1 << q);                                  // exact (power of two)
        if (v == std::floor(v) && v < (float)(1 << 20)) { *q_out = q; *S_out = (int)v; break; }
    }
}

inline float fsinc(float fc, int i, int len)
{
    const int len2 = len / 2;
    return (i == len2) ? (float)(2.0 * fc) : (float)(std::sin(2 * PI_D * fc * (i - len2)) / (PI_D * (i - len2)));
}
inline float blackman(int i, int len)
{
    return (float)(0.42 - 0.50 * std::cos(2.0 * PI_D * i / len) + 0.08 * std::cos(4.0 * PI_D * i / len));
}

// the real parts of fftfilt's impulse response before the window, h2 complex bins at f[2 * i]:
// create_filter(f1, f2) (fftfilt.cpp:108-146): low pass at f2 minus low pass at f1, plus 1 at the centre for a band stop
inline void fftfilt_fill_band(float f1, float f2, float* f, int h2)
{
    const bool lp = f2 != 0, hp = f1 != 0;
    for (int i = 0; i < h2; i++) {
        float v = 0;
        if (lp) v += fsinc(f2, i, h2);
        if (hp) v -= fsinc(f1, i, h2);
        f[(size_t)(2 * i)] = v;
    }
    if (hp && f2 < f1) f[(size_t)(2 * (h2 / 2))] += 1;
}
// create_dsb_filter(fc) and either half of create_asym_filter: a low pass at fc
inline void fftfilt_fill_lowpass(float fc, float* f, int h2)
{
    for (int i = 0; i < h2; i++) f[(size_t)(2 * i)] = fsinc(fc, i, h2);
}

// create_rrc_filter(fb, a) (fftfilt.cpp:223-246) with frrc (fftfilt.h:68-87): the root raised cosine written straight into the
// len complex bins at f[2 * i], f[2 * i + 1], then normalised to max |H| over all of them.  frrc's operand order and widths:
// x and tr are floats, the fold and the transition's argument are double expressions stored as floats, and cos() sees a float.
inline void fftfilt_rrc(float fb, float a, float* f, int len)
{
    for (int i = 0; i < len; i++) {
        float x = i / (float)len;
        x = (float)(0.5 - std::fabs((double)x - 0.5));
        const float tr = fb * a;
        float v;
        if (x < fb - tr) v = 1.0f;
        else if (x < fb + tr) {
            const float y = (float)(((double)(x - (fb - tr)) / (2.0 * (double)tr)) * PI_D);
            v = (std::cos(y) + 1.0f) / 2.0f;
        } else v = 0.0f;
        f[(size_t)(2 * i)] = v; f[(size_t)(2 * i + 1)] = 0.0f;
    }
    float scale = 0;
    for (int i = 0; i < len; i++) { const float mag = hypotf(f[(size_t)(2 * i)], f[(size_t)(2 * i + 1)]); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < 2 * len; i++) f[(size_t)i] /= scale;
}

#if defined(__HIPCC__)          // after sdrx_common.hpp and gfft_kernel.hpp
// a design table into device memory of its own
inline int design_upload(float** dst, const std::vector<float>& t)
{
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(dst), t.size() * 4));
    SDRX_HIP(hipMemcpy(*dst, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    return SDRX_OK;
}

// fftfilt::create_filter and its kin (fftfilt.cpp:108-146) for an FLEN-point filter at dst: fill(f, FLEN / 2) writes the
// impulse response's real parts, then the Blackman window, the forward FFT by the kernel code of the data path (utbl:
// design_gfft_table(FLEN) on the device), normalisation to max |H| over bins 0 .. FLEN / 2 - 1, and back to dst; host_copy
// gets the FLEN complex bins.  FLEN is a template argument so that a file instantiates only the kernels it had.
template <int FLEN, class Fill>
int design_fft_filter(float2* dst, const float* utbl, hipStream_t stream, float* host_copy, Fill fill)
{
    constexpr int h2 = FLEN / 2;
    std::vector<float> f((size_t)FLEN * 2, 0.0f);
    fill(f.data(), h2);
    for (int i = 0; i < h2; i++) { const float w = blackman(i, h2); f[(size_t)(2 * i)] *= w; f[(size_t)(2 * i + 1)] *= w; }
    SDRX_HIP(hipMemcpy(dst, f.data(), (size_t)FLEN * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(be_fft_design_kernel<FLEN>, dim3(1), dim3(FLEN / 8), 0, stream, dst, utbl);
    SDRX_HIP(hipGetLastError());
    SDRX_HIP(hipStreamSynchronize(stream));
    SDRX_HIP(hipMemcpy(f.data(), dst, (size_t)FLEN * 8, hipMemcpyDeviceToHost));
    float scale = 0;
    for (int i = 0; i < h2; i++) { const float mag = hypotf(f[(size_t)(2 * i)], f[(size_t)(2 * i + 1)]); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < FLEN * 2; i++) f[(size_t)i] /= scale;
    SDRX_HIP(hipMemcpy(dst, f.data(), (size_t)FLEN * 8, hipMemcpyHostToDevice));
    std::copy(f.begin(), f.end(), host_copy);
    return SDRX_OK;
}
#endif

} // namespace sdrx
