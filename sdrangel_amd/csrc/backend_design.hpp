// Host-side design shared by the channel back-end and the WFM demodulator, exactly as the reference does it at configure
// time: Interpolator::create (interpolator.cpp:21-129) and the fsinc / blackman helpers of fftfilt (fftfilt.h:52-64).
#pragma once
#include <cmath>
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

inline float fsinc(float fc, int i, int len)
{
    const int len2 = len / 2;
    return (i == len2) ? (float)(2.0 * fc) : (float)(std::sin(2 * PI_D * fc * (i - len2)) / (PI_D * (i - len2)));
}
inline float blackman(int i, int len)
{
    return (float)(0.42 - 0.50 * std::cos(2.0 * PI_D * i / len) + 0.08 * std::cos(4.0 * PI_D * i / len));
}

} // namespace sdrx
