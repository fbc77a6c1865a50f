// Recorder of the reference's own SpectrumVis (sdrgui/dsp/spectrumvis.cpp, v4.0.6, kissfft engine), linked from the
// reference's sources by tests/golden/make_golden_spectrum.py.  GLSpectrum is replaced by a header of the same name
// that the recipe writes (only newSpectrum is used), and this file records each newSpectrum call.
//
//   spectrum_rec <input.bin> <output.bin>   commands on stdin, one per line:
//     cfg N pct avg_nb mode window linear    SpectrumVis::handleMessage(MsgConfigureSpectrumVis(...)) == handleConfigure
//     feed n positive_only                   feed() of the next n Samples of input.bin (int16 I, Q)
//     new scalef                             a fresh SpectrumVis(scalef)
//   output.bin: per feed, int64 frame count, int64 fft size, then the frames (float32)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "dsp/spectrumvis.h"
#include "gui/glspectrum.h"

static std::vector<std::vector<float>> g_frames;

void GLSpectrum::newSpectrum(const std::vector<Real>& spectrum, int fftSize)
{
    g_frames.emplace_back(spectrum.begin(), spectrum.begin() + fftSize);
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: spectrum_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    GLSpectrum gl;
    SpectrumVis* vis = new SpectrumVis(32768.0f, &gl);
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            float scalef = 32768.0f;
            std::sscanf(line, "%*s %f", &scalef);
            delete vis;
            vis = new SpectrumVis(scalef, &gl);
        } else if (!std::strcmp(cmd, "cfg")) {
            int n, pct, mode, win, lin; unsigned avg;
            if (std::sscanf(line, "%*s %d %d %u %d %d %d", &n, &pct, &avg, &mode, &win, &lin) != 6) return 3;
            SpectrumVis::MsgConfigureSpectrumVis msg(n, pct, avg, mode, (FFTWindow::Function)win, lin != 0);
            vis->handleMessage(msg);
        } else if (!std::strcmp(cmd, "feed")) {
            long n; int po;
            if (std::sscanf(line, "%*s %ld %d", &n, &po) != 2) return 3;
            SampleVector s((size_t)n);
            for (long i = 0; i < n; i++) {
                int16_t iq[2];
                if (std::fread(iq, 2, 2, in) != 2) return 4;
                s[(size_t)i] = Sample(iq[0], iq[1]);
            }
            g_frames.clear();
            vis->feed(s.begin(), s.end(), po != 0);
            const int64_t k = (int64_t)g_frames.size(), nfft = k ? (int64_t)g_frames[0].size() : 0;
            std::fwrite(&k, 8, 1, out); std::fwrite(&nfft, 8, 1, out);
            for (auto& f : g_frames) std::fwrite(f.data(), 4, f.size(), out);
        }
    }
    delete vis;
    std::fclose(out);
    return 0;
}
