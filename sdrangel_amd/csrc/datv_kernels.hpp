// DATV receiver bank kernel: leansdr's cstln_receiver<f32>::run with its sampler (plugins/channelrx/demoddatv/leansdr/sdr.h:
// 699-1105) behind DATVDemod::feed's NCO mix and RF filter (datvdemod.cpp:826-859).  The front -- the mix and fftfilt::runFilt on
// 1024 points -- is the channel back-end's in bypass with filter mode 1; this kernel starts from its output, the samples
// p_rawiq_writer is given.
//     datv_walk_kernel   one wave per channel.  The filtered samples held back by the feed before and this feed's are one
//                        stream; while 128 + readahead of it are left, a chunk runs: 192 samples go to LDS, fir_sampler's
//                        throttled do_update_freq rebuilds shifted_coeffs in LDS with a lane per coefficient, then the 128
//                        samples are stepped through with wave-uniform values.  A symbol's FIR forms its products a lane per
//                        tap and adds them in the reference's order, one readlane per term; the trig and constellation tables
//                        are read from global memory by every lane at one address.  Lane 0 stores the soft symbol.  Behind the
//                        chunk: datv_chunk_end, the constellation point and the measurements.  Behind the last chunk the wave
//                        copies what is left of the stream to the other history set.
// Every output is bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  datv_scan.hpp has the per-symbol and per-chunk step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "datv_scan.hpp"
#include "wave_walk.hpp"

namespace sdrx {

constexpr int DATV_WIN = DATV_CHUNK + DATV_TAPS_MAX;        // samples of a chunk an interp can reach

struct DatvChan {                           // device resident: config + carried state of one channel
    // --- config
    DatvDesign d;
    const float2* trig;                     // trig16's lut: 65536 (cos, sin), shared by the handle's channels
    const DatvLutEntry* lut;                // 65536 entries, shared by the channels with the same (modulation, fec, hard_metric)
    const signed char* symbols;             // nsymbols (re, im) pairs
    const float* coeffs;                    // ncoeffs RRC coefficients
    // --- state
    DatvState s;
    // --- per feed
    int n_sym, n_pts, n_meas;               // soft symbols, constellation points, measurements of the last feed
    int n_chunks;                           // chunks the last feed ran
};

struct DatvBufs {                           // per channel device pointers (per feed capacity ensured by the host)
    const float2* y;                        // the front's output of this feed: the filtered samples
    const int* n_ptr;                       // its count (device side)
    const float2* held; float2* held_next;  // DATV_HOLD: the samples held back, oldest first
    int16_t* cost; uint8_t* symbol;         // per soft symbol
    float2* pts;                            // per chunk with a symbol: p_sampled
    DatvMeas* meas;                         // per measurement
};

typedef __attribute__((address_space(1))) short walk_global_i16;
typedef __attribute__((address_space(1))) unsigned char walk_global_byte;

// sample j of the stream the receiver reads: the held ones, then the feed's
__device__ __forceinline__ float2 datv_in_at(const DatvBufs& b, int held, long j)
{
    return j < held ? walk_global_load(b.held + j) : walk_global_load(b.y + (j - held));
}

// fir_sampler::do_update_freq: shifted_coeffs[i] = trig.expi(-f * (i - ncoeffs / 2)) * coeffs[i], a lane per coefficient
__device__ __forceinline__ void datv_shift_coeffs(const DatvChan& q, float2* sh, float freqw, int lane)
{
    const int nc = q.d.ncoeffs;
    const float f = freqw / q.d.subsampling;
    for (int i = lane; i < nc; i += 64) {
        const float2 e = walk_global_load(q.trig + datv_angle(-f * (i - nc / 2)));
        const float k = walk_global_load(q.coeffs + i);
        sh[i] = make_float2(e.x * k, e.y * k);
    }
}

__global__ __launch_bounds__(64)
void datv_walk_kernel(DatvChan* __restrict__ ch, const DatvBufs* __restrict__ bufs, int n_ch)
{
    __shared__ float2 sh[DATV_NCOEFFS_MAX];                 // shifted_coeffs
    __shared__ float2 win[DATV_WIN];
    __shared__ float2 pts[256];                             // symbols[] as floats
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n_ch) return;
    DatvChan& q = ch[c];
    const DatvBufs b = bufs[c];
    const DatvDesign d = q.d;
    DatvState s = q.s;
    const int n = *b.n_ptr, held = s.held;
    const long total = (long)held + n;
    const int chunks = total >= DATV_CHUNK + d.readahead ? (int)((total - d.readahead) / DATV_CHUNK) : 0;
    for (int i = lane; i < d.nsymbols; i += 64) pts[i] = make_float2((float)q.symbols[2 * i], (float)q.symbols[2 * i + 1]);
    if (d.sampler == DATV_SAMP_RRC && s.coeffs_built) datv_shift_coeffs(q, sh, s.sampler_freqw, lane);
    __syncthreads();
    int n_sym = 0, n_pts = 0, n_meas = 0;
    walk_global_i16* costs = (walk_global_i16*)b.cost;
    walk_global_byte* syms = (walk_global_byte*)b.symbol;
    const int sub = d.subsampling, nc = d.ncoeffs;
    for (int k = 0; k < chunks; k++) {
        const long base = (long)k * DATV_CHUNK;
        __syncthreads();                                    // the chunk before has read its window
        for (int i = lane; i < DATV_WIN; i += 64) win[i] = base + i < total ? datv_in_at(b, held, base + i) : make_float2(0.0f, 0.0f);
        // sampler->update_freq(freqw)
        if (d.sampler == DATV_SAMP_RRC) {
            s.update_freq_phase -= DATV_CHUNK;
            if (s.update_freq_phase <= 0) {
                s.update_freq_phase = nc * 16;
                s.sampler_freqw = s.freqw; s.coeffs_built = 1;
                datv_shift_coeffs(q, sh, s.freqw, lane);
            }
        } else if (d.sampler == DATV_SAMP_LINEAR) {
            s.sampler_freqw = s.freqw;
        }
        __syncthreads();
        int had = 0, pe_c = 0, pe_i = 0;
        float sgre = 0.0f, sgim = 0.0f, sre = 0.0f, sim = 0.0f;
        for (int pin = 0; pin < DATV_CHUNK; pin++) {
            if (s.mu < 1) {
                float gre, gim;
                if (d.sampler == DATV_SAMP_RRC) {
                    const int start = datv_f2i((1 - s.mu) * sub);
                    const long idx = (long)start + (long)lane * sub;
                    float pr = 0.0f, pi = 0.0f;
                    if (start >= 0 && idx < nc) {
                        const float2 a = sh[idx], x = win[pin + lane];
                        pr = a.x * x.x - a.y * x.y;
                        pi = a.x * x.y + a.y * x.x;
                    }
                    const int cnt = (start >= 0 && start < nc) ? (nc - start + sub - 1) / sub : 0;
                    float are = 0.0f, aim = 0.0f;
                    for (int t = 0; t < cnt; t++) {
                        are += walk_lane_value(pr, t);
                        aim += walk_lane_value(pi, t);
                    }
                    const float2 e = walk_global_load(q.trig + datv_angle(-s.phase));
                    gre = e.x * are - e.y * aim;
                    gim = e.x * aim + e.y * are;
                } else if (d.sampler == DATV_SAMP_LINEAR) {
                    const float2 e0 = walk_global_load(q.trig + datv_angle(-s.phase));
                    const float2 e1 = walk_global_load(q.trig + datv_angle(-(s.phase + s.sampler_freqw)));
                    const float2 p0 = win[pin], p1 = win[pin + 1];
                    const float s0r = p0.x * e0.x - p0.y * e0.y, s0i = p0.x * e0.y + p0.y * e0.x;
                    const float s1r = p1.x * e1.x - p1.y * e1.y, s1i = p1.x * e1.y + p1.y * e1.x;
                    const float w0 = 1 - s.mu;
                    gre = s0r * w0 + s1r * s.mu;
                    gim = s0i * w0 + s1i * s.mu;
                } else {
                    const float2 e = walk_global_load(q.trig + datv_angle(-s.phase));
                    const float2 p0 = win[pin];
                    gre = p0.x * e.x - p0.y * e.y;
                    gim = p0.x * e.y + p0.y * e.x;
                }
                sgre = gre; sgim = gim;
                sre = gre * s.agc_gain; sim = gim * s.agc_gain;
                const unsigned long long r = *(const walk_global_u64*)(q.lut + datv_lut_index(sre, sim));
                const int cost = (int)(short)(r & 0xffffu), perr = (int)(short)((r >> 16) & 0xffffu), sy = (int)((r >> 32) & 0xffu);
                if (lane == 0) { costs[n_sym] = (short)cost; syms[n_sym] = (unsigned char)sy; }
                n_sym++;
                const float2 cp = pts[sy];
                datv_symbol(d, s, sre, sim, perr, cp.x, cp.y, nullptr);
                pe_c = (int)cp.x; pe_i = (int)cp.y;
                had = 1;
            }
            s.mu = s.mu - 1;
            s.phase += s.freqw;
        }
        DatvMeas m[3];
        const int nm = datv_chunk_end(d, s, had, sgre, sgim, sre, sim, pe_c, pe_i, m, nullptr);
        if (lane == 0) {
            if (had) walk_global_store(b.pts + n_pts, make_float2(sre, sim));
            for (int j = 0; j < nm; j++) b.meas[n_meas + j] = m[j];
        }
        n_pts += had; n_meas += nm;
    }
    // what the next feed starts from
    const long used = (long)chunks * DATV_CHUNK;
    const int left = (int)(total - used);
    for (int i = lane; i < left; i += 64) b.held_next[i] = datv_in_at(b, held, used + i);
    if (lane == 0) {
        s.held = left; s.chunks += chunks; s.n_in += n; s.n_symbols += n_sym;
        q.s = s;
        q.n_sym = n_sym; q.n_pts = n_pts; q.n_meas = n_meas; q.n_chunks = chunks;
    }
}

} // namespace sdrx
