// How should one LoRa channel's 2 x 127 sliding-FFT bins be spread over waves?  The recurrence of lora_walk_kernel
// (sdrangel_amd/csrc/lora_kernels.hpp), bins = (bins + z) * vrot for both filters, on synthetic z, nothing else of the walk:
//   WAVES = 1   one wave per channel, lane l holds bins l and l + 64 of both filters (four chains per lane): the product's layout
//   WAVES = 2   two waves per channel, one bin of each filter per lane (two chains per lane)
//   WAVES = 4   four waves per channel, one bin of one filter per lane (one chain per lane)
// With more than one wave the waves of a channel meet every 64 steps, where the product has its fetch: the magnitudes go
// through LDS and a workgroup barrier, as a multi-wave walk would have to do.  Every variant runs `channels` channels of `steps`
// steps and writes the bins' magnitudes at the end, so that nothing is optimised away.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ubench_lora_walk.hip -o tools/ubench_lora_walk
//   tools/ubench_lora_walk [channels = 256] [steps = 62500] [runs = 9]      one JSON line: median ms and ns per step per variant
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ __forceinline__ float lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ void bin_step(float2& bin, float zx, float zy, float2 v)
{
    const float tx = bin.x + zx, ty = bin.y + zy;
    bin = make_float2(tx * v.x - ty * v.y, tx * v.y + ty * v.x);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void walk(const float4* __restrict__ z, const float2* __restrict__ vrot, float* __restrict__ out, int steps)
{
    __shared__ float mags[256];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4* zc = z + (size_t)c * steps;
    constexpr int CHAINS = 4 / WAVES;                       // bins per lane
    float2 bins[CHAINS], v[CHAINS];
    bool second[CHAINS];                                    // the chain belongs to the second filter
    for (int k = 0; k < CHAINS; k++) {
        const int flat = (wave * CHAINS + k) * 64 + lane;   // 0 .. 255: filter = flat / 128, bin = flat % 128
        bins[k] = make_float2(0.0f, 0.0f);
        v[k] = vrot[flat & 127];
        second[k] = flat >= 128;
    }
    float acc = 0.0f;
    float4 next = lane < steps ? zc[lane] : make_float4(0, 0, 0, 0);
    for (int base = 0; base < steps; base += 64) {
        const float4 cur = next;
        if (base + 64 + lane < steps) next = zc[base + 64 + lane];
        const int cnt = min(64, steps - base);
        for (int j = 0; j < cnt; j++) {
            const float ax = lane_value(cur.x, j), ay = lane_value(cur.y, j), bx = lane_value(cur.z, j), by = lane_value(cur.w, j);
#pragma unroll
            for (int k = 0; k < CHAINS; k++) bin_step(bins[k], second[k] ? bx : ax, second[k] ? by : ay, v[k]);
        }
        if (WAVES > 1) {                                    // the fetch: every wave's magnitudes where one wave can pick the peaks
#pragma unroll
            for (int k = 0; k < CHAINS; k++) mags[(wave * CHAINS + k) * 64 + lane] = bins[k].x * bins[k].x + bins[k].y * bins[k].y;
            __syncthreads();
            if (wave == 0) acc += mags[lane] + mags[64 + lane] + mags[128 + lane] + mags[192 + lane];
            __syncthreads();
        } else {
#pragma unroll
            for (int k = 0; k < CHAINS; k++) acc += bins[k].x * bins[k].x + bins[k].y * bins[k].y;
        }
    }
    if (wave == 0) out[(size_t)c * 64 + lane] = acc;
}

template <int WAVES>
static int run(const char* name, int channels, int steps, int runs, const float4* z, const float2* vrot, float* out, bool last)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    std::vector<float> ms;
    for (int r = 0; r < runs + 2; r++) {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL(walk<WAVES>, dim3(channels), dim3(64 * WAVES), 0, 0, z, vrot, out, steps);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float t = 0;
        CHECK(hipEventElapsedTime(&t, a, b));
        if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const float med = ms[ms.size() / 2];
    std::printf("\"%s_ms\": %.4f, \"%s_ms_min\": %.4f, \"%s_ms_max\": %.4f, \"%s_ns_per_step\": %.2f%s", name, med, name, ms.front(), name, ms.back(), name,
                med * 1e6 / steps, last ? "" : ", ");
    return 0;
}

int main(int argc, char** argv)
{
    const int channels = argc > 1 ? std::atoi(argv[1]) : 256, steps = argc > 2 ? std::atoi(argv[2]) : 62500, runs = argc > 3 ? std::atoi(argv[3]) : 9;
    if (channels < 1 || channels > 4096 || steps < 1 || steps > (1 << 20) || runs < 1 || runs > 100) { std::fprintf(stderr, "bad argument\n"); return 2; }
    std::vector<float4> hz((size_t)channels * steps);
    unsigned s = 12345;
    for (auto& q : hz) {
        float f[4];
        for (float& x : f) { s = s * 1664525u + 1013904223u; x = ((int)(s >> 8) % 2001 - 1000) * 1e-4f; }
        q = make_float4(f[0], f[1], f[2], f[3]);
    }
    std::vector<float2> hv(128);
    for (int i = 0; i < 128; i++) hv[(size_t)i] = make_float2((float)(0.99999 * std::cos(2.0 * M_PI * i / 128)), (float)(0.99999 * std::sin(2.0 * M_PI * i / 128)));
    float4* z; float2* vrot; float* out;
    CHECK(hipMalloc(reinterpret_cast<void**>(&z), hz.size() * sizeof(float4)));
    CHECK(hipMalloc(reinterpret_cast<void**>(&vrot), hv.size() * sizeof(float2)));
    CHECK(hipMalloc(reinterpret_cast<void**>(&out), (size_t)channels * 64 * sizeof(float)));
    CHECK(hipMemcpy(z, hz.data(), hz.size() * sizeof(float4), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(vrot, hv.data(), hv.size() * sizeof(float2), hipMemcpyHostToDevice));
    std::printf("{\"tool\": \"ubench_lora_walk\", \"channels\": %d, \"steps\": %d, \"runs\": %d, ", channels, steps, runs);
    if (run<1>("one_wave", channels, steps, runs, z, vrot, out, false)) return 1;
    if (run<2>("two_waves", channels, steps, runs, z, vrot, out, false)) return 1;
    if (run<4>("four_waves", channels, steps, runs, z, vrot, out, true)) return 1;
    std::printf("}\n");
    CHECK(hipFree(z)); CHECK(hipFree(vrot)); CHECK(hipFree(out));
    return 0;
}
