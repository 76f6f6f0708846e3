// Probe: where k_log_projection's time goes.  The pixel arithmetic alone over a flat
// array of 2048^2 floats, a quad (or Q quads) a lane, no rows: a copy, with the IEEE division, with
// xrt_logf_regular, both, both under xrt_logf's per-pixel branches (k<V, Q>); both with the table forced
// to one entry, with the table in LDS, and with one test of the special cases a lane (k2<V, Q>).
// Prints microseconds per launch (device events over 200 launches), two rounds.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fno-fast-math \
//         -Iinclude -Isimpleraytracing_amd/csrc tools/probes/projection_costs.hip -o tools/probes/projection_costs
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "kernels/xrt_device.h"
using namespace xrt;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <int V>
__device__ __forceinline__ float px(float v, float f)
{
    if constexpr (V == 0) return v;                                         // copy
    if constexpr (V == 1) return v / f;                                     // division only
    if constexpr (V == 2) return 0.0f - xrt_logf_regular(__float_as_uint(v));   // log only
    if constexpr (V == 3) return 0.0f - xrt_logf_regular(__float_as_uint(v / f));   // both, no special cases
    if constexpr (V == 4) return 0.0f - xrt_logf(v / f);                    // both, branches per pixel
    return v;
}

// log with the table forced to one entry (no gather) -- timing only
__device__ __forceinline__ float logf_nogather(uint32_t ix, LogfEntry e)
{
    constexpr double kLn2 = 0x1.62e42fefa39efp-1, kA0 = -0x1.00ea348b88334p-2, kA1 = 0x1.5575b0be00b6ap-2, kA2 = -0x1.ffffef20a4123p-2;
    const uint32_t tmp = ix - 0x3f330000u;
    const int32_t k = (int32_t)tmp >> 23;
    const double z = (double)xrt_f32_from_bits(ix - (tmp & 0xff800000u));
    const double r = z * e.invc - 1.0;
    const double y0 = e.logc + (double)k * kLn2;
    const double r2 = r * r;
    double y = kA1 * r + kA2;
    y = kA0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

template <int V, int Q>
__global__ __launch_bounds__(256) void k(const float* __restrict__ in, float* __restrict__ out, float f, size_t nquads)
{
    const size_t base = (size_t)blockIdx.x * 256 * Q + threadIdx.x;
    float4 v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const size_t j = base + (size_t)q * 256;
        v[q] = j < nquads ? reinterpret_cast<const float4*>(in)[j] : make_float4(1, 1, 1, 1);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        float4 o;
        o.x = px<V>(v[q].x, f), o.y = px<V>(v[q].y, f), o.z = px<V>(v[q].z, f), o.w = px<V>(v[q].w, f);
        const size_t j = base + (size_t)q * 256;
        if (j < nquads) reinterpret_cast<float4*>(out)[j] = o;
    }
}

// V = 5: both, no gather (entry from kernel argument); V = 6: table in LDS; V = 7: lane-test of the special cases
template <int V, int Q>
__global__ __launch_bounds__(256) void k2(const float* __restrict__ in, float* __restrict__ out, float f, size_t nquads, LogfEntry fixed)
{
    __shared__ LogfEntry s_tab[16];
    if constexpr (V == 6) {
        if (threadIdx.x < 16) s_tab[threadIdx.x] = xrt_logf_tab(threadIdx.x);
        __syncthreads();
    }
    const size_t base = (size_t)blockIdx.x * 256 * Q + threadIdx.x;
    float4 v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const size_t j = base + (size_t)q * 256;
        v[q] = j < nquads ? reinterpret_cast<const float4*>(in)[j] : make_float4(1, 1, 1, 1);
    }
    float t[Q][4], o[Q][4];
    bool regular = true;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        t[q][0] = v[q].x / f, t[q][1] = v[q].y / f, t[q][2] = v[q].z / f, t[q][3] = v[q].w / f;
#pragma unroll
        for (int e = 0; e < 4; ++e) regular &= xrt_logf_is_regular(__float_as_uint(t[q][e]));
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t ix = __float_as_uint(t[q][e]);
            if constexpr (V == 5) o[q][e] = 0.0f - logf_nogather(ix, fixed);
            if constexpr (V == 6) o[q][e] = 0.0f - logf_nogather(ix, s_tab[((ix - 0x3f330000u) >> 19) & 15u]);
            if constexpr (V == 7) o[q][e] = 0.0f - xrt_logf_regular(ix);
        }
    if constexpr (V == 7) {
        if (!regular) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[q][e] = 0.0f - xrt_logf(t[q][e]);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const size_t j = base + (size_t)q * 256;
        if (j < nquads) reinterpret_cast<float4*>(out)[j] = make_float4(o[q][0], o[q][1], o[q][2], o[q][3]);
    }
}

template <class F>
static float time_us(F launch)
{
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    for (int i = 0; i < 40; ++i) launch();
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    for (int i = 0; i < 200; ++i) launch();
    hipEventRecord(b, 0);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    return ms * 1000.0f / 200.0f;
}

int main()
{
    const size_t n = 2048ull * 2048ull, nq = n / 4;
    std::vector<float> h(n);
    uint32_t s = 12345;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        h[i] = 1.0f + 79.0f * (float)(s >> 8) / 16777216.0f;
    }
    float *in, *out;
    CK(hipMalloc(&in, n * 4));
    CK(hipMalloc(&out, n * 4));
    CK(hipMemcpy(in, h.data(), n * 4, hipMemcpyHostToDevice));
    const LogfEntry fixed = xrt_logf_tab(9);
#define RUN1(V, Q) printf("k<%d,%d>  %.2f us\n", V, Q, time_us([&] { hipLaunchKernelGGL((k<V, Q>), dim3((unsigned)((nq + 256 * Q - 1) / (256 * Q))), dim3(256), 0, 0, in, out, 80.0f, nq); }))
#define RUN2(V, Q) printf("k2<%d,%d> %.2f us\n", V, Q, time_us([&] { hipLaunchKernelGGL((k2<V, Q>), dim3((unsigned)((nq + 256 * Q - 1) / (256 * Q))), dim3(256), 0, 0, in, out, 80.0f, nq, fixed); }))
    for (int round = 0; round < 2; ++round) {
        RUN1(0, 1); RUN1(0, 2);
        RUN1(1, 1); RUN1(1, 2);
        RUN1(2, 1); RUN1(2, 2);
        RUN1(3, 1); RUN1(3, 2);
        RUN1(4, 1); RUN1(4, 2);
        RUN2(5, 1); RUN2(5, 2);
        RUN2(6, 1); RUN2(6, 2);
        RUN2(7, 1); RUN2(7, 2); RUN2(7, 4);
    }
    CK(hipDeviceSynchronize());
    CK(hipGetLastError());
    return 0;
}
