// scatter_san.cpp -- the scatter model's host code (the argument checks of
// xrt_scatter_source and xrt_scatter_add and the kernels' arithmetic over whole
// planes, xrt_host_scatter_source and xrt_host_scatter_add:
// simpleraytracing_amd/csrc/xrt_scatter_host.inc) over their edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/scatter_san.cpp -o scatter_san
//
// Exact-size heap buffers, so that a read or write one element past a plane, a
// coarse plane or a table is seen.  Prints "scatter_san: OK" and returns 0 when
// every call returned what it should (tests/test_scatter_cpu.py runs it).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_detector_host.inc"
#include "xrt_scatter_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("scatter_san: line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    // --- both steps over shapes that end inside a block, a tile and a batch of rows
    const unsigned shapes[][6] = {{1, 1, 1, 1, 1, 1},   {7, 13, 4, 1, 1, 1},  {64, 64, 8, 2, 3, 8},  {67, 45, 16, 3, 16, 32},
                                  {130, 70, 64, 1, 3, 8}, {200, 3, 2, 3, 1, 1}, {5, 5, 64, 2, 16, 32}};
    for (const auto& s : shapes) {
        const unsigned W = s[0], H = s[1], D = s[2], P = s[3], M = s[4], K = s[5];
        const unsigned Wc = (W + D - 1) / D, Hc = (H + D - 1) / D;
        const size_t n = (size_t)W * H * P, nc = (size_t)Wc * Hc * P;
        float* paths = new float[n * M];
        uint16_t* open = new uint16_t[n];
        float* weight = new float[K];
        float* mu = new float[(size_t)M * K];
        float* sigma = new float[(size_t)M * K];
        float* lb = new float[n];
        float* src = new float[nc];
        for (size_t k = 0; k < n * M; ++k)
            paths[k] = k % 23 == 3 ? NAN : k % 29 == 5 ? inf : k % 31 == 7 ? -0.0f : k % 5 == 0 ? 0.0f : (float)(k % 97) * 0.6f - 4.0f;
        for (size_t k = 0; k < n; ++k) open[k] = k % 19 == 4 ? (uint16_t)0x8001u : (uint16_t)0u;
        for (unsigned e = 0; e < K; ++e) weight[e] = 1.0f + (float)e;
        for (size_t k = 0; k < (size_t)M * K; ++k) {
            mu[k] = k % 7 == 0 ? 0.0f : 0.02f * (float)(k % 11 + 1);
            sigma[k] = k % 5 == 0 ? 0.0f : 0.4f * mu[k];
        }
        EXPECT(xrt_host_scatter_source(W, H, P, M, paths, open, weight, mu, sigma, K, D, lb, src) == XRT_OK);
        for (size_t k = 0; k < n; ++k)
            if (open[k]) EXPECT(lb[k] == -1.0f);
        float* src2 = new float[nc];
        EXPECT(xrt_host_scatter_source(W, H, P, M, paths, nullptr, weight, mu, sigma, K, D, nullptr, src2) == XRT_OK);
        // D = 1 against the pixel function itself
        if (D == 1)
            for (size_t i = 0; i < n; ++i) {
                double E, Q;
                XRT_KERNEL_NS::scatter_pixel(
                    M, K, [&](uint32_t j) { return (double)paths[j * n + i] * 0.1; }, [&](uint32_t j, uint32_t e) { return mu[j * K + e]; },
                    [&](uint32_t j, uint32_t e) { return sigma[j * K + e]; }, [&](uint32_t e) { return weight[e]; }, E, Q);
                const float q = (float)Q;
                EXPECT(std::memcmp(&q, &src2[i], sizeof q) == 0 || (q != q && src2[i] != src2[i]));
            }
        for (unsigned G : {1u, 4u}) {
            float* blurred = new float[nc * G];
            float* amp = new float[G];
            float* prim = new float[n];
            float* out = new float[n];
            float* sc = new float[n];
            uint8_t* u8 = new uint8_t[n];
            for (size_t k = 0; k < nc * G; ++k) blurred[k] = k % 13 == 2 ? -0.0f : (float)(k % 41) * 0.7f;
            for (unsigned g = 0; g < G; ++g) amp[g] = g == 1 ? 0.0f : 0.25f * (float)(g + 1);
            for (size_t k = 0; k < n; ++k) prim[k] = k % 9 == 0 ? -0.0f : (float)(k % 83);
            EXPECT(xrt_host_scatter_add(W, H, P, D, blurred, G, amp, prim, out, sc, u8) == XRT_OK);
            for (size_t k = 0; k < n; ++k) {
                const float want = (float)((double)prim[k] + (double)sc[k]);
                EXPECT(std::fabs(out[k] - want) <= std::fabs(want) * 1.2e-7f);   // (S is rounded once more in sc)
                EXPECT(u8[k] == scatter_host_u8(out[k]));
            }
            // each output alone, no primary
            EXPECT(xrt_host_scatter_add(W, H, P, D, blurred, G, amp, nullptr, out, nullptr, nullptr) == XRT_OK);
            EXPECT(std::memcmp(out, sc, n * sizeof(float)) == 0);
            EXPECT(xrt_host_scatter_add(W, H, P, D, blurred, G, amp, prim, nullptr, sc, nullptr) == XRT_OK);
            EXPECT(xrt_host_scatter_add(W, H, P, D, blurred, G, amp, prim, nullptr, nullptr, u8) == XRT_OK);
            // a constant plane comes back exactly
            for (size_t k = 0; k < nc * G; ++k) blurred[k] = 0.1f;
            EXPECT(xrt_host_scatter_add(W, H, P, D, blurred, 1, amp, nullptr, nullptr, sc, nullptr) == XRT_OK);
            const float c = (float)(0.0 + (double)amp[0] * (double)0.1f);
            for (size_t k = 0; k < n; ++k) EXPECT(std::memcmp(&sc[k], &c, sizeof c) == 0);
            delete[] blurred;
            delete[] amp;
            delete[] prim;
            delete[] out;
            delete[] sc;
            delete[] u8;
        }
        delete[] paths;
        delete[] open;
        delete[] weight;
        delete[] mu;
        delete[] sigma;
        delete[] lb;
        delete[] src;
        delete[] src2;
    }

    // --- the argument checks -------------------------------------------------
    float paths[48] = {0}, lb[24], src[8], blurred[32] = {0}, prim[24] = {0}, out[24], sc[24];
    uint16_t open[24] = {0};
    uint8_t u8[24];
    const float w2[2] = {1.0f, 2.0f}, mu4[4] = {0.1f, 0.2f, 0.0f, 0.3f}, sg4[4] = {0.05f, 0.0f, 0.0f, 0.1f};
    const float sg_neg[4] = {0.05f, -0.1f, 0.0f, 0.1f}, sg_nan[4] = {0.05f, NAN, 0.0f, 0.1f}, sg_inf[4] = {inf, 0.0f, 0.0f, 0.1f};
    const float amp2[2] = {0.5f, 0.0f}, amp_neg[2] = {0.5f, -0.5f}, amp_nan[2] = {NAN, 0.5f};
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) == nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, nullptr, w2, mu4, sg4, 2, 4, nullptr, src) == nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, nullptr, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, nullptr, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, nullptr) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, nullptr, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 17, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 33, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg_neg, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg_nan, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg_inf, 2, 4, lb, src) != nullptr);
    for (unsigned bad : {0u, 3u, 6u, 65u, 128u, 0x80000000u})
        EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, bad, lb, src) != nullptr);
    for (unsigned good : {1u, 2u, 4u, 8u, 16u, 32u, 64u})
        EXPECT(scatter_source_arguments(1, 1, 1, 2, paths, open, w2, mu4, sg4, 2, good, lb, src) == nullptr);
    EXPECT(scatter_source_arguments(0, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 0, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 0, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(0x80000000u, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(1, 4u * 65535u + 1u, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(1, 1, 65536, 2, paths, open, w2, mu4, sg4, 2, 4, lb, src) != nullptr);
    EXPECT(scatter_source_arguments(0x7FFFFFFFu, 0x40000u, 1, 2, paths, open, w2, mu4, sg4, 2, 64, lb, src) != nullptr);   // 2^40
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, paths + 47) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, paths + 47, src) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, reinterpret_cast<float*>(open)) != nullptr);
    EXPECT(scatter_source_arguments(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 4, lb, lb + 23) != nullptr);
    EXPECT(xrt_host_scatter_source(6, 4, 1, 2, paths, open, w2, mu4, sg4, 2, 3, lb, src) == XRT_ERR_ARGUMENT);

    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, out, sc, u8) == nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, nullptr, nullptr, nullptr, u8) == nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, nullptr, 2, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, nullptr, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, nullptr, nullptr, nullptr) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 0, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 5, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp_neg, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp_nan, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 3, blurred, 2, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(0, 4, 1, 4, blurred, 2, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(1, 64u * 65535u + 1u, 1, 4, blurred, 2, amp2, prim, out, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, prim, sc, u8) != nullptr);               // in place
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, out, prim + 23, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, out, sc, reinterpret_cast<uint8_t*>(prim) + 95) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, blurred + 3, sc, u8) != nullptr);
    EXPECT(scatter_add_arguments(6, 4, 1, 4, blurred, 2, amp2, prim, blurred + 4, sc, u8) == nullptr);       // side by side
    EXPECT(xrt_host_scatter_add(6, 4, 1, 4, blurred, 5, amp2, prim, out, sc, u8) == XRT_ERR_ARGUMENT);
    if (!failures) std::printf("scatter_san: OK\n");
    return failures ? 1 : 0;
}
