// projection_san.cpp -- the line-integral projections' host code (the argument
// checks of xrt_log_projection, xrt_host_logf_batch and the pixel function over
// whole buffers, xrt_host_log_projection:
// simpleraytracing_amd/csrc/xrt_projection_host.inc) over their edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/projection_san.cpp \
//         -o projection_san
//
// Exact-size heap buffers, so that a read or write one element past a plane is
// seen.  Prints "projection_san: OK" and returns 0 when every call returned
// what it should (tests/test_projection_cpu.py runs it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_projection_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("projection_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static uint32_t bits_of(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

static bool same(float a, float b) { return bits_of(a) == bits_of(b) || (std::isnan(a) && std::isnan(b)); }

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    // --- logf: the specials, the subnormal path, a stride over every exponent, against libm ---
    std::vector<float> x;
    for (uint32_t b : {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0xbf800000u,
                       0x00000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x3f800000u, 0x3f7fffffu, 0x3f800001u}) {
        float f;
        std::memcpy(&f, &b, 4);
        x.push_back(f);
    }
    for (uint64_t b = 0; b < (1ull << 32); b += 65521u) {
        const uint32_t u = (uint32_t)b;
        float f;
        std::memcpy(&f, &u, 4);
        x.push_back(f);
    }
    {
        float* in = new float[x.size()];
        float* out = new float[x.size()];
        std::memcpy(in, x.data(), x.size() * sizeof(float));
        xrt_host_logf_batch(in, out, x.size());
        for (size_t k = 0; k < x.size(); ++k) {
            volatile float v = in[k];
            EXPECT(same(out[k], std::log(v)));
        }
        EXPECT(bits_of(out[11]) == 0u);                                  // log(1) = +0.0
        xrt_host_logf_batch(in, out, 0);
        delete[] in;
        delete[] out;
    }

    // --- the pixel function over planes: every flat/dark combination, both orders, t_min 0 and 0.01 ---
    const int shapes[][3] = {{1, 1, 1}, {7, 13, 3}, {13, 7, 5}, {65, 3, 2}};
    for (const auto& s : shapes) {
        const size_t W = s[0], H = s[1], P = s[2], n = W * H;
        float* img = new float[n * P];
        float* flat = new float[n];
        float* dark = new float[n];
        float* out = new float[n * P];
        for (size_t k = 0; k < n; ++k) {
            flat[k] = 60.0f + (float)(k % 29);
            dark[k] = 0.5f + (float)(k % 7) * 0.25f;
        }
        for (size_t k = 0; k < n * P; ++k)
            img[k] = k % 17 == 0 ? flat[k % n] : k % 19 == 0 ? 0.0f : k % 23 == 0 ? -1.0f : dark[k % n] + 0.01f + (float)(k % 53);
        for (int combo = 0; combo < 4; ++combo)
            for (float t_min : {0.0f, 0.01f})
                for (int order : {XRT_ORDER_PROJECTIONS, XRT_ORDER_SINOGRAMS}) {
                    const float* f = combo & 1 ? flat : nullptr;
                    const float* d = combo & 2 ? dark : nullptr;
                    EXPECT(xrt_host_log_projection(W, H, P, img, f, d, 80.0f, t_min, order, out) == XRT_OK);
                    for (size_t p = 0; p < P; ++p)
                        for (size_t y = 0; y < H; ++y)
                            for (size_t c = 0; c < W; ++c) {
                                const size_t i = (p * H + y) * W + c, q = y * W + c;
                                const float num = d ? img[i] - d[q] : img[i];
                                const float den = f ? (d ? f[q] - d[q] : f[q]) : (d ? 80.0f - d[q] : 80.0f);
                                volatile float t = num / den;
                                if (t_min > 0.0f && t < t_min) t = t_min;
                                const float want = 0.0f - std::log(t);
                                const size_t o = order == XRT_ORDER_SINOGRAMS ? (y * P + p) * W + c : i;
                                EXPECT(same(out[o], want));
                            }
                }
        // in place, projection order: the same values
        float* copy = new float[n * P];
        std::memcpy(copy, img, n * P * sizeof(float));
        EXPECT(xrt_host_log_projection(W, H, P, img, flat, dark, 0.0f, 0.01f, XRT_ORDER_PROJECTIONS, out) == XRT_OK);
        EXPECT(xrt_host_log_projection(W, H, P, copy, flat, dark, 0.0f, 0.01f, XRT_ORDER_PROJECTIONS, copy) == XRT_OK);
        for (size_t k = 0; k < n * P; ++k) EXPECT(same(out[k], copy[k]));
        delete[] copy;
        delete[] img;
        delete[] flat;
        delete[] dark;
        delete[] out;
    }

    // --- the argument checks -------------------------------------------------
    float img[24] = {0}, fl[12] = {0}, dk[12] = {0}, res[24];
    const int PR = XRT_ORDER_PROJECTIONS, SI = XRT_ORDER_SINOGRAMS;
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 0.0f, 0.0f, PR, res) == nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, nullptr, nullptr, 80.0f, 0.01f, SI, res) == nullptr);
    EXPECT(projection_arguments(4, 3, 2, nullptr, fl, dk, 80.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, 0.0f, PR, nullptr) != nullptr);
    EXPECT(projection_arguments(0, 3, 2, img, fl, dk, 80.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 0, 2, img, fl, dk, 80.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 0, img, fl, dk, 80.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, 0.0f, 2, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, 0.0f, -1, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, NAN, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, inf, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, -0.5f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, nullptr, dk, 0.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, nullptr, dk, -1.0f, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, nullptr, dk, inf, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, nullptr, dk, NAN, 0.0f, PR, res) != nullptr);
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, NAN, 0.0f, PR, res) == nullptr);         // flat_value unread with a plane
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, 0.0f, PR, img) == nullptr);       // in place
    EXPECT(projection_arguments(4, 3, 2, img, fl, dk, 80.0f, 0.0f, SI, img) != nullptr);       // not in sinogram order
    EXPECT(projection_arguments(4, 3, 1, img, fl, dk, 80.0f, 0.0f, PR, img + 1) != nullptr);   // a partial overlap
    EXPECT(projection_arguments(4, 3, 1, img, fl, dk, 80.0f, 0.0f, PR, img + 12) == nullptr);  // side by side
    EXPECT(projection_arguments(4, 3, 1, img, fl, dk, 80.0f, 0.0f, PR, fl) != nullptr);
    EXPECT(projection_arguments(4, 3, 1, img, fl, dk, 80.0f, 0.0f, PR, dk + 11) != nullptr);
    EXPECT(projection_arguments(1, 0xFFFFFFFFu, 2, img, fl, dk, 80.0f, 0.0f, PR, res) != nullptr);   // rows past 32 bits
    EXPECT(xrt_host_log_projection(4, 3, 2, img, fl, dk, 80.0f, 0.0f, 7, res) == XRT_ERR_ARGUMENT);
    if (!failures) std::printf("projection_san: OK\n");
    return failures ? 1 : 0;
}
