// noise_san.cpp -- the photon noise's host code (the argument checks of
// xrt_photon_noise, xrt_host_philox4x32, xrt_host_poisson_batch and the pixel
// function over whole buffers, xrt_host_photon_noise:
// simpleraytracing_amd/csrc/xrt_noise_host.inc) over their edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/noise_san.cpp \
//         -o noise_san
//
// Exact-size heap buffers, so that a read or write one element past a buffer is
// seen.  Prints "noise_san: OK" and returns 0 when every call returned what it
// should (tests/test_noise_cpu.py runs it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_noise_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("noise_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                    \
        }                                                                  \
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
    // --- Philox4x32-10: the known answers published with Random123 ---
    {
        const uint32_t kat[3][10] = {
            {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
            {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu,
             0xa20bc7c6u, 0x6d5451fdu},
            {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu,
             0x5001e420u, 0x24126ea1u}};
        for (const auto& k : kat) {
            uint32_t* c = new uint32_t[4];
            uint32_t* key = new uint32_t[2];
            uint32_t* w = new uint32_t[4];
            std::memcpy(c, k, 16);
            std::memcpy(key, k + 4, 8);
            xrt_host_philox4x32(c, key, w);
            EXPECT(std::memcmp(w, k + 6, 16) == 0);
            delete[] c;
            delete[] key;
            delete[] w;
        }
    }

    // --- the sampler: every class of mean under edge words and a stride over all 2^32 ---
    {
        const double lams[] = {-1.0, -0.0, 0.0, 1e-45, 0.5, 63.999996185302734, 64.0, 100.0, 1e4, 16777216.0, 3e38,
                               (double)inf, std::nan("")};
        std::vector<uint32_t> words = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 322122546u, 322122547u, 322122548u,
                                       3972844748u, 3972844749u, 3972844750u};
        for (uint64_t b = 0; b < (1ull << 32); b += 1048573u) words.push_back((uint32_t)b);
        const size_t n = words.size();
        double* lam = new double[n];
        uint32_t* w = new uint32_t[n];
        double* out = new double[n];
        std::memcpy(w, words.data(), n * sizeof(uint32_t));
        for (double l : lams) {
            for (size_t k = 0; k < n; ++k) lam[k] = l;
            xrt_host_poisson_batch(lam, w, n, out);
            for (size_t k = 0; k < n; ++k) {
                if (std::isnan(l) || l < 0.0) EXPECT(std::isnan(out[k]));
                else if (std::isinf(l)) EXPECT(out[k] == (double)inf);
                else EXPECT(out[k] >= 0.0 && out[k] == std::floor(out[k]) && (l >= 64.0 || out[k] <= 255.0));
                if (l == 0.0 || l == 1e-45) EXPECT(out[k] == 0.0);
                if (l == 1e4) EXPECT(std::fabs(out[k] - l) < 700.0);            // within 7 standard deviations
            }
        }
        xrt_host_poisson_batch(lam, w, 0, out);
        // the deviate is odd in u - 1/2 and grows with the word
        EXPECT(XRT_KERNEL_NS::xrt_normal_from_word(0u) == -XRT_KERNEL_NS::xrt_normal_from_word(0xffffffffu));
        EXPECT(XRT_KERNEL_NS::xrt_normal_from_word(0x7fffffffu) == -XRT_KERNEL_NS::xrt_normal_from_word(0x80000000u));
        EXPECT(XRT_KERNEL_NS::xrt_normal_from_word(0u) < -6.0 && XRT_KERNEL_NS::xrt_normal_from_word(0u) > -6.5);
        for (size_t k = 11; k + 1 < n; ++k)
            EXPECT(XRT_KERNEL_NS::xrt_normal_from_word(w[k]) < XRT_KERNEL_NS::xrt_normal_from_word(w[k + 1]));
        delete[] lam;
        delete[] w;
        delete[] out;
    }

    // --- the pixel function over buffers: ragged sizes, first indices that cut a group, both modes, in place ---
    const int shapes[][3] = {{1, 1, 1}, {2, 1, 1}, {3, 1, 1}, {5, 1, 1}, {7, 13, 3}, {70, 67, 3}};
    for (const auto& s : shapes) {
        const uint32_t W = s[0], H = s[1], P = s[2];
        const size_t n = (size_t)W * H * P;
        float* img = new float[n];
        float* out = new float[n];
        float* copy = new float[n];
        for (size_t k = 0; k < n; ++k)
            img[k] = k % 17 == 0 ? 0.0f : k % 19 == 0 ? -1.0f : k % 23 == 0 ? inf : k % 29 == 0 ? NAN : (float)(k % 53) * (float)(k % 7);
        for (uint64_t first : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, ((uint64_t)1 << 34) - 3u, UINT64_MAX - (uint64_t)n})
            for (int mode : {XRT_NOISE_INTENSITY, XRT_NOISE_COUNTS}) {
                EXPECT(xrt_host_photon_noise(W, H, P, img, 1.5f, 77u, first, mode, out) == XRT_OK);
                for (size_t k = 0; k < n; ++k) {
                    const uint64_t g = first + k;
                    uint32_t w[4];
                    XRT_KERNEL_NS::xrt_noise_words(g >> 2, 77u, w);
                    volatile float lam_f = img[k] * 1.5f;
                    const float c = (float)XRT_KERNEL_NS::xrt_poisson_from_word((double)lam_f, w[g & 3u]);
                    EXPECT(same(out[k], mode == XRT_NOISE_COUNTS ? c : c / 1.5f));
                }
                std::memcpy(copy, img, n * sizeof(float));
                EXPECT(xrt_host_photon_noise(W, H, P, copy, 1.5f, 77u, first, mode, copy) == XRT_OK);   // in place
                for (size_t k = 0; k < n; ++k) EXPECT(same(out[k], copy[k]));
            }
        delete[] img;
        delete[] out;
        delete[] copy;
    }

    // --- the argument checks -------------------------------------------------
    float img[24] = {0}, res[24];
    uint64_t n = 0;
    const int IN = XRT_NOISE_INTENSITY, CO = XRT_NOISE_COUNTS;
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, 0, IN, res, &n) == nullptr && n == 24);
    EXPECT(noise_arguments(4, 3, 2, img, 1e-3f, UINT64_MAX - 24, CO, res, &n) == nullptr);
    EXPECT(noise_arguments(4, 3, 2, nullptr, 1.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, 0, IN, nullptr, &n) != nullptr);
    EXPECT(noise_arguments(0, 3, 2, img, 1.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 0, 2, img, 1.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 0, img, 1.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, 0, 2, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, 0, -1, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, 0.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, -1.0f, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, inf, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, NAN, 0, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, UINT64_MAX - 23, IN, res, &n) != nullptr);          // first_index + n = 2^64
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, UINT64_MAX, IN, res, &n) != nullptr);
    EXPECT(noise_arguments(0xFFFFFFFFu, 0xFFFFFFFFu, 1, img, 1.0f, 0, IN, res, &n) != nullptr);   // one launch's workgroups
    EXPECT(noise_arguments(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, img, 1.0f, 0, IN, res, &n) != nullptr);   // n past 64 bits
    EXPECT(noise_arguments(0x80000000u, 1024, 1, img, 1.0f, 0, IN, res, &n) != nullptr);          // 2^41 pixels
    EXPECT(noise_arguments(4, 3, 2, img, 1.0f, 0, IN, img, &n) == nullptr);                        // in place
    EXPECT(noise_arguments(4, 3, 1, img, 1.0f, 0, IN, img + 1, &n) != nullptr);                    // a partial overlap
    EXPECT(noise_arguments(4, 3, 1, img, 1.0f, 0, IN, img + 11, &n) != nullptr);                   // the last pixel
    EXPECT(noise_arguments(4, 3, 1, img, 1.0f, 0, IN, img + 12, &n) == nullptr);                   // side by side
    EXPECT(xrt_host_photon_noise(4, 3, 2, img, 1.0f, 0, 0, 7, res) == XRT_ERR_ARGUMENT);
    EXPECT(XRT_KERNEL_NS::photon_noise_lanes(0, 1) == 1 && XRT_KERNEL_NS::photon_noise_lanes(3, 2) == 2 &&
           XRT_KERNEL_NS::photon_noise_lanes(3, 6) == 3 && XRT_KERNEL_NS::photon_noise_lanes(UINT64_MAX - 4, 4) == 2);
    if (!failures) std::printf("noise_san: OK\n");
    return failures ? 1 : 0;
}
