// lsf_san.cpp -- the detector response's host code (the argument checks of
// xrt_detector_response, xrt_lsf_gaussian and the kernel's tap loop over whole
// planes, xrt_host_lsf: simpleraytracing_amd/csrc/xrt_lsf_host.inc) over their
// edge cases, as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/lsf_san.cpp -o lsf_san
//
// Exact-size heap buffers, so that a read or write one element past a plane or
// a tap table is seen.  Prints "lsf_san: OK" and returns 0 when every call
// returned what it should (tests/test_lsf_cpu.py runs it).
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
#include "xrt_lsf_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("lsf_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// The contract of include/xrt.h, one tap at a time with clamped indices.
static void reference(const float* in, int W, int H, const float* hx, int nx, const float* hy, int ny, float* out)
{
    std::vector<float> tmp((size_t)W * H);
    const int rx = (nx - 1) / 2, ry = (ny - 1) / 2;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            double acc = 0.0;
            for (int k = 0; k < nx; ++k) {
                const double p = (double)hx[k] * (double)in[y * W + std::min(std::max(x + k - rx, 0), W - 1)];
                acc = k ? acc + p : p;
            }
            tmp[(size_t)y * W + x] = (float)acc;
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            double acc = 0.0;
            for (int k = 0; k < ny; ++k) {
                const double p = (double)hy[k] * (double)tmp[(size_t)std::min(std::max(y + k - ry, 0), H - 1) * W + x];
                acc = k ? acc + p : p;
            }
            out[(size_t)y * W + x] = (float)acc;
        }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    // --- the Gaussian ------------------------------------------------------
    for (double sigma : {0.3, 1.0, 2.5, 10.0, 40.0})
        for (unsigned taps : {1u, 3u, 41u, 129u}) {
            float* h = new float[taps];
            EXPECT(xrt_lsf_gaussian(sigma, taps, h) == XRT_OK);
            double sum = 0.0;
            for (unsigned k = 0; k < taps; ++k) {
                EXPECT(std::memcmp(&h[k], &h[taps - 1 - k], sizeof(float)) == 0);
                sum += h[k];
            }
            EXPECT(std::fabs(sum - 1.0) <= taps * std::ldexp(1.0, -24));
            delete[] h;
        }
    float one_tap[1];
    EXPECT(xrt_lsf_gaussian(0.0, 1, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(-1.0, 1, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian((double)inf, 1, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(NAN, 1, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(1.0, 0, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(1.0, 2, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(1.0, 131, one_tap) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_lsf_gaussian(1.0, 1, nullptr) == XRT_ERR_ARGUMENT);

    // --- the host restatement: 7 x 13 under 129 taps (the radius exceeds both sizes), and others
    const int shapes[][4] = {{7, 13, 129, 129}, {7, 13, 1, 1}, {13, 7, 5, 9}, {1, 1, 129, 3}, {17, 9, 41, 1}};
    for (const auto& s : shapes) {
        const int W = s[0], H = s[1], nx = s[2], ny = s[3];
        const size_t n = (size_t)W * H;
        float* in = new float[n];
        float* out = new float[n];
        float* want = new float[n];
        uint8_t* u8 = new uint8_t[n];
        float* hx = new float[nx];
        float* hy = new float[ny];
        for (size_t k = 0; k < n; ++k)
            in[k] = k % 11 == 0 ? -0.0f : k % 13 == 0 ? 1e-41f : k % 17 == 0 ? 3e4f : (float)k * 0.37f - 10.0f;
        for (int k = 0; k < nx; ++k) hx[k] = nx == 1 ? 1.0f : (float)((k * 7) % 5 - 1) / (float)nx;
        for (int k = 0; k < ny; ++k) hy[k] = ny == 1 ? 1.0f : (float)((k * 3) % 4) / (float)ny;
        EXPECT(xrt_host_lsf(W, H, 1, in, hx, nx, hy, ny, out, u8) == XRT_OK);
        reference(in, W, H, hx, nx, hy, ny, want);
        EXPECT(std::memcmp(out, want, n * sizeof(float)) == 0);
        if (nx == 1 && ny == 1) EXPECT(std::memcmp(out, in, n * sizeof(float)) == 0);    // the identity: the input's bits
        for (size_t k = 0; k < n; ++k) EXPECT(u8[k] == lsf_host_u8(want[k]));
        EXPECT(xrt_host_lsf(W, H, 1, in, hx, nx, hy, ny, out, nullptr) == XRT_OK);    // either output alone
        EXPECT(xrt_host_lsf(W, H, 1, in, hx, nx, hy, ny, nullptr, u8) == XRT_OK);
        delete[] in;
        delete[] out;
        delete[] want;
        delete[] u8;
        delete[] hx;
        delete[] hy;
    }

    // --- the argument checks -------------------------------------------------
    float img[12] = {0}, res[12];
    uint8_t res8[12];
    const float h3[3] = {0.25f, 0.5f, 0.25f}, bad_nan[3] = {0.25f, NAN, 0.25f}, bad_inf[3] = {inf, 0.0f, 0.0f};
    std::vector<float> big(131, 0.0f);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, h3, 3, res, res8) == nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, nullptr, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, nullptr, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 2, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, h3, 0, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, big.data(), 131, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, bad_nan, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, bad_inf, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(0, 3, 1, img, h3, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 0, 1, img, h3, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 0, img, h3, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, nullptr, h3, 3, h3, 3, res, res8) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, h3, 3, nullptr, nullptr) != nullptr);
    EXPECT(lsf_arguments(4, 3, 1, img, h3, 3, h3, 3, img, res8) != nullptr);                 // in place
    EXPECT(lsf_arguments(2, 3, 1, img, h3, 3, h3, 3, img + 5, nullptr) != nullptr);          // a partial overlap
    EXPECT(lsf_arguments(2, 3, 1, img, h3, 3, h3, 3, img + 6, nullptr) == nullptr);          // side by side
    EXPECT(lsf_arguments(2, 3, 1, img, h3, 3, h3, 3, nullptr, reinterpret_cast<uint8_t*>(img) + 23) != nullptr);
    EXPECT(xrt_host_lsf(4, 3, 1, img, h3, 2, h3, 3, res, res8) == XRT_ERR_ARGUMENT);
    if (!failures) std::printf("lsf_san: OK\n");
    return failures ? 1 : 0;
}
