// detector_san.cpp -- the spectral detector's host code (the argument checks of
// xrt_spectral_detector, the tables k_spectral_detector takes and the pixel
// function over whole buffers, xrt_host_spectral_detector:
// simpleraytracing_amd/csrc/xrt_detector_host.inc) over their edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/detector_san.cpp \
//         -o detector_san
//
// Exact-size heap buffers, so that a read or write one element past a buffer is
// seen.  Prints "detector_san: OK" and returns 0 when every call returned what
// it should (tests/test_detector_cpu.py runs it).
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
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("detector_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static uint32_t bits_of(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

static uint64_t bits_of(double x)
{
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

static bool same(float a, float b) { return bits_of(a) == bits_of(b) || (std::isnan(a) && std::isnan(b)); }
static bool same(double a, double b) { return bits_of(a) == bits_of(b) || (std::isnan(a) && std::isnan(b)); }

// One pixel as the contract writes it, bin by bin, from the scalar pieces.
static void pixel(uint32_t M, uint32_t K, uint32_t C, const float* d, const float* weight, const float* mu,
                  const float* response, float gain, float read_noise, uint64_t seed, uint64_t g, bool noisy, bool counts,
                  float* out)
{
    using namespace XRT_KERNEL_NS;
    double acc[XRT_MAX_CHANNELS] = {0.0};
    for (uint32_t e = 0; e < K; ++e) {
        double x = 0.0;
        for (uint32_t m = 0; m < M; ++m) x = x + (double)mu[m * K + e] * ((double)d[m] * 0.1);
        const double lam = ((double)weight[e] * xrt_exp(-x)) * (double)gain;
        uint32_t w[4];
        xrt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), e >> 2, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        const double N = noisy ? xrt_poisson_from_word(lam, w[e & 3u]) : lam;
        for (uint32_t c = 0; c < C; ++c) acc[c] = acc[c] + (double)response[c * K + e] * N;
    }
    if (noisy && read_noise > 0.0f)
        for (uint32_t c = 0; c < C; ++c) {
            uint32_t v[4];
            xrt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), c >> 2, 2u, (uint32_t)seed, (uint32_t)(seed >> 32), v);
            acc[c] = acc[c] + (double)read_noise * xrt_normal_from_word(v[c & 3u]);
        }
    for (uint32_t c = 0; c < C; ++c) out[c] = counts ? (float)acc[c] : (float)(acc[c] / (double)gain);
}

int main()
{
    using namespace XRT_KERNEL_NS;
    const float inf = std::numeric_limits<float>::infinity();

    // --- four exp at once equal xrt_exp of each: every class of argument, and a sweep ---
    {
        std::vector<double> xs = {0.0, -0.0, 1e-300, -1e-300, 0x1p-55, -0x1p-55, 0x1p-54, -0x1p-54, 1.0, -1.0, -20.0, 511.9, -511.9,
                                  512.0, -512.0, 700.0, -700.0, 709.78, 709.79, -708.0, -708.4, -740.0, -745.13, -745.14, 1023.9,
                                  -1023.9, 1024.0, -1024.0, 1e300, -1e300, (double)inf, -(double)inf, std::nan("")};
        for (int k = -4000; k <= 4000; ++k) xs.push_back(k * 0.1873);
        while (xs.size() % 4) xs.push_back(0.5);
        for (size_t k = 0; k < xs.size(); k += 4) {
            // each value in each of the four places, beside the other classes
            for (int rot = 0; rot < 4; ++rot) {
                double x[4], y[4];
                for (int j = 0; j < 4; ++j) x[j] = xs[(k + (size_t)((j + rot) & 3) * 7u) % xs.size()];
                xrt_exp_quad(x, y);
                for (int j = 0; j < 4; ++j) EXPECT(same(y[j], xrt_exp(x[j])));
            }
        }
    }

    // --- four counts at once equal xrt_poisson_from_word of each ---
    {
        const double lams[] = {-1.0, -0.0, 0.0, 1e-45, 0.5, 20.0, 63.999996185302734, 64.0, 100.0, 1e4, 16777217.0, 3e38,
                               (double)inf, std::nan("")};
        const size_t L = sizeof(lams) / sizeof(lams[0]);
        uint32_t word = 12345u;
        for (size_t a = 0; a < L; ++a)
            for (size_t b = 0; b < L; ++b) {
                double lam[4] = {lams[a], lams[b], lams[(a + b) % L], lams[(a * 3 + b + 1) % L]}, N[4];
                uint32_t w[4];
                for (int j = 0; j < 4; ++j) w[j] = (word = word * 1664525u + 1013904223u);
                xrt_poisson_quad(lam, w, N);
                for (int j = 0; j < 4; ++j) EXPECT(same(N[j], xrt_poisson_from_word(lam[j], w[j])));
            }
    }

    // --- the pixel function over buffers: every quad edge, mesh and channel count, both modes of each kind ---
    const uint32_t shapes[][4] = {{1, 1, 1, 1}, {63, 1, 3, 2}, {65, 3, 4, 3}, {7 * 13, 3, 5, 8}, {33, 16, 8, 1}, {17, 2, 32, 4}};
    for (const auto& s : shapes) {
        const uint32_t n = s[0], M = s[1], K = s[2], C = s[3];
        float* paths = new float[(size_t)n * M];
        uint16_t* open = new uint16_t[n];
        float* weight = new float[K];
        float* mu = new float[(size_t)M * K];
        float* response = new float[(size_t)C * K];
        float* out = new float[(size_t)n * C];
        for (uint32_t k = 0; k < n * M; ++k)
            paths[k] = k % 11 == 0 ? 0.0f : k % 13 == 0 ? -0.0f : k % 29 == 0 ? NAN : k % 31 == 0 ? 1e6f : (float)(k % 37) * 0.75f;
        for (uint32_t k = 0; k < n; ++k) open[k] = k % 9 == 4 ? (uint16_t)(1u << (k % 16)) : (uint16_t)0;
        for (uint32_t e = 0; e < K; ++e) weight[e] = 0.5f + (float)(e % 5);
        for (uint32_t k = 0; k < M * K; ++k) mu[k] = k % 7 == 0 ? 0.0f : 0.02f * (float)(k % 9);
        for (uint32_t k = 0; k < C * K; ++k) response[k] = k % 5 == 0 ? 0.0f : (float)(k % 4);
        for (uint64_t first : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << 32) - 3u, UINT64_MAX - (uint64_t)n})
            for (float gain : {1e-3f, 3.0f, 40.0f, 5000.0f})
                for (int noisy = 0; noisy < 2; ++noisy)
                    for (int counts = 0; counts < 2; ++counts) {
                        const float rn = noisy && counts ? 2.5f : 0.0f;
                        for (const uint16_t* mask : {(const uint16_t*)open, (const uint16_t*)nullptr}) {
                            EXPECT(xrt_host_spectral_detector(n, M, paths, mask, weight, mu, K, response, C, gain, rn, 77u, first,
                                                              noisy ? XRT_DETECT_NOISY : XRT_DETECT_EXPECTED,
                                                              counts ? XRT_DETECT_COUNTS : XRT_DETECT_INTENSITY, out) == XRT_OK);
                            for (uint32_t i = 0; i < n; ++i) {
                                float want[XRT_MAX_CHANNELS], d[XRT_MAX_MESHES];
                                for (uint32_t m = 0; m < M; ++m) d[m] = paths[(size_t)m * n + i];
                                pixel(M, K, C, d, weight, mu, response, gain, rn, 77u, first + i, noisy != 0, counts != 0, want);
                                for (uint32_t c = 0; c < C; ++c)
                                    EXPECT(same(out[(size_t)c * n + i], mask && mask[i] ? -1.0f : want[c]));
                            }
                        }
                    }
        // the tables the kernel takes: zero past the meshes, bins and channels, the miss value a zero pixel's
        DetectorSpectrum* tab = new DetectorSpectrum;
        DetectorTable* det = new DetectorTable;
        detector_tables(weight, mu, M, K, response, C, 3.0f, 0.0f, XRT_DETECT_EXPECTED, XRT_DETECT_INTENSITY, tab, det);
        EXPECT(tab->num_bins == K && det->num_channels == C && det->counts == 0u && det->gain == 3.0f);
        for (uint32_t e = 0; e < kMaxBins; ++e) {
            EXPECT(tab->weight[e] == (e < K ? weight[e] : 0.0f));
            for (uint32_t m = 0; m < kMaxMeshes; ++m) EXPECT(tab->mu[detector_mu_index(m, e)] == (e < K && m < M ? mu[m * K + e] : 0.0f));
            for (uint32_t c = 0; c < kMaxChannels; ++c)
                EXPECT(det->response[c * kMaxBins + e] == (e < K && c < C ? response[c * K + e] : 0.0f));
        }
        {
            float want[XRT_MAX_CHANNELS];
            const float zero[XRT_MAX_MESHES] = {0.0f};
            pixel(M, K, C, zero, weight, mu, response, 3.0f, 0.0f, 0u, 0u, false, false, want);
            for (uint32_t c = 0; c < kMaxChannels; ++c) EXPECT(same(det->miss[c], c < C ? want[c] : 0.0f));
        }
        delete tab;
        delete det;
        delete[] paths;
        delete[] open;
        delete[] weight;
        delete[] mu;
        delete[] response;
        delete[] out;
    }

    // --- the argument checks -------------------------------------------------
    float paths[48] = {0}, res[48], w[2] = {1.0f, 2.0f}, mu[4] = {0.1f, 0.2f, 0.0f, 0.3f}, r[4] = {1.0f, 0.0f, 0.0f, 1.0f};
    uint16_t open[24] = {0};
    const int EX = XRT_DETECT_EXPECTED, NO = XRT_DETECT_NOISY, CO = XRT_DETECT_COUNTS, IN = XRT_DETECT_INTENSITY;
#define ARGS(n, M, p, o, wt, m, K, rr, C, gain, rn, first, draw, mode, out) \
    detector_arguments(n, M, p, o, wt, m, K, rr, C, gain, rn, first, draw, mode, out)
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) == nullptr);
    EXPECT(ARGS(24, 2, paths, nullptr, w, mu, 2, r, 2, 1e-3f, 4.0f, UINT64_MAX - 24, NO, IN, res) == nullptr);
    EXPECT(ARGS(24, 2, nullptr, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, nullptr, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, nullptr, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, nullptr, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, nullptr) != nullptr);
    EXPECT(ARGS(24, 0, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 17, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 0, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 33, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 0, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 9, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    for (float bad : {-1.0f, inf, NAN}) {
        float rb[4] = {1.0f, 0.0f, 0.0f, bad};
        EXPECT(ARGS(24, 2, paths, open, w, mu, 2, rb, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
        EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, bad, 0, NO, CO, res) != nullptr);
    }
    for (float bad : {0.0f, -1.0f, inf, NAN}) EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, bad, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 1.0f, 0, EX, CO, res) != nullptr);      // read noise without a draw
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, 2, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, -1, res) != nullptr);
    EXPECT(ARGS(0, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(0x7FFFFFFFull * 256u + 1u, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, UINT64_MAX - 23, EX, CO, res) != nullptr);
    EXPECT(ARGS(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, UINT64_MAX, EX, CO, res) != nullptr);
    EXPECT(ARGS(12, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, paths) != nullptr);          // in place
    EXPECT(ARGS(12, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, paths + 23) != nullptr);     // the last path
    EXPECT(ARGS(12, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, paths + 24) == nullptr);     // side by side
    EXPECT(ARGS(12, 2, paths + 24, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, paths) == nullptr);
    EXPECT(ARGS(12, 2, paths + 23, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, paths) != nullptr);
    EXPECT(ARGS(6, 2, paths, reinterpret_cast<uint16_t*>(res + 11), w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) != nullptr);
    EXPECT(ARGS(6, 2, paths, reinterpret_cast<uint16_t*>(res + 12), w, mu, 2, r, 2, 1.0f, 0.0f, 0, EX, CO, res) == nullptr);
    EXPECT(xrt_host_spectral_detector(24, 2, paths, open, w, mu, 2, r, 2, 1.0f, 0.0f, 0, 0, 7, CO, res) == XRT_ERR_ARGUMENT);
    if (!failures) std::printf("detector_san: OK\n");
    return failures ? 1 : 0;
}
