// decompose_san.cpp -- material decomposition's host code (the argument checks
// of xrt_decompose, the table k_decompose takes, xrt_decompose_guess' matrix and
// the pixel function over whole buffers, xrt_host_decompose:
// simpleraytracing_amd/csrc/xrt_decompose_host.inc) over their edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/decompose_san.cpp \
//         -o decompose_san
//
// Exact-size heap buffers, so that a read or write one element past a buffer is
// seen.  Prints "decompose_san: OK" and returns 0 when every call returned what
// it should (tests/test_decompose_cpu.py runs it).
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
#include "xrt_decompose_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("decompose_san: line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static bool same(float a, float b)
{
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y || (std::isnan(a) && std::isnan(b));
}

// One unmasked pixel as the contract writes it, bin by bin and channel by
// channel, over exactly B bases, C channels and K bins: no padding, xrt_exp one
// at a time.  y is the pixel's counts; returns the status.
static uint32_t pixel(uint32_t B, uint32_t C, uint32_t K, const double* y, const float* weight, const float* mu,
                      const float* response, float gain, const double* guess, uint32_t max_iter, double tol, double damping,
                      double* A)
{
    using namespace XRT_KERNEL_NS;
    for (uint32_t b = 0; b < B; ++b) A[b] = 0.0;
    if (guess) {
        double p[XRT_MAX_CHANNELS];
        for (uint32_t c = 0; c < C; ++c) {
            double y0 = 0.0;
            for (uint32_t e = 0; e < K; ++e) y0 = y0 + (double)response[c * K + e] * (((double)weight[e] * 1.0) * (double)gain);
            float t = (float)(y[c] / y0);
            if (!(t >= 1e-30f)) t = 1e-30f;
            p[c] = -(double)xrt_logf(t);
        }
        for (uint32_t b = 0; b < B; ++b)
            for (uint32_t c = 0; c < C; ++c) A[b] = A[b] + guess[b * C + c] * p[c];
    }
    uint32_t it = 0;
    while (it < max_iter) {
        double ybar[XRT_MAX_CHANNELS] = {0.0}, J[XRT_MAX_CHANNELS][XRT_MAX_BASIS] = {{0.0}};
        for (uint32_t e = 0; e < K; ++e) {
            double x = 0.0;
            for (uint32_t b = 0; b < B; ++b) x = x + (double)mu[b * K + e] * (A[b] * 0.1);
            const double lam = ((double)weight[e] * xrt_exp(-x)) * (double)gain;
            for (uint32_t c = 0; c < C; ++c) {
                const double t = (double)response[c * K + e] * lam;
                ybar[c] = ybar[c] + t;
                for (uint32_t b = 0; b < B; ++b) J[c][b] = J[c][b] + (double)mu[b * K + e] * t;
            }
        }
        double g[XRT_MAX_BASIS] = {0.0}, H[XRT_MAX_BASIS][XRT_MAX_BASIS] = {{0.0}};
        for (uint32_t c = 0; c < C; ++c) {
            if (!(ybar[c] > 0.0)) continue;
            const double q = y[c] / ybar[c], r = 1.0 - q, v = 1.0 / ybar[c];
            for (uint32_t b = 0; b < B; ++b) g[b] = g[b] + J[c][b] * r;
            for (uint32_t b = 0; b < B; ++b)
                for (uint32_t b2 = b; b2 < B; ++b2) H[b][b2] = H[b][b2] + (J[c][b] * J[c][b2]) * v;
        }
        for (uint32_t b = 0; b < B; ++b) H[b][b] = H[b][b] + H[b][b] * damping;
        double x[XRT_MAX_BASIS] = {0.0};
        const double d0 = H[0][0];
        if (!(d0 > 0.0)) return XRT_DECOMPOSE_FAILED;
        if (B == 1) {
            x[0] = g[0] / d0;
        } else {
            const double l10 = H[0][1] / d0, d1 = H[1][1] - l10 * H[0][1];
            const double z0 = g[0], z1 = g[1] - l10 * z0;
            if (!(d1 > 0.0)) return XRT_DECOMPOSE_FAILED;
            if (B == 2) {
                x[1] = z1 / d1;
                x[0] = z0 / d0 - l10 * x[1];
            } else {
                const double l20 = H[0][2] / d0, l21 = (H[1][2] - l20 * H[0][1]) / d1;
                const double d2 = (H[2][2] - l20 * H[0][2]) - l21 * (l21 * d1);
                const double z2 = (g[2] - l20 * z0) - l21 * z1;
                if (!(d2 > 0.0)) return XRT_DECOMPOSE_FAILED;
                x[2] = z2 / d2;
                x[1] = z1 / d1 - l21 * x[2];
                x[0] = (z0 / d0 - l10 * x[1]) - l20 * x[2];
            }
        }
        bool done = true;
        for (uint32_t b = 0; b < B; ++b) {
            const double s = x[b] / 0.1;
            A[b] = A[b] + s;
            done = done && std::fabs(s) <= tol;
        }
        ++it;
        if (done) break;
    }
    return it;
}

// The detector's expected counts of one pixel under the same tables.
static void forward(uint32_t B, uint32_t C, uint32_t K, const float* d, const float* weight, const float* mu,
                    const float* response, float gain, bool counts, float* out)
{
    using namespace XRT_KERNEL_NS;
    double acc[XRT_MAX_CHANNELS] = {0.0};
    for (uint32_t e = 0; e < K; ++e) {
        double x = 0.0;
        for (uint32_t b = 0; b < B; ++b) x = x + (double)mu[b * K + e] * ((double)d[b] * 0.1);
        const double lam = ((double)weight[e] * xrt_exp(-x)) * (double)gain;
        for (uint32_t c = 0; c < C; ++c) acc[c] = acc[c] + (double)response[c * K + e] * lam;
    }
    for (uint32_t c = 0; c < C; ++c) out[c] = counts ? (float)acc[c] : (float)(acc[c] / (double)gain);
}

static void run_case(uint32_t B, uint32_t C, uint32_t K, uint64_t n, bool counts, bool with_guess, bool zero_row,
                     uint32_t max_iter, double tol, double damping)
{
    const float gain = 3.0f;
    std::vector<float> weight(K), mu((size_t)B * K), response((size_t)C * K);
    for (uint32_t e = 0; e < K; ++e) {
        const float u = ((float)e + 0.5f) / (float)K;
        weight[e] = 20.0f + 30.0f * u * (1.0f - u) * 4.0f;
        for (uint32_t b = 0; b < B; ++b)
            mu[b * K + e] = zero_row && b == 1 ? 0.0f : b == 0 ? 0.35f - 0.17f * u : b == 1 ? 2.0f - 1.6f * u : (u < 0.5f ? 0.9f - 0.8f * u : 2.4f - 1.6f * u);
        for (uint32_t c = 0; c < C; ++c) response[c * K + e] = C <= K ? (e * C / K == c ? 1.0f : 0.0f) : 0.2f + 0.1f * (float)((c * 7u + e * 3u) % 8u);
    }
    std::vector<float> channels((size_t)C * n), out((size_t)B * n);
    std::vector<uint16_t> open(n, 0);
    std::vector<uint8_t> iters(n);
    for (uint64_t i = 0; i < n; ++i) {
        float d[XRT_MAX_BASIS], ch[XRT_MAX_CHANNELS];
        for (uint32_t b = 0; b < B; ++b) d[b] = (float)((i * 37u + b * 11u) % 23u) * (b == 0 ? 4.0f : 0.7f);
        forward(B, C, K, d, weight.data(), mu.data(), response.data(), gain, counts, ch);
        for (uint32_t c = 0; c < C; ++c) channels[c * n + i] = ch[c];
    }
    if (n > 8) {
        channels[0 * n + 1] = 0.0f;                                             // a zero count
        channels[(C - 1) * n + 2] = -4.0f;                                      // a negative one
        channels[0 * n + 3] = std::numeric_limits<float>::quiet_NaN();          // a NaN
        open[4] = 0x8000u;                                                      // a masked pixel
    }
    std::vector<double> guess((size_t)B * C);
    const double* gp = nullptr;
    if (with_guess) {
        const char* why = decompose_guess_matrix(weight.data(), mu.data(), B, K, response.data(), C, guess.data());
        EXPECT(zero_row ? why != nullptr : why == nullptr);
        if (!why) gp = guess.data();
    }
    const int mode = counts ? XRT_DETECT_COUNTS : XRT_DETECT_INTENSITY;
    EXPECT(xrt_host_decompose(n, channels.data(), open.data(), weight.data(), mu.data(), B, K, response.data(), C, gain, mode, gp,
                              max_iter, tol, damping, out.data(), iters.data()) == XRT_OK);
    std::vector<float> out2((size_t)B * n);                                     // no mask, no iters plane
    EXPECT(xrt_host_decompose(n, channels.data(), nullptr, weight.data(), mu.data(), B, K, response.data(), C, gain, mode, gp,
                              max_iter, tol, damping, out2.data(), nullptr) == XRT_OK);
    for (uint64_t i = 0; i < n; ++i) {
        if (open[i]) {
            for (uint32_t b = 0; b < B; ++b) EXPECT(same(out[b * n + i], 0.0f));
            EXPECT(iters[i] == XRT_DECOMPOSE_MASKED);
            continue;
        }
        double y[XRT_MAX_CHANNELS], A[XRT_MAX_BASIS];
        for (uint32_t c = 0; c < C; ++c) {
            y[c] = (double)channels[c * n + i];
            if (!counts) y[c] = y[c] * (double)gain;
        }
        const uint32_t status = pixel(B, C, K, y, weight.data(), mu.data(), response.data(), gain, gp, max_iter, tol, damping, A);
        EXPECT(iters[i] == status);
        for (uint32_t b = 0; b < B; ++b) {
            EXPECT(same(out[b * n + i], (float)A[b]));
            EXPECT(same(out2[b * n + i], (float)A[b]));
        }
        if (zero_row && B >= 2) EXPECT(status == XRT_DECOMPOSE_FAILED && A[0] == 0.0);      // a pivot of 0: A as started
        // (a NaN count from zeros under a separable table: the first step makes A a NaN)
        if (n > 8 && i == 3 && !gp && iters[5] != XRT_DECOMPOSE_FAILED) EXPECT(std::isnan(out[i]));
    }
}

int main()
{
    const uint32_t Cs[] = {1, 2, 3, 4, 5, 8}, Ks[] = {1, 4, 5, 32};
    for (uint32_t B = 1; B <= 3; ++B)
        for (uint32_t C : Cs)
            for (uint32_t K : Ks) {
                if (C < B) continue;
                run_case(B, C, K, 67, (B + C + K) % 2 == 0, K >= B && C <= 8 && K > 1, false, 32, 1e-6, 0.0);
            }
    run_case(3, 8, 32, 131, true, true, false, 32, 1e-6, 0.0);
    run_case(3, 8, 32, 131, false, false, false, 200, 0.0, 0.5);
    run_case(3, 8, 32, 1, true, true, false, 1, 1e-6, 0.0);
    run_case(2, 4, 8, 67, true, false, true, 32, 1e-6, 0.0);                    // a basis of zeros: the pivot fails
    run_case(3, 8, 32, 67, true, true, true, 32, 1e-6, 0.0);                    // and the guess refuses it

    // the checks, on exact-size buffers
    {
        const uint32_t B = 2, C = 3, K = 4;
        const uint64_t n = 5;
        std::vector<float> weight(K, 1.0f), mu(B * K, 0.1f), response(C * K, 1.0f), ch(C * n, 1.0f), out(B * n);
        std::vector<uint8_t> iters(n);
        std::vector<double> guess(B * C, 0.0);
        auto why = [&](uint32_t b, uint32_t c, uint32_t k, uint32_t it, double tol, double damping) {
            return decompose_arguments(n, ch.data(), nullptr, weight.data(), mu.data(), b, k, response.data(), c, 1.0f,
                                       XRT_DETECT_COUNTS, guess.data(), it, tol, damping, out.data(), iters.data());
        };
        EXPECT(why(B, C, K, 1, 0.0, 0.0) == nullptr);
        EXPECT(why(0, C, K, 1, 0.0, 0.0) != nullptr && why(4, C, K, 1, 0.0, 0.0) != nullptr);
        EXPECT(why(B, 1, K, 1, 0.0, 0.0) != nullptr && why(B, 9, K, 1, 0.0, 0.0) != nullptr);
        EXPECT(why(B, C, 0, 1, 0.0, 0.0) != nullptr && why(B, C, 33, 1, 0.0, 0.0) != nullptr);
        EXPECT(why(B, C, K, 0, 0.0, 0.0) != nullptr && why(B, C, K, 201, 0.0, 0.0) != nullptr);
        EXPECT(why(B, C, K, 1, -1.0, 0.0) != nullptr && why(B, C, K, 1, 0.0, std::nan("")) != nullptr);
        guess[B * C - 1] = std::numeric_limits<double>::infinity();
        EXPECT(why(B, C, K, 1, 0.0, 0.0) != nullptr);
        XRT_KERNEL_NS::DecomposeTable tab;
        guess[B * C - 1] = 0.25;
        decompose_table(weight.data(), mu.data(), B, K, response.data(), C, 2.0f, XRT_DETECT_INTENSITY, guess.data(), 7, 1e-3,
                        0.5, &tab);
        EXPECT(tab.num_bins == K && tab.num_channels == C && tab.max_iter == 7 && tab.intensity == 1u && tab.has_guess == 1u);
        EXPECT(tab.guess[1 * XRT_MAX_CHANNELS + 2] == 0.25 && tab.y0[0] == 8.0 && tab.y0[C] == 0.0);
        EXPECT(tab.mu[XRT_KERNEL_NS::decompose_mu_index(1, 3)] == 0.1f && tab.mu[XRT_KERNEL_NS::decompose_mu_index(2, 3)] == 0.0f);
    }
    if (!failures) std::printf("decompose_san: OK\n");
    return failures ? 1 : 0;
}
