// xrt_decompose_host.inc -- the host pieces of material decomposition
// (include/xrt.h: the argument checks of xrt_decompose[_device] and
// xrt_decompose_guess; include/xrt_debug.h: xrt_host_decompose), included by
// xrt_abi.hip inside its extern "C" block behind xrt_detector_host.inc, whose
// spectrum_arguments and response_arguments check the tables.  Self-contained
// over those, kernels/xrt_device.h's decompose_pixel, decompose_solve and
// DecomposeTable, <cmath>, <cstring> and <cstdint>, so that a stand-alone
// program can compile it under a host sanitizer (tools/decompose_san.cpp).

static_assert(XRT_MAX_BASIS == XRT_KERNEL_NS::kMaxBasis && XRT_DECOMPOSE_MASKED == XRT_KERNEL_NS::kDecomposeMasked &&
                  XRT_DECOMPOSE_FAILED == XRT_KERNEL_NS::kDecomposeFailed,
              "the contract's constants are the kernel's");

// The checks of the tables xrt_decompose and xrt_decompose_guess share; null when they pass.
static const char* decompose_table_arguments(const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins,
                                             const float* response, uint32_t num_channels, float gain)
{
    if (!response) return "response is NULL";
    if (num_basis < 1 || num_basis > XRT_MAX_BASIS) return "num_basis is not 1 to XRT_MAX_BASIS";
    if (const char* why = spectrum_arguments(weight, mu, num_basis, num_bins)) return why;
    if (const char* why = response_arguments(response, num_channels, num_bins, gain)) return why;
    if (num_channels < num_basis) return "num_channels is below num_basis";
    return nullptr;
}

// Every check of xrt_decompose[_device], none of which needs a context: what is wrong, or NULL.
static const char* decompose_arguments(uint64_t num_pixels, const float* channels, const uint16_t* open, const float* weight,
                                       const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                                       uint32_t num_channels, float gain, int in_mode, const double* guess,
                                       uint32_t max_iter, double tol, double damping, const float* out, const uint8_t* iters)
{
    if (!channels) return "channels is NULL";
    if (!out) return "out is NULL";
    if (const char* why = decompose_table_arguments(weight, mu, num_basis, num_bins, response, num_channels, gain))
        return why;
    if (in_mode != XRT_DETECT_COUNTS && in_mode != XRT_DETECT_INTENSITY)
        return "in_mode is neither XRT_DETECT_COUNTS nor XRT_DETECT_INTENSITY";
    if (max_iter < 1 || max_iter > XRT_KERNEL_NS::kDecomposeMaxIter) return "max_iter is not 1 to 200";
    if (!std::isfinite(tol) || tol < 0.0) return "tol is not finite and >= 0";
    if (!std::isfinite(damping) || damping < 0.0) return "damping is not finite and >= 0";
    if (guess)
        for (uint32_t k = 0; k < num_basis * num_channels; ++k)
            if (!std::isfinite(guess[k])) return "a guess entry must be finite";
    if (num_pixels == 0) return "num_pixels is 0";
    // (k_decompose: a workgroup's 256 pixels, one launch's 2^31 - 1 workgroups)
    if (num_pixels > 0x7FFFFFFFull * XRT_KERNEL_NS::kDecomposeThreads)
        return "num_pixels needs more than 2^31 - 1 workgroups: split the call";
    // (byte counts far below 2^64: num_pixels < 2^39)
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(channels), c1 = c0 + num_pixels * num_channels * sizeof(float);
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(open), m1 = m0 + num_pixels * sizeof(uint16_t);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + num_pixels * num_basis * sizeof(float);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(iters), i1 = i0 + num_pixels;
    if (o0 < c1 && c0 < o1) return "out overlaps channels";
    if (open && o0 < m1 && m0 < o1) return "out overlaps open";
    if (iters && i0 < c1 && c0 < i1) return "iters overlaps channels";
    if (iters && open && i0 < m1 && m0 < i1) return "iters overlaps open";
    return nullptr;
}

// k_decompose's table from validated arguments: the coefficients quad by quad, the response at a row
// stride of kMaxBins, both zero past the bases, bins and channels; with a guess, its rows at a stride of
// kMaxChannels and the expected channels at A = 0 (every exp is 1.0), in the pixel function's own order.
// The pointers and the plane stride are the caller's to set.
static void decompose_table(const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins,
                            const float* response, uint32_t num_channels, float gain, int in_mode, const double* guess,
                            uint32_t max_iter, double tol, double damping, XRT_KERNEL_NS::DecomposeTable* tab)
{
    using namespace XRT_KERNEL_NS;
    std::memset(tab, 0, sizeof(*tab));
    const uint32_t K = num_bins;
    for (uint32_t e = 0; e < K; ++e) {
        tab->weight[e] = weight[e];
        for (uint32_t b = 0; b < num_basis; ++b) tab->mu[decompose_mu_index(b, e)] = mu[b * K + e];
        for (uint32_t c = 0; c < num_channels; ++c) tab->response[c * kMaxBins + e] = response[c * K + e];
    }
    tab->gain = gain;
    tab->num_bins = K;
    tab->num_channels = num_channels;
    tab->max_iter = max_iter;
    tab->tol = tol;
    tab->damping = damping;
    tab->intensity = in_mode == XRT_DETECT_INTENSITY ? 1u : 0u;
    tab->has_guess = guess ? 1u : 0u;
    if (!guess) return;
    for (uint32_t c = 0; c < num_channels; ++c) {
        double y0 = 0.0;
        for (uint32_t e = 0; e < K; ++e) y0 = y0 + (double)response[c * K + e] * (((double)weight[e] * 1.0) * (double)gain);
        tab->y0[c] = y0;
        for (uint32_t b = 0; b < num_basis; ++b) tab->guess[b * kMaxChannels + c] = guess[b * num_channels + c];
    }
}

// xrt_decompose_guess' arithmetic over checked tables: what is wrong, or NULL.
static const char* decompose_guess_matrix(const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins,
                                          const float* response, uint32_t num_channels, double* guess)
{
    using namespace XRT_KERNEL_NS;
    const uint32_t B = num_basis, C = num_channels, K = num_bins;
    double mbar[kMaxChannels][kMaxBasis] = {};
    bool used[kMaxChannels] = {};
    for (uint32_t c = 0; c < C; ++c) {
        double den = 0.0, num[kMaxBasis] = {0.0, 0.0, 0.0};
        for (uint32_t e = 0; e < K; ++e) {
            const double rw = (double)response[c * K + e] * (double)weight[e];
            den = den + rw;
            for (uint32_t b = 0; b < B; ++b) num[b] = num[b] + rw * (double)mu[b * K + e];
        }
        used[c] = den > 0.0;
        for (uint32_t b = 0; b < B; ++b) mbar[c][b] = used[c] ? 0.1 * (num[b] / den) : 0.0;
    }
    double N[kMaxBasis][kMaxBasis] = {};
    for (uint32_t c = 0; c < C; ++c) {
        if (!used[c]) continue;
        for (uint32_t b = 0; b < B; ++b)
            for (uint32_t b2 = b; b2 < B; ++b2) N[b][b2] = N[b][b2] + mbar[c][b] * mbar[c][b2];
    }
    for (uint32_t c = 0; c < C; ++c) {
        double rhs[kMaxBasis] = {mbar[c][0], mbar[c][1], mbar[c][2]}, x[kMaxBasis] = {0.0, 0.0, 0.0};
        const bool ok = B == 1 ? decompose_solve<1>(N, rhs, x) : B == 2 ? decompose_solve<2>(N, rhs, x) : decompose_solve<3>(N, rhs, x);
        if (!ok) return "basis materials are not separable under this response";
        for (uint32_t b = 0; b < B; ++b) guess[b * C + c] = used[c] ? x[b] : 0.0;
    }
    return nullptr;
}

// decompose_pixel over whole host buffers under the widest channel bound.
extern "C++" {
template <uint32_t kB>
static void host_decompose_pixels(uint64_t n, const float* channels, const uint16_t* open, const float* weight, const float* mu,
                                  uint32_t K, const float* response, uint32_t C, float gain, int in_mode, const double* guess,
                                  const double* y0, uint32_t max_iter, double tol, double damping, float* out, uint8_t* iters)
{
    using namespace XRT_KERNEL_NS;
    for (uint64_t i = 0; i < n; ++i) {
        if (open && open[i] != 0) {
            for (uint32_t b = 0; b < kB; ++b) out[b * n + i] = 0.0f;
            if (iters) iters[i] = (uint8_t)kDecomposeMasked;
            continue;
        }
        double y[kMaxChannels], A[kB];
        for (uint32_t c = 0; c < kMaxChannels; ++c) {
            y[c] = c < C ? (double)channels[c * n + i] : 0.0;
            if (in_mode == XRT_DETECT_INTENSITY) y[c] = y[c] * (double)gain;
        }
        const uint32_t status = decompose_pixel<kB, kMaxChannels>(
            K, C, [&](uint32_t b, uint32_t e) { return e < K ? mu[b * K + e] : 0.0f; },
            [&](uint32_t e) { return e < K ? weight[e] : 0.0f; },
            [&](uint32_t c, uint32_t e) { return c < C && e < K ? response[c * K + e] : 0.0f; }, gain, y, guess != nullptr,
            [&](uint32_t b, uint32_t c) { return guess[b * C + c]; }, [&](uint32_t c) { return y0[c]; }, max_iter, tol,
            damping, A);
        for (uint32_t b = 0; b < kB; ++b) out[b * n + i] = (float)A[b];
        if (iters) iters[i] = (uint8_t)status;
    }
}
}  // extern "C++"

// The kernel's pixel function over whole buffers on the host (test
// infrastructure: what k_decompose is compared with on a machine without a
// device, not a fallback).  Arguments and checks as xrt_decompose's.
int xrt_host_decompose(uint64_t num_pixels, const float* channels, const uint16_t* open, const float* weight, const float* mu,
                       uint32_t num_basis, uint32_t num_bins, const float* response, uint32_t num_channels, float gain,
                       int in_mode, const double* guess, uint32_t max_iter, double tol, double damping, float* out,
                       uint8_t* iters)
{
    if (decompose_arguments(num_pixels, channels, open, weight, mu, num_basis, num_bins, response, num_channels, gain, in_mode,
                            guess, max_iter, tol, damping, out, iters))
        return XRT_ERR_ARGUMENT;
    XRT_KERNEL_NS::DecomposeTable tab;                      // (for y0, in the table's own order)
    decompose_table(weight, mu, num_basis, num_bins, response, num_channels, gain, in_mode, guess, max_iter, tol, damping, &tab);
    const auto run = num_basis == 1 ? host_decompose_pixels<1> : num_basis == 2 ? host_decompose_pixels<2> : host_decompose_pixels<3>;
    run(num_pixels, channels, open, weight, mu, num_bins, response, num_channels, gain, in_mode, guess, tab.y0, max_iter, tol,
        damping, out, iters);
    return XRT_OK;
}
