// xrt_detector_host.inc -- the host pieces of the spectral detector
// (include/xrt.h: the argument checks of xrt_spectral_detector[_device] and,
// with them, the spectrum table's, which xrt_set_spectrum and xrt_apply_spectrum
// share; include/xrt_debug.h: xrt_host_spectral_detector), included by
// xrt_abi.hip inside its extern "C" block.  Self-contained over
// kernels/xrt_device.h's detector_pixel, xrt_detector_output, DetectorSpectrum
// and DetectorTable, <cmath>, <cstring> and <cstdint>, so that a stand-alone program
// can compile it under a host sanitizer (tools/detector_san.cpp).

// The argument checks of a spectrum table (no device needed); null when they pass.
static const char* spectrum_arguments(const float* weight, const float* mu, uint32_t num_meshes,
                                      uint32_t num_bins)
{
    if (num_meshes < 1 || num_meshes > XRT_MAX_MESHES) return "1 to XRT_MAX_MESHES meshes";
    if (num_bins < 1 || num_bins > XRT_MAX_BINS) return "1 to XRT_MAX_BINS energy bins";
    if (!weight) return "weight is NULL";
    if (!mu) return "mu is NULL";
    for (uint32_t e = 0; e < num_bins; ++e)
        if (!std::isfinite(weight[e]) || !(weight[e] > 0.0f)) return "a weight must be finite and > 0";
    for (uint32_t i = 0; i < num_meshes * num_bins; ++i)
        if (!std::isfinite(mu[i]) || mu[i] < 0.0f) return "a coefficient must be finite and >= 0";
    return nullptr;
}

static_assert(XRT_MAX_CHANNELS == XRT_KERNEL_NS::kMaxChannels && XRT_MAX_BINS == XRT_KERNEL_NS::kMaxBins,
              "the contract's bounds are the tables'");

// The argument checks of a response matrix (not NULL, under a checked num_bins) and its gain, which
// xrt_decompose shares; null when they pass.
static const char* response_arguments(const float* response, uint32_t num_channels, uint32_t num_bins, float gain)
{
    if (num_channels < 1 || num_channels > XRT_MAX_CHANNELS) return "num_channels is not 1 to XRT_MAX_CHANNELS";
    for (uint32_t k = 0; k < num_channels * num_bins; ++k)
        if (!std::isfinite(response[k]) || response[k] < 0.0f) return "a response must be finite and >= 0";
    if (!std::isfinite(gain) || !(gain > 0.0f)) return "gain is not finite and > 0";
    return nullptr;
}

// Every check of xrt_spectral_detector[_device], none of which needs a context:
// what is wrong, or NULL.
static const char* detector_arguments(uint64_t num_pixels, uint32_t num_meshes, const float* paths, const uint16_t* open,
                                      const float* weight, const float* mu, uint32_t num_bins, const float* response,
                                      uint32_t num_channels, float gain, float read_noise, uint64_t first_index,
                                      int draw_mode, int out_mode, const float* out)
{
    if (!paths) return "paths is NULL";
    if (!response) return "response is NULL";
    if (!out) return "out is NULL";
    if (const char* why = spectrum_arguments(weight, mu, num_meshes, num_bins)) return why;
    if (const char* why = response_arguments(response, num_channels, num_bins, gain)) return why;
    if (draw_mode != XRT_DETECT_EXPECTED && draw_mode != XRT_DETECT_NOISY)
        return "draw_mode is neither XRT_DETECT_EXPECTED nor XRT_DETECT_NOISY";
    if (out_mode != XRT_DETECT_COUNTS && out_mode != XRT_DETECT_INTENSITY)
        return "out_mode is neither XRT_DETECT_COUNTS nor XRT_DETECT_INTENSITY";
    if (!std::isfinite(read_noise) || read_noise < 0.0f) return "read_noise is not finite and >= 0";
    if (draw_mode == XRT_DETECT_EXPECTED && read_noise != 0.0f) return "read_noise must be 0 under XRT_DETECT_EXPECTED";
    if (num_pixels == 0) return "num_pixels is 0";
    // (k_spectral_detector: a workgroup's 256 pixels, one launch's 2^31 - 1 workgroups)
    if (num_pixels > 0x7FFFFFFFull * XRT_KERNEL_NS::kDetectorThreads)
        return "num_pixels needs more than 2^31 - 1 workgroups: split the call";
    if (first_index > UINT64_MAX - num_pixels) return "first_index + num_pixels overflows 64 bits";
    // (byte counts far below 2^64: num_pixels < 2^39)
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + num_pixels * num_channels * sizeof(float);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(paths), p1 = p0 + num_pixels * num_meshes * sizeof(float);
    if (o0 < p1 && p0 < o1) return "out overlaps paths";
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(open), m1 = m0 + num_pixels * sizeof(uint16_t);
    if (open && o0 < m1 && m0 < o1) return "out overlaps open";
    return nullptr;
}

// k_spectral_detector's tables from validated arguments: the spectrum quad
// by quad, the response at a row stride of kMaxBins, both zero past the
// meshes, bins and channels; under XRT_DETECT_EXPECTED a channel's miss value
// is detector_pixel's own result over zero distances.
static void detector_tables(const float* weight, const float* mu, uint32_t num_meshes, uint32_t num_bins,
                            const float* response, uint32_t num_channels, float gain, float read_noise, int draw_mode,
                            int out_mode, XRT_KERNEL_NS::DetectorSpectrum* tab, XRT_KERNEL_NS::DetectorTable* det)
{
    using namespace XRT_KERNEL_NS;
    std::memset(tab, 0, sizeof(*tab));
    std::memset(det, 0, sizeof(*det));
    const uint32_t K = num_bins;
    tab->num_bins = K;
    for (uint32_t e = 0; e < K; ++e) {
        tab->weight[e] = weight[e];
        for (uint32_t m = 0; m < num_meshes; ++m) tab->mu[detector_mu_index(m, e)] = mu[m * K + e];
        for (uint32_t c = 0; c < num_channels; ++c) det->response[c * kMaxBins + e] = response[c * K + e];
    }
    det->gain = gain;
    det->read_noise = read_noise;
    det->num_channels = num_channels;
    det->counts = out_mode == XRT_DETECT_COUNTS ? 1u : 0u;
    if (draw_mode != XRT_DETECT_EXPECTED) return;
    double acc[kMaxChannels];
    detector_pixel<kMaxChannels, false>(
        K, [](uint32_t, double (&)[4]) {}, [&](uint32_t e) { return tab->weight[e]; },
        [&](uint32_t c, uint32_t e) { return det->response[c * kMaxBins + e]; }, gain, 0u, 0u, []() { return 0.0f; },
        []() { return (uint64_t)0; }, acc);
    for (uint32_t c = 0; c < num_channels; ++c) det->miss[c] = xrt_detector_output(acc[c], gain, det->counts != 0u);
}

// The kernel's pixel function over whole buffers on the host (test
// infrastructure: what k_spectral_detector is compared with on a machine
// without a device, not a fallback).  Arguments and checks as
// xrt_spectral_detector's.
int xrt_host_spectral_detector(uint64_t num_pixels, uint32_t num_meshes, const float* paths, const uint16_t* open,
                               const float* weight, const float* mu, uint32_t num_bins, const float* response,
                               uint32_t num_channels, float gain, float read_noise, uint64_t seed, uint64_t first_index,
                               int draw_mode, int out_mode, float* out)
{
    using namespace XRT_KERNEL_NS;
    if (detector_arguments(num_pixels, num_meshes, paths, open, weight, mu, num_bins, response, num_channels, gain,
                           read_noise, first_index, draw_mode, out_mode, out))
        return XRT_ERR_ARGUMENT;
    const uint32_t K = num_bins, M = num_meshes, C = num_channels;
    const bool counts = out_mode == XRT_DETECT_COUNTS;
    for (uint64_t i = 0; i < num_pixels; ++i) {
        if (open && open[i] != 0) {
            for (uint32_t c = 0; c < C; ++c) out[c * num_pixels + i] = -1.0f;
            continue;
        }
        double acc[kMaxChannels];
        auto quad_x = [&](uint32_t q, double (&x)[4]) {
            for (uint32_t m = 0; m < M; ++m) {
                const double pd = (double)paths[m * num_pixels + i] * 0.1;
                for (uint32_t r = 0; r < 4; ++r) {
                    const uint32_t e = 4u * q + r;
                    x[r] = x[r] + (double)(e < K ? mu[m * K + e] : 0.0f) * pd;
                }
            }
        };
        auto wt = [&](uint32_t e) { return e < K ? weight[e] : 0.0f; };
        auto resp = [&](uint32_t c, uint32_t e) { return c < C && e < K ? response[c * K + e] : 0.0f; };
        auto rn = [&]() { return read_noise; };
        auto s2 = [&]() { return seed; };
        if (draw_mode == XRT_DETECT_NOISY)
            detector_pixel<kMaxChannels, true>(K, quad_x, wt, resp, gain, seed, first_index + i, rn, s2, acc);
        else
            detector_pixel<kMaxChannels, false>(K, quad_x, wt, resp, gain, seed, first_index + i, rn, s2, acc);
        for (uint32_t c = 0; c < C; ++c) out[c * num_pixels + i] = xrt_detector_output(acc[c], gain, counts);
    }
    return XRT_OK;
}
