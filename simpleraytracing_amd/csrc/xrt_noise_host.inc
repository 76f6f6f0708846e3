// xrt_noise_host.inc -- the host pieces of the photon noise (include/xrt.h: the
// argument checks of xrt_photon_noise[_device]; include/xrt_debug.h:
// xrt_host_philox4x32, xrt_host_poisson_batch, xrt_host_photon_noise), included
// by xrt_abi.hip inside its extern "C" block.  Self-contained over
// kernels/xrt_device.h's xrt_philox4x32_10, xrt_poisson_from_word,
// xrt_noise_output and photon_noise_lanes, <cmath> and <cstdint>, so that a
// stand-alone program can compile it under a host sanitizer
// (tools/noise_san.cpp).

// Every check of xrt_photon_noise[_device], none of which needs a context: what
// is wrong, or NULL; *num_pixels = width * height * num_planes where it is NULL.
static const char* noise_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, float gain,
                                   uint64_t first_index, int mode, const float* out, uint64_t* num_pixels)
{
    if (!image) return "the image is NULL";
    if (!out) return "out is NULL";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (mode != XRT_NOISE_INTENSITY && mode != XRT_NOISE_COUNTS) return "mode is neither XRT_NOISE_INTENSITY nor XRT_NOISE_COUNTS";
    if (!std::isfinite(gain) || !(gain > 0.0f)) return "gain is not finite and > 0";
    // (k_photon_noise: 256 lanes of 4 pixels a workgroup, one launch's 2^31 - 1 workgroups; two more lanes where
    // first_index cuts the first group)
    constexpr uint64_t kMaxPixels = ((0x7FFFFFFFull * XRT_KERNEL_NS::kNoiseThreads) - 2u) * 4u;
    const uint64_t plane = (uint64_t)width * height;                    // (below 2^64)
    if (plane > kMaxPixels || num_planes > kMaxPixels / plane)
        return "the planes need more than 2^31 - 1 workgroups: split the call";
    const uint64_t n = plane * num_planes;
    if (first_index > UINT64_MAX - n) return "first_index + the number of pixels overflows 64 bits";
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(image), b0 = reinterpret_cast<uintptr_t>(out);
    const uint64_t bytes = n * sizeof(float);
    if (out != image && a0 < b0 + bytes && b0 < a0 + bytes)
        return "out overlaps the image (in place is out == image exactly)";
    *num_pixels = n;
    return nullptr;
}

void xrt_host_philox4x32(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t w[4];
    XRT_KERNEL_NS::xrt_philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], w);
    for (int e = 0; e < 4; ++e) out[e] = w[e];
}

void xrt_host_poisson_batch(const double* lam, const uint32_t* words, uint64_t n, double* outp)
{
    for (uint64_t i = 0; i < n; ++i) outp[i] = XRT_KERNEL_NS::xrt_poisson_from_word(lam[i], words[i]);
}

// The kernel's pixel function over whole buffers on the host (test
// infrastructure: what k_photon_noise is compared with on a machine without a
// device, not a fallback).  In place, a pixel is read before it is written.
int xrt_host_photon_noise(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, float gain,
                          uint64_t seed, uint64_t first_index, int mode, float* out)
{
    uint64_t n = 0;
    if (noise_arguments(width, height, num_planes, image, gain, first_index, mode, out, &n)) return XRT_ERR_ARGUMENT;
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t have = UINT64_MAX;                                         // the counter w holds (none yet)
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t g = first_index + i;
        if ((g >> 2) != have || i == 0) {
            have = g >> 2;
            XRT_KERNEL_NS::xrt_noise_words(have, seed, w);
        }
        const float lam_f = image[i] * gain;
        out[i] = XRT_KERNEL_NS::xrt_noise_output(XRT_KERNEL_NS::xrt_poisson_from_word((double)lam_f, w[g & 3u]), gain,
                                                 mode == XRT_NOISE_COUNTS);
    }
    return XRT_OK;
}
