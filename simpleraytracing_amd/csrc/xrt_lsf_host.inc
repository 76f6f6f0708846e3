// xrt_lsf_host.inc -- the host pieces of the detector response (include/xrt.h:
// xrt_lsf_gaussian; include/xrt_debug.h: xrt_host_lsf; the argument checks of
// xrt_detector_response[_device]), included by xrt_abi.hip inside its
// extern "C" block.  Self-contained over kernels/xrt_device.h's lsf_chunk and
// lut_u8, <cmath>, <cstdint> and <vector>, so that a stand-alone program can
// compile it under a host sanitizer (tools/lsf_san.cpp).

// What is wrong with a pair of tap tables, or NULL.
static const char* lsf_tap_arguments(const float* lsf_x, uint32_t taps_x, const float* lsf_y, uint32_t taps_y)
{
    if (!lsf_x || !lsf_y) return "a tap table is NULL";
    if (taps_x == 0 || taps_x > XRT_MAX_LSF_TAPS || taps_y == 0 || taps_y > XRT_MAX_LSF_TAPS)
        return "a tap count is outside 1..XRT_MAX_LSF_TAPS";
    if (taps_x % 2u == 0u || taps_y % 2u == 0u) return "a tap count is even";
    for (uint32_t k = 0; k < taps_x; ++k)
        if (!std::isfinite(lsf_x[k])) return "a tap is not finite";
    for (uint32_t k = 0; k < taps_y; ++k)
        if (!std::isfinite(lsf_y[k])) return "a tap is not finite";
    return nullptr;
}

static bool lsf_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every check of xrt_detector_response[_device] that needs no context, the
// taps' first: what is wrong, or NULL.
static const char* lsf_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                                 const float* lsf_x, uint32_t taps_x, const float* lsf_y, uint32_t taps_y,
                                 const float* out, const uint8_t* out_u8)
{
    if (const char* why = lsf_tap_arguments(lsf_x, taps_x, lsf_y, taps_y)) return why;
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    // (k_lsf: 32-bit signed pixel coordinates; one workgroup per 64 x 64 tile and plane, the grid's y and z extents)
    if (width > 0x7FFFFFFFu) return "width is above 2^31 - 1";
    if (((uint64_t)height + 63u) / 64u > 65535u || num_planes > 65535u) return "more than 65535 tile rows or planes";
    if (!image) return "the image is NULL";
    if (!out && !out_u8) return "out and out_u8 are both NULL";
    const uint64_t n = (uint64_t)width * height * num_planes;
    if ((out && lsf_overlap(image, n * sizeof(float), out, n * sizeof(float))) ||
        (out_u8 && lsf_overlap(image, n * sizeof(float), out_u8, n)))
        return "an output overlaps the image (the response is not computed in place)";
    return nullptr;
}

int xrt_lsf_gaussian(double sigma_pixels, uint32_t taps, float* lsf)
{
    if (!lsf || !std::isfinite(sigma_pixels) || !(sigma_pixels > 0.0)) return XRT_ERR_ARGUMENT;
    if (taps == 0 || taps > XRT_MAX_LSF_TAPS || taps % 2u == 0u) return XRT_ERR_ARGUMENT;
    const double r = (double)((taps - 1u) / 2u);
    double g[XRT_MAX_LSF_TAPS];
    double s = 0.0;
    for (uint32_t k = 0; k < taps; ++k) {
        const double u = ((double)k - r) / sigma_pixels;
        g[k] = std::exp(-0.5 * (u * u));
        s = s + g[k];
    }
    for (uint32_t k = 0; k < taps; ++k) lsf[k] = (float)(g[k] / s);
    return XRT_OK;
}

// lut_u8 on the host: the same values, without its discarded conversion of an
// out-of-window product to an unsigned integer (undefined in host C++).
static uint8_t lsf_host_u8(float v)
{
    return v >= 0.0f && v <= 80.0f ? XRT_KERNEL_NS::lut_u8(v) : v > 80.0f ? (uint8_t)255u : (uint8_t)0u;
}

// The kernel's arithmetic over whole planes on the host: lsf_chunk along x into
// an f32 plane, lsf_chunk along y out of it (test infrastructure: what k_lsf is
// compared with on a machine without a device, not a fallback).
int xrt_host_lsf(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, const float* lsf_x,
                 uint32_t taps_x, const float* lsf_y, uint32_t taps_y, float* out, uint8_t* out_u8)
{
    using namespace XRT_KERNEL_NS;
    if (lsf_arguments(width, height, num_planes, image, lsf_x, taps_x, lsf_y, taps_y, out, out_u8))
        return XRT_ERR_ARGUMENT;
    const int64_t W = width, H = height;
    const int64_t rx = (taps_x - 1u) / 2u, ry = (taps_y - 1u) / 2u;
    std::vector<float> tmp((size_t)W * (size_t)H);
    LsfTable tab;
    lsf_table_set(tab, lsf_x, taps_x, lsf_y, taps_y);
    for (uint32_t p = 0; p < num_planes; ++p) {
        const size_t plane = (size_t)p * (size_t)W * (size_t)H;
        const float* in = image + plane;
        for (int64_t y = 0; y < H; ++y)
            for (int64_t x0 = 0; x0 < W; x0 += kLsfChunk) {
                double acc[kLsfChunk];
                lsf_chunk(tab.hx, taps_x, [&](uint32_t i) {
                    const int64_t x = std::min(std::max(x0 + (int64_t)i - rx, (int64_t)0), W - 1);
                    return in[(size_t)y * (size_t)W + (size_t)x];
                }, acc);
                for (int64_t r = 0; r < (int64_t)kLsfChunk && x0 + r < W; ++r)
                    tmp[(size_t)y * (size_t)W + (size_t)(x0 + r)] = (float)acc[r];
            }
        for (int64_t y0 = 0; y0 < H; y0 += kLsfChunk)
            for (int64_t x = 0; x < W; ++x) {
                double acc[kLsfChunk];
                lsf_chunk(tab.hy, taps_y, [&](uint32_t i) {
                    const int64_t y = std::min(std::max(y0 + (int64_t)i - ry, (int64_t)0), H - 1);
                    return tmp[(size_t)y * (size_t)W + (size_t)x];
                }, acc);
                for (int64_t r = 0; r < (int64_t)kLsfChunk && y0 + r < H; ++r) {
                    const size_t o = plane + (size_t)(y0 + r) * (size_t)W + (size_t)x;
                    const float f = (float)acc[r];
                    if (out) out[o] = f;
                    if (out_u8) out_u8[o] = lsf_host_u8(f);
                }
            }
    }
    return XRT_OK;
}
