// xrt_area_host.inc -- the host pieces of the area sampling (include/xrt.h: the
// argument checks of xrt_area_integrate[_device], xrt_camera_supersample,
// xrt_focal_spot; include/xrt_debug.h: xrt_host_area_integrate), included by
// xrt_abi.hip inside its extern "C" block.  Self-contained over
// kernels/xrt_device.h's area_pixel, area_weights_set, area_plan and lut_u8,
// <cmath> and <cstdint>, so that a stand-alone program can compile it under a
// host sanitizer (tools/area_san.cpp).

static bool area_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every check of xrt_area_integrate[_device], none of which needs a context:
// what is wrong, or NULL.  `weight` is host memory in both forms.
static const char* area_arguments(uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y, uint32_t num_sources,
                                  uint32_t num_planes, const float* weight, const float* image, const float* out,
                                  const uint8_t* out_u8)
{
    if (!image) return "the image is NULL";
    if (!weight) return "weight is NULL";
    if (!out && !out_u8) return "out and out_u8 are both NULL";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (bin_x == 0 || bin_x > XRT_MAX_BIN || bin_y == 0 || bin_y > XRT_MAX_BIN) return "bin_x or bin_y is outside 1..XRT_MAX_BIN";
    if (num_sources == 0 || num_sources > XRT_MAX_SOURCES) return "num_sources is outside 1..XRT_MAX_SOURCES";
    double sum = 0.0;
    for (uint32_t s = 0; s < num_sources; ++s) {
        if (!std::isfinite(weight[s]) || weight[s] < 0.0f) return "a weight is NaN, infinite or negative";
        sum = sum + (double)weight[s];
    }
    if (!(sum > 0.0)) return "the weight sum is 0";
    // (k_area_integrate: 32-bit signed input coordinates, a 32-bit output row number, one launch's workgroups)
    const uint64_t Wb = (uint64_t)width * bin_x, Hb = (uint64_t)height * bin_y;
    if (Wb > 0x7FFFFFFFull || Hb > 0x7FFFFFFFull) return "width * bin_x or height * bin_y is above 2^31 - 1";
    const uint64_t rows = (uint64_t)num_planes * height;
    if (rows > 0xFFFFFFFFull) return "num_planes * height is above 2^32 - 1";
    if (XRT_KERNEL_NS::area_plan(width, rows, bin_x, bin_y, num_sources, height).blocks > 0x7FFFFFFFull)
        return "the planes need more than 2^31 - 1 workgroups: split the call";
    // (a workgroup holds at most 256 units of at most 4 outputs, so rows * width <= 2^41 here, and the input, at most
    // 64 * 64 samples an output, stays below 2^55 bytes: no product below wraps)
    const uint64_t n = rows * width, in_bytes = n * bin_x * bin_y * num_sources * sizeof(float);
    if ((out && area_overlap(image, in_bytes, out, n * sizeof(float))) || (out_u8 && area_overlap(image, in_bytes, out_u8, n)))
        return "an output overlaps the image (the integration is not computed in place)";
    return nullptr;
}

int xrt_camera_supersample(const xrt_camera* cam, uint32_t bin, xrt_camera* out)
{
    if (!cam || !out || bin == 0 || bin > XRT_MAX_BIN) return XRT_ERR_ARGUMENT;
    if ((uint64_t)cam->width * bin > 0x7FFFFFFFull || (uint64_t)cam->height * bin > 0x7FFFFFFFull) return XRT_ERR_ARGUMENT;
    const xrt_camera c = *cam;                          // (out may be cam)
    *out = c;
    out->width = c.width * bin;
    out->height = c.height * bin;
    out->pixel_spacing = c.pixel_spacing / (float)bin;
    return XRT_OK;
}

int xrt_focal_spot(const xrt_camera* cam, float size_u, float size_v, uint32_t nu, uint32_t nv, xrt_camera* cams,
                   float* weight)
{
    if (!cam || !cams || !weight) return XRT_ERR_ARGUMENT;
    if (!std::isfinite(size_u) || !std::isfinite(size_v) || size_u < 0.0f || size_v < 0.0f) return XRT_ERR_ARGUMENT;
    if (nu == 0 || nv == 0 || (uint64_t)nu * nv > XRT_MAX_SOURCES) return XRT_ERR_ARGUMENT;
    const xrt_camera c = *cam;
    for (uint32_t j = 0; j < nv; ++j)
        for (uint32_t i = 0; i < nu; ++i) {
            const float a = (float)((double)size_u * (((double)i + 0.5) / (double)nu - 0.5));
            const float b = (float)((double)size_v * (((double)j + 0.5) / (double)nv - 0.5));
            xrt_camera& o = cams[j * nu + i];
            o = c;
            for (int k = 0; k < 3; ++k) {
                const float ra = c.right[k] * a, ub = c.up[k] * b;
                const float t = c.origin[k] + ra;
                o.origin[k] = t + ub;
            }
            weight[j * nu + i] = 1.0f;
        }
    return XRT_OK;
}

// lut_u8 on the host (as xrt_lsf_host.inc's): the same values, without the
// discarded conversion of an out-of-window product to an unsigned integer.
static uint8_t area_host_u8(float v)
{
    return v >= 0.0f && v <= 80.0f ? XRT_KERNEL_NS::lut_u8(v) : v > 80.0f ? (uint8_t)255u : (uint8_t)0u;
}

// The kernel's pixel function over whole buffers on the host (test
// infrastructure: what k_area_integrate is compared with on a machine without
// a device, not a fallback).
int xrt_host_area_integrate(uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y, uint32_t num_sources,
                            uint32_t num_planes, const float* weight, const float* image, float* out, uint8_t* out_u8)
{
    if (area_arguments(width, height, bin_x, bin_y, num_sources, num_planes, weight, image, out, out_u8))
        return XRT_ERR_ARGUMENT;
    XRT_KERNEL_NS::AreaWeights tab;
    XRT_KERNEL_NS::area_weights_set(tab, weight, num_sources, bin_x, bin_y);
    const size_t W = width, H = height, Wb = W * bin_x, plane = Wb * (H * bin_y);
    for (size_t p = 0; p < num_planes; ++p)
        for (size_t y = 0; y < H; ++y)
            for (size_t x = 0; x < W; ++x) {
                const float* at = image + p * num_sources * plane + y * bin_y * Wb + x * bin_x;
                const float f = XRT_KERNEL_NS::area_pixel(tab, num_sources, bin_x, bin_y,
                                                          [&](uint32_t s, uint32_t dy, uint32_t dx) {
                                                              return at[s * plane + dy * Wb + dx];
                                                          });
                const size_t o = (p * H + y) * W + x;
                if (out) out[o] = f;
                if (out_u8) out_u8[o] = area_host_u8(f);
            }
    return XRT_OK;
}
