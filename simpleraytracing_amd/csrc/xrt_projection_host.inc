// xrt_projection_host.inc -- the host pieces of the line-integral projections
// (include/xrt.h: the argument checks of xrt_log_projection[_device];
// include/xrt_debug.h: xrt_host_logf_batch, xrt_host_log_projection), included
// by xrt_abi.hip inside its extern "C" block.  Self-contained over
// kernels/xrt_device.h's xrt_logf, log_projection_pixel and
// log_projection_plan, <cmath> and <cstdint>, so that a stand-alone program can
// compile it under a host sanitizer (tools/projection_san.cpp).

static bool projection_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every check of xrt_log_projection[_device], none of which needs a context:
// what is wrong, or NULL.
static const char* projection_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                                        const float* flat, const float* dark, float flat_value, float t_min, int order,
                                        const float* out)
{
    if (!image) return "the image is NULL";
    if (!out) return "out is NULL";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (order != XRT_ORDER_PROJECTIONS && order != XRT_ORDER_SINOGRAMS)
        return "order is neither XRT_ORDER_PROJECTIONS nor XRT_ORDER_SINOGRAMS";
    if (!(t_min >= 0.0f) || std::isinf(t_min)) return "t_min is NaN, infinite or negative";
    if (!flat && (!std::isfinite(flat_value) || !(flat_value > 0.0f))) return "flat_value is not finite and > 0 (and flat is NULL)";
    // (k_log_projection: 32-bit pixel coordinates with room for a workgroup's span, a 32-bit row number, one launch's
    // workgroups)
    if (width > 0x7FFFF000u) return "width is above 2^31 - 4096";
    const uint64_t rows = (uint64_t)num_planes * height;
    if (rows > 0xFFFFFFFFull) return "num_planes * height is above 2^32 - 1";
    if (XRT_KERNEL_NS::log_projection_plan(width, rows).blocks > 0x7FFFFFFFull)
        return "the planes need more than 2^31 - 1 workgroups: split the call";
    const uint64_t plane = (uint64_t)width * height * sizeof(float), all = plane * num_planes;
    const bool in_place = out == image && order == XRT_ORDER_PROJECTIONS;
    if (!in_place && projection_overlap(out, all, image, all))
        return "out overlaps the image (in place is out == image in XRT_ORDER_PROJECTIONS only)";
    if ((flat && projection_overlap(out, all, flat, plane)) || (dark && projection_overlap(out, all, dark, plane)))
        return "out overlaps the flat or the dark plane";
    return nullptr;
}

void xrt_host_logf_batch(const float* in, float* outp, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) outp[i] = XRT_KERNEL_NS::xrt_logf(in[i]);
}

// The kernel's pixel function over whole buffers on the host (test
// infrastructure: what k_log_projection is compared with on a machine without
// a device, not a fallback).  In place, a pixel is read before it is written.
int xrt_host_log_projection(uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                            const float* flat, const float* dark, float flat_value, float t_min, int order, float* out)
{
    if (projection_arguments(width, height, num_planes, image, flat, dark, flat_value, t_min, order, out))
        return XRT_ERR_ARGUMENT;
    const size_t W = width, H = height, P = num_planes;
    for (size_t p = 0; p < P; ++p)
        for (size_t y = 0; y < H; ++y) {
            const float* src = image + (p * H + y) * W;
            float* dst = out + (order == XRT_ORDER_SINOGRAMS ? (y * P + p) * W : (p * H + y) * W);
            for (size_t x = 0; x < W; ++x)
                dst[x] = XRT_KERNEL_NS::log_projection_pixel(src[x], flat ? flat[y * W + x] : flat_value,
                                                             dark ? dark[y * W + x] : 0.0f, dark != nullptr, t_min);
        }
    return XRT_OK;
}
