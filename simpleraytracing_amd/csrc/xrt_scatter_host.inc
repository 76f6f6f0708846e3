// xrt_scatter_host.inc -- the host pieces of the scatter model (include/xrt.h:
// the argument checks of xrt_scatter_source[_device] and
// xrt_scatter_add[_device]; include/xrt_debug.h: xrt_host_scatter_source and
// xrt_host_scatter_add), included by xrt_abi.hip inside its extern "C" block
// after xrt_detector_host.inc, whose spectrum_arguments checks the table.
// Self-contained over kernels/xrt_device.h's scatter_pixel, scatter_lbuffer,
// scatter_axis, scatter_sample and lut_u8, <cmath> and <cstdint>, so that a
// stand-alone program can compile it under a host sanitizer
// (tools/scatter_san.cpp).

static_assert(XRT_MAX_SCATTER_BIN == XRT_KERNEL_NS::kMaxScatterBin &&
                  XRT_MAX_SCATTER_KERNELS == XRT_KERNEL_NS::kMaxScatterKernels,
              "the contract's bounds are the tables'");

static bool scatter_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// log2 of a binning factor, or -1 when it is no power of two in 1..XRT_MAX_SCATTER_BIN.
static int scatter_bin_log2(uint32_t bin)
{
    for (uint32_t k = 0; (1u << k) <= XRT_MAX_SCATTER_BIN; ++k)
        if (bin == (1u << k)) return (int)k;
    return -1;
}

// The sizes' checks both steps share (the kernels: 32-bit pixel coordinates; one workgroup per tile of 64 columns
// and `tile_rows` rows and per plane, the grid's y and z extents).
static const char* scatter_sizes(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin, uint32_t tile_rows)
{
    if (scatter_bin_log2(bin) < 0) return "bin is not a power of two in 1..XRT_MAX_SCATTER_BIN";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return "width or height is above 2^31 - 1";
    if (((uint64_t)height + tile_rows - 1u) / tile_rows > 65535u || num_planes > 65535u)
        return "more than 65535 tile rows or planes";
    return nullptr;
}

// Every check of xrt_scatter_source[_device], none of which needs a context:
// what is wrong, or NULL.  The tables are host memory in both forms.
static const char* scatter_source_arguments(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                                            const float* paths, const uint16_t* open, const float* weight, const float* mu,
                                            const float* sigma, uint32_t num_bins, uint32_t bin, const float* lbuffer,
                                            const float* source)
{
    if (!paths) return "paths is NULL";
    if (!sigma) return "sigma is NULL";
    if (!source) return "source is NULL";
    if (const char* why = spectrum_arguments(weight, mu, num_meshes, num_bins)) return why;
    for (uint32_t i = 0; i < num_meshes * num_bins; ++i)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0f) return "a sigma entry is NaN, infinite or negative";
    const int lg = scatter_bin_log2(bin);
    if (const char* why = scatter_sizes(width, height, num_planes, bin, lg < 0 ? 1u : XRT_KERNEL_NS::scatter_tile_rows((uint32_t)lg)))
        return why;
    // (width, height < 2^31 and num_planes < 2^16: n < 2^78 would wrap, so the product is formed in steps)
    const uint64_t plane = (uint64_t)width * height;
    if (plane > (1ull << 40)) return "a plane holds more than 2^40 pixels";
    const uint64_t n = plane * num_planes;
    const uint64_t wc = ((uint64_t)width + bin - 1u) / bin, hc = ((uint64_t)height + bin - 1u) / bin;
    const uint64_t paths_bytes = n * num_meshes * sizeof(float), open_bytes = n * sizeof(uint16_t);
    const uint64_t source_bytes = wc * hc * num_planes * sizeof(float), l_bytes = n * sizeof(float);
    if (scatter_overlap(source, source_bytes, paths, paths_bytes) || scatter_overlap(source, source_bytes, open, open_bytes) ||
        scatter_overlap(lbuffer, l_bytes, paths, paths_bytes) || scatter_overlap(lbuffer, l_bytes, open, open_bytes))
        return "an output overlaps paths or open";
    if (scatter_overlap(source, source_bytes, lbuffer, l_bytes)) return "source overlaps lbuffer";
    return nullptr;
}

// Every check of xrt_scatter_add[_device], none of which needs a context: what
// is wrong, or NULL.  `amp` is host memory in both forms.
static const char* scatter_add_arguments(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                                         const float* blurred, uint32_t num_kernels, const float* amp, const float* primary,
                                         const float* out, const float* out_scatter, const uint8_t* out_u8)
{
    if (!blurred) return "blurred is NULL";
    if (!amp) return "amp is NULL";
    if (!out && !out_scatter && !out_u8) return "out, out_scatter and out_u8 are all NULL";
    if (num_kernels == 0 || num_kernels > XRT_MAX_SCATTER_KERNELS) return "num_kernels is outside 1..XRT_MAX_SCATTER_KERNELS";
    for (uint32_t g = 0; g < num_kernels; ++g)
        if (!std::isfinite(amp[g]) || amp[g] < 0.0f) return "an amp is NaN, infinite or negative";
    if (const char* why = scatter_sizes(width, height, num_planes, bin, XRT_KERNEL_NS::kScatterTile)) return why;
    const uint64_t plane = (uint64_t)width * height;
    if (plane > (1ull << 40)) return "a plane holds more than 2^40 pixels";
    const uint64_t n = plane * num_planes;
    const uint64_t wc = ((uint64_t)width + bin - 1u) / bin, hc = ((uint64_t)height + bin - 1u) / bin;
    const uint64_t coarse_bytes = wc * hc * num_planes * num_kernels * sizeof(float), f_bytes = n * sizeof(float);
    const void* outs[3] = {out, out_scatter, out_u8};
    const uint64_t out_bytes[3] = {f_bytes, f_bytes, n};
    for (int k = 0; k < 3; ++k)
        if (scatter_overlap(outs[k], out_bytes[k], blurred, coarse_bytes) || scatter_overlap(outs[k], out_bytes[k], primary, f_bytes))
            return "an output overlaps blurred or primary (the sum is not formed in place)";
    return nullptr;
}

// lut_u8 on the host (as xrt_lsf_host.inc's): the same values, without the
// discarded conversion of an out-of-window product to an unsigned integer.
static uint8_t scatter_host_u8(float v)
{
    return v >= 0.0f && v <= 80.0f ? XRT_KERNEL_NS::lut_u8(v) : v > 80.0f ? (uint8_t)255u : (uint8_t)0u;
}

// The source kernel's arithmetic over whole planes on the host: scatter_pixel
// a pixel, a block's rows summed in column order, the rows in row order (test
// infrastructure: what k_scatter_source is compared with on a machine without
// a device, not a fallback).
int xrt_host_scatter_source(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes, const float* paths,
                            const uint16_t* open, const float* weight, const float* mu, const float* sigma,
                            uint32_t num_bins, uint32_t bin, float* lbuffer, float* source)
{
    using namespace XRT_KERNEL_NS;
    if (scatter_source_arguments(width, height, num_planes, num_meshes, paths, open, weight, mu, sigma, num_bins, bin, lbuffer,
                                 source))
        return XRT_ERR_ARGUMENT;
    const size_t W = width, H = height, D = bin, Wc = (W + D - 1) / D, Hc = (H + D - 1) / D;
    const size_t N = W * H * num_planes;
    const uint32_t K = num_bins;
    for (size_t p = 0; p < num_planes; ++p)
        for (size_t yc = 0; yc < Hc; ++yc)
            for (size_t xc = 0; xc < Wc; ++xc) {
                const size_t rows = std::min(D, H - yc * D), cols = std::min(D, W - xc * D);
                double acc = -0.0;
                for (size_t y = yc * D; y < yc * D + rows; ++y) {
                    double r = -0.0;
                    for (size_t x = xc * D; x < xc * D + cols; ++x) {
                        const size_t i = (p * H + y) * W + x;
                        double E, Q;
                        scatter_pixel(
                            num_meshes, K, [&](uint32_t j) { return (double)paths[j * N + i] * 0.1; },
                            [&](uint32_t j, uint32_t e) { return mu[j * K + e]; },
                            [&](uint32_t j, uint32_t e) { return sigma[j * K + e]; }, [&](uint32_t e) { return weight[e]; }, E, Q);
                        const bool flagged = open && open[i] != 0;
                        if (lbuffer) lbuffer[i] = flagged ? -1.0f : scatter_lbuffer(E);
                        r = r + (flagged ? 0.0 : Q);
                    }
                    acc = acc + r;
                }
                source[(p * Hc + yc) * Wc + xc] = (float)(acc / (double)(rows * cols));
            }
    return XRT_OK;
}

// The add kernel's pixel function over whole planes on the host (test
// infrastructure, as above).
int xrt_host_scatter_add(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin, const float* blurred,
                         uint32_t num_kernels, const float* amp, const float* primary, float* out, float* out_scatter,
                         uint8_t* out_u8)
{
    using namespace XRT_KERNEL_NS;
    if (scatter_add_arguments(width, height, num_planes, bin, blurred, num_kernels, amp, primary, out, out_scatter, out_u8))
        return XRT_ERR_ARGUMENT;
    const uint32_t lg = (uint32_t)scatter_bin_log2(bin);
    const uint32_t wc = (width + bin - 1u) / bin, hc = (height + bin - 1u) / bin;
    const size_t W = width, H = height, P = num_planes, coarse_plane = (size_t)wc * hc;
    for (size_t p = 0; p < P; ++p)
        for (uint32_t y = 0; y < height; ++y) {
            const ScatterAxis ay = scatter_axis(y, lg, hc);
            for (uint32_t x = 0; x < width; ++x) {
                const ScatterAxis ax = scatter_axis(x, lg, wc);
                const double S = scatter_sample(
                    ax, ay, num_kernels, [&](uint32_t g) { return amp[g]; },
                    [&](uint32_t g, uint32_t yi, uint32_t xi) { return blurred[(g * P + p) * coarse_plane + (size_t)yi * wc + xi]; });
                const size_t i = (p * H + y) * W + x;
                const float total = primary ? (float)((double)primary[i] + S) : (float)S;
                if (out_scatter) out_scatter[i] = (float)S;
                if (out) out[i] = total;
                if (out_u8) out_u8[i] = scatter_host_u8(total);
            }
        }
    return XRT_OK;
}
