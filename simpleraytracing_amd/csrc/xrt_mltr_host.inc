// xrt_mltr_host.inc -- the host pieces of OS-MLTR (DESIGN 10.17;
// include/xrt.h: the argument checks of xrt_poisson_project[_device],
// xrt_backproject_update[_device] and xrt_mltr[_device]; include/xrt_debug.h:
// xrt_host_poisson_project, xrt_host_backproject_update and xrt_host_mltr),
// included by xrt_abi.hip inside its extern "C" block behind
// xrt_tv_host.inc, whose checks, plan and descent it uses.  Self-contained
// over kernels/xrt_device.h's poisson_pixel, backproject_pair_term and
// volume_update_voxel, <cmath>, <cstdint> and <vector>, so that a
// stand-alone program can compile it under a host sanitizer.

static bool mltr_misaligned(const void* pairs) { return (reinterpret_cast<uintptr_t>(pairs) & 7u) != 0u; }

// Every check of xrt_poisson_project[_device] that needs no context: what is
// wrong, or NULL.  host_rays: the ray matrices can be read here.
static const char* poisson_project_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                                             const uint32_t* dims, const float* spacing, const double* rays,
                                             const float* counts, const float* flat, const float* background,
                                             const float* pairs, bool host_rays)
{
    if (!volume) return "the volume is NULL";
    if (!dims) return "dims is NULL";
    if (!spacing) return "spacing is NULL";
    if (!rays) return "the ray matrices are NULL";
    if (!counts) return "the counts are NULL";
    if (!flat) return "the flat field is NULL";
    if (!pairs) return "pairs is NULL";
    if (mltr_misaligned(pairs)) return "pairs is not aligned to 8 bytes";
    if (const char* why = sirt_plane_arguments(width, height, num_planes)) return why;
    if (const char* why = sirt_grid_arguments(dims, spacing)) return why;
    if (host_rays)
        for (uint64_t i = 0; i < (uint64_t)num_planes * 12u; ++i)
            if (!std::isfinite(rays[i])) return "a ray matrix entry is not finite";
    const uint64_t plane = (uint64_t)width * height * sizeof(float), n = plane * num_planes;
    const uint64_t vol_bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(pairs, 2u * n, volume, vol_bytes) ||
        fdk_overlap(pairs, 2u * n, rays, (uint64_t)num_planes * 12u * sizeof(double)) || fdk_overlap(pairs, 2u * n, counts, n) ||
        fdk_overlap(pairs, 2u * n, flat, plane) || (background && fdk_overlap(pairs, 2u * n, background, n)))
        return "pairs overlaps an input";
    return nullptr;
}

// Every check of xrt_backproject_update[_device] that needs no context: what
// is wrong, or NULL.  host_matrices: the matrices can be read here.
static const char* backproject_update_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs,
                                                const double* matrices, const uint32_t* dims, double relax, float lo,
                                                float hi, const float* volume, bool host_matrices)
{
    if (!pairs) return "pairs is NULL";
    if (!matrices) return "the matrices are NULL";
    if (!dims) return "dims is NULL";
    if (!volume) return "the volume is NULL";
    if (mltr_misaligned(pairs)) return "pairs is not aligned to 8 bytes";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return "width or height is above 2^31 - 1";
    if (num_planes > 65535u) return "more than 65535 planes";
    if ((uint64_t)width * height > (1ull << 40)) return "a plane of more than 2^40 pixels";
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1u || dims[a] > XRT_KERNEL_NS::kMaxVolumeDim) return "a dimension of the volume is not 1 to 2048";
    if (!std::isfinite(relax)) return "relax is not finite";
    if (lo != lo || hi != hi) return "a bound is NaN";
    if (lo > hi) return "lo is above hi";
    if (host_matrices)
        for (uint64_t i = 0; i < (uint64_t)num_planes * 12u; ++i)
            if (!std::isfinite(matrices[i])) return "a matrix entry is not finite";
    const uint64_t vol_bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(volume, vol_bytes, pairs, (uint64_t)width * height * num_planes * 2u * sizeof(float)) ||
        fdk_overlap(volume, vol_bytes, matrices, (uint64_t)num_planes * 12u * sizeof(double)))
        return "the volume overlaps an input";
    return nullptr;
}

// Every check of xrt_mltr[_device] (the matrices are host memory in both
// forms): xrt_sirt's over the counts, and the flat field's and the
// background's.
static const char* mltr_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* counts,
                                  const float* flat, const float* background, const double* matrices, const uint32_t* dims,
                                  const float* spacing, uint32_t iterations, uint32_t subsets, double relax, float lo,
                                  float hi, const float* volume, bool host_buffers)
{
    if (!counts) return "the counts are NULL";
    if (!flat) return "the flat field is NULL";
    if (const char* why = sirt_arguments(width, height, num_planes, counts, matrices, dims, spacing, iterations, subsets, relax,
                                         lo, hi, volume, host_buffers))
        return why;
    const uint64_t plane = (uint64_t)width * height * sizeof(float);
    const uint64_t vol_bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(volume, vol_bytes, flat, plane) || (background && fdk_overlap(volume, vol_bytes, background, plane * num_planes)))
        return "the volume overlaps an input";
    return nullptr;
}

// The pixel stage's contract over whole host buffers with no device (test
// infrastructure: what k_poisson_project is compared with on a machine
// without a device, not a fallback).  stride: floats between the planes of
// the counts and of the background.
static void mltr_host_project(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume, const uint32_t* dims,
                              const float* spacing, const double* rays, const float* counts, const float* flat,
                              const float* background, uint64_t stride, float* pairs)
{
    using namespace XRT_KERNEL_NS;
    const uint64_t plane = (uint64_t)width * height;
    for (uint32_t p = 0; p < num_planes; ++p)
        for (uint32_t row = 0; row < height; ++row)
            for (uint32_t col = 0; col < width; ++col) {
                const uint64_t pix = (uint64_t)row * width + col;
                float* out = pairs + 2u * (p * plane + pix);
                poisson_pixel(volume, dims[0], dims[1], dims[2], (double)spacing[0], (double)spacing[1], (double)spacing[2],
                              rays + (size_t)p * 12u, row, col, counts[p * stride + pix], flat[pix], background != nullptr,
                              background ? background[p * stride + pix] : 0.0f, out[0], out[1]);
            }
}

// The fused backprojector's contract over whole host buffers (test infrastructure, as above).
static void mltr_host_update(uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs, const double* matrices,
                             const uint32_t* dims, double relax, float lo, float hi, float* volume)
{
    using namespace XRT_KERNEL_NS;
    const size_t plane = (size_t)width * height;
    const FloatPair* planes = reinterpret_cast<const FloatPair*>(pairs);
    for (uint32_t k = 0; k < dims[2]; ++k)
        for (uint32_t j = 0; j < dims[1]; ++j)
            for (uint32_t i = 0; i < dims[0]; ++i) {
                double accn = 0.0, accd = 0.0;
                for (uint32_t p = 0; p < num_planes; ++p) {
                    const double* A = matrices + (size_t)p * 12u;
                    const double dj = (double)j, dk = (double)k, di = (double)i;
                    backproject_pair_term(planes + (size_t)p * plane, width, height, A[0] * di + backproject_bracket(A, dj, dk),
                                          A[4] * di + backproject_bracket(A + 4, dj, dk),
                                          A[8] * di + backproject_bracket(A + 8, dj, dk), accn, accd);
                }
                float& x = volume[((size_t)k * dims[1] + j) * dims[0] + i];
                x = volume_update_voxel(x, (float)accn, (float)accd, relax, lo, hi);
            }
}

int xrt_host_poisson_project(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                             const uint32_t dims[3], const float spacing[3], const double* rays, const float* counts,
                             const float* flat, const float* background, float* pairs)
{
    if (poisson_project_arguments(width, height, num_planes, volume, dims, spacing, rays, counts, flat, background, pairs, true))
        return XRT_ERR_ARGUMENT;
    mltr_host_project(width, height, num_planes, volume, dims, spacing, rays, counts, flat, background,
                      (uint64_t)width * height, pairs);
    return XRT_OK;
}

int xrt_host_backproject_update(uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs,
                                const double* matrices, const uint32_t dims[3], double relax, float lo, float hi,
                                float* volume)
{
    if (backproject_update_arguments(width, height, num_planes, pairs, matrices, dims, relax, lo, hi, volume, true))
        return XRT_ERR_ARGUMENT;
    mltr_host_update(width, height, num_planes, pairs, matrices, dims, relax, lo, hi, volume);
    return XRT_OK;
}

// xrt_mltr's algorithm over the host restatements (test infrastructure, as above).
int xrt_host_mltr(uint32_t width, uint32_t height, uint32_t num_planes, const float* counts, const float* flat,
                  const float* background, const double* matrices, const uint32_t dims[3], const float spacing[3],
                  uint32_t iterations, uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv,
                  float* volume)
{
    if (mltr_arguments(width, height, num_planes, counts, flat, background, matrices, dims, spacing, iterations, subsets, relax,
                       lo, hi, volume, true) ||
        tv_params_arguments(tv))
        return XRT_ERR_ARGUMENT;
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return XRT_ERR_ARGUMENT;
    const bool with_tv = tv && tv->steps > 0u;
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<double> pairs(plane * plan.widest);          // (doubles: a pair each, aligned to 8 bytes)
    std::vector<float> x0(with_tv ? voxels : 0u), g(with_tv ? voxels : 0u);
    double a_k = with_tv ? tv->alpha : 0.0;
    for (uint32_t k = 0; k < iterations; ++k) {
        if (with_tv) x0.assign(volume, volume + voxels);
        for (uint32_t s = 0; s < subsets; ++s) {
            // subset s's planes lie `subsets` planes apart in the scan, from plane s
            mltr_host_project(width, height, plan.count[s], volume, dims, spacing, plan.R.data() + (size_t)plan.first[s] * 12u,
                              counts + plane * s, flat, background ? background + plane * s : nullptr,
                              (uint64_t)plane * subsets, reinterpret_cast<float*>(pairs.data()));
            mltr_host_update(width, height, plan.count[s], reinterpret_cast<const float*>(pairs.data()),
                             plan.A.data() + (size_t)plan.first[s] * 12u, dims, relax, lo, hi, volume);
        }
        if (with_tv) {
            const double D = sumsq_host(voxels, volume, x0.data());
            tv_host_descend(volume, dims, tv->eps, tv->steps, a_k, &D, lo, hi, g.data());
            a_k = a_k * tv->reduction;
        }
    }
    return XRT_OK;
}
