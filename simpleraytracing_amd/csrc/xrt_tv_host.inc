// xrt_tv_host.inc -- the host pieces of TV-regularised SIRT (DESIGN 10.13;
// include/xrt.h: the argument checks of xrt_tv_gradient[_device],
// xrt_volume_sumsq[_device], xrt_tv_descend[_device] and xrt_sirt_tv[_device];
// include/xrt_debug.h: xrt_host_tv_gradient, xrt_host_volume_sumsq,
// xrt_host_tv_descend and xrt_host_sirt_tv), included by xrt_abi.hip inside
// its extern "C" block behind xrt_sirt_host.inc, whose checks, plan and
// restatements it uses.  Self-contained over kernels/xrt_device.h's tv_* and
// sumsq_*, <cmath>, <cstdint> and <vector>, so that a stand-alone program can
// compile it under a host sanitizer (tools/tv_san.cpp).

static const char* tv_grid_arguments(const uint32_t* dims)
{
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1u || dims[a] > XRT_KERNEL_NS::kMaxVolumeDim) return "a dimension of the volume is not 1 to 2048";
    return nullptr;
}

// Every check of xrt_tv_gradient[_device]: what is wrong, or NULL.
static const char* tv_gradient_arguments(const float* volume, const uint32_t* dims, double eps, const float* out)
{
    if (!volume) return "the volume is NULL";
    if (!dims) return "dims is NULL";
    if (!out) return "out is NULL";
    if (const char* why = tv_grid_arguments(dims)) return why;
    if (!std::isfinite(eps) || !(eps > 0.0)) return "eps is not finite and > 0";
    const uint64_t bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(out, bytes, volume, bytes)) return "out overlaps the volume";
    return nullptr;
}

// Every check of xrt_volume_sumsq[_device] (b may be NULL): what is wrong, or NULL.
static const char* sumsq_arguments(uint64_t n, const float* a, const float* b, const double* out)
{
    if (!a) return "a is NULL";
    if (!out) return "out is NULL";
    if (n == 0) return "n is 0";
    if (n > (1ull << 33)) return "n is above 2^33 (2048^3 voxels)";
    if (fdk_overlap(out, sizeof(double), a, n * sizeof(float)) || (b && fdk_overlap(out, sizeof(double), b, n * sizeof(float))))
        return "out overlaps an input";
    return nullptr;
}

// Every check of xrt_tv_descend[_device]: what is wrong, or NULL.
static const char* tv_descend_arguments(const float* volume, const uint32_t* dims, double eps, double length, float lo, float hi)
{
    if (!volume) return "the volume is NULL";
    if (!dims) return "dims is NULL";
    if (const char* why = tv_grid_arguments(dims)) return why;
    if (!std::isfinite(eps) || !(eps > 0.0)) return "eps is not finite and > 0";
    if (!std::isfinite(length) || !(length >= 0.0)) return "length is not finite and >= 0";
    if (lo != lo || hi != hi) return "a bound is NaN";
    if (lo > hi) return "lo is above hi";
    return nullptr;
}

// The checks of xrt_sirt_tv[_device]'s TV parameters (tv NULL, or steps 0: nothing to check): what is wrong, or NULL.
static const char* tv_params_arguments(const xrt_tv_params* tv)
{
    if (!tv || tv->steps == 0u) return nullptr;
    if (!std::isfinite(tv->alpha) || !(tv->alpha >= 0.0)) return "tv: alpha is not finite and >= 0";
    if (!std::isfinite(tv->reduction) || !(tv->reduction > 0.0) || !(tv->reduction <= 1.0)) return "tv: reduction is not in (0, 1]";
    if (!std::isfinite(tv->eps) || !(tv->eps > 0.0)) return "tv: eps is not finite and > 0";
    return nullptr;
}

// The number of chunks of a level of m entries.
static uint64_t sumsq_chunks(uint64_t m) { return (m + XRT_KERNEL_NS::kSumsqChunk - 1u) / XRT_KERNEL_NS::kSumsqChunk; }

// The gradient's contract over a whole host volume with no device (test
// infrastructure: what k_tv_gradient is compared with, not a fallback): every
// voxel forms its own quotients and its three lower neighbours' again.
static void tv_host_gradient(const float* x, const uint32_t* dims, double eps, float* g)
{
    using namespace XRT_KERNEL_NS;
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2];
    for (uint32_t k = 0; k < nz; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i) {
                double qx, qy, qz, bx = 0.0, by = 0.0, bz = 0.0, u, w;
                tv_quotients_at(x, nx, ny, nz, i, j, k, eps, qx, qy, qz);
                if (i > 0u) tv_quotients_at(x, nx, ny, nz, i - 1u, j, k, eps, bx, u, w);
                if (j > 0u) tv_quotients_at(x, nx, ny, nz, i, j - 1u, k, eps, u, by, w);
                if (k > 0u) tv_quotients_at(x, nx, ny, nz, i, j, k - 1u, eps, u, w, bz);
                g[((uint64_t)k * ny + j) * nx + i] = tv_voxel(bx, by, bz, qx, qy, qz);
            }
}

// One level of the sum's order: `next` receives the partial of every chunk of the m entries, which are w's, or
// where w is NULL the first level's (sumsq_entry over a and b).
static void sumsq_host_level(uint64_t m, const float* a, const float* b, const double* w, std::vector<double>& next)
{
    using namespace XRT_KERNEL_NS;
    next.assign((size_t)sumsq_chunks(m), 0.0);
    for (uint64_t c = 0; c < next.size(); ++c) {
        double acc[kSumsqLanes];
        for (uint32_t l = 0; l < kSumsqLanes; ++l) acc[l] = 0.0;
        for (uint32_t r = 0; r < kSumsqRounds; ++r)
            for (uint32_t l = 0; l < kSumsqLanes; ++l) {
                const uint64_t i = c * kSumsqChunk + (uint64_t)r * kSumsqLanes + l;
                acc[l] = acc[l] + (i < m ? (w ? w[i] : sumsq_entry(a, b, i)) : 0.0);
            }
        for (uint32_t h = kSumsqLanes / 2u; h >= 1u; h >>= 1)
            for (uint32_t l = 0; l < h; ++l) acc[l] = acc[l] + acc[l + h];
        next[(size_t)c] = acc[0];
    }
}

// xrt_volume_sumsq's contract on the host (test infrastructure, as above).
static double sumsq_host(uint64_t n, const float* a, const float* b)
{
    if (n == 1u) return XRT_KERNEL_NS::sumsq_entry(a, b, 0u);
    std::vector<double> w, next;
    sumsq_host_level(n, a, b, nullptr, w);
    while (w.size() > 1u) {
        sumsq_host_level(w.size(), nullptr, nullptr, w.data(), next);
        w.swap(next);
    }
    return w[0];
}

// xrt_tv_descend's steps on the host (test infrastructure, as above); g: a volume's worth of floats.  The step's
// length is `scale`, or scale * sqrt(*moved) (the solver's).
static void tv_host_descend(float* x, const uint32_t* dims, double eps, uint32_t steps, double scale, const double* moved,
                            float lo, float hi, float* g)
{
    const uint64_t voxels = (uint64_t)dims[0] * dims[1] * dims[2];
    for (uint32_t s = 0; s < steps; ++s) {
        tv_host_gradient(x, dims, eps, g);
        const double G = sumsq_host(voxels, g, nullptr);
        const double gn = std::sqrt(G);
        if (!(gn > 0.0)) continue;
        const double c = XRT_KERNEL_NS::tv_step_length(scale, moved) / gn;
        for (uint64_t i = 0; i < voxels; ++i) x[i] = XRT_KERNEL_NS::tv_step_voxel(x[i], g[i], c, lo, hi);
    }
}

int xrt_host_tv_gradient(const float* volume, const uint32_t dims[3], double eps, float* out)
{
    if (tv_gradient_arguments(volume, dims, eps, out)) return XRT_ERR_ARGUMENT;
    tv_host_gradient(volume, dims, eps, out);
    return XRT_OK;
}

int xrt_host_volume_sumsq(uint64_t n, const float* a, const float* b, double* out)
{
    if (sumsq_arguments(n, a, b, out)) return XRT_ERR_ARGUMENT;
    *out = sumsq_host(n, a, b);
    return XRT_OK;
}

int xrt_host_tv_descend(float* volume, const uint32_t dims[3], double eps, uint32_t steps, double length, float lo, float hi)
{
    if (tv_descend_arguments(volume, dims, eps, length, lo, hi)) return XRT_ERR_ARGUMENT;
    std::vector<float> g((size_t)dims[0] * dims[1] * dims[2]);
    tv_host_descend(volume, dims, eps, steps, length, nullptr, lo, hi, g.data());
    return XRT_OK;
}

// xrt_sirt_tv's algorithm over the host restatements (test infrastructure, as above).
int xrt_host_sirt_tv(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                     const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets, double relax,
                     float lo, float hi, const xrt_tv_params* tv, float* volume)
{
    if (sirt_arguments(width, height, num_planes, proj, matrices, dims, spacing, iterations, subsets, relax, lo, hi, volume,
                       true) ||
        tv_params_arguments(tv))
        return XRT_ERR_ARGUMENT;
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return XRT_ERR_ARGUMENT;
    const bool with_tv = tv && tv->steps > 0u;
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<float> residual(plane * plan.widest, 1.0f), corr(voxels), norms(voxels * subsets), x0(with_tv ? voxels : 0u);
    for (uint32_t s = 0; s < subsets; ++s)
        if (xrt_host_backproject(width, height, plan.count[s], residual.data(), plan.A.data() + (size_t)plan.first[s] * 12u,
                                 dims, 0, dims[2], 1.0, 0, norms.data() + voxels * s) != XRT_OK)
            return XRT_ERR_ARGUMENT;
    double a_k = with_tv ? tv->alpha : 0.0;
    for (uint32_t k = 0; k < iterations; ++k) {
        if (with_tv) x0.assign(volume, volume + voxels);
        for (uint32_t s = 0; s < subsets; ++s) {
            sirt_host_forward(width, height, plan.count[s], volume, dims, spacing, plan.R.data() + (size_t)plan.first[s] * 12u,
                              XRT_FP_RESIDUAL, proj + plane * s, (uint64_t)plane * subsets, residual.data());
            if (xrt_host_backproject(width, height, plan.count[s], residual.data(),
                                     plan.A.data() + (size_t)plan.first[s] * 12u, dims, 0, dims[2], 1.0, 0,
                                     corr.data()) != XRT_OK)
                return XRT_ERR_ARGUMENT;
            for (size_t i = 0; i < voxels; ++i)
                volume[i] = XRT_KERNEL_NS::volume_update_voxel(volume[i], corr[i], norms[voxels * s + i], relax, lo, hi);
        }
        if (with_tv) {
            const double D = sumsq_host(voxels, volume, x0.data());
            tv_host_descend(volume, dims, tv->eps, tv->steps, a_k, &D, lo, hi, corr.data());   // (the correction is free)
            a_k = a_k * tv->reduction;
        }
    }
    return XRT_OK;
}
