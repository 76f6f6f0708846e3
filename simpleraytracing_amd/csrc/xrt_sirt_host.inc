// xrt_sirt_host.inc -- the host pieces of SIRT / OS-SART (DESIGN 10.12;
// include/xrt.h: the argument checks of xrt_forward_project[_device],
// xrt_volume_update[_device] and xrt_sirt[_device], xrt_ray_matrix and the
// solver's plan; include/xrt_debug.h: xrt_host_forward_project,
// xrt_host_volume_update and xrt_host_sirt), included by xrt_abi.hip inside
// its extern "C" block behind xrt_fdk_host.inc, whose fdk_overlap and
// xrt_host_backproject it uses.  Self-contained over kernels/xrt_device.h's
// forward_* and volume_update_voxel, <cmath>, <cstdint> and <vector>, so that
// a stand-alone program can compile it under a host sanitizer
// (tools/sirt_san.cpp).

// The limits that xrt_backproject sets a stack of planes; NULL when they hold.
static const char* sirt_plane_arguments(uint32_t width, uint32_t height, uint32_t num_planes)
{
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return "width or height is above 2^31 - 1";
    if (num_planes > 65535u) return "more than 65535 planes";
    if ((uint64_t)width * height > (1ull << 40)) return "a plane of more than 2^40 pixels";
    // (k_forward_project: one 64-lane workgroup per 8 x 8 tile along the grid's x extent, which holds fewer than
    // 2^32 work-items)
    if ((((uint64_t)width + 7u) / 8u) * (((uint64_t)height + 7u) / 8u) > 0x3FFFFFFull) return "a plane of more than 2^26 - 1 tiles";
    return nullptr;
}

static const char* sirt_grid_arguments(const uint32_t* dims, const float* spacing)
{
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1u || dims[a] > XRT_KERNEL_NS::kMaxVolumeDim) return "a dimension of the volume is not 1 to 2048";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0f)) return "a spacing is not finite and > 0";
    return nullptr;
}

// Every check of xrt_forward_project[_device] that needs no context: what is
// wrong, or NULL.  host_rays: the ray matrices can be read here.
static const char* forward_project_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                                             const uint32_t* dims, const float* spacing, const double* rays, int mode,
                                             const float* meas, const float* out, bool host_rays)
{
    if (!volume) return "the volume is NULL";
    if (!dims) return "dims is NULL";
    if (!spacing) return "spacing is NULL";
    if (!rays) return "the ray matrices are NULL";
    if (!out) return "out is NULL";
    if (const char* why = sirt_plane_arguments(width, height, num_planes)) return why;
    if (const char* why = sirt_grid_arguments(dims, spacing)) return why;
    if (mode != XRT_FP_PROJECT && mode != XRT_FP_RESIDUAL) return "the mode is not one of XRT_FP_*";
    if (mode == XRT_FP_RESIDUAL && !meas) return "the residual mode needs meas";
    if (host_rays)
        for (uint64_t i = 0; i < (uint64_t)num_planes * 12u; ++i)
            if (!std::isfinite(rays[i])) return "a ray matrix entry is not finite";
    const uint64_t n = (uint64_t)width * height * num_planes * sizeof(float);
    const uint64_t vol_bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(out, n, volume, vol_bytes) || fdk_overlap(out, n, rays, (uint64_t)num_planes * 12u * sizeof(double)) ||
        (meas && fdk_overlap(out, n, meas, n)))
        return "out overlaps an input";
    return nullptr;
}

// Every check of xrt_volume_update[_device]: what is wrong, or NULL.
static const char* volume_update_arguments(uint64_t n, const float* x, const float* corr, const float* norm, double relax,
                                           float lo, float hi)
{
    if (!x) return "x is NULL";
    if (!corr) return "corr is NULL";
    if (!norm) return "norm is NULL";
    if (n == 0) return "n is 0";
    if (n > (1ull << 33)) return "n is above 2^33 (2048^3 voxels)";
    if (!std::isfinite(relax)) return "relax is not finite";
    if (lo != lo || hi != hi) return "a bound is NaN";
    if (lo > hi) return "lo is above hi";
    if (fdk_overlap(x, n * sizeof(float), corr, n * sizeof(float)) || fdk_overlap(x, n * sizeof(float), norm, n * sizeof(float)))
        return "x overlaps corr or norm";
    return nullptr;
}

// Every check of xrt_sirt[_device] (the matrices are host memory in both
// forms): what is wrong, or NULL.  host_buffers: the volume can be compared
// with the matrices' addresses.
static const char* sirt_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                                  const double* matrices, const uint32_t* dims, const float* spacing, uint32_t iterations,
                                  uint32_t subsets, double relax, float lo, float hi, const float* volume, bool host_buffers)
{
    if (!proj) return "the projections are NULL";
    if (!matrices) return "the matrices are NULL";
    if (!dims) return "dims is NULL";
    if (!spacing) return "spacing is NULL";
    if (!volume) return "the volume is NULL";
    if (const char* why = sirt_plane_arguments(width, height, num_planes)) return why;
    if (const char* why = sirt_grid_arguments(dims, spacing)) return why;
    if (iterations == 0) return "iterations is 0";
    if (subsets == 0 || subsets > num_planes || subsets > XRT_MAX_SUBSETS) return "subsets is not 1 to min(num_planes, XRT_MAX_SUBSETS)";
    if (!std::isfinite(relax)) return "relax is not finite";
    if (lo != lo || hi != hi) return "a bound is NaN";
    if (lo > hi) return "lo is above hi";
    for (uint64_t i = 0; i < (uint64_t)num_planes * 12u; ++i)
        if (!std::isfinite(matrices[i])) return "a matrix entry is not finite";
    const uint64_t vol_bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    if (fdk_overlap(volume, vol_bytes, proj, (uint64_t)width * height * num_planes * sizeof(float)) ||
        (host_buffers && fdk_overlap(volume, vol_bytes, matrices, (uint64_t)num_planes * 12u * sizeof(double))))
        return "the volume overlaps an input";
    return nullptr;
}

int xrt_ray_matrix(const double A[12], double R[12])
{
    if (!A || !R) return XRT_ERR_ARGUMENT;
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(A[e])) return XRT_ERR_ARGUMENT;
    // M = A3, N = its inverse by cofactors (xrt_backprojection_matrix's order)
    double M[3][3], C[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = A[4 * i + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];
        }
    const double det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2];
    if (!std::isfinite(det) || det == 0.0) return XRT_ERR_ARGUMENT;
    double out[12];
    for (int i = 0; i < 3; ++i) {
        double N[3];
        for (int j = 0; j < 3; ++j) N[j] = C[j][i] / det;
        out[4 * i] = N[0];
        out[4 * i + 1] = N[1];
        out[4 * i + 2] = N[2];
        out[4 * i + 3] = -((N[0] * A[3] + N[1] * A[7]) + N[2] * A[11]);
    }
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(out[e])) return XRT_ERR_ARGUMENT;
    for (int e = 0; e < 12; ++e) R[e] = out[e];
    return XRT_OK;
}

// The solver's plan: the scan's planes subset-major -- subset s holds the
// planes p with p mod S == s, ascending -- with each plane's A and R.
struct SirtPlan {
    std::vector<uint32_t> first, count;       // per subset: where it starts in the order below, and its planes
    std::vector<uint32_t> plane;              // the scan's plane of each gathered slot
    std::vector<double> A, R;                 // [num_planes][12], gathered
    uint32_t widest = 0;                      // the largest subset's planes
};

// false: a matrix has no ray matrix (singular, or a result that is not finite).
static bool sirt_plan(uint32_t num_planes, uint32_t subsets, const double* matrices, SirtPlan& plan)
{
    plan.first.assign(subsets, 0u);
    plan.count.assign(subsets, 0u);
    plan.plane.clear();
    plan.A.resize((size_t)num_planes * 12u);
    plan.R.resize((size_t)num_planes * 12u);
    for (uint32_t s = 0; s < subsets; ++s) {
        plan.first[s] = (uint32_t)plan.plane.size();
        for (uint32_t p = s; p < num_planes; p += subsets) plan.plane.push_back(p);
        plan.count[s] = (uint32_t)plan.plane.size() - plan.first[s];
        plan.widest = plan.count[s] > plan.widest ? plan.count[s] : plan.widest;
    }
    for (uint32_t g = 0; g < num_planes; ++g) {
        const double* A = matrices + (size_t)plan.plane[g] * 12u;
        for (int e = 0; e < 12; ++e) plan.A[(size_t)g * 12u + e] = A[e];
        if (xrt_ray_matrix(A, plan.R.data() + (size_t)g * 12u) != XRT_OK) return false;
    }
    return true;
}

// The forward projector's contract over whole host buffers with no device
// (test infrastructure: what k_forward_project is compared with on a machine
// without a device, not a fallback).  meas_stride: floats between planes.
static void sirt_host_forward(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                              const uint32_t* dims, const float* spacing, const double* rays, int mode, const float* meas,
                              uint64_t meas_stride, float* out)
{
    using namespace XRT_KERNEL_NS;
    const uint64_t plane = (uint64_t)width * height;
    for (uint32_t p = 0; p < num_planes; ++p)
        for (uint32_t row = 0; row < height; ++row)
            for (uint32_t col = 0; col < width; ++col) {
                const uint64_t pix = (uint64_t)row * width + col;
                const float m = mode == XRT_FP_RESIDUAL ? meas[p * meas_stride + pix] : 0.0f;
                out[p * plane + pix] = forward_pixel(volume, dims[0], dims[1], dims[2], (double)spacing[0], (double)spacing[1],
                                                     (double)spacing[2], rays + (size_t)p * 12u, row, col, mode, m);
            }
}

int xrt_host_forward_project(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                             const uint32_t dims[3], const float spacing[3], const double* rays, int mode,
                             const float* meas, float* out)
{
    if (forward_project_arguments(width, height, num_planes, volume, dims, spacing, rays, mode, meas, out, true))
        return XRT_ERR_ARGUMENT;
    sirt_host_forward(width, height, num_planes, volume, dims, spacing, rays, mode, meas, (uint64_t)width * height, out);
    return XRT_OK;
}

int xrt_host_volume_update(uint64_t n, float* x, const float* corr, const float* norm, double relax, float lo, float hi)
{
    if (volume_update_arguments(n, x, corr, norm, relax, lo, hi)) return XRT_ERR_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i) x[i] = XRT_KERNEL_NS::volume_update_voxel(x[i], corr[i], norm[i], relax, lo, hi);
    return XRT_OK;
}

// xrt_sirt's algorithm over the host restatements (test infrastructure, as above).
int xrt_host_sirt(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                  const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets, double relax,
                  float lo, float hi, float* volume)
{
    if (sirt_arguments(width, height, num_planes, proj, matrices, dims, spacing, iterations, subsets, relax, lo, hi, volume,
                       true))
        return XRT_ERR_ARGUMENT;
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return XRT_ERR_ARGUMENT;
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<float> residual(plane * plan.widest, 1.0f), corr(voxels), norms(voxels * subsets);
    for (uint32_t s = 0; s < subsets; ++s)
        if (xrt_host_backproject(width, height, plan.count[s], residual.data(), plan.A.data() + (size_t)plan.first[s] * 12u,
                                 dims, 0, dims[2], 1.0, 0, norms.data() + voxels * s) != XRT_OK)
            return XRT_ERR_ARGUMENT;
    for (uint32_t k = 0; k < iterations; ++k)
        for (uint32_t s = 0; s < subsets; ++s) {
            // subset s's planes lie `subsets` planes apart in the scan, from plane s
            sirt_host_forward(width, height, plan.count[s], volume, dims, spacing, plan.R.data() + (size_t)plan.first[s] * 12u,
                              XRT_FP_RESIDUAL, proj + plane * s, (uint64_t)plane * subsets, residual.data());
            if (xrt_host_backproject(width, height, plan.count[s], residual.data(),
                                     plan.A.data() + (size_t)plan.first[s] * 12u, dims, 0, dims[2], 1.0, 0,
                                     corr.data()) != XRT_OK)
                return XRT_ERR_ARGUMENT;
            for (size_t i = 0; i < voxels; ++i)
                volume[i] = XRT_KERNEL_NS::volume_update_voxel(volume[i], corr[i], norms[voxels * s + i], relax, lo, hi);
        }
    return XRT_OK;
}
