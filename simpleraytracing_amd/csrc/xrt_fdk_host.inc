// xrt_fdk_host.inc -- the host pieces of FDK reconstruction (DESIGN 10.11;
// include/xrt.h: the argument checks of xrt_fdk_filter[_device] and
// xrt_backproject[_device], xrt_ramp_filter, xrt_fdk_weights, xrt_fdk_scale and
// xrt_backprojection_matrix; include/xrt_debug.h: xrt_host_fdk_filter and
// xrt_host_backproject), included by xrt_abi.hip inside its extern "C" block.
// Self-contained over kernels/xrt_device.h's backproject_* functions, <cmath>,
// <cstdint> and <vector>, so that a stand-alone program can compile it under a
// host sanitizer (tools/fdk_san.cpp).

static bool fdk_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every check of xrt_fdk_filter[_device] that needs no context: what is wrong,
// or NULL.  host_taps: the taps can be read here (the device form's cannot).
static const char* fdk_filter_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                                        const float* weight, const float* taps, uint32_t num_taps, const float* out,
                                        bool host_taps)
{
    if (!image) return "the image is NULL";
    if (!taps) return "the taps are NULL";
    if (!out) return "out is NULL";
    if (num_taps == 0 || num_taps > 2u * XRT_MAX_RAMP_WIDTH - 1u) return "the tap count is outside 1..2*XRT_MAX_RAMP_WIDTH-1";
    if (num_taps % 2u == 0u) return "the tap count is even";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (width > XRT_MAX_RAMP_WIDTH) return "width is above XRT_MAX_RAMP_WIDTH";
    // (k_fdk_filter: one workgroup per row segment, the grid's x extent)
    if ((uint64_t)height * num_planes * 2u > 0x7FFFFFFFull) return "more than 2^30 rows";
    if (host_taps)
        for (uint32_t k = 0; k < num_taps; ++k)
            if (!std::isfinite(taps[k])) return "a tap is not finite";
    const uint64_t plane = (uint64_t)width * height * sizeof(float), n = plane * num_planes;
    if (fdk_overlap(out, n, image, n) || (weight && fdk_overlap(out, n, weight, plane)) ||
        fdk_overlap(out, n, taps, (uint64_t)num_taps * sizeof(float)))
        return "out overlaps an input (the filter is not computed in place)";
    return nullptr;
}

// Every check of xrt_backproject[_device] that needs no context: what is
// wrong, or NULL.  host_matrices: the matrices can be read here.
static const char* backproject_arguments(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                                         const double* matrices, const uint32_t* dims, uint32_t slab_begin,
                                         uint32_t slab_end, double scale, const float* volume, bool host_matrices)
{
    if (!proj) return "the projections are NULL";
    if (!matrices) return "the matrices are NULL";
    if (!dims) return "dims is NULL";
    if (!volume) return "the volume is NULL";
    if (width == 0 || height == 0 || num_planes == 0) return "width, height or num_planes is 0";
    if (width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return "width or height is above 2^31 - 1";
    if (num_planes > 65535u) return "more than 65535 planes";
    // (the byte counts below stay within 64 bits)
    if ((uint64_t)width * height > (1ull << 40)) return "a plane of more than 2^40 pixels";
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1u || dims[a] > XRT_KERNEL_NS::kMaxVolumeDim) return "a dimension of the volume is not 1 to 2048";
    if (slab_begin > slab_end || slab_end > dims[2]) return "the slab range is outside the volume";
    if (!std::isfinite(scale)) return "scale is not finite";
    if (host_matrices)
        for (uint64_t i = 0; i < (uint64_t)num_planes * 12u; ++i)
            if (!std::isfinite(matrices[i])) return "a matrix entry is not finite";
    const uint64_t vol_bytes = (uint64_t)(slab_end - slab_begin) * dims[1] * dims[0] * sizeof(float);
    if (vol_bytes && (fdk_overlap(volume, vol_bytes, proj, (uint64_t)width * height * num_planes * sizeof(float)) ||
                      fdk_overlap(volume, vol_bytes, matrices, (uint64_t)num_planes * 12u * sizeof(double))))
        return "the volume overlaps an input";
    return nullptr;
}

// g[n] of the band-limited ramp at unit sample distance (Ram-Lak).
static double fdk_ramlak(int64_t n)
{
    const double pi = 3.14159265358979323846;
    if (n == 0) return 0.25;
    if (n % 2 == 0) return 0.0;
    const double dn = (double)n;
    return -1.0 / ((pi * pi) * (dn * dn));
}

int xrt_ramp_filter(uint32_t num_taps, int window, float* taps)
{
    if (!taps || num_taps == 0 || num_taps % 2u == 0u || num_taps > 2u * XRT_MAX_RAMP_WIDTH - 1u) return XRT_ERR_ARGUMENT;
    if (window != XRT_RAMP_RAMLAK && window != XRT_RAMP_HANN) return XRT_ERR_ARGUMENT;
    const int64_t r = (int64_t)((num_taps - 1u) / 2u);
    for (int64_t k = 0; k < (int64_t)num_taps; ++k) {
        const int64_t n = k - r;
        const double g = window == XRT_RAMP_RAMLAK
                             ? fdk_ramlak(n)
                             : (0.25 * fdk_ramlak(n - 1) + 0.5 * fdk_ramlak(n)) + 0.25 * fdk_ramlak(n + 1);
        taps[k] = (float)g;
    }
    return XRT_OK;
}

static double fdk_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static bool fdk_camera_ok(const xrt_camera* cam)
{
    if (!cam || cam->width == 0 || cam->height == 0 || !std::isfinite(cam->pixel_spacing)) return false;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cam->origin[a]) || !std::isfinite(cam->detector[a]) || !std::isfinite(cam->up[a]) ||
            !std::isfinite(cam->right[a]))
            return false;
    return true;
}

// The offset of pixel i of n along a detector axis, the render's formula (pixel_offset) kept in f64.
static double fdk_pixel_offset(double spacing, uint32_t i, uint32_t n) { return spacing * ((0.5 + (double)i) - (double)n / 2.0); }

int xrt_fdk_weights(const xrt_camera* cam, float* weight)
{
    if (!fdk_camera_ok(cam) || !weight) return XRT_ERR_ARGUMENT;
    double ax[3], up[3], right[3];
    for (int a = 0; a < 3; ++a) {
        ax[a] = (double)cam->detector[a] - (double)cam->origin[a];
        up[a] = (double)cam->up[a];
        right[a] = (double)cam->right[a];
    }
    const double len_ax = std::sqrt(fdk_dot(ax, ax));
    if (!(len_ax > 0.0)) return XRT_ERR_ARGUMENT;
    for (uint32_t y = 0; y < cam->height; ++y) {
        const double v = fdk_pixel_offset((double)cam->pixel_spacing, y, cam->height);
        for (uint32_t x = 0; x < cam->width; ++x) {
            const double u = fdk_pixel_offset((double)cam->pixel_spacing, x, cam->width);
            double d[3];
            for (int a = 0; a < 3; ++a) d[a] = (ax[a] + up[a] * v) + right[a] * u;
            weight[(size_t)y * cam->width + x] = (float)(fdk_dot(d, ax) / (std::sqrt(fdk_dot(d, d)) * len_ax));
        }
    }
    return XRT_OK;
}

int xrt_fdk_scale(const xrt_camera* cam, const float axis_point[3], uint32_t num_projections, double* scale)
{
    if (!fdk_camera_ok(cam) || !axis_point || !scale || num_projections == 0) return XRT_ERR_ARGUMENT;
    const double pi = 3.14159265358979323846;
    double ax[3], right[3], q[3];
    for (int a = 0; a < 3; ++a) {
        ax[a] = (double)cam->detector[a] - (double)cam->origin[a];
        right[a] = (double)cam->right[a];
        q[a] = (double)axis_point[a] - (double)cam->origin[a];
    }
    const double sdd = std::sqrt(fdk_dot(ax, ax));
    const double sod = fdk_dot(q, ax) / sdd;
    const double s = ((pi / (double)num_projections) * (sod / sdd)) / ((double)cam->pixel_spacing * std::sqrt(fdk_dot(right, right)));
    if (!std::isfinite(s)) return XRT_ERR_ARGUMENT;
    *scale = s;
    return XRT_OK;
}

int xrt_backprojection_matrix(const xrt_camera* cam, const float pose[12], const float origin[3], const float spacing[3],
                              double A[12])
{
    if (!fdk_camera_ok(cam) || !origin || !spacing || !A) return XRT_ERR_ARGUMENT;
    // M = [right | up | detector - origin], N = its inverse by cofactors
    double M[3][3];
    for (int a = 0; a < 3; ++a) {
        M[a][0] = (double)cam->right[a];
        M[a][1] = (double)cam->up[a];
        M[a][2] = (double)cam->detector[a] - (double)cam->origin[a];
    }
    double C[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];
        }
    const double det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2];
    if (!std::isfinite(det) || det == 0.0) return XRT_ERR_ARGUMENT;
    double N[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) N[i][j] = C[j][i] / det;
    // the voxel index -> the world: Xw = G idx + h, G = R diag(spacing), h = R (origin + spacing / 2) + t
    double G[3][3], h[3];
    for (int i = 0; i < 3; ++i) {
        double acc = pose ? (double)pose[4 * i + 3] : 0.0;
        for (int j = 0; j < 3; ++j) {
            const double Rij = pose ? (double)pose[4 * i + j] : (i == j ? 1.0 : 0.0);
            G[i][j] = Rij * (double)spacing[j];
            acc += Rij * ((double)origin[j] + 0.5 * (double)spacing[j]);
        }
        h[i] = acc - (double)cam->origin[i];
    }
    double Q[3][4];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Q[i][j] = (N[i][0] * G[0][j] + N[i][1] * G[1][j]) + N[i][2] * G[2][j];
        Q[i][3] = (N[i][0] * h[0] + N[i][1] * h[1]) + N[i][2] * h[2];
    }
    const double ps = (double)cam->pixel_spacing;
    const double cx = (double)cam->width / 2.0 - 0.5, cy = (double)cam->height / 2.0 - 0.5;
    double R[12];
    for (int j = 0; j < 4; ++j) {
        R[j] = Q[0][j] / ps + cx * Q[2][j];
        R[4 + j] = Q[1][j] / ps + cy * Q[2][j];
        R[8 + j] = Q[2][j];
    }
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(R[e])) return XRT_ERR_ARGUMENT;
    for (int e = 0; e < 12; ++e) A[e] = R[e];
    return XRT_OK;
}

// The filter's contract over whole planes on the host, as written in
// include/xrt.h (test infrastructure: what k_fdk_filter is compared with on a
// machine without a device, not a fallback).
int xrt_host_fdk_filter(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, const float* weight,
                        const float* taps, uint32_t num_taps, float* out)
{
    if (fdk_filter_arguments(width, height, num_planes, image, weight, taps, num_taps, out, true)) return XRT_ERR_ARGUMENT;
    const int64_t W = width, r = (num_taps - 1u) / 2u;
    std::vector<float> pw((size_t)W);
    for (uint64_t row = 0; row < (uint64_t)height * num_planes; ++row) {
        const float* src = image + row * (uint64_t)W;
        const float* wrow = weight ? weight + (row % height) * (uint64_t)W : nullptr;
        for (int64_t x = 0; x < W; ++x) pw[(size_t)x] = wrow ? src[x] * wrow[x] : src[x];
        for (int64_t x = 0; x < W; ++x) {
            double s = 0.0;
            for (int64_t k = 0; k < (int64_t)num_taps; ++k) {
                const int64_t i = x + k - r;
                if (i >= 0 && i < W) s = s + (double)taps[k] * (double)pw[(size_t)i];
            }
            out[row * (uint64_t)W + (uint64_t)x] = (float)s;
        }
    }
    return XRT_OK;
}

// The kernel's arithmetic over a whole slab range on the host (test
// infrastructure, as above).
int xrt_host_backproject(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                         const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end, double scale, int accumulate,
                         float* volume)
{
    using namespace XRT_KERNEL_NS;
    if (backproject_arguments(width, height, num_planes, proj, matrices, dims, slab_begin, slab_end, scale, volume, true))
        return XRT_ERR_ARGUMENT;
    const uint32_t nx = dims[0], ny = dims[1];
    const size_t plane = (size_t)width * height;
    for (uint32_t k = slab_begin; k < slab_end; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i) {
                double acc = 0.0;
                for (uint32_t p = 0; p < num_planes; ++p) {
                    const double* A = matrices + (size_t)p * 12u;
                    backproject_term(proj + (size_t)p * plane, width, height,
                                     A[0] * (double)i + backproject_bracket(A, (double)j, (double)k),
                                     A[4] * (double)i + backproject_bracket(A + 4, (double)j, (double)k),
                                     A[8] * (double)i + backproject_bracket(A + 8, (double)j, (double)k), acc);
                }
                float& o = volume[((size_t)(k - slab_begin) * ny + j) * nx + i];
                o = backproject_output(acc, scale, accumulate != 0, accumulate ? o : 0.0f);
            }
    return XRT_OK;
}
