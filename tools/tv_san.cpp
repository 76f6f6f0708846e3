// tv_san.cpp -- TV-regularised SIRT's host code (the argument checks of
// xrt_tv_gradient, xrt_volume_sumsq, xrt_tv_descend and xrt_sirt_tv and the four
// host restatements: simpleraytracing_amd/csrc/xrt_tv_host.inc over
// xrt_sirt_host.inc and xrt_fdk_host.inc) over its edge cases, as a stand-alone
// program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/tv_san.cpp \
//         -o tv_san
//
// Exact-size heap buffers, so that a read one voxel past the volume or below
// it -- the stencil's neighbours on the border --, one entry past a chunk of
// the sum or a write past the gradient is seen.  Prints "tv_san: OK" and
// returns 0 when every call returned what it should (tests/test_tv_cpu.py runs
// it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_fdk_host.inc"
#include "xrt_sirt_host.inc"
#include "xrt_tv_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("tv_san: line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static uint32_t lcg(uint32_t& s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static std::vector<float> noise(size_t n, uint32_t seed, float lo, float hi)
{
    std::vector<float> v(n);
    for (float& x : v) x = lo + (hi - lo) * (float)(lcg(seed) % 2001u) / 2000.0f;
    return v;
}

// A source on -x at `sod`, the detector centre on +x at `sdd - sod`, turned by `theta` about z; up = z.
static xrt_camera camera(double theta, uint32_t W, uint32_t H, float pitch)
{
    const double sod = 100.0, sdd = 150.0, cs = std::cos(theta), sn = std::sin(theta);
    xrt_camera c;
    c.origin[0] = (float)(-sod * cs); c.origin[1] = (float)(-sod * sn); c.origin[2] = 0.0f;
    c.detector[0] = (float)((sdd - sod) * cs); c.detector[1] = (float)((sdd - sod) * sn); c.detector[2] = 0.0f;
    c.right[0] = (float)-sn; c.right[1] = (float)cs; c.right[2] = 0.0f;
    c.up[0] = 0.0f; c.up[1] = 0.0f; c.up[2] = 1.0f;
    c.pixel_spacing = pitch;
    c.width = W;
    c.height = H;
    return c;
}

static void check_gradient(uint32_t nx, uint32_t ny, uint32_t nz, double eps)
{
    const uint32_t dims[3] = {nx, ny, nz};
    const size_t voxels = (size_t)nx * ny * nz;
    const std::vector<float> vol = noise(voxels, nx + 3u * ny + 7u * nz, 0.0f, 2.0f);
    std::vector<float> g(voxels, -7.0f);
    EXPECT(xrt_host_tv_gradient(vol.data(), dims, eps, g.data()) == XRT_OK);
    double sum = 0.0;
    for (float v : g) {
        EXPECT(std::isfinite(v) && std::fabs(v) <= 6.0f);
        sum += (double)v;
    }
    EXPECT(std::fabs(sum) <= 1e-5 * (double)voxels);                      // every quotient once with each sign
    const std::vector<float> flat(voxels, 0.75f);
    EXPECT(xrt_host_tv_gradient(flat.data(), dims, eps, g.data()) == XRT_OK);
    for (float v : g) EXPECT(v == 0.0f && !std::signbit(v));
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the gradient: one voxel, lines along each axis, odd sizes, special voxels
    check_gradient(1, 1, 1, 1e-8);
    check_gradient(2, 1, 1, 1e-8);
    check_gradient(1, 1, 5, 1.0);
    check_gradient(1, 4, 1, 1e-300);
    check_gradient(5, 3, 2, 1e-8);
    check_gradient(67, 9, 3, 1e-2);
    check_gradient(33, 9, 34, 1e-8);
    {
        const uint32_t dims[3] = {5, 3, 2};
        std::vector<float> vol = noise(30, 1u, 0.0f, 2.0f), g(30, -7.0f);
        vol[3] = nan; vol[7] = inf; vol[11] = -inf; vol[13] = -0.0f;
        EXPECT(xrt_host_tv_gradient(vol.data(), dims, 1e-8, g.data()) == XRT_OK);
        EXPECT(std::isnan(g[3]) && std::isnan(g[2]) && g[29] != -7.0f);
        EXPECT(tv_gradient_arguments(vol.data(), dims, 1e-8, g.data()) == nullptr);
        EXPECT(tv_gradient_arguments(nullptr, dims, 1e-8, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), nullptr, 1e-8, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), dims, 1e-8, nullptr));
        EXPECT(tv_gradient_arguments(vol.data(), dims, 0.0, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), dims, -1.0, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), dims, (double)inf, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), dims, (double)nan, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), dims, 1e-8, vol.data() + 29));        // the last voxel
        const uint32_t big[3] = {5, 2049, 2}, none[3] = {0, 3, 2};
        EXPECT(tv_gradient_arguments(vol.data(), big, 1e-8, g.data()));
        EXPECT(tv_gradient_arguments(vol.data(), none, 1e-8, g.data()));
        EXPECT(xrt_host_tv_gradient(vol.data(), dims, 0.0, g.data()) == XRT_ERR_ARGUMENT);
    }

    // the sum of squares: about a lane row, a chunk and two levels, with and without b
    for (uint64_t n : {1ull, 255ull, 256ull, 257ull, 4095ull, 4096ull, 4097ull, 4096ull * 3u + 5u, 4096ull * 4096ull + 4097ull}) {
        const std::vector<float> a = noise((size_t)n, (uint32_t)n, -1.0f, 1.0f), b = noise((size_t)n, 5u, -1.0f, 1.0f);
        double s = -7.0, d = -7.0, plain = 0.0, diff = 0.0;
        EXPECT(xrt_host_volume_sumsq(n, a.data(), nullptr, &s) == XRT_OK);
        EXPECT(xrt_host_volume_sumsq(n, a.data(), b.data(), &d) == XRT_OK);
        for (uint64_t i = 0; i < n; ++i) {
            plain += (double)a[i] * (double)a[i];
            diff += ((double)a[i] - (double)b[i]) * ((double)a[i] - (double)b[i]);
        }
        EXPECT(std::fabs(s - plain) <= 1e-9 * plain && std::fabs(d - diff) <= 1e-9 * diff);
        EXPECT(xrt_host_volume_sumsq(0, a.data(), nullptr, &s) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_sumsq(n, nullptr, nullptr, &s) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_sumsq(n, a.data(), nullptr, nullptr) == XRT_ERR_ARGUMENT);
    }
    {
        std::vector<double> both(4, 0.0);
        const float* inside = reinterpret_cast<const float*>(both.data());
        EXPECT(sumsq_arguments(8, inside, nullptr, both.data() + 3));               // out inside a
        EXPECT(sumsq_arguments((1ull << 33) + 1u, inside, nullptr, both.data()));
        const float one = 3.0f;
        double s = 0.0;
        EXPECT(xrt_host_volume_sumsq(1, &one, nullptr, &s) == XRT_OK && s == 9.0);
    }

    // the descent: bounds, a constant volume, a zero length, a NaN among the voxels
    {
        const uint32_t dims[3] = {67, 9, 3};
        const size_t voxels = 67u * 9u * 3u;
        std::vector<float> vol = noise(voxels, 9u, 0.0f, 2.0f);
        const std::vector<float> before = vol;
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 3, 0.7, 0.25f, 1.75f) == XRT_OK);
        bool moved = false;
        for (size_t i = 0; i < voxels; ++i) {
            EXPECT(vol[i] >= 0.25f && vol[i] <= 1.75f);
            moved = moved || vol[i] != before[i];
        }
        EXPECT(moved);
        std::vector<float> flat(voxels, 0.5f);
        EXPECT(xrt_host_tv_descend(flat.data(), dims, 1e-8, 3, 0.7, -inf, inf) == XRT_OK);
        for (float v : flat) EXPECT(v == 0.5f);
        vol = before;
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 3, 0.0, -inf, inf) == XRT_OK);
        EXPECT(std::memcmp(vol.data(), before.data(), voxels * sizeof(float)) == 0);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 0, 0.7, -inf, inf) == XRT_OK);
        EXPECT(std::memcmp(vol.data(), before.data(), voxels * sizeof(float)) == 0);
        vol[100] = nan;
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 2, 0.7, -inf, inf) == XRT_OK);
        EXPECT(vol[0] == before[0] && std::isnan(vol[100]));                      // G is NaN: nothing moves
        EXPECT(xrt_host_tv_descend(nullptr, dims, 1e-8, 2, 0.7, -inf, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), nullptr, 1e-8, 2, 0.7, -inf, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 0.0, 2, 0.7, -inf, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 2, -0.1, -inf, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 2, (double)inf, -inf, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 2, 0.7, nan, inf) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_tv_descend(vol.data(), dims, 1e-8, 2, 0.7, 1.0f, 0.5f) == XRT_ERR_ARGUMENT);
    }

    // the solver: 7 planes in 1 and 3 subsets, with TV, without steps, and the parameters' checks
    {
        const uint32_t dims[3] = {9, 8, 7}, W = 16, H = 12, P = 7;
        const float spacing[3] = {0.5f, 0.5f, 0.5f};
        const float origin[3] = {-0.25f * dims[0], -0.25f * dims[1], -0.25f * dims[2]};
        std::vector<double> A((size_t)P * 12u), R((size_t)P * 12u);
        for (uint32_t p = 0; p < P; ++p) {
            const xrt_camera c = camera(0.3 + 6.283185307179586 * p / P, W, H, 0.6f);
            EXPECT(xrt_backprojection_matrix(&c, nullptr, origin, spacing, A.data() + 12u * p) == XRT_OK);
            EXPECT(xrt_ray_matrix(A.data() + 12u * p, R.data() + 12u * p) == XRT_OK);
        }
        const size_t voxels = (size_t)dims[0] * dims[1] * dims[2], all = (size_t)W * H * P;
        const std::vector<float> truth = noise(voxels, 77u, 0.0f, 1.0f);
        std::vector<float> proj(all);
        EXPECT(xrt_host_forward_project(W, H, P, truth.data(), dims, spacing, R.data(), XRT_FP_PROJECT, nullptr, proj.data()) == XRT_OK);
        const xrt_tv_params tv = {3u, 0.2, 0.9, 1e-8}, off = {0u, (double)nan, 0.0, -1.0};
        for (uint32_t S : {1u, 3u}) {
            std::vector<float> plain(voxels, 0.0f), smooth(voxels, 0.0f), same(voxels, 0.0f), null(voxels, 0.0f);
            EXPECT(xrt_host_sirt(W, H, P, proj.data(), A.data(), dims, spacing, 2, S, 1.0, 0.0f, inf, plain.data()) == XRT_OK);
            EXPECT(xrt_host_sirt_tv(W, H, P, proj.data(), A.data(), dims, spacing, 2, S, 1.0, 0.0f, inf, &tv, smooth.data()) == XRT_OK);
            EXPECT(xrt_host_sirt_tv(W, H, P, proj.data(), A.data(), dims, spacing, 2, S, 1.0, 0.0f, inf, &off, same.data()) == XRT_OK);
            EXPECT(xrt_host_sirt_tv(W, H, P, proj.data(), A.data(), dims, spacing, 2, S, 1.0, 0.0f, inf, nullptr, null.data()) == XRT_OK);
            EXPECT(std::memcmp(plain.data(), same.data(), voxels * sizeof(float)) == 0);
            EXPECT(std::memcmp(plain.data(), null.data(), voxels * sizeof(float)) == 0);
            EXPECT(std::memcmp(plain.data(), smooth.data(), voxels * sizeof(float)) != 0);
            for (float v : smooth) EXPECT(std::isfinite(v) && v >= 0.0f);
        }
        std::vector<float> vol(voxels, 0.0f);
        const xrt_tv_params bad_alpha = {3u, -0.1, 1.0, 1e-8}, bad_reduction = {3u, 0.2, 1.5, 1e-8}, zero_reduction = {3u, 0.2, 0.0, 1e-8},
                            bad_eps = {3u, 0.2, 1.0, 0.0}, nan_alpha = {3u, (double)nan, 1.0, 1e-8};
        EXPECT(tv_params_arguments(&tv) == nullptr && tv_params_arguments(&off) == nullptr && tv_params_arguments(nullptr) == nullptr);
        for (const xrt_tv_params* p : {&bad_alpha, &bad_reduction, &zero_reduction, &bad_eps, &nan_alpha}) {
            EXPECT(tv_params_arguments(p));
            EXPECT(xrt_host_sirt_tv(W, H, P, proj.data(), A.data(), dims, spacing, 2, 1, 1.0, 0.0f, inf, p, vol.data()) == XRT_ERR_ARGUMENT);
        }
        EXPECT(xrt_host_sirt_tv(W, H, P, proj.data(), A.data(), dims, spacing, 0, 1, 1.0, 0.0f, inf, &tv, vol.data()) == XRT_ERR_ARGUMENT);
    }

    if (failures) {
        std::printf("tv_san: %d failures\n", failures);
        return 1;
    }
    std::printf("tv_san: OK\n");
    return 0;
}
