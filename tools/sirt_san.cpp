// sirt_san.cpp -- SIRT / OS-SART's host code (the argument checks of
// xrt_forward_project, xrt_volume_update and xrt_sirt, xrt_ray_matrix, the
// solver's plan and the three host restatements:
// simpleraytracing_amd/csrc/xrt_sirt_host.inc over xrt_fdk_host.inc) over its
// edge cases, as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/sirt_san.cpp \
//         -o sirt_san
//
// Exact-size heap buffers, so that a read one voxel past the volume, one pixel
// past a plane or one entry past a ray matrix, or a write past a plane, is
// seen.  Prints "sirt_san: OK" and returns 0 when every call returned what it
// should (tests/test_sirt_cpu.py runs it).
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
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("sirt_san: line %d: %s\n", __LINE__, #cond);          \
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

// P matrices of a turn about a grid of `dims` voxels of 0.5 centred on the axis.
static std::vector<double> matrices(uint32_t P, uint32_t W, uint32_t H, const uint32_t dims[3], float pitch)
{
    std::vector<double> mats((size_t)P * 12u);
    const float spacing[3] = {0.5f, 0.5f, 0.5f};
    const float origin[3] = {-0.25f * dims[0], -0.25f * dims[1], -0.25f * dims[2]};
    for (uint32_t p = 0; p < P; ++p) {
        const xrt_camera c = camera(0.3 + 6.283185307179586 * p / P, W, H, pitch);
        EXPECT(xrt_backprojection_matrix(&c, nullptr, origin, spacing, mats.data() + 12u * p) == XRT_OK);
    }
    return mats;
}

static void check_forward(uint32_t W, uint32_t H, uint32_t P, const uint32_t dims[3], float pitch)
{
    const float spacing[3] = {0.5f, 0.5f, 0.5f};
    const std::vector<double> A = matrices(P, W, H, dims, pitch);
    std::vector<double> R((size_t)P * 12u);
    for (uint32_t p = 0; p < P; ++p) EXPECT(xrt_ray_matrix(A.data() + 12u * p, R.data() + 12u * p) == XRT_OK);
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2], all = (size_t)W * H * P;
    const std::vector<float> vol = noise(voxels, W + 7u * P, 0.0f, 2.0f), meas = noise(all, 3u, 0.0f, 9.0f);
    std::vector<float> out(all, -7.0f), res(all, -7.0f);
    EXPECT(xrt_host_forward_project(W, H, P, vol.data(), dims, spacing, R.data(), XRT_FP_PROJECT, nullptr, out.data()) == XRT_OK);
    EXPECT(xrt_host_forward_project(W, H, P, vol.data(), dims, spacing, R.data(), XRT_FP_RESIDUAL, meas.data(), res.data()) == XRT_OK);
    bool any = false;
    for (size_t i = 0; i < all; ++i) {
        EXPECT(std::isfinite(out[i]) && out[i] >= 0.0f && std::isfinite(res[i]) && res[i] != -7.0f);
        any = any || out[i] > 0.0f;
    }
    EXPECT(any);                                                          // the grid is in view
    // every plane on its own, into a buffer of exactly its size, is the stack's plane
    for (uint32_t p = 0; p < P; ++p) {
        std::vector<float> one((size_t)W * H, -7.0f);
        EXPECT(xrt_host_forward_project(W, H, 1, vol.data(), dims, spacing, R.data() + 12u * p, XRT_FP_PROJECT, nullptr, one.data()) == XRT_OK);
        EXPECT(std::memcmp(one.data(), out.data() + (size_t)p * W * H, one.size() * sizeof(float)) == 0);
    }
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the forward projector: one voxel, odd sizes, a detector of more than one tile a side
    {
        const uint32_t one[3] = {1, 1, 1}, odd[3] = {5, 3, 2}, wide[3] = {67, 9, 3}, row[3] = {130, 2, 2};
        check_forward(1, 1, 1, one, 0.1f);
        check_forward(7, 13, 3, odd, 0.2f);
        check_forward(33, 21, 5, wide, 1.2f);
        check_forward(16, 9, 2, row, 3.0f);
    }
    {
        // hand-built rays over (5, 3, 2): inside faces, a source inside, on the far boundary (a miss), special voxels
        const uint32_t dims[3] = {5, 3, 2};
        const float spacing[3] = {0.5f, 0.25f, 2.0f};
        std::vector<float> vol(30, 1.0f), out(9, -7.0f);
        const double faces[12] = {0, 0, 1, -3, 0, 0.4, -0.4, 0.5, 0.125, 0, -0.125, 0.5};
        EXPECT(xrt_host_forward_project(3, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, out.data()) == XRT_OK);
        EXPECT(out[4] == 2.5f && out[0] == 0.0f && out[7] > 1.0f && out[7] < 2.5f);   // (row 2 leaves through y = 2.5)
        const double inside[12] = {1, 0, -1.5, 2.2, 0, 1, -1.5, 1.1, 0, 0, 0.25, 0.3};
        std::vector<float> out16(16, -7.0f), meas16(16, 1.0f);
        EXPECT(xrt_host_forward_project(4, 4, 1, vol.data(), dims, spacing, inside, XRT_FP_RESIDUAL, meas16.data(), out16.data()) == XRT_OK);
        for (float v : out16) EXPECT(std::isfinite(v));
        const double far_side[12] = {1, 0, 0.5, 2.0, 0, 0, 0, 2.5, 0, 0.5, -0.25, 0.5};
        EXPECT(xrt_host_forward_project(2, 2, 1, vol.data(), dims, spacing, far_side, XRT_FP_RESIDUAL, meas16.data(), out16.data()) == XRT_OK);
        for (int i = 0; i < 4; ++i) EXPECT(out16[i] == 0.0f && !std::signbit(out16[i]));
        vol[3] = nan; vol[7] = inf; vol[11] = -inf; vol[13] = -0.0f;
        EXPECT(xrt_host_forward_project(4, 4, 1, vol.data(), dims, spacing, inside, XRT_FP_PROJECT, nullptr, out16.data()) == XRT_OK);
        // the checks
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true) == nullptr);
        EXPECT(forward_project_arguments(3, 3, 1, nullptr, dims, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), nullptr, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, nullptr, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, nullptr, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, nullptr, true));
        EXPECT(forward_project_arguments(0, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 65536, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), false));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, faces, 2, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_RESIDUAL, nullptr, out.data(), true));
        const float bad_spacing[3] = {0.5f, 0.0f, 2.0f};
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, bad_spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        const uint32_t big[3] = {5, 2049, 2};
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), big, spacing, faces, XRT_FP_PROJECT, nullptr, out.data(), true));
        double bad[12];
        std::memcpy(bad, faces, sizeof bad);
        bad[11] = (double)nan;
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, bad, XRT_FP_PROJECT, nullptr, out.data(), true));
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, bad, XRT_FP_PROJECT, nullptr, out.data(), false) == nullptr);
        EXPECT(forward_project_arguments(3, 3, 1, vol.data(), dims, spacing, faces, XRT_FP_PROJECT, nullptr, vol.data() + 29, true));   // the last voxel
        EXPECT(xrt_host_forward_project(3, 3, 1, vol.data(), dims, spacing, bad, XRT_FP_PROJECT, nullptr, out.data()) == XRT_ERR_ARGUMENT);
    }

    // xrt_ray_matrix
    {
        const double A[12] = {2, 0, 0, 1, 0, 4, 0, 2, 0, 0, 8, 4};
        double R[12];
        EXPECT(xrt_ray_matrix(A, R) == XRT_OK);
        EXPECT(R[0] == 0.5 && R[5] == 0.25 && R[10] == 0.125 && R[3] == -0.5 && R[7] == -0.5 && R[11] == -0.5);
        EXPECT(xrt_ray_matrix(nullptr, R) == XRT_ERR_ARGUMENT && xrt_ray_matrix(A, nullptr) == XRT_ERR_ARGUMENT);
        double B[12];
        std::memcpy(B, A, sizeof B);
        B[5] = 0.0;                                                       // a zero determinant
        EXPECT(xrt_ray_matrix(B, R) == XRT_ERR_ARGUMENT);
        B[5] = (double)inf;
        EXPECT(xrt_ray_matrix(B, R) == XRT_ERR_ARGUMENT);
        const double tiny[12] = {1e-200, 0, 0, 1e200, 0, 1, 0, 0, 0, 0, 1, 0};   // a source that is not finite
        EXPECT(xrt_ray_matrix(tiny, R) == XRT_ERR_ARGUMENT);
    }

    // the update
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 1025ull}) {
        std::vector<float> x = noise(n, (uint32_t)n, -1.0f, 2.0f), corr = noise(n, 5u, -1.0f, 1.0f), norm = noise(n, 9u, 0.5f, 2.0f);
        norm[0] = n % 2 ? 0.0f : nan;
        const std::vector<float> before = x;
        EXPECT(xrt_host_volume_update(n, x.data(), corr.data(), norm.data(), 1.0, 0.0f, 1.5f) == XRT_OK);
        EXPECT(std::memcmp(&x[0], &before[0], sizeof(float)) == 0);       // norm 0 or NaN: x stays
        for (uint64_t i = 1; i < n; ++i) EXPECT(x[i] >= 0.0f && x[i] <= 1.5f);
        EXPECT(xrt_host_volume_update(n, x.data(), corr.data(), norm.data(), 0.5, -inf, inf) == XRT_OK);
        EXPECT(xrt_host_volume_update(n, x.data(), corr.data(), norm.data(), (double)nan, 0.0f, 1.0f) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_update(n, x.data(), corr.data(), norm.data(), 1.0, nan, 1.0f) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_update(n, x.data(), corr.data(), norm.data(), 1.0, 1.0f, 0.5f) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_update(n, x.data(), x.data(), norm.data(), 1.0, 0.0f, 1.0f) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_update(0, x.data(), corr.data(), norm.data(), 1.0, 0.0f, 1.0f) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_host_volume_update(n, nullptr, corr.data(), norm.data(), 1.0, 0.0f, 1.0f) == XRT_ERR_ARGUMENT);
    }

    // the solver: subsets of unequal sizes (7 planes in 1, 3 and 7 subsets), measurements of a known volume
    {
        const uint32_t dims[3] = {9, 8, 7}, W = 16, H = 12, P = 7;
        const float spacing[3] = {0.5f, 0.5f, 0.5f};
        const std::vector<double> A = matrices(P, W, H, dims, 0.6f);
        std::vector<double> R((size_t)P * 12u);
        for (uint32_t p = 0; p < P; ++p) EXPECT(xrt_ray_matrix(A.data() + 12u * p, R.data() + 12u * p) == XRT_OK);
        const size_t voxels = (size_t)dims[0] * dims[1] * dims[2], all = (size_t)W * H * P;
        const std::vector<float> truth = noise(voxels, 77u, 0.0f, 1.0f);
        std::vector<float> proj(all);
        EXPECT(xrt_host_forward_project(W, H, P, truth.data(), dims, spacing, R.data(), XRT_FP_PROJECT, nullptr, proj.data()) == XRT_OK);
        for (uint32_t S : {1u, 3u, 7u}) {
            std::vector<float> vol(voxels, 0.0f);
            EXPECT(xrt_host_sirt(W, H, P, proj.data(), A.data(), dims, spacing, 2, S, 1.0, 0.0f, inf, vol.data()) == XRT_OK);
            bool any = false;
            for (float v : vol) {
                EXPECT(std::isfinite(v) && v >= 0.0f);
                any = any || v > 0.0f;
            }
            EXPECT(any);
            SirtPlan plan;
            EXPECT(sirt_plan(P, S, A.data(), plan));
            uint32_t total = 0;
            for (uint32_t s = 0; s < S; ++s) total += plan.count[s];
            EXPECT(total == P && plan.plane.size() == P && plan.widest == (P + S - 1u) / S && plan.plane[plan.first[S - 1u]] == S - 1u);
        }
        std::vector<float> vol(voxels, 0.0f);
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 3, 1.0, 0.0f, inf, vol.data(), true) == nullptr);
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 0, 3, 1.0, 0.0f, inf, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 0, 1.0, 0.0f, inf, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 8, 1.0, 0.0f, inf, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 3, (double)inf, 0.0f, inf, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 3, 1.0, 1.0f, 0.0f, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 3, 1.0, nan, inf, vol.data(), true));
        EXPECT(sirt_arguments(W, H, P, proj.data(), A.data(), dims, spacing, 2, 3, 1.0, 0.0f, inf, proj.data() + 5, true));
        EXPECT(sirt_arguments(W, H, P, nullptr, A.data(), dims, spacing, 2, 3, 1.0, 0.0f, inf, vol.data(), true));
        std::vector<double> flat = A;
        for (int e = 0; e < 4; ++e) flat[12 + 8 + e] = flat[12 + e] = flat[12 + 4 + e];   // plane 1: three equal lines
        EXPECT(xrt_host_sirt(W, H, P, proj.data(), flat.data(), dims, spacing, 1, 1, 1.0, 0.0f, inf, vol.data()) == XRT_ERR_ARGUMENT);
    }

    if (failures) {
        std::printf("sirt_san: %d failures\n", failures);
        return 1;
    }
    std::printf("sirt_san: OK\n");
    return 0;
}
