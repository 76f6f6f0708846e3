// mltr_san.cpp -- OS-MLTR's host code (the argument checks of
// xrt_poisson_project, xrt_backproject_update and xrt_mltr and the three host
// restatements: simpleraytracing_amd/csrc/xrt_mltr_host.inc over
// xrt_tv_host.inc, xrt_sirt_host.inc and xrt_fdk_host.inc) over its edge cases,
// as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/mltr_san.cpp \
//         -o mltr_san
//
// Exact-size heap buffers, so that a gather one pair past a plane or before
// it -- the bilinear corners at col = -1 and col = W - 1 --, a read of a
// background that is not there or a store past the pairs is seen.  Prints
// "mltr_san: OK" and returns 0 when every call returned what it should
// (tests/test_mltr_cpu.py runs it).
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
#include "xrt_mltr_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("mltr_san: line %d: %s\n", __LINE__, #cond);          \
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// A scan of P planes of W x H over a grid a little larger than the detector's shadow, so that voxels project
// outside the planes and rays miss the grid: the stages one by one, the fused update against its composition, the
// solver against the stages.
static void check_scan(uint32_t P, uint32_t W, uint32_t H, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t subsets)
{
    const uint32_t dims[3] = {nx, ny, nz};
    const uint32_t top = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    const float side = 1.3f * 0.4f * (float)(W > H ? W : H) * 100.0f / 150.0f;
    const float spacing[3] = {side / top, side / top, side / top};
    const float origin[3] = {-0.5f * nx * spacing[0], -0.5f * ny * spacing[1], -0.5f * nz * spacing[2]};
    const size_t plane = (size_t)W * H, voxels = (size_t)nx * ny * nz;
    std::vector<double> A(12u * P), R(12u * P);
    for (uint32_t p = 0; p < P; ++p) {
        const xrt_camera cam = camera(2.0 * 3.14159265358979323846 * p / P, W, H, 0.4f);
        EXPECT(xrt_backprojection_matrix(&cam, nullptr, origin, spacing, A.data() + 12u * p) == XRT_OK);
        EXPECT(xrt_ray_matrix(A.data() + 12u * p, R.data() + 12u * p) == XRT_OK);
    }
    const std::vector<float> vol = noise(voxels, P + W, 0.0f, 0.2f), flat = noise(plane, 5u, 80.0f, 120.0f);
    std::vector<float> counts = noise(plane * P, 7u, 0.0f, 100.0f), bg = noise(plane * P, 9u, 0.0f, 5.0f);
    counts[0] = 0.0f;
    counts[plane * P - 1u] = std::numeric_limits<float>::quiet_NaN();
    std::vector<double> aligned(plane * P);                  // (a pair a double: aligned to 8 bytes, exactly the pairs' size)
    float* pairs = reinterpret_cast<float*>(aligned.data());
    for (int with_bg = 0; with_bg < 2; ++with_bg)
        EXPECT(xrt_host_poisson_project(W, H, P, vol.data(), dims, spacing, R.data(), counts.data(), flat.data(),
                                        with_bg ? bg.data() : nullptr, pairs) == XRT_OK);
    // the fused update against xrt_host_backproject x 2 and xrt_host_volume_update
    std::vector<float> num(plane * P), den(plane * P), corr(voxels), norm(voxels);
    for (size_t i = 0; i < plane * P; ++i) {
        num[i] = pairs[2u * i];
        den[i] = pairs[2u * i + 1u];
    }
    std::vector<float> fused = vol, composed = vol;
    EXPECT(xrt_host_backproject_update(W, H, P, pairs, A.data(), dims, 0.9, 0.0f, 1.5f, fused.data()) == XRT_OK);
    EXPECT(xrt_host_backproject(W, H, P, num.data(), A.data(), dims, 0, nz, 1.0, 0, corr.data()) == XRT_OK);
    EXPECT(xrt_host_backproject(W, H, P, den.data(), A.data(), dims, 0, nz, 1.0, 0, norm.data()) == XRT_OK);
    EXPECT(xrt_host_volume_update(voxels, composed.data(), corr.data(), norm.data(), 0.9, 0.0f, 1.5f) == XRT_OK);
    EXPECT(same_bits(fused, composed));
    // the solver: one subset, one iteration, is the two stages
    std::vector<float> solved(voxels, 0.0f), staged(voxels, 0.0f);
    EXPECT(xrt_host_mltr(W, H, P, counts.data(), flat.data(), bg.data(), A.data(), dims, spacing, 1, 1, 1.0, 0.0f,
                         std::numeric_limits<float>::infinity(), nullptr, solved.data()) == XRT_OK);
    EXPECT(xrt_host_poisson_project(W, H, P, staged.data(), dims, spacing, R.data(), counts.data(), flat.data(), bg.data(),
                                    pairs) == XRT_OK);
    EXPECT(xrt_host_backproject_update(W, H, P, pairs, A.data(), dims, 1.0, 0.0f, std::numeric_limits<float>::infinity(),
                                       staged.data()) == XRT_OK);
    EXPECT(same_bits(solved, staged));
    // subsets (the planes read at their stride), with and without tv and a background
    const xrt_tv_params tv = {2u, 0.2, 0.9, 1e-8};
    counts[plane * P - 1u] = 3.0f;                           // (a NaN count spreads to the voxels its ray meets)
    for (int form = 0; form < 3; ++form) {
        std::vector<float> x(voxels, 0.0f);
        EXPECT(xrt_host_mltr(W, H, P, counts.data(), flat.data(), form == 1 ? nullptr : bg.data(), A.data(), dims, spacing, 2,
                             subsets, 0.9, 0.0f, 4.0f, form == 2 ? &tv : nullptr, x.data()) == XRT_OK);
        for (float v : x) EXPECT(v >= 0.0f && v <= 4.0f);
    }
}

// Hand-built matrices under which voxels land exactly on col = -1, 0, W - 1, W and beyond, and a slab with c = 0.
static void check_edges(uint32_t W, uint32_t H)
{
    const uint32_t dims[3] = {W + 3u, H + 3u, 2u};
    const double A[24] = {1, 0, 0, -1, 0, 1, 0, -1, 0, 0, -1, 1, 1, 0, 0, -1, 0, 1, 0, -1, 0, 0, 0, 2};
    const size_t plane = (size_t)W * H, voxels = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<double> aligned(plane * 2u);
    float* pairs = reinterpret_cast<float*>(aligned.data());
    uint32_t seed = W + H;
    for (size_t i = 0; i < plane * 4u; ++i) pairs[i] = 0.5f + (float)(lcg(seed) % 100u) / 50.0f;
    const std::vector<float> start = noise(voxels, 3u, -1.0f, 1.0f);
    std::vector<float> x = start;
    EXPECT(xrt_host_backproject_update(W, H, 2, pairs, A, dims, 1.0, -10.0f, 10.0f, x.data()) == XRT_OK);
    std::vector<float> once = start;
    EXPECT(xrt_host_backproject_update(W, H, 1, pairs, A, dims, 1.0, -10.0f, 10.0f, once.data()) == XRT_OK);
    const size_t slab = (size_t)dims[0] * dims[1];           // k = 1: c = 0 under the first matrix, unseen
    EXPECT(std::memcmp(once.data() + slab, start.data() + slab, slab * sizeof(float)) == 0);
}

static void check_refusals()
{
    const uint32_t dims[3] = {5, 4, 3};
    const float spacing[3] = {1.0f, 1.0f, 1.0f};
    std::vector<float> vol(60), counts(24), flat(12), x(60);
    std::vector<double> rays(24, 1.0), aligned(24);
    float* pairs = reinterpret_cast<float*>(aligned.data());
    EXPECT(xrt_host_poisson_project(4, 3, 2, vol.data(), dims, spacing, rays.data(), counts.data(), flat.data(), nullptr,
                                    pairs + 1) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_poisson_project(4, 3, 2, vol.data(), dims, spacing, rays.data(), nullptr, flat.data(), nullptr, pairs) ==
           XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_poisson_project(4, 3, 2, vol.data(), dims, spacing, rays.data(), counts.data(), nullptr, nullptr, pairs) ==
           XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_poisson_project(4, 3, 0, vol.data(), dims, spacing, rays.data(), counts.data(), flat.data(), nullptr,
                                    pairs) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_backproject_update(4, 3, 2, pairs, rays.data(), dims, std::nan(""), 0.0f, 1.0f, x.data()) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_backproject_update(4, 3, 2, pairs, rays.data(), dims, 1.0, 1.0f, 0.0f, x.data()) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_backproject_update(4, 3, 2, pairs + 1, rays.data(), dims, 1.0, 0.0f, 1.0f, x.data()) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_mltr(4, 3, 2, counts.data(), flat.data(), nullptr, rays.data(), dims, spacing, 0, 1, 1.0, 0.0f, 1.0f, nullptr,
                         x.data()) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_mltr(4, 3, 2, counts.data(), flat.data(), nullptr, rays.data(), dims, spacing, 1, 3, 1.0, 0.0f, 1.0f, nullptr,
                         x.data()) == XRT_ERR_ARGUMENT);
    // (matrices of ones have no ray matrix)
    EXPECT(xrt_host_mltr(4, 3, 2, counts.data(), flat.data(), nullptr, rays.data(), dims, spacing, 1, 1, 1.0, 0.0f, 1.0f, nullptr,
                         x.data()) == XRT_ERR_ARGUMENT);
}

int main()
{
    check_scan(1, 1, 1, 1, 1, 1, 1);
    check_scan(3, 7, 13, 5, 3, 2, 3);
    check_scan(5, 19, 11, 67, 4, 3, 2);
    check_edges(2, 2);
    check_edges(7, 5);
    check_refusals();
    if (failures) return 1;
    std::printf("mltr_san: OK\n");
    return 0;
}
