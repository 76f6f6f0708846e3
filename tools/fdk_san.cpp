// fdk_san.cpp -- FDK reconstruction's host code (the argument checks of
// xrt_fdk_filter and xrt_backproject, xrt_ramp_filter, xrt_fdk_weights,
// xrt_fdk_scale, xrt_backprojection_matrix and the two host restatements:
// simpleraytracing_amd/csrc/xrt_fdk_host.inc) over its edge cases, as a
// stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/fdk_san.cpp \
//         -o fdk_san
//
// Exact-size heap buffers, so that a read one pixel past a row, a plane or a
// tap table, or a write one voxel past a slab, is seen.  Prints "fdk_san: OK"
// and returns 0 when every call returned what it should
// (tests/test_fdk_cpu.py runs it).
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
}

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("fdk_san: line %d: %s\n", __LINE__, #cond);           \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static uint32_t lcg(uint32_t& s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static std::vector<float> noise(size_t n, uint32_t seed)
{
    std::vector<float> v(n);
    for (float& x : v) x = (float)(lcg(seed) % 2001u) * 0.001f - 1.0f;
    return v;
}

// A source on -x at `sod`, the detector centre on +x at `sdd - sod`, turned by `theta` about z; up = z.
static xrt_camera camera(double theta, uint32_t W, uint32_t H)
{
    const double sod = 100.0, sdd = 150.0, cs = std::cos(theta), sn = std::sin(theta);
    xrt_camera c;
    c.origin[0] = (float)(-sod * cs); c.origin[1] = (float)(-sod * sn); c.origin[2] = 0.0f;
    c.detector[0] = (float)((sdd - sod) * cs); c.detector[1] = (float)((sdd - sod) * sn); c.detector[2] = 0.0f;
    c.right[0] = (float)-sn; c.right[1] = (float)cs; c.right[2] = 0.0f;
    c.up[0] = 0.0f; c.up[1] = 0.0f; c.up[2] = 1.0f;
    c.pixel_spacing = 0.4f;
    c.width = W;
    c.height = H;
    return c;
}

static void check_filter(uint32_t W, uint32_t H, uint32_t P, uint32_t T, bool weighted)
{
    const std::vector<float> image = noise((size_t)W * H * P, W * 31u + T), weight = noise((size_t)W * H, 7u);
    std::vector<float> taps = noise(T, T), out((size_t)W * H * P, -7.0f);
    EXPECT(xrt_host_fdk_filter(W, H, P, image.data(), weighted ? weight.data() : nullptr, taps.data(), T, out.data()) == XRT_OK);
    for (float v : out) EXPECT(std::isfinite(v) && v != -7.0f);
    // one tap of 1: the weighted image (a -0.0 product becomes +0.0: the sum starts at +0.0)
    if (T == 1) {
        taps[0] = 1.0f;
        EXPECT(xrt_host_fdk_filter(W, H, P, image.data(), weighted ? weight.data() : nullptr, taps.data(), T, out.data()) == XRT_OK);
        for (size_t i = 0; i < out.size(); ++i) EXPECT(out[i] == (weighted ? image[i] * weight[i % ((size_t)W * H)] : image[i]));
    }
}

static void check_backproject(uint32_t W, uint32_t H, uint32_t P, const uint32_t dims[3])
{
    const std::vector<float> proj = noise((size_t)W * H * P, W + 13u * P);
    std::vector<double> mats((size_t)P * 12u);
    const float spacing[3] = {0.5f, 0.5f, 0.5f};
    const float origin[3] = {-0.25f * dims[0], -0.25f * dims[1], -0.25f * dims[2]};
    for (uint32_t p = 0; p < P; ++p) {
        const xrt_camera c = camera(6.283185307179586 * p / P, W, H);
        EXPECT(xrt_backprojection_matrix(&c, nullptr, origin, spacing, mats.data() + 12u * p) == XRT_OK);
    }
    const size_t slab = (size_t)dims[0] * dims[1];
    std::vector<float> whole(slab * dims[2], -7.0f);
    EXPECT(xrt_host_backproject(W, H, P, proj.data(), mats.data(), dims, 0, dims[2], 0.5, 0, whole.data()) == XRT_OK);
    for (float v : whole) EXPECT(std::isfinite(v) && v != -7.0f);
    // every slab on its own, into a buffer of exactly its size, is the whole volume's slab
    for (uint32_t k = 0; k < dims[2]; ++k) {
        std::vector<float> one(slab, -7.0f);
        EXPECT(xrt_host_backproject(W, H, P, proj.data(), mats.data(), dims, k, k + 1, 0.5, 0, one.data()) == XRT_OK);
        EXPECT(std::memcmp(one.data(), whole.data() + k * slab, slab * sizeof(float)) == 0);
    }
    // an empty range writes nothing
    float guard = -7.0f;
    EXPECT(xrt_host_backproject(W, H, P, proj.data(), mats.data(), dims, 1 % (dims[2] + 1u), 1 % (dims[2] + 1u), 0.5, 0, &guard) == XRT_OK);
    EXPECT(guard == -7.0f);
    // accumulation onto zeros is the plain result
    std::vector<float> sum(whole.size(), 0.0f);
    EXPECT(xrt_host_backproject(W, H, P, proj.data(), mats.data(), dims, 0, dims[2], 0.5, 1, sum.data()) == XRT_OK);
    for (size_t i = 0; i < sum.size(); ++i) EXPECT(sum[i] == whole[i]);
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the filter: one pixel, odd sizes, tables shorter and longer than the row, the widest row with the longest table
    for (uint32_t T : {1u, 3u, 13u, 27u}) {
        check_filter(1, 1, 1, T, false);
        check_filter(7, 13, 2, T, true);
        check_filter(67, 5, 3, T, T == 3u);
    }
    check_filter(XRT_MAX_RAMP_WIDTH, 1, 1, 2u * XRT_MAX_RAMP_WIDTH - 1u, true);
    {
        // pixels outside the row are skipped, not replicated; taps[0] meets the pixel to the left
        const float row[3] = {1.0f, 2.0f, 4.0f}, ones[3] = {1.0f, 1.0f, 1.0f}, left[3] = {1.0f, 0.0f, 0.0f};
        float out[3];
        EXPECT(xrt_host_fdk_filter(3, 1, 1, row, nullptr, ones, 3, out) == XRT_OK && out[0] == 3.0f && out[1] == 7.0f && out[2] == 6.0f);
        EXPECT(xrt_host_fdk_filter(3, 1, 1, row, nullptr, left, 3, out) == XRT_OK && out[0] == 0.0f && out[1] == 1.0f && out[2] == 2.0f);
        // non-finite pixels travel as IEEE arithmetic has them
        const float bad[3] = {inf, 1.0f, nan};
        EXPECT(xrt_host_fdk_filter(3, 1, 1, bad, nullptr, left, 3, out) == XRT_OK && std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]));   // (0 * inf)
        EXPECT(xrt_host_fdk_filter(3, 1, 1, bad, nullptr, ones, 3, out) == XRT_OK && out[0] == inf && std::isnan(out[1]) && std::isnan(out[2]));
    }
    {
        // the checks
        std::vector<float> buf(64, 0.0f), taps(5, 1.0f), out(24);
        const float* img = buf.data();
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, out.data(), true) == nullptr);
        EXPECT(fdk_filter_arguments(4, 3, 2, nullptr, nullptr, taps.data(), 5, out.data(), true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, nullptr, 5, out.data(), true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, nullptr, true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 4, out.data(), true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 0, out.data(), true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 2u * XRT_MAX_RAMP_WIDTH + 1u, out.data(), false));
        EXPECT(fdk_filter_arguments(0, 3, 2, img, nullptr, taps.data(), 5, out.data(), true));
        EXPECT(fdk_filter_arguments(XRT_MAX_RAMP_WIDTH + 1u, 1, 1, img, nullptr, taps.data(), 5, out.data(), false));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, buf.data() + 23, true));          // the last pixel
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, buf.data() + 24, true) == nullptr);
        EXPECT(fdk_filter_arguments(4, 3, 2, img + 40, img + 20, taps.data(), 5, buf.data(), true));         // the weight plane
        taps[4] = nan;
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, out.data(), true));
        EXPECT(fdk_filter_arguments(4, 3, 2, img, nullptr, taps.data(), 5, out.data(), false) == nullptr);   // (the device form)
        EXPECT(xrt_host_fdk_filter(4, 3, 2, img, nullptr, taps.data(), 5, out.data()) == XRT_ERR_ARGUMENT);
    }

    // the backprojector: one voxel, odd sizes, a row longer than a wave's span
    {
        const uint32_t one[3] = {1, 1, 1}, odd[3] = {5, 3, 2}, wide[3] = {67, 9, 3}, row[3] = {261, 2, 2};
        check_backproject(1, 1, 1, one);
        check_backproject(7, 13, 3, odd);
        check_backproject(33, 21, 5, wide);
        check_backproject(16, 8, 2, row);
    }
    {
        // voxels exactly on col = -1, 0, W - 1 and W, and behind the source
        const uint32_t W = 4, H = 1, dims[3] = {W + 2, 1, 2};
        const float proj[4] = {1.0f, 2.0f, 4.0f, 8.0f};
        const double A[12] = {1, 0, 0, -1, 0, 0, 0, 0, 0, 0, -1, 1};        // col = i - 1, row = 0, c = 1 - k
        std::vector<float> vol(12, -7.0f);
        EXPECT(xrt_host_backproject(W, H, 1, proj, A, dims, 0, 2, 1.0, 0, vol.data()) == XRT_OK);
        const float want[12] = {0, 1, 2, 4, 8, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 12; ++i) EXPECT(vol[i] == want[i]);
        const double half[12] = {1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 2};      // col = (i - 1) / 2, weight 1 / 4
        EXPECT(xrt_host_backproject(W, H, 1, proj, half, dims, 0, 1, 4.0, 0, vol.data()) == XRT_OK);
        const float mid[6] = {0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f};
        for (int i = 0; i < 6; ++i) EXPECT(vol[i] == mid[i]);
        // the checks
        EXPECT(backproject_arguments(W, H, 1, proj, A, dims, 0, 2, 1.0, vol.data(), true) == nullptr);
        EXPECT(backproject_arguments(W, H, 1, nullptr, A, dims, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, nullptr, dims, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, A, nullptr, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, A, dims, 0, 2, 1.0, nullptr, true));
        EXPECT(backproject_arguments(0, H, 1, proj, A, dims, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 65536, proj, A, dims, 0, 2, 1.0, vol.data(), false));
        EXPECT(backproject_arguments(W, H, 1, proj, A, dims, 2, 1, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, A, dims, 0, 3, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, A, dims, 0, 2, (double)inf, vol.data(), true));
        const uint32_t zero[3] = {6, 0, 2}, big[3] = {6, 2049, 2};
        EXPECT(backproject_arguments(W, H, 1, proj, A, zero, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, A, big, 0, 2, 1.0, vol.data(), true));
        double bad[12];
        std::memcpy(bad, A, sizeof bad);
        bad[11] = (double)nan;
        EXPECT(backproject_arguments(W, H, 1, proj, bad, dims, 0, 2, 1.0, vol.data(), true));
        EXPECT(backproject_arguments(W, H, 1, proj, bad, dims, 0, 2, 1.0, vol.data(), false) == nullptr);
        std::vector<float> both(16, 0.0f);
        EXPECT(backproject_arguments(W, H, 1, both.data(), A, dims, 0, 2, 1.0, both.data() + 3, true));      // overlap
        EXPECT(backproject_arguments(W, H, 1, both.data(), A, dims, 1, 1, 1.0, both.data() + 3, true) == nullptr);
    }

    // the helpers
    {
        std::vector<float> t(2u * XRT_MAX_RAMP_WIDTH - 1u);
        EXPECT(xrt_ramp_filter((uint32_t)t.size(), XRT_RAMP_RAMLAK, t.data()) == XRT_OK);
        EXPECT(t[XRT_MAX_RAMP_WIDTH - 1u] == 0.25f && t[XRT_MAX_RAMP_WIDTH + 1u] == 0.0f && t[XRT_MAX_RAMP_WIDTH] < 0.0f);
        EXPECT(xrt_ramp_filter((uint32_t)t.size(), XRT_RAMP_HANN, t.data()) == XRT_OK);
        float one[1];
        EXPECT(xrt_ramp_filter(1, XRT_RAMP_HANN, one) == XRT_OK && one[0] > 0.0f && one[0] < 0.25f);
        EXPECT(xrt_ramp_filter(0, 0, one) == XRT_ERR_ARGUMENT && xrt_ramp_filter(2, 0, t.data()) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_ramp_filter(3, 2, t.data()) == XRT_ERR_ARGUMENT && xrt_ramp_filter(3, 0, nullptr) == XRT_ERR_ARGUMENT);
        EXPECT(xrt_ramp_filter(2u * XRT_MAX_RAMP_WIDTH + 1u, 0, t.data()) == XRT_ERR_ARGUMENT);

        xrt_camera c = camera(0.7, 7, 13);
        std::vector<float> w(7 * 13, -7.0f);
        EXPECT(xrt_fdk_weights(&c, w.data()) == XRT_OK);
        for (float v : w) EXPECT(v > 0.9f && v <= 1.0f);
        EXPECT(std::fabs(w[6 * 7 + 3] - 1.0f) < 1e-6f);                                 // the central pixel of an odd detector
        EXPECT(xrt_fdk_weights(nullptr, w.data()) == XRT_ERR_ARGUMENT && xrt_fdk_weights(&c, nullptr) == XRT_ERR_ARGUMENT);
        const float axis_point[3] = {0.0f, 0.0f, 5.0f};
        double s = 0.0;
        EXPECT(xrt_fdk_scale(&c, axis_point, 36, &s) == XRT_OK);
        EXPECT(std::fabs(s - 3.14159265358979323846 / 36.0 * (100.0 / 150.0) / 0.4) < 1e-6);
        EXPECT(xrt_fdk_scale(&c, axis_point, 0, &s) == XRT_ERR_ARGUMENT && xrt_fdk_scale(&c, nullptr, 3, &s) == XRT_ERR_ARGUMENT);
        const float origin[3] = {-1.0f, -1.0f, -1.0f}, spacing[3] = {0.5f, 0.5f, 0.5f};
        const float pose[12] = {0, -1, 0, 0.5f, 1, 0, 0, 0, 0, 0, 1, 0};
        double A[12];
        EXPECT(xrt_backprojection_matrix(&c, pose, origin, spacing, A) == XRT_OK);
        EXPECT(xrt_backprojection_matrix(&c, nullptr, origin, nullptr, A) == XRT_ERR_ARGUMENT);
        xrt_camera flat = c;
        for (int a = 0; a < 3; ++a) flat.up[a] = flat.right[a];          // a singular M
        EXPECT(xrt_backprojection_matrix(&flat, nullptr, origin, spacing, A) == XRT_ERR_ARGUMENT);
        flat = c;
        flat.pixel_spacing = 0.0f;                                      // a result that is not finite
        EXPECT(xrt_backprojection_matrix(&flat, nullptr, origin, spacing, A) == XRT_ERR_ARGUMENT);
        flat = c;
        flat.origin[1] = nan;
        EXPECT(xrt_backprojection_matrix(&flat, nullptr, origin, spacing, A) == XRT_ERR_ARGUMENT);
    }

    if (failures) {
        std::printf("fdk_san: %d failures\n", failures);
        return 1;
    }
    std::printf("fdk_san: OK\n");
    return 0;
}
