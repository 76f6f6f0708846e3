// cull_san.cpp -- the tile cull's host code (make_cull_params, direction_grid
// and the footprints by compute_footprint compiled for the host:
// simpleraytracing_amd/csrc/xrt_cull_host.inc) over general cameras -- rolled,
// pitched, skewed, anisotropic, mirrored, off-centre -- and degenerate ones
// (zero spacing, NaN or infinite components, 1 x 1), as a stand-alone program
// for a host sanitizer build:
//
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/cull_san.cpp \
//         -o cull_san
//
// (the kernels' header brings the kernels along, so their code object is built
// and registered too; only the host code is sanitised, and no kernel is launched.)
//
// Exact-size heap buffers, so that a read or write one element past a buffer is
// seen.  Prints "cull_san: OK" and returns 0 when every call returned what it
// should.  With arguments `time` it instead times make_cull_params
// (microseconds per call) on the same cameras at 2048^2 and 8192^2.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "xrt.h"
#include "kernels/xrt_kernels.h"

using namespace XRT_KERNEL_NS;
#include "xrt_cull_host.inc"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("cull_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct V3 {
    double x, y, z;
};
static V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V3 turn(V3 v, V3 axis, double deg)
{
    const V3 k = (1.0 / std::sqrt(dot(axis, axis))) * axis;
    const double t = deg * 3.14159265358979323846 / 180.0;
    return std::cos(t) * v + std::sin(t) * cross(k, v) + (dot(k, v) * (1.0 - std::cos(t))) * k;
}

struct Case {
    const char* name;
    double yaw, pitch, roll, skew, su, sv, shift_u, shift_v, src_u, src_v;
};
// tests/camera_kit.py's CASES, after the base camera
static const Case kCases[] = {
    {"base", 0, 0, 0, 0, 1, 1, 0, 0, 0, 0},
    {"roll30", 0, 0, 30, 0, 1, 1, 0, 0, 0, 0},
    {"roll45", 0, 0, 45, 0, 1, 1, 0, 0, 0, 0},
    {"roll90", 0, 0, 90, 0, 1, 1, 0, 0, 0, 0},
    {"pitch25", 0, 25, 0, 0, 1, 1, 0, 0, 0, 0},
    {"pitch90", 0, 90, 0, 0, 1, 1, 0, 0, 0, 0},
    {"yaw33_pitch20_roll17", 33, 20, 17, 0, 1, 1, 0, 0, 0, 0},
    {"skew", 0, 0, 10, 0.35, 1, 1, 0, 0, 0, 0},
    {"aniso", 0, 0, -20, 0, 1.5, 0.7, 0, 0, 0, 0},
    {"mirror", 0, 12, 0, 0, -1, 1, 0, 0, 0, 0},
    {"offaxis", 0, 5, 7, 0, 1, 1, 0.3, -0.2, -0.1, 0.15},
    {"all", -40, 15, 63, -0.2, 1.2, 0.9, 0.1, 0.1, 0, 0},
};

// A camera looking along +x at a box of 200 units about (10, -700, 250) (the
// dragon's neighbourhood), turned about the box's centre as
// tests/camera_kit.py's general_camera does.
static xrt_camera make_camera(const Case& c, uint32_t W, uint32_t H)
{
    const V3 centre = {10.0, -700.0, 250.0};
    const double ps = 2.0 * 200.0 / (double)std::max(W, H);
    V3 origin = centre - V3{800.0, 0, 0}, detector = centre + V3{200.0, 0, 0}, up = {0, 0, 1}, right = {0, 1, 0};
    const double degs[3] = {c.yaw, c.pitch, c.roll};
    for (int k = 0; k < 3; ++k) {
        const V3 axis = k == 0 ? up : k == 1 ? right : detector - origin;
        origin = centre + turn(origin - centre, axis, degs[k]);
        detector = centre + turn(detector - centre, axis, degs[k]);
        up = turn(up, axis, degs[k]);
        right = turn(right, axis, degs[k]);
    }
    detector = detector + (c.shift_u * W * ps) * right + (c.shift_v * H * ps) * up;
    origin = origin + (c.src_u * W * ps) * right + (c.src_v * H * ps) * up;
    right = c.su * (right + c.skew * up);
    up = c.sv * up;
    xrt_camera cam;
    const V3 v[4] = {origin, detector, up, right};
    float* dst[4] = {cam.origin, cam.detector, cam.up, cam.right};
    for (int k = 0; k < 4; ++k) {
        dst[k][0] = (float)v[k].x;
        dst[k][1] = (float)v[k].y;
        dst[k][2] = (float)v[k].z;
    }
    cam.pixel_spacing = (float)ps;
    cam.width = W;
    cam.height = H;
    return cam;
}

// Triangles about the centre: ordinary ones, slivers, a zero edge, tiny and huge ones, NaN and inf vertices.
static std::vector<float> make_triangles()
{
    std::vector<float> t;
    uint32_t s = 12345u;
    auto rnd = [&]() {
        s = s * 1664525u + 1013904223u;
        return (double)(s >> 8) / 16777216.0 - 0.5;
    };
    for (int i = 0; i < 400; ++i) {
        const double scale = i % 7 == 0 ? 1e-3 : i % 11 == 0 ? 1e-20 : i % 13 == 0 ? 1e4 : 8.0;
        const double c[3] = {10.0 + 150.0 * rnd(), -700.0 + 150.0 * rnd(), 250.0 + 150.0 * rnd()};
        float p[9];
        for (int k = 0; k < 9; ++k) p[k] = (float)(c[k % 3] + scale * rnd());
        if (i % 17 == 0) for (int k = 0; k < 3; ++k) p[6 + k] = p[k] + 2.0f * (p[3 + k] - p[k]);   // collinear
        if (i % 19 == 0) for (int k = 0; k < 3; ++k) p[3 + k] = p[k];                               // zero edge
        if (i == 33) p[4] = std::numeric_limits<float>::quiet_NaN();
        if (i == 34) p[8] = std::numeric_limits<float>::infinity();
        if (i == 35) p[0] = 3e38f, p[3] = -3e38f;
        t.insert(t.end(), p, p + 9);
    }
    return t;
}

static void check_camera_footprints(const xrt_camera& cam, const std::vector<float>& tris, bool clean, bool sane)
{
    const uint64_t n = tris.size() / 9;
    float* soup = new float[tris.size()];
    float* fp = new float[16 * n];
    std::memcpy(soup, tris.data(), tris.size() * sizeof(float));
    host_footprints(cam, soup, n, fp);
    uint64_t bounded = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float* f = fp + 16 * i;
        if (clean) {
            EXPECT(!std::isnan(f[0]) && !std::isnan(f[1]) && !std::isnan(f[2]) && !std::isnan(f[3]));
            for (int k = 0; k < 3; ++k)
                EXPECT(!std::isnan(f[4 + 4 * k]) && !std::isnan(f[5 + 4 * k]) && !std::isnan(f[6 + 4 * k]));
        }
        if (std::isfinite(f[0]) && std::isfinite(f[1]) && f[0] <= f[1]) ++bounded;
    }
    if (sane) EXPECT(bounded > n / 2);
    host_footprints(cam, soup, 0, fp);
    delete[] soup;
    delete[] fp;
}

static int time_make_cull_params()
{
    for (uint32_t size : {2048u, 8192u})
        for (const Case& c : kCases) {
            const xrt_camera cam = make_camera(c, size, size);
            const int reps = 200000;
            volatile int sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < reps; ++r) {
                xrt_camera q = cam;
                q.origin[0] += (float)(r & 1);              // (not hoisted)
                sink = sink + make_cull_params(q).dir_grid;
            }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            std::printf("make_cull_params %ux%u %-22s %.3f us  dir_grid %d\n", size, size, c.name, us / reps,
                        make_cull_params(cam).dir_grid);
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "time") return time_make_cull_params();
    const float inf = std::numeric_limits<float>::infinity();
    const std::vector<float> tris = make_triangles();

    // --- every case at even, odd, tiny and large sizes: a finite grid below 0, footprints without NaN ---
    const uint32_t sizes[][2] = {{64, 48}, {67, 45}, {1, 1}, {1, 90}, {512, 512}, {8192, 8192}};
    for (const auto& wh : sizes)
        for (const Case& c : kCases) {
            const xrt_camera cam = make_camera(c, wh[0], wh[1]);
            const CullParams cp = make_cull_params(cam);
            EXPECT(cp.dmax > 0.0 && std::isfinite(cp.dmax) && cp.mag > 0.0);
            EXPECT(cp.dir_grid >= -149 && cp.dir_grid < 0);
            EXPECT(direction_grid(cam, cp.dmax, true) <= 0);
            // the magnitudes carried through the mixed branch never put the bound below the grids' own
            for (int k = 0; k < 3; ++k) EXPECT(min_nonzero_x(cam, k) >= 0.0);
            if (wh[0] <= 512) check_camera_footprints(cam, tris, true, wh[0] > 1);
        }

    // --- degenerate cameras: nothing traps, reads or writes out of bounds ---
    {
        const xrt_camera base = make_camera(kCases[11], 67, 45);
        std::vector<xrt_camera> cams;
        xrt_camera c = base;
        c.pixel_spacing = 0.0f;
        cams.push_back(c);
        c = base;
        c.pixel_spacing = -base.pixel_spacing;
        cams.push_back(c);
        c = base;
        c.pixel_spacing = 1e-45f;
        cams.push_back(c);
        for (float bad : {NAN, inf, -inf, 3e38f, 1e-45f, 0.0f})
            for (int field = 0; field < 4; ++field)
                for (int k = 0; k < 3; ++k) {
                    c = base;
                    (field == 0 ? c.origin : field == 1 ? c.detector : field == 2 ? c.up : c.right)[k] = bad;
                    cams.push_back(c);
                }
        c = base;
        for (int k = 0; k < 3; ++k) c.up[k] = c.right[k] = 0.0f;
        cams.push_back(c);
        c = base;
        std::memcpy(c.detector, c.origin, sizeof c.origin);       // detector on the source
        cams.push_back(c);
        c = base;
        c.pixel_spacing = NAN;
        cams.push_back(c);
        c = base;
        c.pixel_spacing = inf;
        cams.push_back(c);
        c = base;
        c.width = c.height = 1;
        cams.push_back(c);
        c = base;
        c.width = 0xFFFFFFFFu;
        c.height = 1;
        cams.push_back(c);
        c = base;
        c.width = 3;
        c.height = 0xFFFFFFFFu;                                    // past the scanned branches' limit
        cams.push_back(c);
        for (const xrt_camera& q : cams) {
            const CullParams cp = make_cull_params(q);
            EXPECT(cp.dir_grid >= -149 && cp.dir_grid <= kNoGrid);
            (void)direction_grid(q, cp.dmax, q.width <= 4096 && q.height <= 4096);
            check_camera_footprints(q, tris, false, false);
        }
    }
    if (!failures) std::printf("cull_san: OK\n");
    return failures ? 1 : 0;
}
