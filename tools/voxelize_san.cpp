// voxelize_san.cpp -- the voxeliser's host code (the argument checks of
// xrt_voxelize and the crossing, footprint and voxel functions over whole
// buffers, xrt_host_voxelize: simpleraytracing_amd/csrc/xrt_voxel_host.inc over
// kernels/xrt_device.h) over its edge cases, as a stand-alone program for a
// host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/voxelize_san.cpp \
//         -o voxelize_san
//
// Exact-size heap buffers, so that a read or write one element past a buffer is
// seen.  Prints "voxelize_san: OK" and returns 0 when every call returned what
// it should (tests/test_voxelize_cpu.py runs it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_volume_host.inc"
#include "xrt_voxel_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("voxelize_san: line %d: %s\n", __LINE__, #cond);    \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// A closed box of 12 triangles, normals pointing out.
static std::vector<float> box(float x0, float y0, float z0, float x1, float y1, float z1)
{
    const float v[8][3] = {{x0, y0, z0}, {x1, y0, z0}, {x1, y1, z0}, {x0, y1, z0},
                           {x0, y0, z1}, {x1, y0, z1}, {x1, y1, z1}, {x0, y1, z1}};
    const int f[12][3] = {{0, 2, 1}, {0, 3, 2}, {4, 5, 6}, {4, 6, 7}, {0, 1, 5}, {0, 5, 4},
                          {2, 3, 7}, {2, 7, 6}, {1, 2, 6}, {1, 6, 5}, {0, 4, 7}, {0, 7, 3}};
    std::vector<float> s;
    for (const auto& t : f)
        for (int c : t) s.insert(s.end(), v[c], v[c] + 3);
    return s;
}

struct Outputs {
    std::vector<uint16_t> mask;
    std::vector<uint8_t> labels;
    std::vector<float> volume;
    std::vector<uint64_t> odd;
    explicit Outputs(const uint32_t dims[3])
        : mask((size_t)dims[0] * dims[1] * dims[2]), labels(mask.size()), volume(mask.size()), odd(XRT_MAX_MESHES)
    {
    }
};

// Two boxes, the second inside the first, on a grid that holds both: every voxel against the boxes' bounds.
static void nested_boxes()
{
    std::vector<float> soup = box(-1.0f, -1.5f, -0.5f, 2.0f, 1.0f, 1.75f), inner = box(0.1f, -0.4f, 0.2f, 1.3f, 0.6f, 1.1f);
    soup.insert(soup.end(), inner.begin(), inner.end());
    const uint64_t counts[2] = {12, 12};
    const uint32_t dims[3] = {13, 11, 9};
    const float origin[3] = {-1.6f, -2.0f, -0.9f}, spacing[3] = {0.31f, 0.33f, 0.35f}, value[2] = {0.25f, 1.5f};
    Outputs o(dims);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 2, dims, origin, spacing, value, o.mask.data(), o.labels.data(),
                             o.volume.data(), o.odd.data()) == XRT_OK);
    for (uint64_t c : o.odd) EXPECT(c == 0);
    for (uint32_t k = 0; k < dims[2]; ++k)
        for (uint32_t j = 0; j < dims[1]; ++j)
            for (uint32_t i = 0; i < dims[0]; ++i) {
                const double x = XRT_KERNEL_NS::voxel_centre(origin[0], spacing[0], i);
                const double y = XRT_KERNEL_NS::voxel_centre(origin[1], spacing[1], j);
                const double z = XRT_KERNEL_NS::voxel_centre(origin[2], spacing[2], k);
                const bool a = x > -1.0 && x < 2.0 && y > -1.5 && y < 1.0 && z > -0.5 && z < 1.75;
                const bool b = x > (double)0.1f && x < (double)1.3f && y > (double)-0.4f && y < (double)0.6f &&
                               z > (double)0.2f && z < (double)1.1f;
                const size_t e = ((size_t)k * dims[1] + j) * dims[0] + i;
                EXPECT(o.mask[e] == (uint16_t)((a ? 1 : 0) | (b ? 2 : 0)));
                EXPECT(o.labels[e] == (b ? 2 : a ? 1 : 0));
                EXPECT(o.volume[e] == (float)((a ? 0.25 : 0.0) + (b ? 1.5 : 0.0)));
            }
}

// Grids that cut the box, a one-voxel grid, triangles far larger than the grid and far outside it, one output at a time.
static void edges()
{
    const std::vector<float> soup = box(-1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f);
    const uint64_t counts[1] = {12};
    {
        const uint32_t dims[3] = {5, 7, 3};                          // the box's corner: crossings below slice 0 and in plane nz
        const float origin[3] = {0.2f, -1.7f, -0.3f}, spacing[3] = {0.4f, 0.3f, 0.2f};
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, spacing, nullptr, o.mask.data(), nullptr, nullptr,
                                 o.odd.data()) == XRT_OK);
        EXPECT(o.odd[0] == 0);
        size_t inside = 0;
        for (uint16_t m : o.mask) inside += m;
        EXPECT(inside == 2u * 5u * 3u);                              // x < 1: two columns; y in (-1, 1): five rows (centres -0.95 ... 0.25); all z
    }
    {
        const uint32_t dims[3] = {1, 1, 1};
        const float origin[3] = {-0.5f, -0.5f, -0.5f}, spacing[3] = {1.0f, 1.0f, 1.0f};
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, spacing, nullptr, nullptr, o.labels.data(), nullptr,
                                 nullptr) == XRT_OK);
        EXPECT(o.labels[0] == 1);
    }
    {
        const uint32_t dims[3] = {6, 4, 5};                          // the grid deep inside a huge box, and far outside a tiny one
        const float origin[3] = {-0.3f, -0.2f, -0.25f}, spacing[3] = {0.1f, 0.1f, 0.1f}, value[1] = {3.0f};
        const std::vector<float> huge = box(-1e30f, -1e30f, -1e30f, 1e30f, 1e30f, 1e30f);
        const std::vector<float> tiny = box(1e-30f, 1e-30f, 1e-30f, 2e-30f, 2e-30f, 2e-30f);
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(huge.data(), counts, 1, dims, origin, spacing, value, nullptr, nullptr, o.volume.data(),
                                 o.odd.data()) == XRT_OK);
        EXPECT(o.odd[0] == 0);
        for (float v : o.volume) EXPECT(v == 3.0f);
        EXPECT(xrt_host_voxelize(tiny.data(), counts, 1, dims, origin, spacing, value, o.mask.data(), nullptr, nullptr,
                                 nullptr) == XRT_OK);
        for (uint16_t m : o.mask) EXPECT(m == 0);
    }
}

// An open soup, degenerate triangles, empty meshes and sixteen meshes.
static void odd_and_degenerate()
{
    const uint32_t dims[3] = {8, 8, 4};
    const float origin[3] = {0.0f, 0.0f, 0.0f}, spacing[3] = {0.25f, 0.25f, 0.5f};
    {
        const float tri[9] = {0.1f, 0.2f, 0.3f, 1.9f, 0.4f, 1.1f, 0.9f, 1.8f, 1.9f};
        const uint64_t counts[1] = {1};
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(tri, counts, 1, dims, origin, spacing, nullptr, o.mask.data(), nullptr, nullptr, o.odd.data()) ==
               XRT_OK);
        EXPECT(o.odd[0] > 0);
    }
    {
        const float soup[27] = {1, 1, 1, 1, 1, 1, 1, 1, 1,                      // a point
                                0.5f, 1.0f, 0.0f, 1.5f, 1.0f, 0.0f, 1.0f, 1.0f, 2.0f,   // edge-on: n.z == 0
                                0.25f, 0.25f, 0.25f, 0.75f, 0.75f, 0.75f, 1.25f, 1.25f, 1.25f};   // collinear
        const uint64_t counts[3] = {0, 3, 0};
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(soup, counts, 3, dims, origin, spacing, nullptr, o.mask.data(), o.labels.data(), nullptr,
                                 o.odd.data()) == XRT_OK);
        for (uint16_t m : o.mask) EXPECT(m == 0);
        for (uint64_t c : o.odd) EXPECT(c == 0);
    }
    {
        std::vector<float> soup;
        uint64_t counts[XRT_MAX_MESHES];
        float value[XRT_MAX_MESHES];
        for (uint32_t m = 0; m < XRT_MAX_MESHES; ++m) {
            const std::vector<float> b = box(0.05f * m, 0.05f * m, 0.05f * m, 1.0f + 0.05f * m, 1.0f + 0.05f * m, 1.0f + 0.05f * m);
            soup.insert(soup.end(), b.begin(), b.end());
            counts[m] = 12;
            value[m] = 1.0f;
        }
        Outputs o(dims);
        EXPECT(xrt_host_voxelize(soup.data(), counts, XRT_MAX_MESHES, dims, origin, spacing, value, o.mask.data(),
                                 o.labels.data(), o.volume.data(), o.odd.data()) == XRT_OK);
        bool top = false;
        for (size_t e = 0; e < o.mask.size(); ++e) {
            top = top || (o.mask[e] & 0x8000u);
            EXPECT((o.labels[e] == 16) == ((o.mask[e] & 0x8000u) != 0));
            EXPECT(o.volume[e] == (float)__builtin_popcount(o.mask[e]));
        }
        EXPECT(top);
    }
}

static void refusals()
{
    const std::vector<float> soup = box(-1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f);
    const uint64_t counts[1] = {12};
    const uint32_t dims[3] = {4, 4, 4}, zero[3] = {4, 0, 4}, large[3] = {4, 4, 2049};
    const float origin[3] = {-2.0f, -2.0f, -2.0f}, spacing[3] = {1.0f, 1.0f, 1.0f}, value[1] = {1.0f};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad_spacing[3] = {1.0f, 0.0f, 1.0f}, nan_spacing[3] = {1.0f, 1.0f, nan}, inf_origin[3] = {inf, 0.0f, 0.0f};
    const float far_origin[3] = {3.4e38f, 0.0f, 0.0f}, far_spacing[3] = {1e37f, 1.0f, 1.0f};    // the far corner overflows f32
    Outputs o(dims);
    uint16_t* mask = o.mask.data();
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, nullptr, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, nullptr, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, nullptr, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, zero, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, large, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, bad_spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, nan_spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, inf_origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, far_origin, far_spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, spacing, value, nullptr, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 1, dims, origin, spacing, nullptr, nullptr, nullptr, o.volume.data(), nullptr) ==
           XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(nullptr, counts, 1, dims, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), nullptr, 1, dims, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, 0, dims, origin, spacing, value, mask, nullptr, nullptr, nullptr) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_host_voxelize(soup.data(), counts, XRT_MAX_MESHES + 1, dims, origin, spacing, value, mask, nullptr, nullptr, nullptr) ==
           XRT_ERR_ARGUMENT);
    EXPECT(voxelize_arguments(dims, origin, spacing, nullptr, nullptr, nullptr, o.volume.data(), nullptr).find("value") !=
           std::string::npos);
    EXPECT(voxelize_arguments(dims, origin, spacing, value, nullptr, nullptr, nullptr, nullptr).find("no output") !=
           std::string::npos);
    EXPECT(voxelize_arguments(zero, origin, spacing, value, mask, nullptr, nullptr, nullptr).find("dims[y]") != std::string::npos);
}

int main()
{
    nested_boxes();
    edges();
    odd_and_degenerate();
    refusals();
    if (failures) {
        std::printf("voxelize_san: %d failures\n", failures);
        return 1;
    }
    std::printf("voxelize_san: OK\n");
    return 0;
}
