// pose_san.cpp -- the mesh poses' host arithmetic (xrt_pose_triangles,
// xrt_pose_rotation: simpleraytracing_amd/csrc/xrt_pose_host.inc) over their
// edge cases, as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/pose_san.cpp -o pose_san
//
// Exact-size heap buffers, so that a read or write one float past a soup is
// seen.  Prints "pose_san: OK" and returns 0 when every call returned what it
// should (tests/test_pose_cpu.py runs it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels/xrt_device.h"
#include "xrt.h"

extern "C" {
#include "xrt_pose_host.inc"
}

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("pose_san: line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float rest[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float flip[12] = {1, 0, 0, -0.0f, 0, -1, 0, -0.0f, 0, 0, 1, 0.0f};
    const float move[12] = {0.5f, -2, 3e38f, 1e-42f, 0, 1e-40f, 0, 7, -1, 0, 1, -inf};
    for (unsigned long n : {0ul, 1ul, 2ul, 7ul, 1000ul}) {
        float* in = new float[9 * n + (n ? 0 : 1)];
        float* out = new float[9 * n + (n ? 0 : 1)];
        for (unsigned long k = 0; k < 9 * n; ++k)
            in[k] = k % 11 == 0 ? -0.0f : k % 13 == 0 ? 1e-41f : k % 17 == 0 ? -3e38f : (float)k * 0.37f - 50.0f;
        EXPECT(xrt_pose_triangles(n ? in : nullptr, n, rest, n ? out : nullptr) == XRT_OK);
        EXPECT(n == 0 || std::memcmp(in, out, 9 * n * sizeof(float)) == 0);          // the identity: the input's bits
        EXPECT(xrt_pose_triangles(in, n, flip, out) == XRT_OK);
        EXPECT(xrt_pose_triangles(in, n, move, out) == XRT_OK);
        std::vector<float> want(out, out + 9 * n);
        EXPECT(xrt_pose_triangles(in, n, move, in) == XRT_OK);                       // in place
        EXPECT(n == 0 || std::memcmp(in, want.data(), 9 * n * sizeof(float)) == 0);
        delete[] in;
        delete[] out;
    }
    float one[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    EXPECT(xrt_pose_triangles(nullptr, 1, rest, one) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_triangles(one, 1, nullptr, one) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_triangles(one, 1, rest, nullptr) == XRT_ERR_ARGUMENT);

    float* pose = new float[12];
    const float axes[][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, -2, 3}, {1e-30f, 0, 0}, {3e38f, 3e38f, 3e38f}};
    const float centre[3] = {60.0f, -3.5f, 1e6f};
    for (const auto& axis : axes)
        for (double deg : {0.0, 30.0, 90.0, 180.0, 360.0, -725.5, 1e300}) {
            EXPECT(xrt_pose_rotation(axis, deg, centre, pose) == XRT_OK);
            for (int k = 0; k < 12; ++k) EXPECT(std::isfinite(pose[k]));
        }
    const float zero[3] = {0, 0, 0}, nan_axis[3] = {0, NAN, 1}, inf_axis[3] = {inf, 0, 0};
    EXPECT(xrt_pose_rotation(zero, 10.0, centre, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(nan_axis, 10.0, centre, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(inf_axis, 10.0, centre, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(axes[0], (double)inf, centre, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(nullptr, 10.0, centre, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(axes[0], 10.0, nullptr, pose) == XRT_ERR_ARGUMENT);
    EXPECT(xrt_pose_rotation(axes[0], 10.0, centre, nullptr) == XRT_ERR_ARGUMENT);
    delete[] pose;
    if (!failures) std::printf("pose_san: OK\n");
    return failures ? 1 : 0;
}
