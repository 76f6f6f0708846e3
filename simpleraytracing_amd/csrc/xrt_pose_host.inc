// xrt_pose_host.inc -- the host arithmetic of the mesh poses (include/xrt.h:
// xrt_pose_rotation, xrt_pose_triangles), included by xrt_abi.hip inside its
// extern "C" block.  Self-contained over kernels/xrt_device.h's pose_vertex,
// <cmath> and <cstring>, so that a stand-alone program can compile it under a
// host sanitizer (tools/pose_san.cpp).

int xrt_pose_rotation(const float axis[3], double degrees, const float centre[3], float pose[12])
{
    if (!axis || !centre || !pose) return XRT_ERR_ARGUMENT;
    // Rodrigues in f64 about the normalised axis, t = c - R c in f64, each rounded once
    const double ax = axis[0], ay = axis[1], az = axis[2];
    const double len = std::sqrt(ax * ax + ay * ay + az * az);
    if (!std::isfinite(len) || !(len > 0.0) || !std::isfinite(degrees)) return XRT_ERR_ARGUMENT;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(centre[k])) return XRT_ERR_ARGUMENT;
    const double u[3] = {ax / len, ay / len, az / len};
    const double a = degrees * (3.14159265358979323846 / 180.0);
    const double c = std::cos(a), s = std::sin(a), k1 = 1.0 - c;
    const double R[3][3] = {
        {c + u[0] * u[0] * k1, u[0] * u[1] * k1 - u[2] * s, u[0] * u[2] * k1 + u[1] * s},
        {u[1] * u[0] * k1 + u[2] * s, c + u[1] * u[1] * k1, u[1] * u[2] * k1 - u[0] * s},
        {u[2] * u[0] * k1 - u[1] * s, u[2] * u[1] * k1 + u[0] * s, c + u[2] * u[2] * k1}};
    for (int i = 0; i < 3; ++i) {
        const double Rc = (R[i][0] * (double)centre[0] + R[i][1] * (double)centre[1]) + R[i][2] * (double)centre[2];
        for (int j = 0; j < 3; ++j) pose[4 * i + j] = (float)R[i][j];
        pose[4 * i + 3] = (float)((double)centre[i] - Rc);
    }
    return XRT_OK;
}

int xrt_pose_triangles(const float* tris, uint64_t n, const float pose[12], float* out)
{
    if ((n && (!tris || !out)) || !pose) return XRT_ERR_ARGUMENT;
    static const float rest[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float q[12];
    std::memcpy(q, pose, sizeof q);
    const bool identity = std::memcmp(q, rest, sizeof q) == 0;    // bit for bit: the rest vertices as they are
    for (uint64_t v = 0; v < 3 * n; ++v) {
        const float x = tris[3 * v], y = tris[3 * v + 1], z = tris[3 * v + 2];
        float ox = x, oy = y, oz = z;
        if (!identity) XRT_KERNEL_NS::pose_vertex(q, x, y, z, ox, oy, oz);
        out[3 * v] = ox;
        out[3 * v + 1] = oy;
        out[3 * v + 2] = oz;
    }
    return XRT_OK;
}
