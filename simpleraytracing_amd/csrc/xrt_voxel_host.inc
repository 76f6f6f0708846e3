// xrt_voxel_host.inc -- the host pieces of the voxeliser (DESIGN 10.15;
// include/xrt.h: the argument checks of xrt_voxelize[_device];
// include/xrt_debug.h: xrt_host_voxelize), included by xrt_abi.hip inside its
// extern "C" block after xrt_volume_host.inc, whose volume_geometry_arguments
// checks the grid.  Self-contained over kernels/xrt_device.h's voxel_*
// functions, <string>, <vector> and <cstdint>, so that a stand-alone program
// can compile it under a host sanitizer (tools/voxelize_san.cpp).

// Every check of a voxelisation's arguments (none needs a device): what is wrong, or empty.
static std::string voxelize_arguments(const uint32_t* dims, const float* origin, const float* spacing, const float* value,
                                      const void* mask, const void* labels, const void* volume, const void* odd_columns)
{
    std::string why = volume_geometry_arguments(dims, origin, spacing);
    if (!why.empty()) return why;
    if (!mask && !labels && !volume && !odd_columns) return "no output is given (mask, labels, volume, odd_columns)";
    if (volume && !value) return "volume is given without value";
    return std::string();
}

static XRT_KERNEL_NS::VoxelGrid voxel_grid(const uint32_t* dims, const float* origin, const float* spacing)
{
    XRT_KERNEL_NS::VoxelGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    g.sx = spacing[0]; g.sy = spacing[1]; g.sz = spacing[2];
    return g;
}

// The voxeliser's three steps over host buffers with no device (test
// infrastructure: what the kernels are compared with on a machine without a
// device, not a fallback): the scatter through voxel_footprint and
// voxel_crossing, the scan through voxel_label and voxel_value.  `soup` holds
// the triangles of the num_meshes meshes one after another, as the posed scene
// does; arguments and checks otherwise as xrt_voxelize's.
int xrt_host_voxelize(const float* soup, const uint64_t* mesh_triangles, uint32_t num_meshes, const uint32_t dims[3],
                      const float origin[3], const float spacing[3], const float* value, uint16_t* mask, uint8_t* labels,
                      float* volume, uint64_t* odd_columns)
{
    using namespace XRT_KERNEL_NS;
    if (!mesh_triangles || num_meshes < 1u || num_meshes > XRT_MAX_MESHES) return XRT_ERR_ARGUMENT;
    uint64_t T = 0;
    for (uint32_t m = 0; m < num_meshes; ++m) T += mesh_triangles[m];
    if (T && !soup) return XRT_ERR_ARGUMENT;
    if (!voxelize_arguments(dims, origin, spacing, value, mask, labels, volume, odd_columns).empty()) return XRT_ERR_ARGUMENT;
    const VoxelGrid g = voxel_grid(dims, origin, spacing);
    const uint64_t plane = (uint64_t)g.nx * g.ny;
    std::vector<uint16_t> flip((size_t)(plane * (g.nz + 1u)), (uint16_t)0);
    uint64_t t = 0;
    for (uint32_t m = 0; m < num_meshes; ++m)
        for (const uint64_t end = t + mesh_triangles[m]; t < end; ++t) {
            const VoxelTriangle tri = voxel_triangle(soup + 9u * t);
            const VoxelBox b = voxel_footprint(tri, g);
            for (uint32_t j = b.j0; j < b.j1; ++j)
                for (uint32_t i = b.i0; i < b.i1; ++i) {
                    uint32_t k;
                    if (voxel_crossing(tri, g, voxel_centre(g.ox, g.sx, i), voxel_centre(g.oy, g.sy, j), k))
                        flip[(size_t)voxel_index(g, i, j, k)] ^= (uint16_t)(1u << m);
                }
        }
    if (odd_columns)
        for (uint32_t m = 0; m < XRT_MAX_MESHES; ++m) odd_columns[m] = 0;
    std::vector<uint16_t> run((size_t)plane, (uint16_t)0);    // every column's running XOR, slice after slice
    for (uint32_t k = 0; k < g.nz; ++k)
        for (uint64_t c = 0; c < plane; ++c) {
            const size_t e = (size_t)(k * plane + c);
            const uint32_t acc = run[(size_t)c] ^= flip[e];
            if (mask) mask[e] = (uint16_t)acc;
            if (labels) labels[e] = voxel_label(acc);
            if (volume) volume[e] = voxel_value(acc, num_meshes, [&](uint32_t q) { return value[q]; });
        }
    if (odd_columns)
        for (uint64_t c = 0; c < plane; ++c) {
            const uint32_t total = run[(size_t)c] ^ flip[(size_t)(g.nz * plane + c)];
            for (uint32_t m = 0; m < num_meshes; ++m) odd_columns[m] += total >> m & 1u;
        }
    return XRT_OK;
}
