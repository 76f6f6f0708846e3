// xrt_volume_host.inc -- the host pieces of the voxel trace (DESIGN 10.10;
// include/xrt.h: the argument checks of xrt_upload_volume and
// xrt_volume_paths[_device], and xrt_volume_bbox; include/xrt_debug.h:
// xrt_host_volume_paths), included by xrt_abi.hip inside its extern "C" block.
// Self-contained over kernels/xrt_device.h's volume_ray, make_ray, VolumeDesc
// and RenderParams, <cmath>, <string> and <cstdint>, so that a stand-alone
// program can compile it under a host sanitizer (tools/volume_san.cpp).

// What is wrong with a volume's geometry (no device needed), or empty.
static std::string volume_geometry_arguments(const uint32_t* dims, const float* origin, const float* spacing)
{
    static const char axis[3] = {'x', 'y', 'z'};
    if (!dims) return "dims is NULL";
    if (!origin) return "origin is NULL";
    if (!spacing) return "spacing is NULL";
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1u || dims[a] > XRT_KERNEL_NS::kMaxVolumeDim)
            return std::string("dims[") + axis[a] + "] = " + std::to_string(dims[a]) + " is not 1 to 2048";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0f))
            return std::string("spacing[") + axis[a] + "] is not finite and > 0";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) return std::string("origin[") + axis[a] + "] is not finite";
        const float far_corner = (float)XRT_KERNEL_NS::volume_plane((double)origin[a], (double)spacing[a], dims[a]);
        if (!std::isfinite(far_corner)) return std::string("the far corner on ") + axis[a] + " is not finite in f32";
    }
    return std::string();
}

// Every check of a volume's arrays (none needs a device): what is wrong, or empty.
static std::string volume_arguments(const uint8_t* labels, const float* density, const uint32_t* dims,
                                    const float* origin, const float* spacing, uint32_t num_labels)
{
    if (!labels) return "labels is NULL";
    if (num_labels < 1u || num_labels > XRT_MAX_MESHES) return "num_labels is not 1 to XRT_MAX_MESHES";
    std::string why = volume_geometry_arguments(dims, origin, spacing);
    if (!why.empty()) return why;
    const uint64_t nx = dims[0], ny = dims[1], n = nx * ny * dims[2];
    auto voxel = [&](uint64_t i) {
        return "voxel (x " + std::to_string(i % nx) + ", y " + std::to_string(i / nx % ny) + ", z " +
               std::to_string(i / (nx * ny)) + ")";
    };
    for (uint64_t i = 0; i < n; ++i)
        if (labels[i] > num_labels)
            return "label " + std::to_string(labels[i]) + " of " + voxel(i) + " is above num_labels";
    if (density)
        for (uint64_t i = 0; i < n; ++i)
            if (!std::isfinite(density[i])) return "density of " + voxel(i) + " is not finite";
    return std::string();
}

// The checks of a trace's camera, strip and buffer (no context needed); null when they pass.
static const char* volume_trace_arguments(const xrt_camera* cam, uint32_t row_begin, uint32_t row_end,
                                          uint32_t num_labels, const float* paths)
{
    if (!cam) return "camera is NULL";
    if (cam->width == 0 || cam->height == 0) return "image size must be non-zero";
    if (row_begin > row_end || row_end > cam->height) return "row range outside the image height";
    if ((uint64_t)cam->width * cam->height > (1ull << 32) - 1) return "image larger than 2^32-1 pixels";
    if (num_labels < 1u || num_labels > XRT_MAX_MESHES) return "num_labels is not 1 to XRT_MAX_MESHES";
    if (!paths && row_end > row_begin) return "paths is NULL";
    return nullptr;
}

// k_volume_paths' camera and strip.
static XRT_KERNEL_NS::RenderParams volume_params(const xrt_camera& c, uint32_t row_begin, uint32_t row_end)
{
    XRT_KERNEL_NS::RenderParams p = {};
    p.ox = c.origin[0]; p.oy = c.origin[1]; p.oz = c.origin[2];
    p.cx = c.detector[0]; p.cy = c.detector[1]; p.cz = c.detector[2];
    p.ux = c.up[0]; p.uy = c.up[1]; p.uz = c.up[2];
    p.rx = c.right[0]; p.ry = c.right[1]; p.rz = c.right[2];
    p.spacing = c.pixel_spacing;
    p.width = c.width;
    p.height = c.height;
    p.row_begin = row_begin;
    p.row_end = row_end;
    return p;
}

static XRT_KERNEL_NS::VolumeDesc volume_desc(const uint8_t* labels, const float* density, const uint32_t* dims,
                                             const float* origin, const float* spacing, uint32_t num_labels)
{
    XRT_KERNEL_NS::VolumeDesc v = {};
    v.labels = labels;
    v.density = density;
    v.num_labels = num_labels;
    for (int a = 0; a < 3; ++a) {
        v.n[a] = dims[a];
        v.origin[a] = origin[a];
        v.spacing[a] = spacing[a];
    }
    return v;
}

int xrt_volume_bbox(const uint32_t dims[3], const float origin[3], const float spacing[3], float lower[3],
                    float upper[3])
{
    if (!lower || !upper || !volume_geometry_arguments(dims, origin, spacing).empty()) return XRT_ERR_ARGUMENT;
    for (int a = 0; a < 3; ++a) {
        lower[a] = origin[a];
        upper[a] = (float)XRT_KERNEL_NS::volume_plane((double)origin[a], (double)spacing[a], dims[a]);
    }
    return XRT_OK;
}

// The kernel's ray function over whole host buffers with no device (test
// infrastructure: what k_volume_paths is compared with on a machine without
// a device, not a fallback).  Arguments and checks as xrt_upload_volume's and
// xrt_volume_paths'.
int xrt_host_volume_paths(const xrt_camera* camera, uint32_t row_begin, uint32_t row_end, const uint8_t* labels,
                          const float* density, const uint32_t dims[3], const float origin[3], const float spacing[3],
                          uint32_t num_labels, float* paths)
{
    using namespace XRT_KERNEL_NS;
    if (volume_trace_arguments(camera, row_begin, row_end, num_labels, paths)) return XRT_ERR_ARGUMENT;
    if (!volume_arguments(labels, density, dims, origin, spacing, num_labels).empty()) return XRT_ERR_ARGUMENT;
    const RenderParams p = volume_params(*camera, row_begin, row_end);
    const VolumeDesc v = volume_desc(labels, density, dims, origin, spacing, num_labels);
    const size_t plane = (size_t)(row_end - row_begin) * p.width;
    for (uint32_t row = row_begin; row < row_end; ++row)
        for (uint32_t col = 0; col < p.width; ++col) {
            float dx, dy, dz;
            make_ray(p, row, col, dx, dy, dz);
            double acc[kMaxMeshes] = {};
            volume_ray(v, (double)p.ox, (double)p.oy, (double)p.oz, (double)dx, (double)dy, (double)dz,
                       [&](uint32_t m, double run) { acc[m] = acc[m] + run; });
            const size_t pix = (size_t)(row - row_begin) * p.width + col;
            for (uint32_t m = 0; m < num_labels; ++m) paths[m * plane + pix] = (float)acc[m];
        }
    return XRT_OK;
}
