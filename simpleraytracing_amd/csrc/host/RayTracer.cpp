// RayTracer.cpp -- see RayTracer.h.
#include "RayTracer.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "PlyLoader.h"
#include "xrt.h"
#include "xrt_host.h"

namespace {

int g_kernel = -1;
int g_device = -1;
std::vector<std::array<float, 12>> g_poses;   // setMeshPoses (empty: every mesh at rest)
unsigned g_volume_labels = 0;                 // uploadVolume's label count (renderLoopVolumePaths' planes)

int kernel_choice()
{
    if (g_kernel >= 0) return g_kernel;
    const char* k = std::getenv("XRT_KERNEL");
    if (k && std::strcmp(k, "brute") == 0) return XRT_KERNEL_BRUTE;
    if (k && std::strcmp(k, "tiled") == 0) return XRT_KERNEL_TILED;
    if (k && std::strcmp(k, "binned") == 0) return XRT_KERNEL_BINNED;
    return XRT_KERNEL_AUTO;
}

int device_choice()
{
    if (g_device >= 0) return g_device;
    const char* d = std::getenv("XRT_DEVICE");
    return d ? std::atoi(d) : 0;
}

void check(xrt_context* ctx, int rc, const char* what)
{
    if (rc != XRT_OK)
        throw std::runtime_error(std::string(what) + ": " + xrt_last_error(ctx));
}

// setMeshPoses' poses onto the context's scene: the first `uploaded` of the
// scene's `scene_meshes` meshes are on the device (the attenuation and signed
// models upload mesh 0 only).  A pose the context already has costs nothing.
void apply_poses(xrt_context* ctx, size_t scene_meshes, size_t uploaded)
{
    if (g_poses.empty()) {
        check(ctx, xrt_reset_poses(ctx), "xrt_reset_poses");
        return;
    }
    if (g_poses.size() != scene_meshes) throw std::invalid_argument("setMeshPoses: one pose per mesh of the scene");
    for (size_t m = 0; m < uploaded && m < scene_meshes; ++m)
        check(ctx, xrt_set_pose(ctx, (uint32_t)m, g_poses[m].data()), "xrt_set_pose");
}

}  // namespace

// One context per device for the process lifetime (contexts are not
// thread-safe, so each is guarded by its own mutex).  Contexts are released by
// process exit, not by static destructors that could run after the HIP
// runtime has been torn down.
struct DeviceSlot {
    std::mutex lock;
    xrt_context* ctx = nullptr;
    std::vector<float> mesh;   // the soup last uploaded (renders of the same mesh skip the upload)
    bool uploaded = false;
};

static DeviceSlot& device_slot(int device)
{
    static std::mutex registry_lock;
    static std::map<int, std::unique_ptr<DeviceSlot>> slots;
    std::lock_guard<std::mutex> g(registry_lock);
    auto& slot = slots[device];
    if (!slot) slot.reset(new DeviceSlot());
    if (!slot->ctx) {
        xrt_context* ctx = nullptr;
        int rc = xrt_create(device, &ctx);
        if (rc != XRT_OK) throw std::runtime_error(std::string("xrt_create: ") + xrt_last_error(nullptr));
        slot->ctx = ctx;
    }
    return *slot;
}

xrt_context* xrt_host_device_context(int device) { return device_slot(device).ctx; }

void setRenderKernel(int kernel) { g_kernel = kernel; }
void setRenderDevice(int device) { g_device = device; }
void setMeshPoses(const std::vector<std::array<float, 12>>& poses) { g_poses = poses; }

// Assimp-free loadMeshes (main.cxx:455-508): each mesh of the file through
// TriangleMesh::setGeometry(vertices, indices), in file order.
void appendMeshes(const std::string& file_name, std::vector<TriangleMesh>& meshes)
{
    const std::string ext = file_name.size() >= 4 ? file_name.substr(file_name.size() - 4) : "";
    std::vector<PlyMesh> parts;
    if (ext == ".obj" || ext == ".OBJ") parts = loadObj(file_name);
    else parts.push_back(loadPly(file_name));
    for (const PlyMesh& part : parts) {
        TriangleMesh mesh;
        mesh.setGeometry(part.vertices, part.indices);
        meshes.push_back(mesh);
    }
}

void loadMeshes(const std::string& file_name, std::vector<TriangleMesh>& meshes)
{
    std::vector<TriangleMesh> loaded;
    appendMeshes(file_name, loaded);
    meshes.swap(loaded);
}

// main.cxx:538-563
void getBBox(const std::vector<TriangleMesh>& meshes, Vec3& upper, Vec3& lower)
{
    const float inf = std::numeric_limits<float>::infinity();
    lower = Vec3(inf, inf, inf);
    upper = Vec3(-inf, -inf, -inf);
    for (const TriangleMesh& m : meshes) {
        for (unsigned k = 0; k < 3; ++k) {
            lower[k] = std::min(lower[k], m.getLowerBBoxCorner()[k]);
            upper[k] = std::max(upper[k], m.getUpperBBoxCorner()[k]);
        }
    }
}

// The box of the posed scene: every mesh's vertices under its pose (xrt_pose_triangles).
void getPosedBBox(const std::vector<TriangleMesh>& meshes, const std::vector<std::array<float, 12>>& poses,
                  Vec3& upper, Vec3& lower)
{
    if (!poses.empty() && poses.size() != meshes.size())
        throw std::invalid_argument("getPosedBBox: one pose per mesh of the scene");
    const float inf = std::numeric_limits<float>::infinity();
    lower = Vec3(inf, inf, inf);
    upper = Vec3(-inf, -inf, -inf);
    for (size_t m = 0; m < meshes.size(); ++m) {
        std::vector<float> soup = meshes[m].flatten();
        if (!poses.empty() && xrt_pose_triangles(soup.data(), soup.size() / 9, poses[m].data(), soup.data()) != XRT_OK)
            throw std::runtime_error("getPosedBBox: xrt_pose_triangles");
        float lo[3], hi[3];
        xrt_mesh_bbox(soup.data(), soup.size() / 9, lo, hi);
        for (unsigned k = 0; k < 3; ++k) {
            lower[k] = std::min(lower[k], lo[k]);
            upper[k] = std::max(upper[k], hi[k]);
        }
    }
}

// main.cxx:566-622; the arithmetic is xrt_camera_from_bbox's.
RayTracerInfo initialiseRayTracing(std::vector<TriangleMesh>&, const Vec3& upper, const Vec3& lower,
                                   unsigned int image_height, unsigned int image_width,
                                   Image& output_image, float lut)
{
    float lo[3] = {lower[0], lower[1], lower[2]};
    float hi[3] = {upper[0], upper[1], upper[2]};
    xrt_camera cam;
    if (xrt_camera_from_bbox(lo, hi, image_width, image_height, &cam) != XRT_OK)
        throw std::runtime_error("initialiseRayTracing: invalid image size or bounding box");
    output_image = Image(image_width, image_height, lut);
    RayTracerInfo info;
    info.detector_position = Vec3(cam.detector[0], cam.detector[1], cam.detector[2]);
    info.origin = Vec3(cam.origin[0], cam.origin[1], cam.origin[2]);
    info.up = Vec3(cam.up[0], cam.up[1], cam.up[2]);
    info.right = Vec3(cam.right[0], cam.right[1], cam.right[2]);
    // main.cxx:598-601: a white light at the source, pointing at the box centre
    const Vec3 range = upper - lower;
    Vec3 light_direction = (lower + range / 2.0) - info.origin;
    light_direction.normalise();
    info.light = Light(Vec3(1.0f, 1.0f, 1.0f), light_direction, info.origin);
    info.upper_bbox_corner = upper;
    info.lower_bbox_corner = lower;
    info.range = range;
    return info;
}

namespace {

// Camera for a render: RayTracerInfo + the pixel spacing of renderLoop's
// prologue (main.cxx:634-641), from the bbox of all meshes.
// (range: the box's; null: the meshes' own, as renderLoop forms it)
xrt_camera camera_for(const Image& image, const std::vector<TriangleMesh>& meshes,
                      const RayTracerInfo& info, const Vec3* info_range = nullptr)
{
    Vec3 upper, lower;
    if (!info_range) getBBox(meshes, upper, lower);
    Vec3 range = info_range ? *info_range : upper - lower;
    float res1 = range[2] / image.getWidth();
    float res2 = range[1] / image.getHeight();
    xrt_camera cam;
    for (unsigned k = 0; k < 3; ++k) {
        cam.origin[k] = info.origin[k];
        cam.detector[k] = info.detector_position[k];
        cam.up[k] = info.up[k];
        cam.right[k] = info.right[k];
    }
    cam.pixel_spacing = 2 * std::max(res1, res2);
    cam.width = image.getWidth();
    cam.height = image.getHeight();
    return cam;
}

std::vector<float> mesh0_soup(const std::vector<TriangleMesh>& meshes)
{
    // Only hits on meshes[0] count (main.cxx:687); other meshes cannot change
    // the image, so only mesh 0 is sent to the device.
    return meshes.empty() ? std::vector<float>() : meshes[0].flatten();
}

// What a scene render sends to the device: mesh 0 alone (the attenuation and
// signed models), or every mesh, one soup after another (xrt_upload_scene).
struct SceneSoup {
    std::vector<float> soup;
    std::vector<uint64_t> counts;      // of every mesh's triangles (mesh 0 alone: unused)
    const bool every_mesh;
    const size_t scene_meshes, uploaded;   // apply_poses' pair
    SceneSoup(const std::vector<TriangleMesh>& meshes, bool every_mesh)
        : every_mesh(every_mesh), scene_meshes(meshes.size()), uploaded(every_mesh ? meshes.size() : 1)
    {
        if (!every_mesh) soup = mesh0_soup(meshes);
        else
            for (const TriangleMesh& m : meshes) {
                const std::vector<float> s = m.flatten();
                soup.insert(soup.end(), s.begin(), s.end());
                counts.push_back(s.size() / 9);
            }
    }
};

constexpr bool kMesh0 = false, kEveryMesh = true;            // SceneSoup's every_mesh
constexpr bool kAttenuation = false, kSignedModel = true;    // SceneRender's signed_model

int signed_kernel(int k) { return k == XRT_KERNEL_TILED ? XRT_KERNEL_BINNED : k; }   // they have no TILED variant

// The opening of every scene render on one device, held for its duration: the
// device's context under its slot's lock, the kernel, the scene on the device
// (mesh 0 through the slot's cache, or the whole scene) and setMeshPoses'
// poses.  A render of a signed model (signed_model) then sets its model; the
// destructor puts the context back to XRT_MODEL_ATTENUATION on every exit, a
// throwing check included.
class SceneRender {
    const SceneSoup scene_;             // (built before the lock is taken)
    DeviceSlot& slot_;
    std::lock_guard<std::mutex> lock_;
    const bool signed_model_;

public:
    xrt_context* const ctx;
    SceneRender(const std::vector<TriangleMesh>& meshes, bool every_mesh, bool signed_model)
        : scene_(meshes, every_mesh), slot_(device_slot(device_choice())), lock_(slot_.lock),
          signed_model_(signed_model), ctx(slot_.ctx)
    {
        const int k = kernel_choice();
        check(ctx, xrt_set_kernel(ctx, signed_model ? signed_kernel(k) : k), "xrt_set_kernel");
        if (scene_.every_mesh) {
            slot_.uploaded = false;                        // the slot's cache is of mesh-0 soups
            check(ctx, xrt_upload_scene(ctx, scene_.soup.data(), scene_.counts.data(), (uint32_t)scene_.counts.size()),
                  "xrt_upload_scene");
        } else if (!slot_.uploaded || slot_.mesh != scene_.soup) {   // the mesh lives on the device between renders
            check(ctx, xrt_upload_mesh(ctx, scene_.soup.data(), scene_.soup.size() / 9), "xrt_upload_mesh");
            slot_.mesh = scene_.soup;
            slot_.uploaded = true;
        }
        apply_poses(ctx, scene_.scene_meshes, scene_.uploaded);
    }
    ~SceneRender()
    {
        if (signed_model_) xrt_set_model(ctx, XRT_MODEL_ATTENUATION, 0.0f);
    }
};

void report_odd(unsigned long long odd)
{
    for (unsigned long long i = 0; i < odd; ++i) std::cout << "Only one intersect on this ray" << std::endl;
}

}  // namespace

void renderLoopRows(Image& image, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                    unsigned int row_begin, unsigned int row_end, float* lbuffer_strip,
                    unsigned char* u8_strip, xrt_stats* stats)
{
    if (row_begin > row_end || row_end > image.getHeight())
        throw std::out_of_range("renderLoopRows: row range outside the image");
    xrt_camera cam = camera_for(image, meshes, info);
    SceneRender r(meshes, kMesh0, kAttenuation);
    check(r.ctx, xrt_render_rows(r.ctx, &cam, row_begin, row_end, image.getData() + (size_t)row_begin * image.getWidth(),
                                 lbuffer_strip, u8_strip, stats),
          "xrt_render_rows");
}

double renderLoopFrames(Image& image, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                        unsigned int frames, unsigned int row_begin, unsigned int row_end, xrt_stats* stats)
{
    if (row_begin > row_end || row_end > image.getHeight())
        throw std::out_of_range("renderLoopFrames: row range outside the image");
    xrt_camera cam = camera_for(image, meshes, info);
    SceneRender r(meshes, kMesh0, kAttenuation);
    double ms = 0.0;
    check(r.ctx, xrt_render_frames(r.ctx, &cam, row_begin, row_end, frames,
                                   image.getData() + (size_t)row_begin * image.getWidth(), nullptr, nullptr, stats, &ms),
          "xrt_render_frames");
    return ms;
}

namespace {
thread_local unsigned long long t_last_odd_rays = 0;
}

void renderLoop(Image& image, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info)
{
    xrt_stats stats;
    renderLoopRows(image, meshes, info, 0, image.getHeight(), nullptr, nullptr, &stats);
    report_odd(stats.odd_rays);
    t_last_odd_rays = stats.odd_rays;
}

unsigned long long renderLoopOddRays() { return t_last_odd_rays; }

unsigned long long renderLoopLBuffer(Image& image, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info,
                                     std::vector<float>* lbuffer)
{
    xrt_camera cam = camera_for(image, meshes, info);
    SceneRender r(meshes, kMesh0, kSignedModel);
    check(r.ctx, xrt_set_model(r.ctx, XRT_MODEL_SIGNED, 0.1037f), "xrt_set_model");   // :800
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    check(r.ctx, xrt_render_signed(r.ctx, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
          "xrt_render_signed");
    return stats.odd_rays;
}

unsigned long long renderLoopMaterials(Image& image, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info,
                                       const std::vector<float>& mu, std::vector<float>* lbuffer)
{
    if (mu.size() != meshes.size()) throw std::invalid_argument("renderLoopMaterials: one coefficient per mesh");
    xrt_camera cam = camera_for(image, meshes, info);
    SceneRender r(meshes, kEveryMesh, kSignedModel);
    check(r.ctx, xrt_set_materials(r.ctx, mu.data(), (uint32_t)mu.size()), "xrt_set_materials");
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    check(r.ctx, xrt_render_materials(r.ctx, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
          "xrt_render_materials");
    return stats.odd_rays;
}

unsigned long long renderLoopSpectrum(Image& image, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info,
                                      const std::vector<float>& weight, const std::vector<float>& mu,
                                      std::vector<float>* lbuffer)
{
    if (weight.empty() || mu.size() != meshes.size() * weight.size())
        throw std::invalid_argument("renderLoopSpectrum: one coefficient per mesh and bin");
    xrt_camera cam = camera_for(image, meshes, info);
    SceneRender r(meshes, kEveryMesh, kSignedModel);
    check(r.ctx, xrt_set_spectrum(r.ctx, weight.data(), mu.data(), (uint32_t)meshes.size(), (uint32_t)weight.size()),
          "xrt_set_spectrum");
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    check(r.ctx, xrt_render_spectrum(r.ctx, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
          "xrt_render_spectrum");
    return stats.odd_rays;
}

unsigned long long renderLoopPaths(std::vector<std::vector<float>>& paths, std::vector<unsigned short>& open,
                                   const Image& frame, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info,
                                   bool info_range)
{
    if (meshes.empty() || meshes.size() > XRT_MAX_MESHES)
        throw std::invalid_argument("renderLoopPaths: 1 to XRT_MAX_MESHES meshes");
    xrt_camera cam = camera_for(frame, meshes, info, info_range ? &info.range : nullptr);
    SceneRender r(meshes, kEveryMesh, kSignedModel);
    check(r.ctx, xrt_set_paths(r.ctx), "xrt_set_paths");
    const size_t n = (size_t)frame.getWidth() * frame.getHeight();
    std::vector<float> planes(n * meshes.size());
    open.resize(n);
    xrt_stats stats;
    check(r.ctx, xrt_render_paths(r.ctx, &cam, 0, cam.height, (uint32_t)meshes.size(), planes.data(), open.data(), &stats),
          "xrt_render_paths");
    paths.resize(meshes.size());
    for (size_t m = 0; m < meshes.size(); ++m) paths[m].assign(planes.begin() + m * n, planes.begin() + (m + 1) * n);
    return stats.odd_rays;
}

void getVolumeBBox(const Volume& volume, Vec3& upper, Vec3& lower)
{
    float lo[3], hi[3];
    if (xrt_volume_bbox(volume.dims, volume.origin, volume.spacing, lo, hi) != XRT_OK)
        throw std::invalid_argument("getVolumeBBox: dims of 1 to 2048, a finite origin and spacings above 0");
    lower = Vec3(lo[0], lo[1], lo[2]);
    upper = Vec3(hi[0], hi[1], hi[2]);
}

void uploadVolume(const Volume& volume)
{
    const size_t n = (size_t)volume.dims[0] * volume.dims[1] * volume.dims[2];
    if (volume.labels.size() != n || (!volume.density.empty() && volume.density.size() != n))
        throw std::invalid_argument("uploadVolume: the arrays are not of the volume's dims");
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    g_volume_labels = volume.num_labels;
    check(slot.ctx, xrt_upload_volume(slot.ctx, volume.labels.data(), volume.density.empty() ? nullptr : volume.density.data(),
                                      volume.dims, volume.origin, volume.spacing, volume.num_labels),
          "xrt_upload_volume");
}

unsigned long long voxelizeScene(Volume& volume, const std::vector<TriangleMesh>& meshes, const unsigned dims[3],
                                 const float origin[3], const float spacing[3], const std::vector<float>& value,
                                 std::vector<float>* truth)
{
    if (!dims || !origin || !spacing) throw std::invalid_argument("voxelizeScene: NULL argument");
    if (truth && value.size() != meshes.size()) throw std::invalid_argument("voxelizeScene: one value per mesh");
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    volume = Volume();
    volume.labels.resize(n);
    if (truth) truth->resize(n);
    uint64_t odd[XRT_MAX_MESHES] = {};
    {
        SceneRender r(meshes, kEveryMesh, kAttenuation);
        check(r.ctx, xrt_voxelize(r.ctx, dims, origin, spacing, truth ? value.data() : nullptr, nullptr, volume.labels.data(),
                                  truth ? truth->data() : nullptr, odd),
              "xrt_voxelize");
    }
    for (int a = 0; a < 3; ++a) {
        volume.dims[a] = dims[a];
        volume.origin[a] = origin[a];
        volume.spacing[a] = spacing[a];
    }
    volume.num_labels = (unsigned)meshes.size();
    unsigned long long total = 0;
    for (uint64_t c : odd) total += c;
    return total;
}

void renderLoopVolumePaths(std::vector<std::vector<float>>& planes, const Image& frame, const RayTracerInfo& info)
{
    const xrt_camera cam = camera_for(frame, std::vector<TriangleMesh>(), info, &info.range);
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    const size_t n = (size_t)frame.getWidth() * frame.getHeight(), M = g_volume_labels;
    std::vector<float> all(n * std::max<size_t>(M, 1));
    check(slot.ctx, xrt_volume_paths(slot.ctx, &cam, 0, cam.height, (uint32_t)M, all.data()), "xrt_volume_paths");
    planes.resize(M);
    for (size_t m = 0; m < M; ++m) planes[m].assign(all.begin() + m * n, all.begin() + (m + 1) * n);
}

void applySpectrum(Image& image, const std::vector<std::vector<float>>& paths, const std::vector<unsigned short>& open,
                   const std::vector<float>& weight, const std::vector<float>& mu, std::vector<float>* lbuffer)
{
    const size_t n = (size_t)image.getWidth() * image.getHeight();
    if (weight.empty() || paths.empty() || mu.size() != paths.size() * weight.size())
        throw std::invalid_argument("applySpectrum: one coefficient per mesh and bin");
    if (open.size() != n) throw std::invalid_argument("applySpectrum: the mask is not of the image's size");
    std::vector<float> planes;
    planes.reserve(n * paths.size());
    for (const std::vector<float>& plane : paths) {
        if (plane.size() != n) throw std::invalid_argument("applySpectrum: a plane is not of the image's size");
        planes.insert(planes.end(), plane.begin(), plane.end());
    }
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    std::vector<float> local;
    std::vector<float>& lb = lbuffer ? *lbuffer : local;
    lb.resize(n);
    check(ctx, xrt_apply_spectrum(ctx, n, (uint32_t)paths.size(), planes.data(), open.data(), weight.data(), mu.data(),
                                  (uint32_t)weight.size(), lb.data()), "xrt_apply_spectrum");
    check(ctx, xrt_hole_fill(ctx, image.getWidth(), image.getHeight(), lb.data(), image.getData(), nullptr),
          "xrt_hole_fill");
}

void applySpectralDetector(std::vector<Image>& channels, const std::vector<std::vector<float>>& paths,
                           const std::vector<unsigned short>& open, const std::vector<float>& weight,
                           const std::vector<float>& mu, const std::vector<float>& response, float gain, float read_noise,
                           unsigned long long seed, unsigned long long first_index, bool noisy)
{
    if (channels.empty()) throw std::invalid_argument("applySpectralDetector: no channel images");
    const unsigned width = channels[0].getWidth(), height = channels[0].getHeight();
    const size_t n = (size_t)width * height;
    for (const Image& channel : channels)
        if (channel.getWidth() != width || channel.getHeight() != height)
            throw std::invalid_argument("applySpectralDetector: the channel images differ in size");
    if (weight.empty() || paths.empty() || mu.size() != paths.size() * weight.size())
        throw std::invalid_argument("applySpectralDetector: one coefficient per mesh and bin");
    if (response.size() != channels.size() * weight.size())
        throw std::invalid_argument("applySpectralDetector: one response per channel and bin");
    if (open.size() != n) throw std::invalid_argument("applySpectralDetector: the mask is not of the images' size");
    std::vector<float> planes;
    planes.reserve(n * paths.size());
    for (const std::vector<float>& plane : paths) {
        if (plane.size() != n) throw std::invalid_argument("applySpectralDetector: a plane is not of the images' size");
        planes.insert(planes.end(), plane.begin(), plane.end());
    }
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    std::vector<float> out(n * channels.size());
    check(ctx, xrt_spectral_detector(ctx, n, (uint32_t)paths.size(), planes.data(), open.data(), weight.data(), mu.data(),
                                     (uint32_t)weight.size(), response.data(), (uint32_t)channels.size(), gain,
                                     read_noise, seed, first_index, noisy ? XRT_DETECT_NOISY : XRT_DETECT_EXPECTED,
                                     XRT_DETECT_INTENSITY, out.data()),
          "xrt_spectral_detector");
    for (size_t c = 0; c < channels.size(); ++c)
        check(ctx, xrt_hole_fill(ctx, width, height, out.data() + c * n, channels[c].getData(), nullptr), "xrt_hole_fill");
}

void applyScatter(Image& image, Image& scatter, const std::vector<std::vector<float>>& paths,
                  const std::vector<unsigned short>& open, const std::vector<float>& weight, const std::vector<float>& mu,
                  const ScatterModel& model, std::vector<float>* lbuffer)
{
    const unsigned width = image.getWidth(), height = image.getHeight();
    const size_t n = (size_t)width * height;
    if (scatter.getWidth() != width || scatter.getHeight() != height)
        throw std::invalid_argument("applyScatter: the scatter image is not of the image's size");
    if (weight.empty() || paths.empty() || mu.size() != paths.size() * weight.size())
        throw std::invalid_argument("applyScatter: one coefficient per mesh and bin");
    if (model.sigma.size() != mu.size()) throw std::invalid_argument("applyScatter: one sigma per mesh and bin");
    if (model.kernels.empty() || model.kernels.size() > XRT_MAX_SCATTER_KERNELS)
        throw std::invalid_argument("applyScatter: 1 to XRT_MAX_SCATTER_KERNELS kernels");
    if (model.bin == 0) throw std::invalid_argument("applyScatter: bin is 0");
    if (open.size() != n) throw std::invalid_argument("applyScatter: the mask is not of the image's size");
    std::vector<float> planes;
    planes.reserve(n * paths.size());
    for (const std::vector<float>& plane : paths) {
        if (plane.size() != n) throw std::invalid_argument("applyScatter: a plane is not of the image's size");
        planes.insert(planes.end(), plane.begin(), plane.end());
    }
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    const unsigned wc = (width + model.bin - 1u) / model.bin, hc = (height + model.bin - 1u) / model.bin;
    const size_t nc = (size_t)wc * hc, G = model.kernels.size();
    std::vector<float> local, source(nc), blurred(nc * G), primary(n), amp(G);
    std::vector<float>& lb = lbuffer ? *lbuffer : local;
    lb.resize(n);
    check(ctx, xrt_scatter_source(ctx, width, height, 1, (uint32_t)paths.size(), planes.data(), open.data(), weight.data(),
                                  mu.data(), model.sigma.data(), (uint32_t)weight.size(), model.bin, lb.data(), source.data()),
          "xrt_scatter_source");
    check(ctx, xrt_hole_fill(ctx, width, height, lb.data(), primary.data(), nullptr), "xrt_hole_fill");
    for (size_t k = 0; k < G; ++k) {
        const ScatterKernel& kernel = model.kernels[k];
        amp[k] = kernel.amp;
        check(ctx, xrt_detector_response(ctx, wc, hc, 1, source.data(), kernel.taps_x.data(), (uint32_t)kernel.taps_x.size(),
                                         kernel.taps_y.data(), (uint32_t)kernel.taps_y.size(), blurred.data() + k * nc, nullptr),
              "xrt_detector_response");
    }
    check(ctx, xrt_scatter_add(ctx, width, height, 1, model.bin, blurred.data(), (uint32_t)G, amp.data(), primary.data(),
                               image.getData(), scatter.getData(), nullptr),
          "xrt_scatter_add");
}

unsigned long long decomposeMaterials(std::vector<Image>& basis, const std::vector<Image>& channels,
                                      const std::vector<float>& weight, const std::vector<float>& mu,
                                      const std::vector<float>& response, float gain, unsigned max_iter, double tol,
                                      double damping, bool counts, bool from_guess)
{
    if (channels.empty() || basis.empty()) throw std::invalid_argument("decomposeMaterials: no channel or no basis images");
    const unsigned width = channels[0].getWidth(), height = channels[0].getHeight();
    const size_t n = (size_t)width * height;
    for (const Image& image : channels)
        if (image.getWidth() != width || image.getHeight() != height)
            throw std::invalid_argument("decomposeMaterials: the channel images differ in size");
    for (const Image& image : basis)
        if (image.getWidth() != width || image.getHeight() != height)
            throw std::invalid_argument("decomposeMaterials: a basis image is not of the channels' size");
    if (weight.empty() || mu.size() != basis.size() * weight.size())
        throw std::invalid_argument("decomposeMaterials: one coefficient per basis material and bin");
    if (response.size() != channels.size() * weight.size())
        throw std::invalid_argument("decomposeMaterials: one response per channel and bin");
    const uint32_t B = (uint32_t)basis.size(), C = (uint32_t)channels.size(), K = (uint32_t)weight.size();
    std::vector<float> planes;
    planes.reserve(n * C);
    for (const Image& image : channels) planes.insert(planes.end(), image.getData(), image.getData() + n);
    std::vector<double> guess(from_guess ? (size_t)B * C : 0);
    if (from_guess &&
        xrt_decompose_guess(weight.data(), mu.data(), B, K, response.data(), C, guess.data()) != XRT_OK)
        throw std::runtime_error(std::string("xrt_decompose_guess: ") + xrt_last_error(nullptr));
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    std::vector<float> out(n * B);
    std::vector<uint8_t> iters(n);
    check(ctx, xrt_decompose(ctx, n, planes.data(), nullptr, weight.data(), mu.data(), B, K, response.data(), C, gain,
                             counts ? XRT_DETECT_COUNTS : XRT_DETECT_INTENSITY, from_guess ? guess.data() : nullptr,
                             max_iter, tol, damping, out.data(), iters.data()),
          "xrt_decompose");
    for (uint32_t b = 0; b < B; ++b) std::copy(out.begin() + b * n, out.begin() + (b + 1) * n, basis[b].getData());
    unsigned long long unconverged = 0;
    for (uint8_t it : iters) unconverged += it == XRT_DECOMPOSE_FAILED || it == max_iter;
    return unconverged;
}

void applyDetectorResponse(Image& image, const std::vector<float>& lsf_x, const std::vector<float>& lsf_y)
{
    const size_t n = (size_t)image.getWidth() * image.getHeight();
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    std::vector<float> out(n);
    check(ctx, xrt_detector_response(ctx, image.getWidth(), image.getHeight(), 1, image.getData(), lsf_x.data(),
                                     (uint32_t)lsf_x.size(), lsf_y.data(), (uint32_t)lsf_y.size(), out.data(), nullptr),
          "xrt_detector_response");
    std::copy(out.begin(), out.end(), image.getData());
}

void applyLogProjection(Image& image, float flat_value, float t_min)
{
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    check(ctx, xrt_log_projection(ctx, image.getWidth(), image.getHeight(), 1, image.getData(), nullptr, nullptr,
                                  flat_value, t_min, XRT_ORDER_PROJECTIONS, image.getData()),
          "xrt_log_projection");
}

void applyPhotonNoise(Image& image, float gain, unsigned long long seed, unsigned long long first_index)
{
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    check(ctx, xrt_photon_noise(ctx, image.getWidth(), image.getHeight(), 1, image.getData(), gain, seed, first_index,
                                XRT_NOISE_INTENSITY, image.getData()),
          "xrt_photon_noise");
}

std::vector<RayTracerInfo> focalSpotSources(const RayTracerInfo& info, float size_u, float size_v, unsigned nu, unsigned nv)
{
    xrt_camera cam = {};
    for (unsigned k = 0; k < 3; ++k) {
        cam.origin[k] = info.origin[k];
        cam.detector[k] = info.detector_position[k];
        cam.up[k] = info.up[k];
        cam.right[k] = info.right[k];
    }
    std::vector<xrt_camera> cams((size_t)nu * nv <= XRT_MAX_SOURCES ? (size_t)nu * nv : 0);
    std::vector<float> weight(cams.size());
    if (cams.empty() || xrt_focal_spot(&cam, size_u, size_v, nu, nv, cams.data(), weight.data()) != XRT_OK)
        throw std::runtime_error("focalSpotSources: the sizes must be finite and >= 0, the counts > 0 and nu * nv at most " +
                                 std::to_string(XRT_MAX_SOURCES));
    std::vector<RayTracerInfo> out(cams.size(), info);
    for (size_t s = 0; s < cams.size(); ++s) out[s].origin = Vec3(cams[s].origin[0], cams[s].origin[1], cams[s].origin[2]);
    return out;
}

void applyAreaIntegration(Image& image, const std::vector<Image>& samples, unsigned bin_x, unsigned bin_y,
                          const std::vector<float>& weights)
{
    if (samples.empty() || samples.size() != weights.size())
        throw std::runtime_error("applyAreaIntegration: one weight per sample image, at least one");
    const size_t W = image.getWidth(), H = image.getHeight(), fine = W * bin_x * H * bin_y;
    std::vector<float> stack(fine * samples.size());
    for (size_t s = 0; s < samples.size(); ++s) {
        if (samples[s].getWidth() != W * bin_x || samples[s].getHeight() != H * bin_y)
            throw std::runtime_error("applyAreaIntegration: a sample image is not (width * bin_x) x (height * bin_y)");
        std::copy(samples[s].getData(), samples[s].getData() + fine, stack.begin() + s * fine);
    }
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    check(ctx, xrt_area_integrate(ctx, image.getWidth(), image.getHeight(), bin_x, bin_y, (uint32_t)samples.size(), 1,
                                  weights.data(), stack.data(), image.getData(), nullptr),
          "xrt_area_integrate");
}

void logProjectionSinograms(const std::vector<float>& stack, unsigned width, unsigned height, unsigned num_projections,
                            float flat_value, float t_min, std::vector<float>& sinograms)
{
    if (stack.size() != (size_t)width * height * num_projections)
        throw std::runtime_error("logProjectionSinograms: the stack does not hold num_projections images");
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    sinograms.resize(stack.size());
    check(ctx, xrt_log_projection(ctx, width, height, num_projections, stack.data(), nullptr, nullptr, flat_value, t_min,
                                  XRT_ORDER_SINOGRAMS, sinograms.data()),
          "xrt_log_projection");
}

void reconstructFDK(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                    const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                    const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                    const float spacing[3], const float axis_point[3], int window)
{
    const unsigned W = frame.getWidth(), H = frame.getHeight();
    if (num_projections == 0 || projections.size() != (size_t)W * H * num_projections)
        throw std::runtime_error("reconstructFDK: the stack does not hold num_projections images");
    if (!poses.empty() && poses.size() != num_projections)
        throw std::runtime_error("reconstructFDK: one pose per projection, or none");
    if (W > XRT_MAX_RAMP_WIDTH) throw std::runtime_error("reconstructFDK: the image is wider than XRT_MAX_RAMP_WIDTH");
    const xrt_camera cam = camera_for(frame, meshes, info);
    std::vector<float> weight((size_t)W * H), taps(2u * W - 1u);
    std::vector<double> matrices((size_t)num_projections * 12u);
    double scale = 0.0;
    if (xrt_fdk_weights(&cam, weight.data()) != XRT_OK || xrt_ramp_filter((uint32_t)taps.size(), window, taps.data()) != XRT_OK ||
        xrt_fdk_scale(&cam, axis_point, num_projections, &scale) != XRT_OK)
        throw std::runtime_error("reconstructFDK: the camera is not finite, or the window is not one of XRT_RAMP_*");
    for (unsigned p = 0; p < num_projections; ++p)
        if (xrt_backprojection_matrix(&cam, poses.empty() ? nullptr : poses[p].data(), origin, spacing,
                                      matrices.data() + 12u * p) != XRT_OK)
            throw std::runtime_error("reconstructFDK: the camera's axes are not independent, or the grid is not finite");
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    std::vector<float> filtered(projections.size());
    check(ctx, xrt_fdk_filter(ctx, W, H, num_projections, projections.data(), weight.data(), taps.data(),
                              (uint32_t)taps.size(), filtered.data()),
          "xrt_fdk_filter");
    volume.assign((size_t)dims[0] * dims[1] * dims[2], 0.0f);
    check(ctx, xrt_backproject(ctx, W, H, num_projections, filtered.data(), matrices.data(), dims, 0, dims[2], scale, 0,
                               volume.data()),
          "xrt_backproject");
}

namespace {

// The backprojection matrices of a scan: one per pose, or one at rest.
std::vector<double> scan_matrices(const char* who, const xrt_camera& cam, const std::vector<std::array<float, 12>>& poses,
                                  unsigned count, const float origin[3], const float spacing[3])
{
    std::vector<double> matrices((size_t)count * 12u);
    for (unsigned p = 0; p < count; ++p)
        if (xrt_backprojection_matrix(&cam, poses.empty() ? nullptr : poses[p].data(), origin, spacing,
                                      matrices.data() + 12u * p) != XRT_OK)
            throw std::runtime_error(std::string(who) + ": the camera's axes are not independent, or the grid is not finite");
    return matrices;
}

}  // namespace

void reconstructSIRT(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                     const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets, double relax, float lo, float hi)
{
    reconstructSIRT(volume, projections, num_projections, frame, meshes, info, poses, dims, origin, spacing, iterations,
                    subsets, relax, lo, hi, TVParams());
}

void reconstructSIRT(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                     const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets, double relax, float lo, float hi,
                     const TVParams& tv)
{
    const unsigned W = frame.getWidth(), H = frame.getHeight();
    if (num_projections == 0 || projections.size() != (size_t)W * H * num_projections)
        throw std::runtime_error("reconstructSIRT: the stack does not hold num_projections images");
    if (!poses.empty() && poses.size() != num_projections)
        throw std::runtime_error("reconstructSIRT: one pose per projection, or none");
    const xrt_camera cam = camera_for(frame, meshes, info);
    const std::vector<double> matrices = scan_matrices("reconstructSIRT", cam, poses, num_projections, origin, spacing);
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    if (volume.size() != voxels) volume.assign(voxels, 0.0f);
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    const xrt_tv_params params = {tv.steps, tv.alpha, tv.reduction, tv.eps};
    check(ctx, xrt_sirt_tv(ctx, W, H, num_projections, projections.data(), matrices.data(), dims, spacing, iterations, subsets,
                           relax, lo, hi, tv.steps ? &params : nullptr, volume.data()),
          "xrt_sirt_tv");
}

void reconstructMLTR(std::vector<float>& volume, const std::vector<float>& counts, const std::vector<float>& flat,
                     const std::vector<float>& background, unsigned num_projections, const Image& frame,
                     const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets, double relax, float lo, float hi,
                     const TVParams& tv)
{
    const unsigned W = frame.getWidth(), H = frame.getHeight();
    if (num_projections == 0 || counts.size() != (size_t)W * H * num_projections)
        throw std::runtime_error("reconstructMLTR: the stack does not hold num_projections images");
    if (flat.size() != (size_t)W * H) throw std::runtime_error("reconstructMLTR: the flat field is not one image");
    if (!background.empty() && background.size() != counts.size())
        throw std::runtime_error("reconstructMLTR: one background image per projection, or none");
    if (!poses.empty() && poses.size() != num_projections)
        throw std::runtime_error("reconstructMLTR: one pose per projection, or none");
    const xrt_camera cam = camera_for(frame, meshes, info);
    const std::vector<double> matrices = scan_matrices("reconstructMLTR", cam, poses, num_projections, origin, spacing);
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    if (volume.size() != voxels) volume.assign(voxels, 0.0f);
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    const xrt_tv_params params = {tv.steps, tv.alpha, tv.reduction, tv.eps};
    check(ctx, xrt_mltr(ctx, W, H, num_projections, counts.data(), flat.data(), background.empty() ? nullptr : background.data(),
                        matrices.data(), dims, spacing, iterations, subsets, relax, lo, hi, tv.steps ? &params : nullptr,
                        volume.data()),
          "xrt_mltr");
}

void denoiseTV(std::vector<float>& volume, const unsigned dims[3], unsigned steps, double length, double eps, float lo,
               float hi)
{
    if (volume.size() != (size_t)dims[0] * dims[1] * dims[2])
        throw std::runtime_error("denoiseTV: the volume does not hold dims[0] * dims[1] * dims[2] values");
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    check(ctx, xrt_tv_descend(ctx, volume.data(), dims, eps, steps, length, lo, hi), "xrt_tv_descend");
}

void forwardProject(std::vector<float>& projections, const std::vector<float>& volume, const Image& frame,
                    const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                    const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                    const float spacing[3])
{
    const unsigned W = frame.getWidth(), H = frame.getHeight();
    const unsigned count = poses.empty() ? 1u : (unsigned)poses.size();
    if (volume.size() != (size_t)dims[0] * dims[1] * dims[2])
        throw std::runtime_error("forwardProject: the volume does not hold dims[0] * dims[1] * dims[2] values");
    const xrt_camera cam = camera_for(frame, meshes, info);
    const std::vector<double> matrices = scan_matrices("forwardProject", cam, poses, count, origin, spacing);
    std::vector<double> rays(matrices.size());
    for (unsigned p = 0; p < count; ++p)
        if (xrt_ray_matrix(matrices.data() + 12u * p, rays.data() + 12u * p) != XRT_OK)
            throw std::runtime_error("forwardProject: a projection's matrix has no ray matrix");
    projections.assign((size_t)W * H * count, 0.0f);
    DeviceSlot& slot = device_slot(device_choice());
    std::lock_guard<std::mutex> g(slot.lock);
    xrt_context* ctx = slot.ctx;
    check(ctx, xrt_forward_project(ctx, W, H, count, volume.data(), dims, spacing, rays.data(), XRT_FP_PROJECT, nullptr,
                                   projections.data()),
          "xrt_forward_project");
}

namespace {

// One multi-device context per device list for the process lifetime: the
// devices 0 .. num_gpus-1, or $XRT_MULTI_DEVICES ("0,0" ...; a device listed
// twice rehearses the strip path on one GPU).  Guarded by multi_lock().
std::mutex& multi_lock()
{
    static std::mutex lock;
    return lock;
}

xrt_multi* multi_context(int num_gpus)
{
    std::vector<int> devices;
    if (const char* env = std::getenv("XRT_MULTI_DEVICES")) {
        std::string list(env);
        for (size_t pos = 0; pos < list.size();) {
            size_t next = list.find(',', pos);
            if (next == std::string::npos) next = list.size();
            devices.push_back(std::atoi(list.substr(pos, next - pos).c_str()));
            pos = next + 1;
        }
    } else {
        int available = xrt_device_count();
        if (num_gpus < 1 || num_gpus > available)
            throw std::runtime_error("renderLoopMultiGPU: " + std::to_string(num_gpus) + " GPUs requested, " +
                                     std::to_string(available) + " available");
        for (int g = 0; g < num_gpus; ++g) devices.push_back(g);
    }
    static std::map<std::vector<int>, xrt_multi*> contexts;
    xrt_multi*& m = contexts[devices];
    if (!m && xrt_multi_create(devices.data(), (int)devices.size(), &m) != XRT_OK) {
        m = nullptr;
        throw std::runtime_error(std::string("xrt_multi_create: ") + xrt_multi_last_error(nullptr));
    }
    return m;
}

void mcheck(xrt_multi* m, int rc, const char* what)
{
    if (rc != XRT_OK) throw std::runtime_error(std::string(what) + ": " + xrt_multi_last_error(m));
}

void apply_poses_multi(xrt_multi* m, size_t scene_meshes, size_t uploaded)
{
    if (g_poses.empty()) {
        mcheck(m, xrt_multi_reset_poses(m), "xrt_multi_reset_poses");
        return;
    }
    if (g_poses.size() != scene_meshes) throw std::invalid_argument("setMeshPoses: one pose per mesh of the scene");
    for (size_t k = 0; k < uploaded && k < scene_meshes; ++k)
        mcheck(m, xrt_multi_set_pose(m, (uint32_t)k, g_poses[k].data()), "xrt_multi_set_pose");
}

// SceneRender over the multi-device context of `num_gpus` devices, under
// multi_lock().  A render of the attenuation model sets that model first.
class MultiSceneRender {
    const SceneSoup scene_;
    std::lock_guard<std::mutex> lock_;
    const bool signed_model_;

public:
    xrt_multi* const m;
    MultiSceneRender(int num_gpus, const std::vector<TriangleMesh>& meshes, bool every_mesh, bool signed_model)
        : scene_(meshes, every_mesh), lock_(multi_lock()), signed_model_(signed_model), m(multi_context(num_gpus))
    {
        const int k = kernel_choice();
        if (!signed_model) mcheck(m, xrt_multi_set_model(m, XRT_MODEL_ATTENUATION, 0.0f), "xrt_multi_set_model");
        mcheck(m, xrt_multi_set_kernel(m, signed_model ? signed_kernel(k) : k), "xrt_multi_set_kernel");
        if (scene_.every_mesh)
            mcheck(m, xrt_multi_upload_scene(m, scene_.soup.data(), scene_.counts.data(), (uint32_t)scene_.counts.size()),
                   "xrt_multi_upload_scene");
        else
            mcheck(m, xrt_multi_upload_mesh(m, scene_.soup.data(), scene_.soup.size() / 9), "xrt_multi_upload_mesh");
        apply_poses_multi(m, scene_.scene_meshes, scene_.uploaded);
    }
    ~MultiSceneRender()
    {
        if (signed_model_) xrt_multi_set_model(m, XRT_MODEL_ATTENUATION, 0.0f);
    }
};

}  // namespace

// Row strips over num_gpus devices gathered into device 0 with RCCL
// (xrt_render_rows_multi).
unsigned long long renderLoopMultiGPU(Image& image, const std::vector<TriangleMesh>& meshes,
                                      RayTracerInfo& info, int num_gpus)
{
    xrt_camera cam = camera_for(image, meshes, info);
    MultiSceneRender r(num_gpus, meshes, kMesh0, kAttenuation);
    xrt_stats stats;
    mcheck(r.m, xrt_render_rows_multi(r.m, &cam, image.getData(), nullptr, nullptr, &stats), "xrt_render_rows_multi");
    report_odd(stats.odd_rays);
    return stats.odd_rays;
}

unsigned long long renderLoopLBufferMultiGPU(Image& image, const std::vector<TriangleMesh>& meshes,
                                             RayTracerInfo& info, int num_gpus, std::vector<float>* lbuffer)
{
    xrt_camera cam = camera_for(image, meshes, info);
    MultiSceneRender r(num_gpus, meshes, kMesh0, kSignedModel);
    mcheck(r.m, xrt_multi_set_model(r.m, XRT_MODEL_SIGNED, 0.1037f), "xrt_multi_set_model");   // :800
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    mcheck(r.m, xrt_render_rows_multi(r.m, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
           "xrt_render_rows_multi");
    return stats.odd_rays;
}

unsigned long long renderLoopMaterialsMultiGPU(Image& image, const std::vector<TriangleMesh>& meshes,
                                               RayTracerInfo& info, const std::vector<float>& mu, int num_gpus,
                                               std::vector<float>* lbuffer)
{
    if (mu.size() != meshes.size()) throw std::invalid_argument("renderLoopMaterialsMultiGPU: one coefficient per mesh");
    xrt_camera cam = camera_for(image, meshes, info);
    MultiSceneRender r(num_gpus, meshes, kEveryMesh, kSignedModel);
    mcheck(r.m, xrt_multi_set_materials(r.m, mu.data(), (uint32_t)mu.size()), "xrt_multi_set_materials");
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    mcheck(r.m, xrt_render_rows_multi(r.m, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
           "xrt_render_rows_multi");
    return stats.odd_rays;
}

unsigned long long renderLoopSpectrumMultiGPU(Image& image, const std::vector<TriangleMesh>& meshes,
                                              RayTracerInfo& info, const std::vector<float>& weight,
                                              const std::vector<float>& mu, int num_gpus, std::vector<float>* lbuffer)
{
    if (weight.empty() || mu.size() != meshes.size() * weight.size())
        throw std::invalid_argument("renderLoopSpectrumMultiGPU: one coefficient per mesh and bin");
    xrt_camera cam = camera_for(image, meshes, info);
    MultiSceneRender r(num_gpus, meshes, kEveryMesh, kSignedModel);
    mcheck(r.m, xrt_multi_set_spectrum(r.m, weight.data(), mu.data(), (uint32_t)meshes.size(), (uint32_t)weight.size()),
           "xrt_multi_set_spectrum");
    if (lbuffer) lbuffer->resize((size_t)image.getWidth() * image.getHeight());
    xrt_stats stats;
    mcheck(r.m, xrt_render_rows_multi(r.m, &cam, image.getData(), lbuffer ? lbuffer->data() : nullptr, nullptr, &stats),
           "xrt_render_rows_multi");
    return stats.odd_rays;
}

// --- extern "C" helpers (include/xrt_host.h) --------------------------------
extern "C" int xrt_host_load_ply(const char* path, float** triangles, uint64_t* num_triangles)
{
    if (!path || !triangles || !num_triangles) return XRT_ERR_ARGUMENT;
    *triangles = nullptr;
    *num_triangles = 0;
    try {
        std::vector<TriangleMesh> meshes;
        loadMeshes(path, meshes);
        std::vector<float> soup = mesh0_soup(meshes);
        float* out = static_cast<float*>(std::malloc(sizeof(float) * (soup.size() ? soup.size() : 1)));
        if (!out) return XRT_ERR_ARGUMENT;
        std::memcpy(out, soup.data(), sizeof(float) * soup.size());
        *triangles = out;
        *num_triangles = soup.size() / 9;
        return XRT_OK;
    } catch (const std::exception& e) {
        return std::string(e.what()).find("Cannot open") != std::string::npos ? XRT_ERR_IO : XRT_ERR_FORMAT;
    }
}

extern "C" int xrt_host_load_meshes(const char* path, float** triangles, uint64_t** mesh_triangles,
                                    uint32_t* num_meshes)
{
    if (!path || !triangles || !mesh_triangles || !num_meshes) return XRT_ERR_ARGUMENT;
    *triangles = nullptr;
    *mesh_triangles = nullptr;
    *num_meshes = 0;
    try {
        std::vector<TriangleMesh> meshes;
        loadMeshes(path, meshes);
        std::vector<float> all;
        std::vector<uint64_t> counts;
        for (const TriangleMesh& m : meshes) {
            std::vector<float> soup = m.flatten();
            all.insert(all.end(), soup.begin(), soup.end());
            counts.push_back(soup.size() / 9);
        }
        float* t = static_cast<float*>(std::malloc(sizeof(float) * (all.size() ? all.size() : 1)));
        uint64_t* c = static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * (counts.size() ? counts.size() : 1)));
        if (!t || !c) {
            std::free(t);
            std::free(c);
            return XRT_ERR_ARGUMENT;
        }
        std::memcpy(t, all.data(), sizeof(float) * all.size());
        std::memcpy(c, counts.data(), sizeof(uint64_t) * counts.size());
        *triangles = t;
        *mesh_triangles = c;
        *num_meshes = (uint32_t)counts.size();
        return XRT_OK;
    } catch (const std::exception& e) {
        return std::string(e.what()).find("Cannot open") != std::string::npos ? XRT_ERR_IO : XRT_ERR_FORMAT;
    }
}

extern "C" void xrt_host_free(void* p) { std::free(p); }

namespace {
thread_local std::string t_host_error;
}

extern "C" const char* xrt_host_last_error(void) { return t_host_error.c_str(); }

extern "C" int xrt_host_load_volume(const char* path, void** data, int* element_type, uint32_t dims[3], float origin[3],
                                    float spacing[3])
{
    if (!path || !data || !element_type || !dims || !origin || !spacing) {
        t_host_error = "xrt_host_load_volume: NULL argument";
        return XRT_ERR_ARGUMENT;
    }
    *data = nullptr;
    try {
        const MetaImage img = loadMetaImage(path);
        const bool u8 = !img.u8.empty();
        const size_t bytes = u8 ? img.u8.size() : img.f32.size() * sizeof(float);
        void* out = std::malloc(bytes);
        if (!out) {
            t_host_error = "xrt_host_load_volume: out of memory";
            return XRT_ERR_ARGUMENT;
        }
        std::memcpy(out, u8 ? static_cast<const void*>(img.u8.data()) : static_cast<const void*>(img.f32.data()), bytes);
        *data = out;
        *element_type = u8 ? XRT_VOLUME_U8 : XRT_VOLUME_F32;
        for (int a = 0; a < 3; ++a) {
            dims[a] = img.dims[a];
            origin[a] = img.origin[a];
            spacing[a] = img.spacing[a];
        }
        return XRT_OK;
    } catch (const VolumeError& e) {
        t_host_error = e.what();
        return e.code;
    }
}

extern "C" int xrt_host_save_volume(const char* path, const float* data, const uint32_t dims[3], const float origin[3],
                                    const float spacing[3])
{
    if (!path || !data || !dims || !origin || !spacing) {
        t_host_error = "xrt_host_save_volume: NULL argument";
        return XRT_ERR_ARGUMENT;
    }
    try {
        const unsigned d[3] = {dims[0], dims[1], dims[2]};
        saveVolume(path, d, origin, spacing, data);
        return XRT_OK;
    } catch (const VolumeError& e) {
        t_host_error = e.what();
        return e.code;
    }
}
