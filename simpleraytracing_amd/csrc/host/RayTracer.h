// RayTracer.h -- scene set-up and the render loop of the drop-in host API.
//
// Same free functions and signatures as the reference's src/main.cxx:
//   loadMeshes           main.cxx:139-140, 427-510
//   getBBox              main.cxx:145-147, 538-563
//   initialiseRayTracing main.cxx:149-157, 566-622
//   renderLoop           main.cxx:159-161, 626-743  -> the GPU, via include/xrt.h
// plus renderLoopRows (a row strip, the pthreads twin's pixel-range idea,
// main-pthreads-redo.cxx:627-658) and renderLoopMultiGPU (row strips over
// several GPUs).  Errors surface as exceptions, as in the reference.
#pragma once

#include <array>
#include <limits>
#include <string>
#include <vector>

#include "Image.h"
#include "Light.h"
#include "Material.h"
#include "TriangleMesh.h"
#include "Vec3.h"
#include "VolumeLoader.h"

struct xrt_stats;

// RayTracerInfo (main.cxx:111-121), member for member.
struct RayTracerInfo {
    Vec3 detector_position;
    Vec3 origin;
    Vec3 up;
    Vec3 right;
    Light light;              // initialiseRayTracing's light (main.cxx:598-601); unused by the X-ray path
    Vec3 upper_bbox_corner;
    Vec3 lower_bbox_corner;
    Vec3 range;
};

// Render options (process-wide): kernel = 0 auto, 1 brute force, 2 tiled cull,
// 3 binned cull.  Defaults come from $XRT_KERNEL ("brute" / "tiled" / "binned")
// and $XRT_DEVICE.
void setRenderKernel(int kernel);
void setRenderDevice(int device);
// Mesh poses (process-wide, as the options above): one row-major 3x4 [R | t]
// per mesh of the scene -- the fork's transformMatrix, per mesh and applied on
// the device (include/xrt.h, xrt_set_pose).  Empty (the default): every mesh at
// rest.  Every renderLoop* honours it; a size other than the scene's mesh count
// throws at render time.
void setMeshPoses(const std::vector<std::array<float, 12>>& poses);

// Every mesh of a file, replacing `meshes` (main.cxx:455-508): a PLY file is
// one mesh, an OBJ file one mesh per object.  appendMeshes keeps the meshes
// already loaded (several input files make one scene; mesh 0 stays first).
void loadMeshes(const std::string& file_name, std::vector<TriangleMesh>& meshes);
void appendMeshes(const std::string& file_name, std::vector<TriangleMesh>& meshes);

void getBBox(const std::vector<TriangleMesh>& meshes, Vec3& upper, Vec3& lower);
// getBBox is the reference's, over the rest meshes; this one is over the
// vertices under `poses` (one per mesh; empty: getBBox's vertices).
void getPosedBBox(const std::vector<TriangleMesh>& meshes, const std::vector<std::array<float, 12>>& poses,
                  Vec3& upper, Vec3& lower);

RayTracerInfo initialiseRayTracing(std::vector<TriangleMesh>& meshes, const Vec3& upper,
                                   const Vec3& lower, unsigned int image_height,
                                   unsigned int image_width, Image& output_image, float lut);

// Whole image (main.cxx:159-161, the reference's declaration); prints one
// "Only one intersect on this ray" line per odd ray (main.cxx:710).
void renderLoop(Image& output_image, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info);

// The number of odd rays of this thread's last renderLoop call (the lines it
// printed).
unsigned long long renderLoopOddRays();

// Rows [row_begin, row_end) of output_image only; optional L-buffer / 8-bit
// outputs of the same strip size.  Does not print.
void renderLoopRows(Image& output_image, const std::vector<TriangleMesh>& meshes,
                    const RayTracerInfo& info, unsigned int row_begin, unsigned int row_end,
                    float* lbuffer_strip, unsigned char* u8_strip, xrt_stats* stats);

// renderLoop's rows [row_begin, row_end) rendered `frames` times back to back
// (one xrt_render_frames call: every frame prepared and rendered in full, the
// host side of all of them in one pass); output_image holds the last frame,
// *stats its counters.  Returns the device time per frame in ms.  Does not print.
double renderLoopFrames(Image& output_image, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                        unsigned int frames, unsigned int row_begin, unsigned int row_end, xrt_stats* stats);

// The L-buffer fork, src/main-pthreads-lbuffer.cxx: renderLoopCallBack over
// the whole image (:733-813, the signed multi-material L-buffer, mesh 0's
// coefficient 0.1037) and main's hole fill (:327-404) into output_image.
// `lbuffer` (optional) receives the fork's L_buffer (-1 flags).  Returns the
// number of flagged pixels.
unsigned long long renderLoopLBuffer(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                     RayTracerInfo& info, std::vector<float>* lbuffer = nullptr);

// The same as row strips over `num_gpus` devices (the L-buffer strips gathered
// to device 0, which fills the holes of the assembled frame).
unsigned long long renderLoopLBufferMultiGPU(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                             RayTracerInfo& info, int num_gpus, std::vector<float>* lbuffer = nullptr);

// The materials model (XRT_MODEL_MATERIALS): the fork's loop over every mesh
// of the scene, mesh m attenuating with mu[m] (one value per mesh), and the
// hole fill into output_image.  `lbuffer` (optional) receives the L-buffer
// (-1 flags).  Returns the number of flagged pixels.  MultiGPU: as row strips.
unsigned long long renderLoopMaterials(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                       RayTracerInfo& info, const std::vector<float>& mu,
                                       std::vector<float>* lbuffer = nullptr);
unsigned long long renderLoopMaterialsMultiGPU(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                               RayTracerInfo& info, const std::vector<float>& mu, int num_gpus,
                                               std::vector<float>* lbuffer = nullptr);

// The spectrum model (XRT_MODEL_SPECTRUM): a polychromatic beam of
// weight.size() energy bins over the same scene, mesh m attenuating in bin e
// with mu[m * weight.size() + e], and the hole fill into output_image (whose
// 8-bit window stays 0..80).  `lbuffer` and the return value as above.
unsigned long long renderLoopSpectrum(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                      RayTracerInfo& info, const std::vector<float>& weight,
                                      const std::vector<float>& mu, std::vector<float>* lbuffer = nullptr);
unsigned long long renderLoopSpectrumMultiGPU(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                              RayTracerInfo& info, const std::vector<float>& weight,
                                              const std::vector<float>& mu, int num_gpus,
                                              std::vector<float>* lbuffer = nullptr);

// The paths model (XRT_MODEL_PATHS): one trace of the scene into per-mesh
// planes of signed path lengths (paths[m], row-major, of frame's size -- only
// its size is read) and a mask plane (bit m: mesh m's signs do not cancel on
// the ray); returns the number of rays with a non-zero mask.  applySpectrum
// integrates such planes under a spectrum table (renderLoopSpectrum's weight
// and mu) and runs the hole fill into output_image: what renderLoopSpectrum
// writes for the same scene, view and table, without tracing again.  One
// device (there is no multi-GPU form yet).
// With info_range the pixel spacing comes from info.range -- the box the camera
// was made for, which may hold more than the meshes (a volume) -- and not from
// the meshes' own box.
unsigned long long renderLoopPaths(std::vector<std::vector<float>>& paths, std::vector<unsigned short>& open,
                                   const Image& frame, const std::vector<TriangleMesh>& meshes, RayTracerInfo& info,
                                   bool info_range = false);
void applySpectrum(Image& output_image, const std::vector<std::vector<float>>& paths,
                   const std::vector<unsigned short>& open, const std::vector<float>& weight,
                   const std::vector<float>& mu, std::vector<float>* lbuffer = nullptr);

// The spectral detector (xrt_spectral_detector, XRT_DETECT_INTENSITY) over such
// planes: per pixel and energy bin a photon count of mean gain * weight *
// exp(-x) -- drawn when `noisy`, from seed, first_index + the pixel's index and
// the bin alone; the mean itself otherwise, and then read_noise must be 0 --,
// summed into channels.size() channels under `response` (one row of
// weight.size() values per channel, one after another), plus read_noise
// (additive Gaussian noise, in counts) a channel, divided by gain.  Every
// channel image must come with the planes' width and height; the hole fill
// runs on each as applySpectrum's does on its image.  Projection p of a scan
// of W x H images passes first_index = p * W * H.  One device.
void applySpectralDetector(std::vector<Image>& channels, const std::vector<std::vector<float>>& paths,
                           const std::vector<unsigned short>& open, const std::vector<float>& weight,
                           const std::vector<float>& mu, const std::vector<float>& response, float gain = 1.0f,
                           float read_noise = 0.0f, unsigned long long seed = 0, unsigned long long first_index = 0,
                           bool noisy = false);

// The scatter model (xrt_scatter_source, xrt_detector_response, xrt_scatter_add;
// DESIGN 10.16): `bin`, the power of two in 1..XRT_MAX_SCATTER_BIN the source is
// binned by; `sigma`, the part of each coefficient that scatters, in mu's
// layout (one row of weight.size() values per plane, one after another); and 1
// to XRT_MAX_SCATTER_KERNELS kernels, each an amplitude and its taps along x
// and y on the binned grid (odd counts, at most XRT_MAX_LSF_TAPS).
// applyScatter is applySpectrum with the estimate added: from such planes the
// source and the L-buffer in one pass, the hole fill of the L-buffer (the
// primary), one blur of the coarse source per kernel, and their weighted sum,
// interpolated back, added to the primary.  output_image receives the total,
// scatter_image -- of the same size -- the scatter alone; lbuffer as
// applySpectrum's.  One device.
struct ScatterKernel {
    float amp = 0.0f;
    std::vector<float> taps_x, taps_y;
};
struct ScatterModel {
    unsigned bin = 1;
    std::vector<float> sigma;
    std::vector<ScatterKernel> kernels;
};
void applyScatter(Image& output_image, Image& scatter_image, const std::vector<std::vector<float>>& paths,
                  const std::vector<unsigned short>& open, const std::vector<float>& weight, const std::vector<float>& mu,
                  const ScatterModel& model, std::vector<float>* lbuffer = nullptr);

// Material decomposition (xrt_decompose), the inverse of
// applySpectralDetector without noise: from the channel images (as
// intensities, the detector's output, unless `counts`) the line integrals of
// basis.size() basis materials under the table (`weight`, and `mu`: one row of
// weight.size() coefficients per basis material, one after another), `response`
// and `gain`, all as the detector took them.  Per pixel at most max_iter
// iterations, until no line integral moves by more than tol, from
// xrt_decompose_guess' start (from_guess) or from zero; damping scales the
// normal matrix's diagonal by 1 + damping.  Every basis image must come with
// the channels' width and height.  Returns the number of pixels that failed
// (XRT_DECOMPOSE_FAILED) or ran max_iter iterations.  One device.
unsigned long long decomposeMaterials(std::vector<Image>& basis, const std::vector<Image>& channels,
                                      const std::vector<float>& weight, const std::vector<float>& mu,
                                      const std::vector<float>& response, float gain = 1.0f, unsigned max_iter = 32,
                                      double tol = 1e-6, double damping = 0.0, bool counts = false, bool from_guess = true);

// Voxel volumes (xrt_upload_volume).  getVolumeBBox: the
// volume's box (xrt_volume_bbox), to pass to initialiseRayTracing alone or in
// union with getBBox's.  uploadVolume: the volume onto the render device,
// replacing any earlier one (it stays there between renders, apart from the
// meshes).  renderLoopVolumePaths: one trace of the uploaded volume into one
// plane per label (planes[L - 1], row-major, of frame's size -- only its size
// is read), the path length of each ray inside label L times the voxels'
// density; the pixel spacing comes from info.range.  Such planes go behind
// renderLoopPaths' in applySpectrum's and applySpectralDetector's `paths`
// (the table's rows: the meshes', then the labels'; the mask is the meshes').
// The volume has no pose: setMeshPoses does not move it.  One device.
void getVolumeBBox(const Volume& volume, Vec3& upper, Vec3& lower);
void uploadVolume(const Volume& volume);
void renderLoopVolumePaths(std::vector<std::vector<float>>& planes, const Image& frame, const RayTracerInfo& info);

// The scene under setMeshPoses' poses voxelised on a grid (xrt_voxelize,
// DESIGN 10.15): volume.labels receives 0 outside every mesh, else 1 + the
// last mesh the voxel's centre lies in, on dims voxels of `spacing` whose
// minimum corner is `origin`, num_labels the scene's mesh count, no density --
// what uploadVolume takes.  With `value` (one entry per mesh) `truth` receives
// the sum of the values of the meshes each voxel lies in, e.g. the scene's
// attenuation volume from --materials' coefficients.  Returns the columns over
// which some mesh does not close (0 for closed meshes).  One device.
unsigned long long voxelizeScene(Volume& volume, const std::vector<TriangleMesh>& meshes, const unsigned dims[3],
                                 const float origin[3], const float spacing[3],
                                 const std::vector<float>& value = std::vector<float>(), std::vector<float>* truth = nullptr);

// The detector response (xrt_detector_response): the image under a separable
// line-spread function, lsf_x along the rows and lsf_y down the columns (odd
// counts, at most XRT_MAX_LSF_TAPS; applied as written -- a correlation --,
// edges replicated, nothing normalised), in place in output_image.  One device.
void applyDetectorResponse(Image& output_image, const std::vector<float>& lsf_x, const std::vector<float>& lsf_y);

// Line integrals (xrt_log_projection): output_image becomes -ln(I / flat_value)
// in place, flat_value finite and > 0 (the unattenuated intensity, 80 for the
// models here); a transmission below t_min > 0 is raised to it.  One device.
void applyLogProjection(Image& output_image, float flat_value, float t_min = 0.0f);

// Photon noise (xrt_photon_noise, XRT_NOISE_INTENSITY): every pixel of
// output_image becomes a Poisson count of mean pixel * gain, divided by gain
// again, in place; gain finite and > 0.  The noise is a function of seed and
// first_index + the pixel's index alone: projection p of a scan of W x H
// images passes first_index = p * W * H.  One device.
void applyPhotonNoise(Image& output_image, float gain, unsigned long long seed, unsigned long long first_index = 0);

// The same over a scan: `stack` holds num_projections width x height intensity
// images one after another; `sinograms` receives the line integrals in
// XRT_ORDER_SINOGRAMS, (height, num_projections, width).  One call, one device.
void logProjectionSinograms(const std::vector<float>& stack, unsigned width, unsigned height, unsigned num_projections,
                            float flat_value, float t_min, std::vector<float>& sinograms);

// FDK reconstruction (xrt_fdk_filter and xrt_backproject) of a
// full-turn scan: `projections` holds num_projections line-integral images
// (applyLogProjection's) of frame's size one after another, all taken by the
// camera of `info` over `meshes` (as renderLoop forms it) while the object
// stood under poses[p] (one row-major 3x4 pose per projection; empty: at rest,
// a scan that turns nothing).  `volume` receives dims[0] * dims[1] * dims[2]
// f32, x fastest, of the grid whose voxel (0, 0, 0) has its minimum corner at
// `origin` in the object's rest frame; axis_point lies on the turn axis, which
// is parallel to info.up.  window: XRT_RAMP_RAMLAK or XRT_RAMP_HANN over 2 W - 1
// taps.  One device.
void reconstructFDK(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                    const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                    const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                    const float spacing[3], const float axis_point[3], int window = 0);

// SIRT / OS-SART (xrt_sirt) of the same scan into the same grid,
// arguments as reconstructFDK's: `iterations` passes over `subsets` subsets
// (1: SIRT; subset s holds the projections p with p mod subsets == s), every
// update relaxed by `relax` and clamped to [lo, hi], from `volume` when it
// holds the grid's dims[0] * dims[1] * dims[2] values, else from zeros.  No
// axis is needed: any poses do.  One device.
void reconstructSIRT(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                     const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets = 1, double relax = 1.0, float lo = 0.0f,
                     float hi = std::numeric_limits<float>::infinity());

// TV-regularised SIRT (xrt_sirt_tv): after every iteration the
// volume takes `steps` normalised steepest-descent steps on its smoothed
// isotropic total variation, each alpha times as long as the distance the
// iteration moved the volume; alpha is multiplied by `reduction` (in (0, 1])
// from one iteration to the next and `eps` smooths the norm.  alpha above
// about 0.5 flattens the object's level.  steps == 0: plain reconstructSIRT.
struct TVParams {
    unsigned steps = 0;
    double alpha = 0.2;
    double reduction = 1.0;
    double eps = 1e-8;
};
void reconstructSIRT(std::vector<float>& volume, const std::vector<float>& projections, unsigned num_projections,
                     const Image& frame, const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets, double relax, float lo, float hi,
                     const TVParams& tv);

// OS-MLTR (xrt_mltr): the maximum-likelihood reconstruction of
// the same scan from its transmission counts -- `counts` as reconstructSIRT's
// projections, the intensities themselves, no logarithm --, `flat` one image of
// the expected counts without the object and `background` the expected counts
// that did not come through it, one image per projection (empty: none).  The
// rest as reconstructSIRT's.  One device.
void reconstructMLTR(std::vector<float>& volume, const std::vector<float>& counts, const std::vector<float>& flat,
                     const std::vector<float>& background, unsigned num_projections, const Image& frame,
                     const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                     const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                     const float spacing[3], unsigned iterations, unsigned subsets = 1, double relax = 1.0, float lo = 0.0f,
                     float hi = std::numeric_limits<float>::infinity(), const TVParams& tv = TVParams());

// `steps` descent steps of `length` each on the total variation of a f32
// volume of dims[0] * dims[1] * dims[2] values (x fastest), in place, clamped
// to [lo, hi] (xrt_tv_descend).  One device.
void denoiseTV(std::vector<float>& volume, const unsigned dims[3], unsigned steps, double length, double eps = 1e-8,
               float lo = -std::numeric_limits<float>::infinity(), float hi = std::numeric_limits<float>::infinity());

// The line integrals of a f32 volume (dims[0] * dims[1] * dims[2] values, x
// fastest, the grid of reconstructFDK) along the rays of the camera of `info`
// under every pose (empty: one projection at rest): xrt_forward_project under
// the ray matrices of xrt_backprojection_matrix's matrices.  `projections`
// receives poses.size() (or 1) images of frame's size one after another.
void forwardProject(std::vector<float>& projections, const std::vector<float>& volume, const Image& frame,
                    const std::vector<TriangleMesh>& meshes, const RayTracerInfo& info,
                    const std::vector<std::array<float, 12>>& poses, const unsigned dims[3], const float origin[3],
                    const float spacing[3]);

// Area sampling (xrt_area_integrate).  focalSpotSources: the
// sub-sources of a uniform rectangular focal spot of size_u x size_v (the
// scene's length unit, along info.right and info.up), at the centres of an
// nu x nv grid, nu * nv at most XRT_MAX_SOURCES: `info` with origin moved
// (xrt_focal_spot's arithmetic; the detector does not move), source j * nu + i
// at grid cell (i, j).  applyAreaIntegration: output_image (W x H, its size is
// read) becomes the weighted mean over the samples -- any renderLoop* of an
// Image of (W * bin_x) x (H * bin_y), one per source -- and over each pixel's
// bin_y x bin_x block of them.  Throws on sizes that do not fit.  One device.
std::vector<RayTracerInfo> focalSpotSources(const RayTracerInfo& info, float size_u, float size_v, unsigned nu,
                                            unsigned nv);
void applyAreaIntegration(Image& output_image, const std::vector<Image>& samples, unsigned bin_x, unsigned bin_y,
                          const std::vector<float>& weights);

// Row strips over `num_gpus` devices (rows_per = H / n, remainder to the first
// strips), one host thread per device; returns the number of odd rays.
unsigned long long renderLoopMultiGPU(Image& output_image, const std::vector<TriangleMesh>& meshes,
                                      RayTracerInfo& info, int num_gpus);
