/*
 * xrt.h -- C ABI of the MI355X-native X-ray attenuation render path.
 *
 * This is the drop-in boundary for the reference's per-pixel render loop
 * (Brandagot/SimpleRayTracing):
 *
 *   void renderLoop(Image&, const vector<TriangleMesh>&, RayTracerInfo&)
 *       declared src/main.cxx:159-161, defined src/main.cxx:626-743,
 *       called   src/main.cxx:237
 *   void* renderLoopCallBack(void*)   (pixel-range twin)
 *       src/main-pthreads-redo.cxx:660-771, PThreadData :184-213
 *
 * src/main-cuda.cxx (0 bytes) marks where the reference expected a GPU
 * driver; this ABI fills that slot.  The C++ host library in
 * simpleraytracing_amd/csrc/host keeps the reference's renderLoop signature and
 * calls these entry points; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - Plain C types only.  Every function returns an xrt_status (0 = OK);
 *     xrt_last_error() gives the message.  Nothing throws across the ABI
 *     (the reference throws std::runtime_error / std::out_of_range, which the
 *     C++ host re-raises: main() exits 1 with "ERROR: ...", main.cxx:243-247).
 *   - Image buffers are row-major, index (row - row_begin) * width + col, as
 *     Image::setPixel (include/Image.inl:139-160) with a strip offset.
 *   - One context per device; a context is not thread-safe (the reference's
 *     threads write disjoint pixels of one Image, main-pthreads-redo.cxx:332).
 *
 * Output semantics (bit-exact with the reference):
 *   image    f32  photonOut = 80 * expf(-(0.3971 * (float)(L * 0.1)))   main.cxx:725,739
 *   lbuffer  f32  L = sum of sorted pair differences of the ray's hit
 *                 distances (main.cxx:700-718); 0 for an odd hit count;
 *                 +inf for a ray that hits nothing (z_buffer init, :646)
 *   image_u8 u8   round(255 * image / 80), clamped -- Image::applyLUT's
 *                 per-pixel formula (include/Image.inl:195-211), vmin 0, vmax 80
 */
#ifndef XRT_H
#define XRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRT_ABI_VERSION 5

typedef enum xrt_status {
    XRT_OK = 0,
    XRT_ERR_ARGUMENT = 1,   /* bad pointer / size / row range (Image::setPixel's out_of_range) */
    XRT_ERR_DEVICE = 2,     /* HIP runtime failure */
    XRT_ERR_NO_MESH = 3,    /* render before xrt_upload_mesh */
    XRT_ERR_OVERFLOW = 4,   /* internal capacity exceeded */
    XRT_ERR_IO = 5,         /* file could not be read / written */
    XRT_ERR_FORMAT = 6,     /* malformed input file */
    XRT_ERR_MEMORY = 7      /* a device working set could not be allocated (xrt_sirt) */
} xrt_status;

/* Kernel selection. */
typedef enum xrt_kernel {
    XRT_KERNEL_AUTO = 0,    /* TILED, or BINNED when T x regions > 2e7 */
    XRT_KERNEL_BRUTE = 1,   /* every ray tests every triangle (renderLoop as written) */
    XRT_KERNEL_TILED = 2,   /* every 32x32 region sweeps every triangle's conservative
                               footprint; per 8x8 ray tile the survivors of a relaxed
                               edge-function test get the exact Moller-Trumbore test */
    XRT_KERNEL_BINNED = 3   /* as TILED, but footprints are binned to regions once per
                               frame (atomic slots in fixed-capacity region lists)
                               instead of swept per region */
} xrt_kernel;

/*
 * Camera: RayTracerInfo (src/main.cxx:111-121, built by initialiseRayTracing
 * :566-622) plus the pixel spacing computed in renderLoop's prologue
 * (:634-641) and the image size.
 */
typedef struct xrt_camera {
    float origin[3];        /* point source              RayTracerInfo::origin            */
    float detector[3];      /* detector centre           RayTracerInfo::detector_position */
    float up[3];            /* detector "v" axis         RayTracerInfo::up                */
    float right[3];         /* detector "u" axis         RayTracerInfo::right             */
    float pixel_spacing;    /* 2 * max(range_z / W, range_y / H)  main.cxx:639-641         */
    uint32_t width;         /* Image::getWidth()                                           */
    uint32_t height;        /* Image::getHeight()                                          */
} xrt_camera;

/* Per-render counters (the reference prints one line per odd ray, main.cxx:710). */
typedef struct xrt_stats {
    uint64_t rays;          /* rays rendered */
    uint64_t hit_rays;      /* rays with >= 1 hit on mesh 0 */
    uint64_t odd_rays;      /* rays with an odd hit count ("Only one intersect on this ray") */
    uint64_t overflow_rays; /* rays whose hit list exceeded the register list (resolved exactly) */
    uint64_t hits;          /* total recorded intersections */
    uint32_t max_hits;      /* largest per-ray hit count */
    uint32_t kernel;        /* xrt_kernel actually used */
    double kernel_ms;       /* the last render kernel's span (its waves' s_memrealtime records) */
    uint64_t candidates;    /* TILED: triangles kept by the region footprint test, summed over regions */
    uint64_t tile_tests;    /* triangle tests issued per 8x8 wave tile (64 ray-triangle tests each) */
    uint64_t global_triangles; /* BINNED: footprints too large for the region lists (every region's candidates) */
} xrt_stats;

typedef struct xrt_context xrt_context;

/* --- lifetime ----------------------------------------------------------- */

/* Creates a context on HIP device `device`. */
int xrt_create(int device, xrt_context** out);
void xrt_destroy(xrt_context* ctx);
/* Last error message of `ctx` (or of the last failed xrt_create when ctx is NULL). */
const char* xrt_last_error(const xrt_context* ctx);
int xrt_abi_version(void);
/* Number of visible HIP devices (0 when none). */
int xrt_device_count(void);

/* --- mesh ---------------------------------------------------------------- */

/*
 * Uploads mesh 0 as a triangle soup: triangles[9*i .. 9*i+8] = p1, p2, p3 of
 * TriangleMesh::getTriangle(i) (include/TriangleMesh.inl:208, Triangle.h:125-127).
 * Only mesh 0 contributes to the image (the mesh filter at main.cxx:687), so the
 * host uploads meshes[0] only.  Replaces any previous mesh; num_triangles may be 0.
 */
int xrt_upload_mesh(xrt_context* ctx, const float* triangles, uint64_t num_triangles);

/* --- camera (host-side arithmetic, no device needed) ---------------------- */

/*
 * Bounding box of a triangle soup: TriangleMesh::computeBoundingBox
 * (src/TriangleMesh.cxx:192-228) / getBBox (src/main.cxx:538-563).
 */
int xrt_mesh_bbox(const float* triangles, uint64_t num_triangles, float lower[3], float upper[3]);

/*
 * Bounding box of a scene of several meshes: getBBox over each mesh's
 * computeBoundingBox (src/main.cxx:538-563).  tris holds the meshes' soups one
 * after another; mesh_triangles[m] is mesh m's triangle count.  The camera
 * comes from the box of every mesh (main.cxx:634), while only mesh 0 is
 * uploaded -- the only mesh whose hits count (main.cxx:687).
 */
int xrt_scene_bbox(const float* tris, const uint64_t* mesh_triangles, uint32_t num_meshes, float lower[3],
                   float upper[3]);

/*
 * Camera from the scene bounding box: initialiseRayTracing (main.cxx:566-622)
 * and renderLoop's pixel spacing (main.cxx:634-641), f32/f64 rounding as written.
 */
int xrt_camera_from_bbox(const float lower[3], const float upper[3], uint32_t width,
                         uint32_t height, xrt_camera* out);

/* --- render --------------------------------------------------------------- */

int xrt_set_kernel(xrt_context* ctx, int kernel);

/*
 * Renders image rows [row_begin, row_end) of camera->width x camera->height.
 * HOST buffers (any may be NULL), each (row_end-row_begin)*width elements.
 * Synchronous.  renderLoop == xrt_render_rows(ctx, cam, 0, H, image, ...).
 */
int xrt_render_rows(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin,
                    uint32_t row_end, float* image, float* lbuffer, uint8_t* image_u8,
                    xrt_stats* stats);

/*
 * Same with DEVICE buffers on HIP stream `stream` (hipStream_t, NULL = default
 * stream).  Asynchronous: returns once the render is enqueued.  The frame's
 * preparation (k_prep) runs on the context's own prep stream, beside earlier
 * renders; the render waits for it on the device.  The host waits only when
 * the frame geometry is new (its region lists are sized from a synchronous
 * count, and the first frame over them is checked), when the frame reuses
 * lists sized for another camera (k_prep's check decides its launch), and
 * when four frames are already in flight (for the oldest).  When a call
 * repeats the previous call's frame geometry (mesh, camera, rows) and
 * settings, the preparations of the next two frames of that geometry are
 * enqueued at once; a later call that matches takes one (rendered with no
 * wait), any other call drops them.  Renders enqueued on different streams
 * (each into its own buffers) may run at once: every frame's lists, records
 * and statistics live in its own buffer set.  Call xrt_read_stats() (which
 * synchronises the last frame's stream) for counters and kernel time.
 */
int xrt_render_rows_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin,
                           uint32_t row_end, float* d_image, float* d_lbuffer,
                           uint8_t* d_image_u8, void* stream);

/*
 * Counters and kernel time of the last render.  Enqueues a small reduction
 * kernel (k_reduce_stats) on that render's stream and waits for it: call it
 * after a sequence of frames, not between frames in flight.
 */
int xrt_read_stats(xrt_context* ctx, xrt_stats* stats);

/*
 * Many frames of one geometry (camera, rows) in one call -- a series of
 * projections of a fixed set-up, or a throughput run.  Frame k (k = 0 ..
 * n_frames-1) renders into plane set s = k % n_sets -- d_image[s],
 * d_lbuffer[s], d_u8[s] (device pointers; a NULL array or entry skips that
 * plane) -- on stream streams[s] (hipStream_t; a NULL array or entry is the
 * default stream).  Each frame is prepared and rendered as by one
 * xrt_render_rows_device call (its own k_prep, prepared ahead beside earlier
 * renders; nothing is reused between frames), with the host side of all
 * n_frames frames done in one pass: no per-frame crossing of the boundary,
 * which at 1024^2 costs about as much host time as the GPU's frame.
 * Asynchronous, like xrt_render_rows_device.  Replaces the caller's loop
 * around renderLoop (src/main.cxx:237) for a batch of frames.
 */
int xrt_render_frames_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                             uint32_t n_frames, uint32_t n_sets, float* const* d_image, float* const* d_lbuffer,
                             uint8_t* const* d_u8, void* const* streams);

/*
 * The host-buffer form: n_frames frames rendered back to back into the
 * context's device planes, then the last frame's planes copied into the host
 * buffers (any may be NULL) as xrt_render_rows does.  *ms_per_frame (may be
 * NULL) = host wall time from the first frame's enqueue to the last frame's
 * completion, / n_frames.  Synchronous.
 */
int xrt_render_frames(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                      uint32_t n_frames, float* image, float* lbuffer, uint8_t* image_u8, xrt_stats* stats,
                      double* ms_per_frame);

/*
 * Kernel timing over a region of many renders without host synchronisation.
 * A begin while a region is open ends that region first (its results are
 * dropped).  The record space is sized from the context's last frame, and
 * from the region's first frame when that is larger.
 * Every render's waves store their s_memrealtime start and end beside their
 * statistics records (xrt_stats::kernel_ms is the last frame's span: last end -
 * first start).  After xrt_timing_begin, every render keeps its records apart
 * (up to 2^27 records, 1 GiB, per region); xrt_timing_end synchronises the
 * device and returns the summed spans of those renders and their number.  Every 16th render of the region also
 * carries a HIP start/stop event pair on its dispatch: xrt_timing_events
 * returns their summed durations and number (a cross-check; a start event
 * costs its frame a few microseconds).
 */
int xrt_timing_begin(xrt_context* ctx);
int xrt_timing_end(xrt_context* ctx, double* total_ms, uint64_t* launches);
int xrt_timing_events(xrt_context* ctx, double* total_ms, uint64_t* launches);

/* --- strips in transit ---------------------------------------------------- */

/*
 * The L-buffer alone determines a pixel's image and 8-bit values (image =
 * shade(L) for a hit, 80 for a miss), except that a miss and a ray with a t =
 * +inf "hit" both have L = +inf.  Strips gathered to another device travel as
 * L-buffers with misses written as XRT_MISS_TRANSIT (a signalling NaN no render
 * produces): 4 bytes per pixel instead of 9.
 */
#define XRT_MISS_TRANSIT 0x7F800001u

/* L-buffer bits of a miss for later renders: 0 (+inf, the default) or XRT_MISS_TRANSIT. */
int xrt_set_miss_code(xrt_context* ctx, uint32_t bits);

/*
 * Expands num_pixels of a received L-buffer (misses as XRT_MISS_TRANSIT) in
 * place: d_image / d_u8 (either may be NULL) get the pixels' image and 8-bit
 * values and the miss codes become +inf -- bit-identical to a direct render.
 * Asynchronous on `stream` (device buffers).
 */
int xrt_expand_rows_device(xrt_context* ctx, uint64_t num_pixels, float* d_lbuffer, float* d_image,
                           uint8_t* d_image_u8, void* stream);

/* --- the signed multi-material L-buffer (the L-buffer fork) --------------- */

/*
 * What renders compute per ray:
 *   XRT_MODEL_ATTENUATION  renderLoop, src/main.cxx:626-743 (the default):
 *                          image, L-buffer and 8-bit planes as above.
 *   XRT_MODEL_SIGNED       renderLoopCallBack of src/main-pthreads-lbuffer.cxx
 *                          (:733-813): per ray, distance = the sum of
 *                          sign(direction . normal) * t over the mesh-0 hits
 *                          in triangle order (f32), L = 80 * exp(-(mu *
 *                          (distance * 0.1))) in f64 (glibc exp), or -1 when
 *                          the signs do not cancel (:805-806).  Renders write
 *                          the L-buffer plane only (image and u8 must be NULL);
 *                          xrt_hole_fill makes the image.  Kernels: BRUTE or
 *                          BINNED (AUTO picks BINNED).
 * mu: mesh 0's attenuation coefficient, 0.1037f in the fork (soft tissue,
 * :800).  Other meshes add no hits (the mesh-0 filter, :788), so their
 * coefficient (0.3971f, :802) multiplies L by exp(-0.0) = 1.
 */
#define XRT_MODEL_ATTENUATION 0
#define XRT_MODEL_SIGNED 1
int xrt_set_model(xrt_context* ctx, int model, float mu);

/*
 * The fork's hole fill (main-pthreads-lbuffer.cxx:327-404) over a whole
 * width x height L-buffer: pixels flagged -1 become the mean of the first
 * unflagged non-zero value within 4 steps in each of four directions; others
 * keep their value.  Writes image (f32) and/or image_u8 (the LUT of
 * image_u8's plane above).  Host buffers, synchronous; _device: device
 * buffers, asynchronous on `stream`.
 */
int xrt_hole_fill(xrt_context* ctx, uint32_t width, uint32_t height, const float* lbuffer, float* image,
                  uint8_t* image_u8);
int xrt_hole_fill_device(xrt_context* ctx, uint32_t width, uint32_t height, const float* d_lbuffer,
                         float* d_image, uint8_t* d_image_u8, void* stream);

/*
 * The fork end to end on the whole frame (XRT_MODEL_SIGNED): render, hole
 * fill; host buffers (any may be NULL): image = the fork's output image,
 * lbuffer = its L_buffer (-1 flags), image_u8 = the image's LUT.  stats.odd_rays
 * counts the flagged rays.
 */
int xrt_render_signed(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                      uint8_t* image_u8, xrt_stats* stats);

/* --- the materials model: every mesh with its own coefficient ------------- */

/*
 * A scene of num_meshes meshes (1..XRT_MAX_MESHES, any of them empty): their
 * triangle soups one after another in `triangles`, mesh m holding
 * mesh_triangles[m] of them.  xrt_upload_mesh is a one-mesh scene.  The
 * attenuation and the signed model render mesh 0 only, as the reference does
 * (src/main.cxx:687, main-pthreads-lbuffer.cxx:788).
 */
#define XRT_MAX_MESHES 16
int xrt_upload_scene(xrt_context* ctx, const float* triangles, const uint64_t* mesh_triangles,
                     uint32_t num_meshes);

/*
 * XRT_MODEL_MATERIALS: the fork's loop over the meshes (:770-810) with its
 * mesh filter lifted, the model of the paper it follows.  Per ray, with the
 * ray, the once-normalised direction and the unit normals of XRT_MODEL_SIGNED:
 *   L = 80; for each mesh m in scene order, unless L is already -1:
 *     distance = the f32 sum of sign(direction . normal) * t over the hits of
 *     mesh m in triangle order; L = -1 when its signs do not cancel, else
 *     L = (float)((double)L * exp(-(mu[m] * (distance * 0.1)))).
 * With one mesh it is XRT_MODEL_SIGNED.  xrt_set_materials selects the model
 * and sets one coefficient per mesh (finite, >= 0); a render whose scene has
 * another number of meshes fails with XRT_ERR_ARGUMENT.  Renders write the
 * L-buffer plane only, kernels BRUTE or BINNED, as for XRT_MODEL_SIGNED.
 * xrt_render_materials is xrt_render_signed for this model: render and hole
 * fill; stats.odd_rays counts the flagged rays, hits and hit_rays every mesh's.
 */
#define XRT_MODEL_MATERIALS 2
int xrt_set_materials(xrt_context* ctx, const float* mu, uint32_t num_meshes);
int xrt_render_materials(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                         uint8_t* image_u8, xrt_stats* stats);

/* --- the spectrum model: a polychromatic beam over the same scene --------- */

/*
 * XRT_MODEL_SPECTRUM: num_bins energy bins (1..XRT_MAX_BINS), bin e with the
 * weight weight[e] (finite, > 0) and mesh m attenuating in it with
 * mu[m * num_bins + e] (finite, >= 0; mesh-major).  Per ray, with the per-mesh
 * f32 sums and flags of XRT_MODEL_MATERIALS:
 *   L = -1 when some mesh's signs do not cancel, else, in f64 and in this order,
 *   E = 0; for each bin e: x = 0; for each mesh m: x = x + mu[m][e] * (distance[m] * 0.1);
 *          E = E + weight[e] * exp(-x);      L = (float)E.
 * With one bin, weight {80} and one mesh it is XRT_MODEL_SIGNED.  It is not
 * XRT_MODEL_MATERIALS with one bin and several meshes: that model rounds L to
 * f32 after every mesh, this one once.  xrt_set_spectrum selects the model and
 * sets the table (XRT_ERR_ARGUMENT for a NULL pointer, a count outside its
 * limits, a weight or coefficient outside its range); it waits for the frames
 * in flight, and no frame prepared under the old table is served.  A render
 * whose scene has another number of meshes fails with XRT_ERR_ARGUMENT.
 * Renders write the L-buffer plane only, kernels BRUTE or BINNED (AUTO:
 * BINNED).  xrt_set_model and xrt_set_materials leave the model.
 * xrt_render_spectrum is xrt_render_materials for this model: render and hole
 * fill.  The 8-bit plane keeps its fixed window 0..80: weights that sum above
 * 80 clamp to 255 there.
 */
#define XRT_MODEL_SPECTRUM 3
#define XRT_MAX_BINS 32
int xrt_set_spectrum(xrt_context* ctx, const float* weight, const float* mu, uint32_t num_meshes,
                     uint32_t num_bins);
int xrt_render_spectrum(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                        uint8_t* image_u8, xrt_stats* stats);

/* --- the paths model: trace once, apply any spectrum afterwards ----------- */

/*
 * XRT_MODEL_PATHS: the render stores what the materials and spectrum models
 * integrate -- per ray and mesh m of the uploaded scene, the f32 sum of
 * sign * t over the mesh's hits in triangle order (0.0f for a mesh the ray did
 * not hit), and a mask whose bit m is set when mesh m's signs do not cancel
 * (the rays those models flag with -1).  `paths` is num_meshes row-major f32
 * planes of (row_end - row_begin) * width pixels, one after another; `open`
 * one uint16 plane of the strip, or NULL.  Every pixel of every plane is
 * written.  A flagged ray's distances are exact too.  A NaN distance
 * (inf - inf) is stored as a NaN whose sign and payload are not specified.
 * xrt_set_paths selects the model; the mesh count is the uploaded scene's at
 * render time (a later xrt_upload_scene needs no new call), and num_meshes is
 * the caller's statement of its buffers' size: another value fails with
 * XRT_ERR_ARGUMENT.  Kernels BRUTE or BINNED (AUTO: BINNED).  With this model
 * selected only xrt_render_paths[_device] render -- the other entries' planes
 * mean something else and fail with XRT_ERR_ARGUMENT, as these two do under
 * another model.  xrt_set_model, xrt_set_materials and xrt_set_spectrum leave
 * the model.  xrt_render_paths: host buffers, synchronous; _device: device
 * buffers, asynchronous on `stream`, pipelined as xrt_render_rows_device.
 * There is no xrt_multi_ form yet: the model is single-device.
 *
 * xrt_apply_spectrum[_device]: the spectrum model's L-buffer (above) of
 * num_pixels rays from such planes (contiguous, plane stride num_pixels; open
 * NULL: no ray flagged) under the table (weight, mu, num_bins) -- bit for bit
 * what xrt_render_spectrum stores for the scene, camera and table the planes
 * came from.  The table is checked as xrt_set_spectrum checks it, before the
 * context is looked at.  Neither entry touches the context's model, and the
 * device entry may be called again with another table at once: each launch
 * carries its own copy.
 */
#define XRT_MODEL_PATHS 4
int xrt_set_paths(xrt_context* ctx);
int xrt_render_paths(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                     uint32_t num_meshes, float* paths, uint16_t* open, xrt_stats* stats);
int xrt_render_paths_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                            uint32_t num_meshes, float* d_paths, uint16_t* d_open, void* stream);
int xrt_apply_spectrum(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* paths,
                       const uint16_t* open, const float* weight, const float* mu, uint32_t num_bins,
                       float* lbuffer);
int xrt_apply_spectrum_device(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* d_paths,
                              const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                              float* d_lbuffer, void* stream);

/*
 * Mesh poses: the fork's transformMatrix hook
 * (src/main-pthreads-lbuffer.cxx:561-564), per mesh and on the device -- a
 * sample turning on a turntable beside a fixture that stays put, without an
 * upload.  A pose is 12 f32, row-major 3x4: [r00 r01 r02 t0 | r10 r11 r12 t1 |
 * r20 r21 r22 t2].  A vertex (x, y, z) of the mesh's REST soup (what was
 * uploaded) becomes
 *     p_i  = (r_i0 * x + r_i1 * y) + r_i2 * z
 *     v'_i = p_i + t_i   if some t_j is not +-0, else p_i
 * every product and sum a separately rounded f32 operation in that order:
 * with t = 0 this is the fork's expression bit for bit.  A mesh whose 12
 * values are bitwise the identity (1 and +0.0) is not computed: its rest
 * vertices are used.  Poses always apply to the rest soup, never to an earlier
 * pose.  Every model and kernel then renders the posed scene exactly as an
 * upload of the same numbers would.
 *
 * xrt_set_pose sets the pose of mesh `mesh` of the uploaded scene (NULL: the
 * identity); XRT_ERR_ARGUMENT when the mesh is not one of the scene or a value
 * is not finite.  xrt_reset_poses returns every mesh to the identity, as
 * xrt_upload_scene and xrt_upload_mesh do.  A change waits for the frames in
 * flight; the posed soup is written on the device by the next render (only
 * the meshes whose pose changed), and a frame whose only change is a pose is
 * a new geometry over the same layout: where a moving camera reuses the region
 * lists of the frame before (the attenuation model's BINNED frames), it does.
 * While every pose is the identity nothing is allocated or launched.
 */
int xrt_set_pose(xrt_context* ctx, uint32_t mesh, const float pose[12]);
int xrt_reset_poses(xrt_context* ctx);
/*
 * Host arithmetic (no device).  xrt_pose_rotation: the rotation by `degrees`
 * about `axis` (normalised in f64) through `centre` -- R by Rodrigues' formula
 * and t = centre - R centre in f64, each rounded once to f32;
 * XRT_ERR_ARGUMENT for a zero or non-finite axis.  xrt_pose_triangles: the
 * arithmetic above over a soup of n triangles (out may alias tris).
 */
int xrt_pose_rotation(const float axis[3], double degrees, const float centre[3], float pose[12]);
int xrt_pose_triangles(const float* tris, uint64_t n, const float pose[12], float* out);

/* --- the detector response: a separable line-spread function -------------- */

/*
 * What a real flat panel adds to the ideal detector's image (DESIGN.md section
 * 10.5): every photon value spread over its neighbours by a separable
 * line-spread function (LSF).  `image` is num_planes row-major f32 planes of
 * width x height pixels, one after another (a scan's projections in one call);
 * lsf_x[taps_x] and lsf_y[taps_y] are the taps, each count odd and in
 * 1..XRT_MAX_LSF_TAPS, rx = (taps_x - 1) / 2, ry = (taps_y - 1) / 2.  With
 * cx(i) = min(max(i, 0), width - 1) and cy likewise (the edge pixels are
 * replicated), per plane
 *   tmp[y][x] = (float)(sum over k = 0..taps_x-1, in this order, in f64, of
 *                       (double)lsf_x[k] * (double)image[y][cx(x + k - rx)])
 *   out[y][x] = (float)(sum over k = 0..taps_y-1, in this order, in f64, of
 *                       (double)lsf_y[k] * (double)tmp[cy(y + k - ry)][x])
 * each sum starting from its k = 0 product (not from +0.0: the one-tap LSF
 * {1.0f} on both axes returns the image bit for bit, -0.0 included) and tmp
 * rounded to f32.  The taps are applied as written -- a correlation: lsf_x[0]
 * meets the pixel rx to the LEFT of the output, so an asymmetric LSF given as a
 * convolution kernel is the caller's to flip -- and as given: nothing is
 * normalised.  out_u8 is the 8-bit image of out in the fixed window 0..80.  A
 * pixel whose window holds a non-finite value is NaN or +-inf as IEEE
 * arithmetic gives it; a NaN's sign and payload are not specified.
 *
 * Either of out and out_u8 may be NULL, not both.  XRT_ERR_ARGUMENT for a NULL
 * image or tap pointer, an even tap count or one outside 1..XRT_MAX_LSF_TAPS, a
 * tap that is not finite, a width, height or num_planes of 0 (or more than
 * 65535 planes or 64-row bands), and an output that overlaps the image: a
 * pixel is computed from its neighbours' input, so in place is refused.  All of
 * that is checked, the taps first, before the context is looked at.
 * xrt_detector_response: host buffers, synchronous.  _device: device buffers,
 * asynchronous on `stream`; the taps travel with the launch, so it may be
 * called again with other taps at once.  Neither touches the context's model,
 * scene or frames in flight.  There is no xrt_multi_ form.
 *
 * xrt_lsf_gaussian (host arithmetic, no device): g[k] = exp(-0.5 * ((k - r) /
 * sigma_pixels)^2) in f64, s = the sum of g in index order, lsf[k] =
 * (float)(g[k] / s); XRT_ERR_ARGUMENT unless sigma_pixels is finite and > 0 and
 * taps odd and in range.
 */
#define XRT_MAX_LSF_TAPS 129
int xrt_detector_response(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                          const float* image, const float* lsf_x, uint32_t taps_x, const float* lsf_y,
                          uint32_t taps_y, float* out, uint8_t* out_u8);
int xrt_detector_response_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                 const float* d_image, const float* lsf_x, uint32_t taps_x, const float* lsf_y,
                                 uint32_t taps_y, float* d_out, uint8_t* d_out_u8, void* stream);
int xrt_lsf_gaussian(double sigma_pixels, uint32_t taps, float* lsf);

/* --- line-integral projections: flat field, -log, sinograms --------------- */

/*
 * What reconstruction consumes: intensities turned
 * into line integrals p = -ln((I - dark) / (flat - dark)), on the device behind
 * the render, the spectrum integrator, the hole fill and the detector
 * response.  `image` is num_planes row-major f32 planes of width x height
 * pixels, one after another (a scan's projections in one call); `flat` and
 * `dark` are one width x height plane each, shared by every projection, or
 * NULL.  Per pixel, every operation a separately rounded f32 operation:
 *   num = dark ? image - dark : image
 *   den = flat ? (dark ? flat - dark : flat) : (dark ? flat_value - dark : flat_value)
 *   t   = num / den                           (IEEE division)
 *   if (t_min > 0 && t < t_min) t = t_min     (a NaN stays a NaN)
 *   out = 0.0f - logf(t)
 * with logf glibc 2.35's, restated bit for bit on every input: t = 1 gives
 * +0.0, t = 0 gives +inf, t = +inf gives -inf, t < 0 gives NaN; a NaN's sign
 * and payload are not specified.  flat_value is read only where flat is NULL.
 * `order` places the output rows:
 *   XRT_ORDER_PROJECTIONS  out[p][y][x], as the image
 *   XRT_ORDER_SINOGRAMS    out[y][p][x]: one num_planes x width sinogram per
 *                          detector row
 *
 * XRT_ERR_ARGUMENT for a NULL image or out; a width, height or num_planes of 0
 * (or a width above 2^31 - 4096, num_planes * height above 2^32 - 1, or a
 * plane stack past the 2^31 - 1 workgroups of one launch); an order other than the two; a t_min that is NaN,
 * infinite or negative; flat == NULL with a flat_value that is not finite or
 * not > 0; an out that overlaps image, flat or dark -- with one exception: in
 * XRT_ORDER_PROJECTIONS out == image exactly is allowed (in place: the pass is
 * pointwise; a partial overlap is refused, and so is in place in sinogram
 * order, which moves rows).  All of that is checked before the context is
 * looked at.  xrt_log_projection: host buffers, synchronous.  _device: device
 * buffers, asynchronous on `stream`.  Neither touches the context's model,
 * scene or frames in flight.  There is no xrt_multi_ form.
 */
#define XRT_ORDER_PROJECTIONS 0
#define XRT_ORDER_SINOGRAMS 1
int xrt_log_projection(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                       const float* flat, const float* dark, float flat_value, float t_min, int order, float* out);
int xrt_log_projection_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                              const float* d_image, const float* d_flat, const float* d_dark, float flat_value,
                              float t_min, int order, float* d_out, void* stream);

/* --- photon noise: a counter-based Poisson sampler ------------------------ */

/*
 * The quantum noise of a detector that counts photons (DESIGN.md section
 * 10.7), on the device behind the detector response and ahead of the line
 * integrals.  `image` is num_planes row-major f32 planes of width x height
 * pixels, one after another, taken as one flat buffer: pixel i in [0, n),
 * n = width * height * num_planes, has the global index g = first_index + i.
 * `gain` is the photons per unit of image value.  The noise is a pure function
 * of (seed, g, the pixel's mean): the same under any launch shape, for a strip
 * or one projection of a scan given its first_index, and on host and device.
 *
 * The random word.  w is word g & 3 of Philox4x32-10 (multipliers 0xD2511F53
 * and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85) at the counter
 * (lo32(g >> 2), hi32(g >> 2), 0, 0) under the key (lo32(seed), hi32(seed)).
 *   u = ((double)w + 0.5) * 2^-32             (exact in f64, never 0 or 1)
 * The mean.
 *   lam_f = image[i] * gain                   (one f32 rounding)
 *   lam   = (double)lam_f
 * A NaN or lam < 0 gives NaN (sign and payload not specified), +inf gives
 * +inf, -0.0 counts as 0.
 * lam < 64: inversion by sequential search, with xrt_exp glibc 2.35's exp
 * restated bit for bit:
 *   p = xrt_exp(-lam); s = p; N = 0
 *   while (u > s && N < 255) { N += 1; p = (p * lam) / (double)N; s = s + p; }
 * (at lam just under 64 the search ends within 108 steps for every word: the
 * cap never binds).
 * Otherwise: a normal deviate -- the normal CDF inverted by Wichura's AS241,
 * PPND7 -- with the second-order Cornish-Fisher term:
 *   q = u - 0.5
 *   if (|q| <= 0.425) {
 *     r = 0.180625 - q*q
 *     z = q*(((A3*r + A2)*r + A1)*r + A0) / (((B3*r + B2)*r + B1)*r + 1)
 *   } else {
 *     t = q < 0 ? u : 1 - u
 *     r = sqrt(-(double)logf((float)t)) - 1.6      (logf as xrt_log_projection's)
 *     z = +-(((C3*r + C2)*r + C1)*r + C0) / ((D2*r + D1)*r + 1), negative for q < 0
 *   }
 *   x = lam + sqrt(lam)*z + (z*z - 1)/6
 *   N = max(floor(x + 0.5), 0)
 * with the f64 literals
 *   A0 3.3871327179   A1 50.434271938   A2 159.29113202   A3 59.109374720
 *                     B1 17.895169469   B2 78.757757664   B3 67.187563600
 *   C0 1.4234372777   C1 2.7568153900   C2 1.3067284816   C3 0.17023821103
 *                     D1 0.73700164250  D2 0.12021132975
 * AS241's third branch (sqrt(-ln t) > 5) is unreachable and left out: the
 * smallest t is 2^-33, and sqrt(-ln 2^-33) < 4.79.  Every f64 and f32
 * operation above is rounded on its own -- no step of a polynomial, of x or of
 * z*z - 1 is fused --, sqrt and / are IEEE-correct, and q*(...) / (...) is the
 * product divided.
 * The output.  XRT_NOISE_COUNTS: (float)N.  XRT_NOISE_INTENSITY: (float)N /
 * gain, an IEEE f32 division.
 *
 * XRT_ERR_ARGUMENT for a NULL image or out; a width, height or num_planes of
 * 0; more pixels than one launch's 2^31 - 1 workgroups, 1024 pixels each, hold;
 * first_index + n overflowing 64 bits; a gain that is not finite or not > 0;
 * a mode other than the two; an out that overlaps the image -- except
 * out == image exactly, which is allowed (in place: the pass is pointwise).
 * All of that is checked before the context is looked at.  xrt_photon_noise:
 * host buffers, synchronous.  _device: device buffers, asynchronous on
 * `stream`.  Neither touches the context's model, scene or frames in flight.
 * There is no xrt_multi_ form: first_index is what lets a strip or a single
 * projection of a scan draw the noise it would have drawn in the whole.
 */
#define XRT_NOISE_INTENSITY 0
#define XRT_NOISE_COUNTS 1
int xrt_photon_noise(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                     float gain, uint64_t seed, uint64_t first_index, int mode, float* out);
int xrt_photon_noise_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                            float gain, uint64_t seed, uint64_t first_index, int mode, float* d_out, void* stream);

/* --- area sampling: a finite focal spot and pixel-area integration -------- */

/*
 * The weighted mean of intensity over the source's area and over each pixel's
 * area, on the device: the reduction that turns the
 * renders of num_sources sub-sources at (height bin_y) x (width bin_x) pixels
 * into one height x width image.  `image` is num_planes * num_sources row-major
 * f32 planes of (height bin_y) x (width bin_x), one after another; plane
 * p S + s (S = num_sources) is projection p seen from sub-source s.  `out` and
 * `out_u8` are num_planes planes of height x width; either may be NULL, not
 * both.  `weight` is num_sources f32 in HOST memory in both forms.  Per output
 * pixel (p, y, x):
 *   acc = -0.0                                                        (f64)
 *   for s in 0..S-1, dy in 0..bin_y-1, dx in 0..bin_x-1, in this order:
 *     acc = acc + (double)weight[s] * (double)image[p S + s][y bin_y + dy][x bin_x + dx]
 *   wsum = (double)(bin_x bin_y) * (sum over s of (double)weight[s], f64, in index order)
 *   out    = (float)(acc / wsum)                          (an IEEE f64 division)
 *   out_u8 = round(255 * out / 80) clamped, NaN -> 0     (as xrt_detector_response's)
 * The product of two f32 values is exact in f64, so a fused multiply-add and
 * the separate operations round identically.  The accumulator starts at -0.0:
 * bin 1 x 1 with one source of weight 1 returns the input's bits, -0.0 and
 * denormals included.  With every weight 1.0 a constant plane returns its value
 * exactly.  Non-finite values propagate as IEEE has it; a NaN's sign and
 * payload are unspecified.
 *
 * XRT_ERR_ARGUMENT, with xrt_last_error naming the argument, for a NULL image
 * or weight; out and out_u8 both NULL; a width, height or num_planes of 0;
 * bin_x or bin_y outside 1..XRT_MAX_BIN; num_sources outside
 * 1..XRT_MAX_SOURCES; a weight that is NaN, infinite or negative, or a weight
 * sum of 0; width bin_x or height bin_y above 2^31 - 1; num_planes * height
 * above 2^32 - 1 or more than one launch's 2^31 - 1 workgroups (256 lanes of at
 * most four outputs each); an output that overlaps the image anywhere (nothing
 * is computed in place: the output is smaller and rows move).  All of that is checked
 * before the context is looked at.  xrt_area_integrate: host buffers,
 * synchronous.  _device: device buffers, asynchronous on `stream`; the weights
 * travel with the launch, so the next call may bring others at once.  Neither
 * touches the context's model, scene or frames in flight.  There is no
 * xrt_multi_ form: apply it to the gathered frame.
 */
#define XRT_MAX_SOURCES 64
#define XRT_MAX_BIN 8
int xrt_area_integrate(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y,
                       uint32_t num_sources, uint32_t num_planes, const float* weight, const float* image, float* out,
                       uint8_t* out_u8);
int xrt_area_integrate_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y,
                              uint32_t num_sources, uint32_t num_planes, const float* weight, const float* d_image,
                              float* d_out, uint8_t* d_out_u8, void* stream);

/*
 * The cameras that area sampling renders.  Host arithmetic, no device; every
 * operation below is a separately rounded f32 operation unless written as f64.
 *
 * xrt_camera_supersample: the camera whose pixels tile `cam`'s, bin x bin to
 * each: width * bin, height * bin, pixel_spacing / (float)bin (one IEEE f32
 * division), everything else copied (out may be cam).  Its pixel centres,
 * spacing/bin * (0.5 + c' - W bin / 2), tile cam's pixels exactly.  For bin a
 * power of two the spacing equals what renderLoop's prologue computes for the
 * larger image, 2 * max(range / (W bin)); for other factors it may differ from
 * that by an ulp.  XRT_ERR_ARGUMENT for a NULL pointer, bin outside
 * 1..XRT_MAX_BIN or a product above 2^31 - 1.
 *
 * xrt_focal_spot: a uniform rectangular focal spot of size_u x size_v (the
 * scene's length unit, along `right` and `up`), sampled at the centres of an
 * nu x nv grid.  Sub-source s = j nu + i, i < nu, j < nv, is cam with
 *   a = (float)((double)size_u * (((double)i + 0.5) / (double)nu - 0.5))
 *   b = (float)((double)size_v * (((double)j + 0.5) / (double)nv - 0.5))
 *   origin'[k] = (origin[k] + right[k] * a) + up[k] * b
 * and weight[s] = 1.0f; detector, up, right, spacing and size are unchanged (the
 * detector does not move).  A size of 0 with a count of 1 is the point source
 * on that axis.  Other profiles are the caller's own offsets and weights.
 * XRT_ERR_ARGUMENT for a NULL pointer, a size that is negative or not finite, a
 * count of 0 or nu * nv above XRT_MAX_SOURCES.
 */
int xrt_camera_supersample(const xrt_camera* cam, uint32_t bin, xrt_camera* out);
int xrt_focal_spot(const xrt_camera* cam, float size_u, float size_v, uint32_t nu, uint32_t nv, xrt_camera* cams,
                   float* weight);

/* --- the spectral detector: per-bin counts into energy channels ----------- */

/*
 * A detector that sees the beam's energy bins one by one (DESIGN.md section
 * 10.9): per pixel and bin a photon count, then a num_channels x num_bins
 * response matrix into num_channels output planes.  A row of bin energies is
 * an energy-integrating panel, rows of 0/1 windows are a photon-counting
 * detector.  `paths`, `open`, `weight`, `mu` and `num_bins` are exactly
 * xrt_apply_spectrum's: num_meshes planes of num_pixels f32 path lengths, the
 * uint16 masks (may be NULL: none set) and the table, `weight` and `mu` in HOST
 * memory in both forms.  `response` is HOST memory in both forms too:
 * num_channels rows of num_bins f32, each finite and >= 0 (a row of zeros is
 * allowed).  `out` is num_channels f32 planes of num_pixels.  Pixel i has the
 * global index g = first_index + i.  Per pixel, in f64 unless written
 * otherwise, every operation rounded on its own (nothing is fused):
 *   if open && open[i] != 0:  out[c][i] = -1.0f for every c     (the hole fill's marker, as L = -1)
 *   else:
 *     acc[c] = 0.0 for every c
 *     for e in 0..num_bins-1:
 *       x = 0; for m in 0..num_meshes-1: x = x + (double)mu[m][e] * ((double)paths[m][i] * 0.1)
 *       lam = ((double)weight[e] * exp(-x)) * (double)gain      (exp as the spectrum model's)
 *       N   = draw_mode == XRT_DETECT_NOISY ? the Poisson count of mean lam under the word w_e : lam
 *       for c: acc[c] = acc[c] + (double)response[c * num_bins + e] * N
 *     if read_noise > 0:  for c: acc[c] = acc[c] + (double)read_noise * z(v_c)
 *     out[c][i] = XRT_DETECT_COUNTS ? (float)acc[c] : (float)(acc[c] / (double)gain)
 * The count is xrt_photon_noise's sampler on the f64 mean (the search below 64,
 * the AS241 deviate with the Cornish-Fisher term from there on), z its normal
 * deviate.  w_e is word e & 3 of Philox4x32-10 at the counter (lo32(g),
 * hi32(g), e >> 2, 1) under the key (lo32(seed), hi32(seed)); v_c is word c & 3
 * at the counter (lo32(g), hi32(g), c >> 2, 2).  xrt_photon_noise's counters
 * end in (0, 0): under one seed the three streams are disjoint, and the bins
 * of a pixel are independent draws.  read_noise is additive Gaussian
 * (electronic) noise in counts, added before the division by gain; a channel
 * may go negative and is kept so.  A NaN path length propagates to every
 * channel of its pixel; the NaN's sign and payload are unspecified.
 *
 * Two consequences.  Under XRT_DETECT_EXPECTED and XRT_DETECT_COUNTS with gain
 * 1, one channel and a response of ones, `out` is xrt_apply_spectrum's
 * L-buffer bit for bit wherever that is no NaN (the products by 1.0 are exact
 * and the chain is the same).  With a 0/1 response and XRT_DETECT_COUNTS (no
 * read noise) the noisy channel planes are exact integers while the sums stay
 * below 2^24, and disjoint windows add up to the channel of all their bins
 * exactly.
 *
 * XRT_ERR_ARGUMENT, with xrt_last_error naming the argument, for a NULL paths,
 * weight, mu, response or out; what xrt_set_spectrum refuses in the table;
 * num_channels outside 1..XRT_MAX_CHANNELS; a response that is NaN, infinite or
 * negative; a gain that is not finite or not > 0; a read_noise that is not
 * finite, negative, or not 0 under XRT_DETECT_EXPECTED; an unknown draw_mode or
 * out_mode; num_pixels of 0 or more than one launch's 2^31 - 1 workgroups of
 * 256 pixels hold; first_index + num_pixels overflowing 64 bits; an out that
 * overlaps paths or open anywhere.  All of that is checked before the context
 * is looked at.  xrt_spectral_detector: host buffers, synchronous.  _device:
 * device buffers, asynchronous on `stream`; the table and the response travel
 * with the launch, so the next call may bring others at once.  Neither touches
 * the context's model, scene or frames in flight.  There is no xrt_multi_ form.
 */
#define XRT_MAX_CHANNELS 8
#define XRT_DETECT_EXPECTED 0   /* N_e = lam_e: no draw, seed ignored, read_noise must be 0 */
#define XRT_DETECT_NOISY    1
#define XRT_DETECT_COUNTS    0  /* out = (float)acc */
#define XRT_DETECT_INTENSITY 1  /* out = (float)(acc / (double)gain) */
int xrt_spectral_detector(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* paths,
                          const uint16_t* open, const float* weight, const float* mu, uint32_t num_bins,
                          const float* response, uint32_t num_channels, float gain, float read_noise, uint64_t seed,
                          uint64_t first_index, int draw_mode, int out_mode, float* out);
int xrt_spectral_detector_device(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* d_paths,
                                 const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                                 const float* response, uint32_t num_channels, float gain, float read_noise,
                                 uint64_t seed, uint64_t first_index, int draw_mode, int out_mode, float* d_out,
                                 void* stream);

/* --- voxel phantoms: a labelled volume traced into paths planes ----------- */

/*
 * A voxel object: u8 labels[nz][ny][nx] (x fastest; dims = {nx, ny, nz}),
 * label 0 empty, label L in 1..num_labels traced into plane L - 1, and an
 * optional f32 density of the same shape (NULL: 1 everywhere).  origin is the
 * minimum corner of voxel (0, 0, 0), spacing the voxel's size, both in x, y, z
 * order; the volume is axis-aligned in scene space and has no pose (turn the
 * camera).  Per ray and label, the length of the ray inside voxels of that
 * label, each segment times its voxel's density, is a paths plane in the sense
 * of xrt_render_paths: xrt_apply_spectrum and xrt_spectral_detector take the
 * planes as they are, with open = NULL.
 *
 * xrt_upload_volume copies the arrays to the device and replaces any earlier
 * volume; labels = NULL or num_labels = 0 frees it.  XRT_ERR_ARGUMENT, with
 * xrt_last_error naming the fault, before any device work and before the
 * context is looked at, unless 1 <= dims[a] <= 2048, 1 <= num_labels <=
 * XRT_MAX_MESHES, every spacing is finite and > 0, the origin and the far
 * corner are finite in f32, every label is <= num_labels (the first offending
 * voxel is named) and every density is finite.  XRT_ERR_DEVICE for a volume
 * that does not fit device memory.  xrt_volume_bbox is host arithmetic: lower
 * = origin, upper[a] = (float)((double)origin[a] + (double)dims[a] *
 * (double)spacing[a]); a camera then comes from xrt_camera_from_bbox, of this
 * box or of its union with xrt_scene_bbox's.
 *
 * xrt_volume_paths[_device] trace the rows [row_begin, row_end) of the camera
 * into num_labels planes of (row_end - row_begin) * width f32, one after
 * another.  num_labels is the caller's statement of its buffer: a value other
 * than the uploaded volume's fails with XRT_ERR_ARGUMENT; without a volume the
 * call fails with XRT_ERR_NO_MESH.  Every plane of every pixel is written; a
 * ray that misses the volume writes +0.0f.  xrt_volume_paths: host buffers,
 * synchronous.  _device: device buffers, asynchronous on `stream`.  Neither
 * looks at or changes the context's model, meshes, poses, prepared-ahead
 * frames or state generation: a mesh render and a volume trace of one context
 * may be enqueued back to back on one stream.  There is no xrt_multi_ form.
 *
 * The ray, all in f64, every operation rounded on its own (nothing is fused;
 * every min and max is the written comparison):  O = camera origin, d = the
 * render's ray direction (the twice-normalised f32 direction, widened),
 * plane(a, i) = origin[a] + (double)i * spacing[a].
 *   te = 0, tx = +inf
 *   for a in x, y, z:
 *     d[a] == 0:  a miss unless plane(a, 0) <= O[a] < plane(a, n[a])
 *     otherwise:  inv[a] = 1 / d[a]; t0 = (plane(a, 0) - O[a]) * inv[a]; t1 = (plane(a, n[a]) - O[a]) * inv[a]
 *                 te = max(te, min(t0, t1)); tx = min(tx, max(t0, t1))
 *   a miss unless te < tx
 *   idx[a] = floor(((O[a] + te * d[a]) - origin[a]) / spacing[a]) clamped to [0, n[a] - 1]
 *   tnext(a) = d[a] == 0 ? +inf : (plane(a, idx[a] + (d[a] > 0 ? 1 : 0)) - O[a]) * inv[a]
 *   tc = te; then, at most nx + ny + nz + 3 times:
 *     a = the axis of the least tnext (ties: x before y before z); t = tnext(a)
 *     tend = min(t, tx); seg = tend - tc
 *     a run is the consecutive steps of one label: its sum `run` starts at 0 and is added to
 *     acc[label - 1] when the label changes and at the end
 *     if label != 0 and seg > 0:  run = run + (density ? seg * (double)density[idx] : seg)
 *     if seg > 0:  tc = tend
 *     stop unless t < tx;  idx[a] += d[a] > 0 ? 1 : -1;  stop when idx[a] leaves the volume
 *   paths[m][pixel] = (float)acc[m]
 *
 * Stacking.  Mesh planes and volume planes may share one buffer and one
 * spectrum table: render a mesh scene's M1 planes with
 * xrt_render_paths_device into the front of a buffer of M1 + M2 planes of
 * num_pixels, trace the volume's M2 planes with xrt_volume_paths_device into
 * d_paths + M1 * num_pixels, and call xrt_apply_spectrum_device (or
 * xrt_spectral_detector_device) with num_meshes = M1 + M2 <= XRT_MAX_MESHES,
 * a table of M1 + M2 rows (the meshes' first) and the mesh scene's open plane.
 */
int xrt_upload_volume(xrt_context* ctx, const uint8_t* labels, const float* density, const uint32_t dims[3],
                      const float origin[3], const float spacing[3], uint32_t num_labels);
int xrt_volume_bbox(const uint32_t dims[3], const float origin[3], const float spacing[3], float lower[3],
                    float upper[3]);
int xrt_volume_paths(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                     uint32_t num_labels, float* paths);
int xrt_volume_paths_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                            uint32_t num_labels, float* d_paths, void* stream);

/* --- FDK reconstruction: ramp filter and cone-beam backprojector ---------- */

/*
 * What consumes the line integrals of xrt_log_projection (DESIGN.md section
 * 10.11): a row filter and a voxel-driven backprojector, which together are
 * FDK for a full turn about an axis parallel to the detector's `up`; the
 * backprojector alone is the adjoint-style operator of iterative methods.
 * Neither looks at or changes the context's model, scene, poses, frames in
 * flight or state generation.  There is no xrt_multi_ form.
 *
 * xrt_fdk_filter[_device].  image: num_planes row-major f32 planes of width x
 * height; weight: one such plane, or NULL; taps[num_taps], num_taps odd and in
 * 1..2 * XRT_MAX_RAMP_WIDTH - 1, r = (num_taps - 1) / 2; width <=
 * XRT_MAX_RAMP_WIDTH.  Per plane
 *   pw[y][x]  = weight ? image[y][x] * weight[y][x] : image[y][x]     (one f32 product)
 *   out[y][x] = (float)s,  s = +0.0 in f64, then for k = 0 .. num_taps - 1 in this order, only
 *               where 0 <= x + k - r < width:  s = s + (double)taps[k] * (double)pw[y][x + k - r]
 * every operation rounded on its own.  A correlation, as xrt_detector_response
 * is; nothing is normalised; pixels outside the row are skipped, not
 * replicated.  XRT_ERR_ARGUMENT, before the context is looked at, for a NULL
 * image, taps or out, an even or out-of-range tap count, a tap that is not
 * finite (the host form only: the device form cannot read its taps), a width,
 * height or num_planes of 0, a width above the limit (or 2^30 rows and more),
 * and an out that overlaps image, weight or taps.  xrt_fdk_filter: host
 * buffers, synchronous.  _device: device pointers for image, weight, taps and
 * out (8191 taps do not fit a launch's arguments), asynchronous on `stream`.
 *
 * xrt_backproject[_device].  proj: num_planes planes of width x height, pixel
 * (row, col) centred on integer coordinates; matrices[num_planes][12], each a
 * row-major 3 x 4 f64 matrix A taking a voxel index to homogeneous detector
 * coordinates; the volume is f32 [nz][ny][nx], x fastest, dims = {nx, ny, nz}
 * as xrt_upload_volume's, each 1..2048.  Only the slabs k in [slab_begin,
 * slab_end) are written, into (slab_end - slab_begin) * ny * nx floats (an
 * empty range: success, nothing written).  Per voxel (i, j, k), exact doubles,
 * and per plane p = 0 .. num_planes - 1 in this order, A = matrices[p]:
 *   a = A[0]*i + ((A[1]*j + A[2]*k) + A[3])       f64, every product and sum rounded on its own
 *   b = A[4]*i + ((A[5]*j + A[6]*k) + A[7])
 *   c = A[8]*i + ((A[9]*j + A[10]*k) + A[11])
 *   contributes only if c > 0                      (a NaN compares false)
 *   w = 1.0 / c;  col = a * w;  row = b * w        f64, IEEE division
 *   contributes only if col > -1 && col < width && row > -1 && row < height
 *   x0 = floor(col), y0 = floor(row);  fx = (float)(col - x0), fy = (float)(row - y0)
 *   s(y, x) = proj[p][y][x] inside the plane, +0.0f outside
 *   top = s(y0,x0)   + fx * (s(y0,x0+1)   - s(y0,x0))       f32, separately rounded
 *   bot = s(y0+1,x0) + fx * (s(y0+1,x0+1) - s(y0+1,x0))
 *   v   = top + fy * (bot - top)
 *   acc = acc + (double)v * (w * w)                f64; acc starts at +0.0
 *   out = accumulate ? (float)((double)old + acc * scale) : (float)(acc * scale)
 * XRT_ERR_ARGUMENT, before the context is looked at, for a NULL pointer, a
 * width, height or num_planes of 0 (or a width or height above 2^31 - 1, or a
 * plane of more than 2^40 pixels), more than 65535 planes, a dims[a] outside 1..2048, slab_begin > slab_end or
 * slab_end > nz, a scale that is not finite, a matrix entry that is not finite
 * (the host form only) and a volume that overlaps the projections or the
 * matrices.  xrt_backproject: host buffers, synchronous.  _device: device
 * buffers, asynchronous on `stream`.
 *
 * Host arithmetic in f64 (no device):
 * xrt_backprojection_matrix: the matrix of a camera for a voxel grid.  A voxel
 * centre is X = origin + (idx + 0.5) * spacing in the rest frame, Xw = pose X
 * in the world (xrt_set_pose's layout; NULL: the identity), (a', b', c) =
 * M^-1 (Xw - S) with S the source and M's columns right, up, detector - S;
 * rows 0 and 1 become pixel coordinates of the render's pixel formula:
 * A_row0 = a'-row / pixel_spacing + (width / 2 - 0.5) * c-row, A_row1 likewise
 * with up's row and the height.  XRT_ERR_ARGUMENT for a singular or
 * non-finite M or a non-finite result.
 * xrt_fdk_weights: weight[y][x] = the cosine between pixel (y, x)'s ray and the
 * central ray detector - origin, rounded once.
 * xrt_ramp_filter: XRT_RAMP_RAMLAK g[0] = 1/4, g[n] = -1 / (pi^2 n^2) for odd
 * n, 0 for even n; XRT_RAMP_HANN (g[n-1] / 4 + g[n] / 2) + g[n+1] / 4, the Hann
 * window's closed form in space; taps[k] = (float)g[k - r], dimensionless.
 * xrt_fdk_scale: pi / P * (SOD / SDD) / (pixel_spacing * |right|), SDD =
 * |detector - origin|, SOD the component of axis_point - origin along the
 * central ray: the full-turn FDK constant, with which a uniform object of
 * mu = 1 reconstructs to 1.
 */
#define XRT_MAX_RAMP_WIDTH 4096
#define XRT_RAMP_RAMLAK 0
#define XRT_RAMP_HANN 1
int xrt_fdk_filter(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                   const float* weight, const float* taps, uint32_t num_taps, float* out);
int xrt_fdk_filter_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                          const float* d_weight, const float* d_taps, uint32_t num_taps, float* d_out, void* stream);
int xrt_backproject(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                    const double* matrices, const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end, double scale,
                    int accumulate, float* volume);
int xrt_backproject_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                           const double* d_matrices, const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end,
                           double scale, int accumulate, float* d_volume, void* stream);
int xrt_backprojection_matrix(const xrt_camera* camera, const float pose[12], const float origin[3],
                              const float spacing[3], double A[12]);
int xrt_fdk_weights(const xrt_camera* camera, float* weight);
int xrt_ramp_filter(uint32_t num_taps, int window, float* taps);
int xrt_fdk_scale(const xrt_camera* camera, const float axis_point[3], uint32_t num_projections, double* scale);

/* --- SIRT / OS-SART: a matrix-driven forward projector and solver ---------- */

/*
 * The iterative side of reconstruction: a forward
 * projector of a device-resident f32 volume under the backprojector's own
 * matrices, a voxel update, and the loop over both and xrt_backproject that
 * is SIRT (one subset) or OS-SART (several).  None of them looks at or
 * changes the context's model, scene, poses, frames in flight or state
 * generation.  There is no xrt_multi_ form.
 *
 * xrt_ray_matrix (host arithmetic in f64, no device).  A = [A3 | a4] is a
 * matrix of xrt_backproject; R = [N | -N a4] with N = A3^-1 by cofactors:
 *   C[i][j] = A3[i1][j1] * A3[i2][j2] - A3[i1][j2] * A3[i2][j1],  i1 = (i+1)%3, i2 = (i+2)%3, j likewise
 *   det     = (A3[0][0] * C[0][0] + A3[0][1] * C[0][1]) + A3[0][2] * C[0][2]
 *   N[i][j] = C[j][i] / det
 *   R[4i+j] = N[i][j],  R[4i+3] = -((N[i][0] * a4[0] + N[i][1] * a4[1]) + N[i][2] * a4[2])
 * every operation rounded on its own.  In centre-index coordinates (voxel i
 * occupies [i - 0.5, i + 0.5]) column 3 of R is the source s, and the ray of
 * pixel (row, col) is s + t d with
 *   d_a = R[4a] * col + (R[4a+1] * row + R[4a+2])
 * A (s + t d, 1) = t (col, row, 1): t is the backprojector's c, and forward is
 * t > 0, the half-space the backprojector accepts.  XRT_ERR_ARGUMENT for a
 * NULL pointer, an input that is not finite, a determinant that is zero or not
 * finite, and a result that is not finite.
 *
 * xrt_forward_project[_device].  volume: f32 [nz][ny][nx], dims = {nx, ny, nz}
 * as xrt_backproject's, each 1..2048; spacing[3] the voxel's size, each finite
 * and > 0; rays[num_planes][12] f64 ray matrices; meas (XRT_FP_RESIDUAL: needed;
 * XRT_FP_PROJECT: not read) and out: num_planes planes of width x height.  Per
 * pixel (row, col) of plane p, R = rays[p], all in f64, every operation
 * rounded on its own (no FMA), every min or max the written select, the grid
 * lo = -0.5, s = 1 with plane(i) = -0.5 + (double)i * 1.0 from the index every
 * time, n = (nx, ny, nz):
 *   O = (R[3], R[7], R[11]);  d as above with (double)row, (double)col
 *   te = 0, tx = +inf;  per axis a in x, y, z order:
 *     d_a == 0:  a miss unless O_a >= plane(0) && O_a < plane(n_a)
 *     else       inv_a = 1 / d_a;  t0 = (plane(0) - O_a) * inv_a;  t1 = (plane(n_a) - O_a) * inv_a
 *                mn = t0 < t1 ? t0 : t1;  mx = t0 < t1 ? t1 : t0
 *                te = mn > te ? mn : te;  tx = mx < tx ? mx : tx
 *   a miss unless te < tx
 *   i_a = floor(((O_a + te * d_a) - (-0.5)) / 1.0), then f >= 0 ? f : 0 and f <= n_a - 1 ? f : n_a - 1
 *   step_a = d_a > 0 ? 1 : -1;  up_a = d_a > 0 ? 1 : 0
 *   tnext_a = d_a == 0 ? +inf : (plane(i_a + up_a) - O_a) * inv_a
 *   tc = te, acc = +0.0; at most nx + ny + nz + 3 times:
 *     t = tnext_x, a = x;  if (tnext_y < t) t = tnext_y, a = y;  if (tnext_z < t) t = tnext_z, a = z
 *     tend = t < tx ? t : tx;  seg = tend - tc
 *     if (seg > 0) { acc = acc + seg * (double)volume[(i_z * ny + i_y) * nx + i_x];  tc = tend }
 *     stop unless t < tx;  i_a += step_a;  stop when i_a leaves 0 .. n_a - 1
 *   ell = sqrt(((sx*dx) * (sx*dx) + (sy*dy) * (sy*dy)) + (sz*dz) * (sz*dz)),  s = (double)spacing
 *   L   = (tx - te) * ell
 *   XRT_FP_PROJECT:   out = (float)(acc * ell); a miss: +0.0f
 *   XRT_FP_RESIDUAL:  out = L > 0 ? (float)(((double)meas - acc * ell) / L) : +0.0f; a miss: +0.0f
 * the residual being SART's row-normalised one.  XRT_ERR_ARGUMENT, before the
 * context is looked at, for a NULL volume, dims, spacing, rays or out, a
 * width, height or num_planes of 0 (or outside xrt_backproject's limits, or a
 * plane of more than 2^26 - 1 tiles of 8 x 8 pixels), more than 65535 planes,
 * a dims[a] outside 1..2048, a spacing that is not finite and > 0, a mode
 * that is not one of XRT_FP_*, XRT_FP_RESIDUAL without meas, a ray matrix
 * entry that is not finite (the host form only) and an out that overlaps the
 * volume, the rays or meas.  xrt_forward_project: host buffers, synchronous.
 * _device: device buffers, asynchronous on `stream`.
 *
 * xrt_volume_update[_device].  Per voxel i < n (n in 1..2^33), only where
 * norm[i] > 0 (a NaN compares false):
 *   v = (float)((double)x[i] + relax * ((double)corr[i] / (double)norm[i]))
 *   v = v < lo ? lo : v;  v = v > hi ? hi : v;  x[i] = v
 * elsewhere x[i] stays.  lo = -inf and hi = +inf: no clamp.  XRT_ERR_ARGUMENT,
 * before the context is looked at, for a NULL pointer, an n of 0 or above
 * 2^33, a relax that is not finite, a bound that is NaN, lo > hi and an x that
 * overlaps corr or norm.
 *
 * xrt_sirt[_device].  proj[P][H][W]: line integrals (xrt_log_projection's);
 * matrices[P][12]: xrt_backproject's, in host memory in both forms -- the
 * library derives every R from its A (xrt_ray_matrix), so the two geometries
 * agree by construction --; `volume` is the start and the result.  Subset s of
 * S holds the planes p with p mod S == s, ascending; A_s, R_s, b_s are its
 * matrices and measurements.  N_s = xrt_backproject of all-ones planes under
 * A_s (scale 1, no accumulate), once.  Then for k = 0 .. iterations - 1 and
 * s = 0 .. S - 1 in this order:
 *   r = xrt_forward_project(volume, R_s, XRT_FP_RESIDUAL, b_s)
 *   c = xrt_backproject(r, A_s, scale 1, no accumulate)
 *   volume = xrt_volume_update(volume, c, N_s, relax, lo, hi)
 * S = 1 is SIRT, S > 1 OS-SART.  XRT_ERR_ARGUMENT, before the context is
 * looked at, for a NULL pointer, sizes outside the limits above, iterations of
 * 0, subsets outside 1..min(P, XRT_MAX_SUBSETS), a relax that is not finite, a
 * NaN bound, lo > hi, a matrix entry that is not finite and a volume that
 * overlaps an input; then for a matrix without a ray matrix.  xrt_sirt: host
 * projections and volume, synchronous.  _device: device projections and
 * volume, asynchronous on `stream` (a call first waits for the context's
 * previous xrt_sirt[_device], whose working set it takes over: two calls on
 * two streams of one context run one after the other, the second's host
 * thread blocked until the first has finished on the device; calls that are
 * to overlap need a context each).  The working
 * set -- the residual planes of the largest subset, one correction volume, S
 * norm volumes and the gathered matrices -- is held by the context and reused;
 * XRT_ERR_MEMORY, with the byte count in xrt_last_error, when it cannot be
 * allocated.
 */
#define XRT_FP_PROJECT 0
#define XRT_FP_RESIDUAL 1
#define XRT_MAX_SUBSETS 64
int xrt_ray_matrix(const double A[12], double R[12]);
int xrt_forward_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                        const uint32_t dims[3], const float spacing[3], const double* rays, int mode, const float* meas,
                        float* out);
int xrt_forward_project_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                               const float* d_volume, const uint32_t dims[3], const float spacing[3], const double* d_rays,
                               int mode, const float* d_meas, float* d_out, void* stream);
int xrt_volume_update(xrt_context* ctx, uint64_t n, float* x, const float* corr, const float* norm, double relax, float lo,
                      float hi);
int xrt_volume_update_device(xrt_context* ctx, uint64_t n, float* d_x, const float* d_corr, const float* d_norm,
                             double relax, float lo, float hi, void* stream);
int xrt_sirt(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
             const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets,
             double relax, float lo, float hi, float* volume);
int xrt_sirt_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                    const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                    uint32_t subsets, double relax, float lo, float hi, float* d_volume, void* stream);

/* --- TV-regularised SIRT: a 3-D TV gradient and descent steps -------------- */

/*
 * A prior beyond the clamp: ASD-POCS without its
 * host-side adaptation.  After every full SIRT iteration the volume takes a
 * fixed number of normalised steepest-descent steps on a smoothed isotropic
 * total variation, their length tied to how far the data step moved the
 * volume.  Nothing comes back to the host inside the loop: the norms stay in
 * device memory and the step reads them there.  Like the SIRT entries, none
 * of these looks at or changes the context's model, scene, poses, frames in
 * flight or state generation, and there is no xrt_multi_ form.  All
 * arithmetic is f64, every operation rounded on its own (no FMA), every
 * select the written one; sqrt and / are IEEE's.
 *
 * xrt_tv_gradient[_device].  volume, out: f32 [nz][ny][nx], dims = {nx, ny,
 * nz} as xrt_forward_project's, each 1..2048; v(i,j,k) = (double)volume[(k *
 * ny + j) * nx + i]; eps finite and > 0.  Per voxel p = (i, j, k):
 *   dx(p) = i + 1 < nx ? v(i+1,j,k) - v(p) : +0.0;  dy, dz likewise
 *   n(p)  = sqrt(((dx * dx + dy * dy) + dz * dz) + eps)
 *   qx(p) = dx(p) / n(p);  qy(p) = dy(p) / n(p);  qz(p) = dz(p) / n(p)
 *   bx = i > 0 ? qx(i-1,j,k) : +0.0;  by = j > 0 ? qy(i,j-1,k) : +0.0;  bz = k > 0 ? qz(i,j,k-1) : +0.0
 *   out(p) = (float)(((bx + by) + bz) - ((qx(p) + qy(p)) + qz(p)))
 * the exact gradient of TV(x) = sum over p of n(p), with no difference across
 * the border.  A 1 x 1 x 1 grid gives +0.0; nz = 1 is 2-D TV.
 * XRT_ERR_ARGUMENT, before the context is looked at, for a NULL volume, dims
 * or out, a dims[a] outside 1..2048, an eps that is not finite and > 0 and an
 * out that overlaps the volume.
 *
 * xrt_volume_sumsq[_device].  n in 1..2^33; b may be NULL.  e_i = b ?
 * (double)a[i] - (double)b[i] : (double)a[i], w_i = e_i * e_i, and *out =
 * reduce(w, n), whose order is part of the contract:
 *   reduce(w, 1) = w[0]
 *   reduce(w, m): chunk c covers w[4096 c .. 4096 c + 4095], entries from m on
 *     being +0.0.  acc_l = +0.0 for l = 0 .. 255; for r = 0 .. 15 in turn
 *     acc_l = acc_l + w[4096 c + 256 r + l]; then for h = 128, 64, .., 1 in
 *     turn acc_l = acc_l + acc_(l+h) for l < h.  partial_c = acc_0, and the
 *     result is reduce(partial, ceil(m / 4096)).
 * At most three levels; no atomics.  The device form writes one double to
 * device memory at d_out; the partials live in the context's working set
 * (below).  XRT_ERR_ARGUMENT, before the context is looked at, for a NULL a or
 * out, an n of 0 or above 2^33 and an out that overlaps an input.
 *
 * xrt_tv_descend[_device].  `steps` times (0: nothing), with the working
 * set's gradient volume g:
 *   g = xrt_tv_gradient(volume, eps);  G = xrt_volume_sumsq(g);  gn = sqrt(G)
 *   where gn > 0 (a NaN compares false):  c = length / gn, and per voxel
 *     v = (float)((double)x - c * (double)g);  v = v < lo ? lo : v;  v = v > hi ? hi : v;  x = v
 *   otherwise the volume stays.
 * XRT_ERR_ARGUMENT, before the context is looked at, for a NULL volume or
 * dims, a dims[a] outside 1..2048, an eps that is not finite and > 0, a
 * length that is not finite and >= 0, a NaN bound and lo > hi.
 *
 * xrt_sirt_tv[_device].  xrt_sirt's arguments and checks, and tv.  With tv
 * NULL or tv->steps == 0 it is xrt_sirt, bit for bit (the other fields are
 * not looked at).  Otherwise a_0 = tv->alpha, and iteration k is
 *   x0 = volume;  xrt_sirt's loop over the subsets;  D = xrt_volume_sumsq(volume, x0)
 *   xrt_tv_descend(volume, tv->eps, tv->steps, length = a_k * sqrt(D), lo, hi)
 *   a_(k+1) = a_k * tv->reduction
 * length being formed on the device from the resident D, the product rounded
 * once (a D that is not finite gives what the formulas give).  XRT_ERR_ARGUMENT
 * also for an alpha that is not finite and >= 0, a reduction that is not
 * finite and in (0, 1] and an eps that is not finite and > 0.
 *
 * Host forms: host buffers, synchronous.  _device: device buffers,
 * asynchronous on `stream`.  The working set -- the partials, the gradient
 * volume (xrt_sirt_tv: the solver's correction volume, free after the
 * update) and the solver's x0 -- is the context's xrt_sirt working set,
 * ordered as xrt_sirt_device says; XRT_ERR_MEMORY, with the byte count in
 * xrt_last_error, when it cannot be allocated.
 */
typedef struct xrt_tv_params {
    uint32_t steps;      /* descent steps after every iteration; 0: none */
    double alpha;        /* the first iteration's step length as a share of the data step's, finite and >= 0 */
    double reduction;    /* alpha's factor from one iteration to the next, in (0, 1] */
    double eps;          /* the smoothing under the square root, finite and > 0 */
} xrt_tv_params;
int xrt_tv_gradient(xrt_context* ctx, const float* volume, const uint32_t dims[3], double eps, float* out);
int xrt_tv_gradient_device(xrt_context* ctx, const float* d_volume, const uint32_t dims[3], double eps, float* d_out,
                           void* stream);
int xrt_volume_sumsq(xrt_context* ctx, uint64_t n, const float* a, const float* b, double* out);
int xrt_volume_sumsq_device(xrt_context* ctx, uint64_t n, const float* d_a, const float* d_b, double* d_out, void* stream);
int xrt_tv_descend(xrt_context* ctx, float* volume, const uint32_t dims[3], double eps, uint32_t steps, double length,
                   float lo, float hi);
int xrt_tv_descend_device(xrt_context* ctx, float* d_volume, const uint32_t dims[3], double eps, uint32_t steps,
                          double length, float lo, float hi, void* stream);
int xrt_sirt_tv(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* volume);
int xrt_sirt_tv_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                       const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                       uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* d_volume,
                       void* stream);

/* --- OS-MLTR: Poisson-likelihood reconstruction from transmission counts --- */

/*
 * The statistical side of reconstruction: a
 * maximum-likelihood solver for transmission counts in ordered subsets.  It
 * takes the counts themselves -- no logarithm, so a pixel that counted zero
 * is an ordinary measurement -- and an optional background, the expected
 * counts that did not come through the object (scatter, dark current).  Like
 * the SIRT entries, none of these looks at or changes the context's model,
 * scene, poses, frames in flight or state generation, and there is no
 * xrt_multi_ form.  All arithmetic is f64 where written, every operation
 * rounded on its own (no FMA), every select the written one; xrt_exp is the
 * library's exp (glibc's, bit for bit).
 *
 * xrt_poisson_project[_device].  volume, dims, spacing and rays as
 * xrt_forward_project's; counts: num_planes planes of width x height, the
 * measured y; flat: one plane, the expected counts without the object, shared
 * by every plane; background: num_planes planes, or NULL; pairs:
 * float[num_planes][height][width][2], (num, den) interleaved, aligned to 8
 * bytes.  Per pixel, with the ray, acc, te, tx and ell of
 * xrt_forward_project:
 *   l   = acc * ell;  L = (tx - te) * ell
 *   psi = (double)flat[row][col] * xrt_exp(-l)
 *   r   = background ? (double)background[p][row][col] : +0.0
 *   yh  = psi + r
 *   a miss, or !(L > 0), or !(yh > 0):  num = den = +0.0f      (a NaN compares false)
 *   else  q = psi / yh;  num = (float)(psi - (double)y * q);  den = (float)((L * psi) * q)
 * With r = 0, q is exactly 1: a NULL background and a plane of zeros give the
 * same bits.  XRT_ERR_ARGUMENT, before the context is looked at, for a NULL
 * volume, dims, spacing, rays, counts, flat or pairs, pairs not aligned to 8
 * bytes, sizes outside xrt_forward_project's limits, a spacing that is not
 * finite and > 0, a ray matrix entry that is not finite (the host form only)
 * and pairs overlapping an input.
 *
 * xrt_backproject_update[_device].  pairs as above, matrices and dims as
 * xrt_backproject's, the whole volume f32 [nz][ny][nx], updated in place.  Per
 * voxel and per plane in order, a, b, c, w, col, row, x0, y0, fx, fy and the
 * acceptance tests are xrt_backproject's, formed once; vn and vd are its
 * three f32 expressions (top, bot, v) over the pairs' first and second
 * components, +0.0f outside the plane;
 *   accn = accn + (double)vn * (w * w);  accd = accd + (double)vd * (w * w)
 * and then x = xrt_volume_update's voxel with corr = (float)accn and norm =
 * (float)accd: only where (float)accd > 0, elsewhere x keeps its bits.  The
 * result equals, bit for bit, xrt_backproject of the num planes and of the den
 * planes (scale 1, no accumulate) followed by xrt_volume_update.
 * XRT_ERR_ARGUMENT, before the context is looked at, for a NULL pointer,
 * pairs not aligned to 8 bytes, sizes outside xrt_backproject's limits, a
 * relax that is not finite, a NaN bound, lo > hi, a matrix entry that is not
 * finite (the host form only) and a volume that overlaps the pairs or the
 * matrices.
 *
 * xrt_mltr[_device].  xrt_sirt_tv's arguments and checks, with counts, flat
 * and background (may be NULL) in the place of proj -- NULL counts or flat and
 * a volume that overlaps any of them are refused too.  Subsets as xrt_sirt's.
 * For k = 0 .. iterations - 1 and s = 0 .. S - 1 in this order:
 *   pairs  = xrt_poisson_project(volume, R_s, counts_s, flat, background_s)
 *   volume = xrt_backproject_update(pairs, A_s, relax, lo, hi)
 * and tv as in xrt_sirt_tv after every iteration (x0, D, xrt_tv_descend with
 * length a_k * sqrt(D), a_(k+1) = a_k * reduction); tv NULL or tv->steps == 0:
 * the plain solver, bit for bit.  One update is x + relax * sum(psi - y q) /
 * sum(L psi q) under the backprojector's weights: the separable-surrogate
 * step of the transmission likelihood with its curvature at the current
 * estimate.  xrt_mltr: host buffers, synchronous.  _device: device counts,
 * flat, background and volume, asynchronous on `stream`.  The working set --
 * the largest subset's pairs and the gathered matrices, with tv x0, the
 * gradient volume and the partials; no norm volumes -- is the context's
 * xrt_sirt working set, ordered as xrt_sirt_device says (a call waits for the
 * context's previous solver call); XRT_ERR_MEMORY, with the byte count in
 * xrt_last_error, when it cannot be allocated.
 */
int xrt_poisson_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                        const uint32_t dims[3], const float spacing[3], const double* rays, const float* counts,
                        const float* flat, const float* background, float* pairs);
int xrt_poisson_project_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                               const float* d_volume, const uint32_t dims[3], const float spacing[3], const double* d_rays,
                               const float* d_counts, const float* d_flat, const float* d_background, float* d_pairs,
                               void* stream);
int xrt_backproject_update(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs,
                           const double* matrices, const uint32_t dims[3], double relax, float lo, float hi, float* volume);
int xrt_backproject_update_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                  const float* d_pairs, const double* d_matrices, const uint32_t dims[3], double relax,
                                  float lo, float hi, float* d_volume, void* stream);
int xrt_mltr(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* counts, const float* flat,
             const float* background, const double* matrices, const uint32_t dims[3], const float spacing[3],
             uint32_t iterations, uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* volume);
int xrt_mltr_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_counts,
                    const float* d_flat, const float* d_background, const double* matrices, const uint32_t dims[3],
                    const float spacing[3], uint32_t iterations, uint32_t subsets, double relax, float lo, float hi,
                    const xrt_tv_params* tv, float* d_volume, void* stream);

/* --- material decomposition: a per-pixel Newton solver -------------------- */

/*
 * The inverse of xrt_spectral_detector under XRT_DETECT_EXPECTED (DESIGN.md
 * section 10.14): projection-domain material decomposition.  Given the
 * num_channels channel planes of a scan and the tables that produced them, per
 * pixel the line integrals A_b of num_basis basis materials whose expected
 * channels match the measured ones.  `weight`, `mu` (num_basis rows of
 * num_bins), `response` (num_channels rows of num_bins) and `gain` mean exactly
 * what they mean to xrt_spectral_detector, with basis materials in place of
 * meshes, and are HOST memory in both forms; `in_mode` is the out_mode the
 * channels were written under.  `channels` is num_channels f32 planes of
 * num_pixels, `open` the uint16 masks (may be NULL: none set), `out` num_basis
 * f32 planes of num_pixels -- path planes again, in xrt_render_paths' units --,
 * `iters` a uint8 plane (may be NULL) of each pixel's status: the iterations
 * it ran, XRT_DECOMPOSE_MASKED or XRT_DECOMPOSE_FAILED.  `guess` is
 * xrt_decompose_guess' num_basis x num_channels f64 matrix in HOST memory in
 * both forms, or NULL to start from zero.  With B = num_basis, C =
 * num_channels, per pixel, in f64 unless written otherwise, every operation
 * rounded on its own (nothing is fused):
 *   if open && open[i] != 0:  out[b][i] = +0.0f for every b; iters[i] = 254; done
 *   y[c] = (double)channels[c][i];  if in_mode == XRT_DETECT_INTENSITY: y[c] = y[c] * (double)gain
 *   if guess == NULL: A[b] = 0.0
 *   else:
 *     y0[c] = the chain below at A = 0 (every exp is 1.0; computed on the host, travels with the launch)
 *     t = (float)(y[c] / y0[c]);  if !(t >= 1e-30f): t = 1e-30f     (zero, negative and NaN counts start at the floor)
 *     p[c] = -(double)logf(t)                                       (logf as xrt_log_projection's)
 *     A[b] = 0.0; for c ascending: A[b] = A[b] + guess[b * C + c] * p[c]
 *   it = 0
 *   while it < max_iter:
 *     ybar[c] = 0; J[c][b] = 0
 *     for e ascending:
 *       x = 0; for b ascending: x = x + (double)mu[b][e] * (A[b] * 0.1)
 *       lam = ((double)weight[e] * exp(-x)) * (double)gain          (the detector's lam)
 *       for c: t = (double)response[c][e] * lam
 *              ybar[c] = ybar[c] + t
 *              for b: J[c][b] = J[c][b] + (double)mu[b][e] * t
 *     g[b] = 0; H[b][b'] = 0 (b' >= b)
 *     for c ascending, skipped if !(ybar[c] > 0):                   (a zero response row, or underflow)
 *       q = y[c] / ybar[c];  r = 1.0 - q;  v = 1.0 / ybar[c]
 *       for b: g[b] = g[b] + J[c][b] * r
 *       for b, b' >= b: H[b][b'] = H[b][b'] + (J[c][b] * J[c][b']) * v
 *     for b: H[b][b] = H[b][b] + H[b][b] * damping
 *     solve H d = g by LDL^T without pivoting, in this order (B = 1, 2 are its leading blocks):
 *       d0 = H00;  l10 = H01/d0;  l20 = H02/d0
 *       d1 = H11 - l10*H01;  l21 = (H12 - l20*H01)/d1
 *       d2 = (H22 - l20*H02) - l21*(l21*d1)
 *       z0 = g0;  z1 = g1 - l10*z0;  z2 = (g2 - l20*z0) - l21*z1
 *       x2 = z2/d2;  x1 = z1/d1 - l21*x2;  x0 = (z0/d0 - l10*x1) - l20*x2
 *     a pivot d_k that is not > 0: iters[i] = 255, A stays as it is, done
 *     s[b] = x_b / 0.1;  A[b] = A[b] + s[b];  it = it + 1
 *     if every |s[b]| <= tol: break
 *   out[b][i] = (float)A[b];  iters[i] = it
 * This is Fisher scoring on the Poisson likelihood of the channels: exp and
 * division only, defined for zero and negative counts (read noise makes
 * those).  For energy-integrating rows it is a consistent estimator, not the
 * exact likelihood.  A NaN count makes the first step, and with it every
 * output of its pixel, a NaN (sign and payload unspecified); as written above
 * its status is then max_iter when max_iter is 1 and XRT_DECOMPOSE_FAILED
 * otherwise (the second iteration's sums are NaN, every channel is left out
 * and the pivot is 0).  With a guess the NaN count starts at the floor, far
 * from the other channels' line integrals, and the pixel may fail in its first
 * iteration instead, its outputs the finite start.  With a guess,
 * a channel whose response row is all zeros has y0 = 0: its p is finite for a
 * count of 0 and infinite otherwise, and 0 * inf starts the pixel at NaN --
 * leave such rows out, or pass guess = NULL.
 *
 * xrt_decompose_guess is a host function and never touches the device:
 *   mbar[c][b] = 0.1 * ((sum_e (r[c][e] * w[e]) * mu[b][e]) / (sum_e r[c][e] * w[e])), in f64 and bin order
 *   guess = (mbar^T mbar)^-1 mbar^T over the channels whose denominator is > 0 (the columns of the others
 *   are 0): N[b][b'] summed over c ascending, each column solved by the LDL^T order above
 * so that guess times the channels' -ln(y / y0) is the least-squares line
 * integral under each channel's mean coefficient.  From A = 0 the iteration
 * advances about one attenuation length a step; from the guess a few steps
 * suffice.  XRT_ERR_ARGUMENT for a NULL guess, what xrt_decompose refuses in the
 * tables, and a pivot that is not > 0 ("basis materials are not separable under
 * this response").
 *
 * xrt_decompose[_device]: XRT_ERR_ARGUMENT, with xrt_last_error naming the
 * argument, for a NULL channels, weight, mu, response or out; what
 * xrt_spectral_detector refuses in its tables, gain or modes; num_basis outside
 * 1..XRT_MAX_BASIS; num_channels below num_basis or outside
 * 1..XRT_MAX_CHANNELS; max_iter outside 1..200; a tol or damping that is
 * negative or not finite; a guess entry that is not finite; num_pixels of 0 or
 * more than one launch's 2^31 - 1 workgroups of 256 pixels hold; an out or
 * iters that overlaps channels or open anywhere.  All of that is checked before
 * the context is looked at.  xrt_decompose: host buffers, synchronous.
 * _device: device buffers, asynchronous on `stream`; the tables and the guess
 * travel with the launch, so the next call may bring others at once.  Neither
 * touches the context's model, scene, state generation or frames in flight.
 * There is no xrt_multi_ form.
 */
#define XRT_MAX_BASIS 3
#define XRT_DECOMPOSE_MASKED 254
#define XRT_DECOMPOSE_FAILED 255
int xrt_decompose(xrt_context* ctx, uint64_t num_pixels, const float* channels, const uint16_t* open, const float* weight,
                  const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response, uint32_t num_channels,
                  float gain, int in_mode, const double* guess, uint32_t max_iter, double tol, double damping, float* out,
                  uint8_t* iters);
int xrt_decompose_device(xrt_context* ctx, uint64_t num_pixels, const float* d_channels, const uint16_t* d_open,
                         const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                         uint32_t num_channels, float gain, int in_mode, const double* guess, uint32_t max_iter, double tol,
                         double damping, float* d_out, uint8_t* d_iters, void* stream);
int xrt_decompose_guess(const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                        uint32_t num_channels, double* guess);

/* --- voxelise the scene: occupancy, labels and truth volumes --------------- */

/*
 * The uploaded scene under its poses -- the soup the next render would read,
 * what xrt_debug_posed_triangles gives -- as a volume on a grid (DESIGN
 * 10.15): which voxel centres lie inside which mesh.  Mesh m is bit m.
 *
 * Grid.  dims = {nx, ny, nz}, origin and spacing as xrt_upload_volume's, with
 * the same checks.  All arithmetic is f64, every operation rounded on its own,
 * nothing fused; the f32 inputs are widened.  Centres:
 *   c_a(i) = (double)origin[a] + ((double)i + 0.5) * (double)spacing[a]
 *
 * Crossing of triangle (p0, p1, p2) with column (i, j); px = c_x(i), py = c_y(j):
 *   e1 = p1 - p0;  e2 = p2 - p0
 *   n.x = e1.y * e2.z - e1.z * e2.y;  n.y = e1.z * e2.x - e1.x * e2.z;  n.z = e1.x * e2.y - e1.y * e2.x
 *   n.z == 0: no crossing
 *   each edge (p0 p1, p1 p2, p2 p0) with its ends named so that a.y < b.y (a.y == b.y: the edge does not count):
 *     straddle = (a.y <= py) != (b.y <= py)
 *     w = (b.x - a.x) * (py - a.y) - (b.y - a.y) * (px - a.x)
 *     the edge counts when straddle && w > 0
 *   the column is crossed when an odd number of the three edges count, and then
 *   z = p0.z - (n.x * (px - p0.x) + n.y * (py - p0.y)) / n.z
 *   the crossing's slice k = the least k in [0, nz] with c_z(k) >= z, nz when none is
 * for every column of the grid: the footprint box the kernels walk leaves no
 * crossing out.  Two triangles that share an edge evaluate the same w on the
 * same operands, so a closed mesh closes over every column.
 *
 * Occupancy.  Voxel (i, j, k) is inside mesh m when the number of mesh-m
 * crossings of column (i, j) with slice <= k is odd.  Crossings with slice nz
 * only enter the column's total; a column whose total for mesh m is odd counts
 * in odd_columns[m] -- the mesh is open or inconsistent there -- and is
 * otherwise left as computed.
 *
 * Outputs, each [nz][ny][nx] (x fastest) and each optional (NULL), at least
 * one of the four given:
 *   mask    u16, bit m set for inside mesh m
 *   labels  u8, 0 for an empty mask, else 1 + the highest set bit (the later
 *           mesh wins: list an insert after its body) -- an xrt_upload_volume
 *           labels array with num_labels = the scene's mesh count
 *   volume  f32, (float) of the f64 sum, from 0 and in mesh order, of
 *           (double)value[m] over the set bits; +0.0f where the mask is empty.
 *           value: one f32 per mesh of the scene, a host array in both forms
 *   odd_columns  XRT_MAX_MESHES u64 counts, 0 past the scene's meshes
 *
 * XRT_ERR_ARGUMENT, with xrt_last_error naming the fault and before the
 * context is looked at, for what xrt_upload_volume refuses in dims, origin and
 * spacing, for no output at all and for volume without value; then
 * XRT_ERR_NO_MESH without a scene; XRT_ERR_MEMORY, with the byte count in
 * xrt_last_error, when the working set -- the flip volume, u16 [nz + 1][ny][nx]
 * -- cannot be allocated.  xrt_voxelize: host buffers, synchronous.
 * xrt_voxelize_device: device buffers, asynchronous on `stream`.  The working
 * flip volume, which the kernels update through 32-bit words, is the context's
 * own (xrt_sirt's working set: a call first waits for that set's previous
 * user, unless that was a voxelisation on the same stream that left the set
 * large enough): d_mask needs no alignment beyond its type's and no padding.  A pose
 * set since the soup was last written makes k_pose due: the call enqueues it
 * on the context's preparation stream, where a render would, and `stream`
 * waits for it through an event, the host does not; the next upload or pose
 * change waits for the call's reads of the soup.  Neither form touches the
 * model, the uploaded volume, the state generation or the frames prepared
 * ahead.  There is no xrt_multi_ form.
 */
int xrt_voxelize(xrt_context* ctx, const uint32_t dims[3], const float origin[3], const float spacing[3], const float* value,
                 uint16_t* mask, uint8_t* labels, float* volume, uint64_t* odd_columns);
int xrt_voxelize_device(xrt_context* ctx, const uint32_t dims[3], const float origin[3], const float spacing[3],
                        const float* value, uint16_t* d_mask, uint8_t* d_labels, float* d_volume, uint64_t* d_odd_columns,
                        void* stream);

/* --- the scatter model -------------------------------------- */

/*
 * A kernel-superposition estimate of scattered radiation from the paths
 * model's planes, in three steps: xrt_scatter_source forms the scatter source
 * per material and energy bin and bins it to a coarse grid; the caller blurs
 * the coarse planes with xrt_detector_response, once per scatter kernel;
 * xrt_scatter_add interpolates the blurred planes back onto the detector,
 * weighs and sums them and adds them to the primary.
 *
 * For num_planes projections of width x height, N = num_planes * height *
 * width: paths is num_meshes mesh-major f32 planes of N values and open the
 * uint16 masks or NULL, as xrt_apply_spectrum takes them; weight[num_bins] and
 * mu[num_meshes][num_bins] are the spectrum table; sigma, in mu's layout, is
 * the part of each coefficient that scatters, every entry finite and >= 0; bin
 * = D is a power of two in 1..XRT_MAX_SCATTER_BIN.  The coarse grid is Wc =
 * (width + D - 1) / D by Hc = (height + D - 1) / D.
 *
 * xrt_scatter_source.  Per fine pixel i = (p * height + y) * width + x, in
 * f64, every operation rounded on its own, exp as the spectrum model's:
 *
 *   E = 0; Q = 0
 *   for e in bins:
 *       xe = 0; se = 0
 *       for m in meshes:
 *           d  = (double)paths[m * N + i] * 0.1
 *           xe = xe + (double)mu[m][e] * d
 *           se = se + (double)sigma[m][e] * d
 *       t = (double)weight[e] * exp(-xe)
 *       E = E + t
 *       Q = Q + t * se
 *   flagged = open && open[i] != 0
 *   lbuffer[i] = flagged ? -1.0f : (float)E     (lbuffer may be NULL)
 *   q = flagged ? +0.0 : Q
 *
 * lbuffer is xrt_apply_spectrum's L-buffer bit for bit (a NaN E is stored as
 * 0x7FC00000, as there).  Per coarse pixel (p, yc, xc), over the rows and
 * columns of its D x D block that lie on the detector (rows x cols pixels,
 * fewer at the right and bottom edges):
 *
 *   acc = -0.0
 *   for y ascending: r = -0.0; for x ascending: r = r + q;  acc = acc + r
 *   source[(p * Hc + yc) * Wc + xc] = (float)(acc / (double)(rows * cols))
 *
 * A row's sum first, then the rows, in that order.  With D = 1 source is
 * (float)Q.  A NaN path length propagates as IEEE 754 has it, its sign and
 * payload unspecified: it is the source of its whole block, and after the blur
 * it reaches every fine pixel within the scatter kernel's width of the block.
 *
 * xrt_scatter_add.  blurred is num_kernels (G, 1..XRT_MAX_SCATTER_KERNELS)
 * stacks [g][p][Hc][Wc] of blurred coarse planes, amp[G] their amplitudes
 * (f32, finite, >= 0, host memory in both forms), primary N values or NULL.
 * Per fine pixel, in f64 with nothing fused:
 *
 *   u  = ((double)x + 0.5) / (double)D - 0.5, clamped to [0, Wc - 1]
 *   x0 = floor(u); fx = u - x0; x1 = min(x0 + 1, Wc - 1)
 *   (v, y0, fy, y1 likewise from y, D, Hc)
 *   S = 0.0
 *   for g in kernels:                         c.. = (double)blurred[g][p][y.][x.]
 *       a  = fx == 0 ? c00 : c00 + fx * (c01 - c00)
 *       b  = fx == 0 ? c10 : c10 + fx * (c11 - c10)
 *       vg = fy == 0 ? a : a + fy * (b - a)
 *       S  = S + (double)amp[g] * vg
 *   out_scatter[i] = (float)S
 *   out[i]         = primary ? (float)((double)primary[i] + S) : (float)S
 *   out_u8[i]      = the 8-bit LUT of out[i]
 *
 * Any of out, out_scatter and out_u8 may be NULL, not all.  A constant coarse
 * plane comes back as that constant exactly; with D = 1 the sample is the
 * coarse value itself.
 *
 * XRT_ERR_ARGUMENT, with xrt_last_error naming the argument and before the
 * context is looked at: a NULL paths, sigma, source, blurred or amp, or no
 * output; what xrt_set_spectrum refuses in the table; a sigma entry that is
 * NaN, infinite or negative; a bin that is no power of two in
 * 1..XRT_MAX_SCATTER_BIN; num_kernels outside 1..XRT_MAX_SCATTER_KERNELS or an
 * amp that is NaN, infinite or negative; a width, height or num_planes of 0, a
 * width or height above 2^31 - 1, more than 65535 planes or tile rows (a tile
 * is max(D, 4) rows in the source, 64 in the sum) or a plane of more than 2^40
 * pixels; an output that overlaps an input.  The host forms take host buffers
 * and are synchronous; the _device forms take device buffers and are
 * asynchronous on `stream`, the tables and amplitudes, host data, travelling
 * with the launch.  Neither entry touches the model, the scene, the frames in
 * flight or the context's working set.  There is no xrt_multi_ form.
 */
#define XRT_MAX_SCATTER_BIN 64
#define XRT_MAX_SCATTER_KERNELS 4
int xrt_scatter_source(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                       const float* paths, const uint16_t* open, const float* weight, const float* mu, const float* sigma,
                       uint32_t num_bins, uint32_t bin, float* lbuffer, float* source);
int xrt_scatter_source_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                              const float* d_paths, const uint16_t* d_open, const float* weight, const float* mu,
                              const float* sigma, uint32_t num_bins, uint32_t bin, float* d_lbuffer, float* d_source,
                              void* stream);
int xrt_scatter_add(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                    const float* blurred, uint32_t num_kernels, const float* amp, const float* primary, float* out,
                    float* out_scatter, uint8_t* out_u8);
int xrt_scatter_add_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                           const float* d_blurred, uint32_t num_kernels, const float* amp, const float* d_primary,
                           float* d_out, float* d_out_scatter, uint8_t* d_out_u8, void* stream);

/* --- multi-GPU: row strips + RCCL root gather (one process) --------------- */

/*
 * The image split into contiguous row strips over several devices, as the
 * reference's parallel drivers split the pixel index space
 * (src/main-pthreads-rows.cxx:311-334, src/main-mpi.cxx:262-290; see
 * xrt_multi_set_split for the two rules).  Strip g renders on devices[g]; the
 * strips' planes are gathered into device 0's frame with grouped ncclSend /
 * ncclRecv over xGMI -- the analogue of the MPI root gather of
 * src/main-mpi.cxx:855-881 -- on one communicator per device
 * (ncclCommInitAll).  A device listed more than once (rehearsing the strip
 * logic on fewer GPUs) gathers with device copies instead.
 */
typedef struct xrt_multi xrt_multi;

int xrt_multi_create(const int* devices, int num_devices, xrt_multi** out);
void xrt_multi_destroy(xrt_multi* m);
const char* xrt_multi_last_error(const xrt_multi* m);
int xrt_multi_num_devices(const xrt_multi* m);
/* The mesh, replicated on every device (xrt_upload_mesh). */
int xrt_multi_upload_mesh(xrt_multi* m, const float* triangles, uint64_t num_triangles);
int xrt_multi_set_kernel(xrt_multi* m, int kernel);

/*
 * Renders the whole camera->height x width frame as strips and gathers it into
 * HOST buffers (any may be NULL).  Synchronous.  `stats` sums the devices'.
 * renderLoop over n GPUs == xrt_render_rows_multi(m, cam, image, ...).
 */
int xrt_render_rows_multi(xrt_multi* m, const xrt_camera* camera, float* image, float* lbuffer,
                          uint8_t* image_u8, xrt_stats* stats);

/*
 * The same into device-0 DEVICE buffers (full-frame planes; NULL planes are
 * neither rendered nor gathered), ordered on device 0's HIP stream `stream`.
 * Asynchronous: the next frame's strips render while this frame's gather is
 * in flight (double-buffered strip planes).
 */
int xrt_render_rows_multi_device(xrt_multi* m, const xrt_camera* camera, float* d_image,
                                 float* d_lbuffer, uint8_t* d_image_u8, void* stream);

/*
 * The per-ray model of every device (xrt_set_model).  With XRT_MODEL_SIGNED the
 * gathered planes are the fork's: lbuffer = its L_buffer, image / image_u8 =
 * the hole-filled image (device 0 fills the assembled frame).
 */
int xrt_multi_set_model(xrt_multi* m, int model, float mu);
/* The scene and the materials model of every device (xrt_upload_scene, xrt_set_materials). */
int xrt_multi_upload_scene(xrt_multi* m, const float* triangles, const uint64_t* mesh_triangles,
                           uint32_t num_meshes);
int xrt_multi_set_materials(xrt_multi* m, const float* mu, uint32_t num_meshes);
/* The spectrum model of every device (xrt_set_spectrum): strips as for the materials model. */
int xrt_multi_set_spectrum(xrt_multi* m, const float* weight, const float* mu, uint32_t num_meshes,
                           uint32_t num_bins);
/* The mesh poses of every device (xrt_set_pose, xrt_reset_poses). */
int xrt_multi_set_pose(xrt_multi* m, uint32_t mesh, const float pose[12]);
int xrt_multi_reset_poses(xrt_multi* m);

/* Waits for the last frame's gathers; the devices' statistics, summed. */
int xrt_multi_read_stats(xrt_multi* m, xrt_stats* stats);

/*
 * How the strips reach device 0.  XRT_GATHER_AUTO (the default): RCCL when
 * every listed device is distinct, device copies when one is listed twice.
 * XRT_GATHER_RCCL on a list that names ONE device n times (a one-GPU
 * rehearsal) gathers through a one-rank RCCL communicator on that device --
 * grouped ncclSend / ncclRecv from the rank to itself, the same calls and
 * stream order as the distinct-device gather.  XRT_GATHER_COPY forces copies.
 * A list that mixes repeated and distinct devices gathers with copies.
 */
#define XRT_GATHER_AUTO 0
#define XRT_GATHER_COPY 1
#define XRT_GATHER_RCCL 2
int xrt_multi_set_gather(xrt_multi* m, int mode);

/*
 * What a sender's strip sends to device 0 (attenuation model).
 * XRT_TRANSIT_HITS (the default): once a strip geometry repeats (the same
 * camera, rows, mesh and kernel as the sender's previous frame), per 8x8 tile
 * of the regions its fill plan leaves a 64-bit hit mask and the hit rays' L
 * values, rendered straight into that layout (xrt_set_transit_hits; the plan
 * is made once per geometry, synchronously); a frame of a new geometry sends
 * the packed layout.  XRT_TRANSIT_PACKED: always the 32x32 blocks of the
 * regions the fill plan leaves (xrt_set_transit_layout's layout).  A received
 * hit mask that disagrees with its sender's plan fails the call that sees it
 * (xrt_render_rows_multi: that frame; the device entry: its next call) with
 * XRT_ERR_DEVICE and drops the hit plans (the next frames travel packed, then
 * plan again).
 */
#define XRT_TRANSIT_PACKED 0
#define XRT_TRANSIT_HITS 1
int xrt_multi_set_transit(xrt_multi* m, int mode);

/*
 * How the rows are split over the devices.
 *   XRT_SPLIT_EQUAL     rows_per = H / n, the remainder going to the first
 *                       strips, strip g = device g in frame order -- the
 *                       reference's row rule (src/main-pthreads-rows.cxx:311-334).
 *   XRT_SPLIT_BALANCED  (the default) the gather bounds a multi-GPU frame: a
 *                       sender's rows cost their transfer over ONE link into
 *                       device 0, device 0's rows only their render.  Device 0
 *                       renders ONE run of 32-row bands anywhere in the frame,
 *                       devices 1 .. n-1 the bands above it, then below it, in
 *                       frame order, so that max(device 0's render + unpack,
 *                       each sender's max(render, bytes / link)) is least
 *                       (xrt_balanced_bounds).  The model comes from the
 *                       strips' own renders of an earlier frame -- per band the
 *                       wave time of its regions (timing records, summed on each
 *                       device behind its render of a new camera) and its
 *                       transit bytes -- never from an extra render; the first
 *                       frame of a multi context has no model and splits
 *                       equally.  Link rate: link_bytes_per_us when > 0, else
 *                       measured once per context and gather path (every sender
 *                       sends 4 MB to device 0 at once through the context's
 *                       gather) when a balanced plan is first made.  A camera
 *                       keeps its plan; a new camera plans from the latest
 *                       complete model without waiting.  The signed model, and
 *                       frames with fewer bands than devices, split equally.
 * Every split is exact: the gathered frame equals one device's frame.
 */
#define XRT_SPLIT_EQUAL 0
#define XRT_SPLIT_BALANCED 1
int xrt_multi_set_split(xrt_multi* m, int mode, double link_bytes_per_us);

/*
 * The strips of `camera`'s frame (planned now from the latest strip model when
 * the camera is new; the equal split, info zeros, before any frame):
 * bounds[2g], bounds[2g+1] = [begin, end) rows of device g's strip (2n
 * entries).  info (may be NULL): [0] the link rate the plan used (bytes per
 * microsecond), [1] the modelled frame's render span (us), [2] the step the
 * plan predicts (us); zeros for an equal split.
 */
int xrt_multi_plan(xrt_multi* m, const xrt_camera* camera, uint32_t* bounds, double* info);

/*
 * The balanced split as host arithmetic (no device): band_cost[b] = render time
 * of band b (us), band_bytes[b] = the bytes band b's strip sends to device 0,
 * n devices, link rate in bytes per microsecond, `band_rows` rows per band
 * (the last band may be shorter: rows are clamped to `height`), unpack_us =
 * device 0's per-frame unpack.  bounds: 2n entries as xrt_multi_plan's;
 * *step_us (may be NULL) = the step the split implies.  XRT_ERR_ARGUMENT when
 * there are fewer bands than devices.
 */
int xrt_balanced_bounds(const double* band_cost, const double* band_bytes, uint32_t n_bands, uint32_t n,
                        double link_bytes_per_us, uint32_t height, uint32_t band_rows, double unpack_us,
                        uint32_t* bounds, double* step_us);

/* --- region-packed transit (multi-GPU gathers) ---------------------------- */

/*
 * Region-packed strips for multi-GPU gathers (DESIGN.md "Multi-GPU").  A strip
 * rendered as an L-buffer with misses coded XRT_MISS_TRANSIT travels as the
 * 32x32 blocks of the regions its fill plan did NOT fill (the filled ones hold
 * only misses): 1024 floats per packed region.
 *
 * xrt_plan_region_map: map[r] for the n_regions = ceil(width/32) x
 * ceil(rows/32) regions of the strip (row-major) -- the packed index of
 * region r, or 0xFFFFFFFF for a region the last enqueued frame filled;
 * *n_packed = packed regions.  Without a plan in that frame every region is
 * packed (map[r] = r).  The map belongs to the strip's geometry: a receiver
 * needs the sender's map once, not per frame.
 * xrt_pack_regions_device: d_lbuffer (the strip, rows x width) -> d_packed
 * (n_packed x 1024 floats, 16-B aligned) on `stream`.
 * xrt_unpack_regions_device: d_packed -> the strip's three planes (any may be
 * NULL), with xrt_expand_rows_device's values.
 */
int xrt_plan_region_map(xrt_context* ctx, uint32_t width, uint32_t rows, uint32_t* map, uint64_t n_regions,
                        uint32_t* n_packed);
int xrt_pack_regions_device(xrt_context* ctx, uint32_t width, uint32_t rows, const uint32_t* d_map,
                            const float* d_lbuffer, float* d_packed, void* stream);
int xrt_unpack_regions_device(xrt_context* ctx, uint32_t width, uint32_t rows, const uint32_t* d_map,
                              const float* d_packed, float* d_lbuffer, float* d_image, uint8_t* d_u8, void* stream);
/*
 * Renders of this context write the L-buffer in the packed layout directly
 * (no xrt_pack_regions_device pass): region r of the strip to block map[r] of
 * d_lbuffer, nothing for the regions the fill plan fills.  For BINNED
 * attenuation renders of the L-buffer only (image and u8 NULL), typically with
 * XRT_MISS_TRANSIT; `packed_floats` is the L-buffer's capacity in floats.  A
 * frame whose fill plan does not hold (or does not fit) is not rendered and
 * returns XRT_ERR_OVERFLOW.  0 restores the row-major layout.
 */
int xrt_set_transit_layout(xrt_context* ctx, uint64_t packed_floats);

/*
 * Many strips' packed regions in one launch: d_desc holds 4 u32 per block --
 * first frame row, rows of the block inside its strip (<= 32), first column,
 * packed block index in d_packed (0xFFFFFFFF: a filled region, all misses).
 * The planes are whole frames (row-major, `width` columns).  16-B aligned.
 */
int xrt_unpack_blocks_device(xrt_context* ctx, uint32_t width, uint64_t n_blocks, const uint32_t* d_desc,
                             const float* d_packed, float* d_lbuffer, float* d_image, uint8_t* d_u8, void* stream);

/* --- hit transit (multi-GPU gathers) ------------------------------------- */

/*
 * Hit-only strips: a strip's message holds, per tile of its fill plan (8x8
 * pixels; tile t of tile slot s is tile i = 16 s + t), a 64-bit mask of the
 * tile's rays that hit mesh 0 (bit 8 y + x for pixel (x, y) of the tile) at
 * 32-bit words [2i, 2i + 2), then the hit rays' L values -- tile by tile, in
 * bit order -- from word 2 n_tiles.  A miss is an unset bit (its L is +inf,
 * image 80, u8 255); the filled regions send nothing.  The per-tile hit counts
 * are a function of the strip's geometry, like the fill plan.
 *
 * xrt_plan_hit_layout: the hit plan of the last frame's geometry, from that
 * frame's records (it must be a BINNED render of that geometry over its fill
 * plan: typically the geometry's first frame, row-major).  *n_tiles = 16 x
 * the plan's tile slots, *words = the message's words (2 n_tiles + hits);
 * tile_hits (nullable, `capacity` entries) receives each tile's hit count.
 * Synchronous.  The tiles' order is xrt_plan_region_map's: tile slot s is
 * packed region s.
 * xrt_set_transit_hits: renders of this context write the hit layout into
 * d_lbuffer (capacity_words >= *words + 64), instead of the packed
 * (xrt_set_transit_layout) or row-major layout; 0 turns it off.  For BINNED
 * attenuation renders of the L-buffer only; a frame of another geometry than
 * the plan's, or whose fill plan does not hold, is not rendered and returns
 * XRT_ERR_OVERFLOW.
 * xrt_unpack_hits_device: many strips' messages in one launch on the receiver
 * -- d_desc as xrt_unpack_blocks_device's, its last word the index in d_tdesc
 * of the region's first tile descriptor (or 0xFFFFFFFF: a filled region);
 * d_tdesc holds 4 u32 per tile: the word of its mask in d_msg, the word of its
 * first hit value, its planned hit count, 0.  A mask whose count is not the
 * planned one sets *d_bad (nullable) to 1.  d_desc, d_tdesc 16-B aligned;
 * d_msg 8-B aligned.
 */
int xrt_plan_hit_layout(xrt_context* ctx, uint32_t* tile_hits, uint64_t capacity, uint64_t* n_tiles,
                        uint64_t* words);
int xrt_set_transit_hits(xrt_context* ctx, uint64_t capacity_words);
int xrt_unpack_hits_device(xrt_context* ctx, uint32_t width, uint64_t n_blocks, const uint32_t* d_desc,
                           const uint32_t* d_tdesc, const uint32_t* d_msg, float* d_lbuffer, float* d_image,
                           uint8_t* d_u8, uint32_t* d_bad, void* stream);

/*
 * Test hooks, device probes and diagnostics: include/xrt_debug.h (not part of
 * the drop-in surface).
 */

#ifdef __cplusplus
}
#endif

#endif /* XRT_H */
