/*
 * xrt_debug.h -- test hooks, device probes and diagnostics of libxrt.so.
 *
 * Not part of the drop-in boundary (include/xrt.h): the parity tests, the
 * benchmark's measurement tools and the CPU test suite use these to reach
 * the exact device code paths (Ray::intersect, expf, the LUT, k_prep), to
 * force the rare exact paths (hit-list overflow, list overflow, fill-plan
 * fallback) and to read the pipeline's counters and timing records.
 */
#ifndef XRT_DEBUG_H
#define XRT_DEBUG_H

#include "xrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- device probes of the exact device code paths ----------------------- */

/*
 * Runs the kernel's Ray::intersect (src/Ray.cxx:72-124) on the device:
 * rays[6*i] = origin xyz, unit direction xyz; triangles[9*i] = p1, p2, p3.
 * hit[i] = 0/1, t[i] = distance (0 when no hit).  Host buffers.
 */
int xrt_probe_intersect(xrt_context* ctx, const float* rays, const float* triangles,
                        uint64_t n, uint8_t* hit, float* t);

typedef enum xrt_probe_op {
    XRT_PROBE_EXPF = 0,     /* std::exp(float) == glibc expf                     */
    XRT_PROBE_SQRTF = 1,    /* std::sqrt(float), correctly rounded               */
    XRT_PROBE_RCP = 2,      /* (float)(1.0 / (double)x), src/Ray.cxx:99           */
    XRT_PROBE_LUT_U8 = 3,   /* 8-bit LUT of a photon value (out[i] = (float)u8)  */
    XRT_PROBE_RCP_FAST = 4, /* the culled tests' 1/det (rcp + Newton where exact) */
    XRT_PROBE_SIGNED_L = 5, /* (float)(80.0 * exp(-(0.1037f * (d * 0.1)))): the signed
                               model's L for distance d (glibc exp in f64)          */
    XRT_PROBE_LOGF = 6      /* std::log(float) == glibc logf (a NaN by class)    */
} xrt_probe_op;

/* Evaluates one scalar device function elementwise.  Host buffers. */
int xrt_probe_math(xrt_context* ctx, int op, const float* in, float* out, uint64_t n);

/*
 * Runs the per-render triangle preparation (k_prep) of the uploaded mesh for
 * `camera` and copies its outputs to the host: records[16*i] = edge1, edge2,
 * tvec, qvec, t*det, pad (the ray-independent terms of Ray::intersect,
 * src/Ray.cxx:86-122) and footprint[16*i] = bbox (xmin, xmax, ymin, ymax) and
 * the three relaxed edge functions (a, b, c, 0) of the tile cull.  Either
 * output may be NULL.
 */
int xrt_probe_prep(xrt_context* ctx, const xrt_camera* camera, float* records, float* footprint);

/*
 * Host-side evaluation of the device expf restatement (the same source,
 * compiled for the host): lets CPU-only tests check it against libm.
 */
void xrt_host_expf_batch(const float* in, float* out, uint64_t n);

/*
 * The same for the signed model: the device glibc exp restatement, and its L
 * update (float)(80.0 * exp(-(mu * (distance * 0.1)))) (-1 for a non-zero
 * sign sum; sign_sum may be NULL for all zero).
 */
void xrt_host_exp_batch(const double* in, double* out, uint64_t n);
void xrt_host_signed_lbuffer_batch(const float* distance, const int32_t* sign_sum, float mu, float* out,
                                   uint64_t n);

/*
 * The materials model's chained update for n rays of given per-mesh sums: ray
 * i's mesh m has distance[i * num_meshes + m] and sign_sum[i * num_meshes + m]
 * (sign_sum may be NULL for all zero); out[i] = L after the last mesh, from
 * L = 80.  _host_: the device source compiled for the host; _probe_: the same
 * on the device (beside XRT_PROBE_SIGNED_L).  Host buffers.
 */
void xrt_host_materials_lbuffer_batch(const float* distance, const int32_t* sign_sum, const float* mu,
                                      uint32_t num_meshes, float* out, uint64_t n);
int xrt_probe_materials(xrt_context* ctx, const float* distance, const int32_t* sign_sum, const float* mu,
                        uint32_t num_meshes, float* out, uint64_t n);

/*
 * The spectrum model's L (xrt.h, XRT_MODEL_SPECTRUM) for n rays of given
 * per-mesh sums, laid out as the materials pair's; weight[num_bins] and
 * mu[num_meshes * num_bins], mesh-major, as xrt_set_spectrum takes them (not
 * validated here).  _host_: the device source compiled for the host; _probe_:
 * the same on the device.  xrt_host_spectrum_miss: the value of a ray without
 * a hit, the weight chain the device table carries.  Host buffers.
 */
void xrt_host_spectrum_lbuffer_batch(const float* distance, const int32_t* sign_sum, const float* weight,
                                     const float* mu, uint32_t num_meshes, uint32_t num_bins, float* out,
                                     uint64_t n);
float xrt_host_spectrum_miss(const float* weight, uint32_t num_bins);
int xrt_probe_spectrum(xrt_context* ctx, const float* distance, const int32_t* sign_sum, const float* weight,
                       const float* mu, uint32_t num_meshes, uint32_t num_bins, float* out, uint64_t n);

/*
 * Test hook: caps the per-ray register hit list at `capacity` (1..12) so the
 * exact overflow path runs.  0 restores the default (12).
 */
int xrt_set_hit_capacity(xrt_context* ctx, uint32_t capacity);

/*
 * Test hook: caps the BINNED kernel's region-list capacity at `entries` so the
 * whole-mesh fallback runs.  0 restores automatic sizing.
 */
int xrt_set_bin_capacity(xrt_context* ctx, uint64_t entries);

/*
 * The BINNED kernel's fill plan (DESIGN.md "Fill plan"): regions whose lists
 * the geometry's sizing frame counted empty render as one miss-filling
 * workgroup each instead of 16 tile waves.  mode 1 (default) on, 0 off;
 * test hook 2 plans every region as empty, so every workgroup takes the
 * exact fallback of a region that is not.  The next frame re-sizes (after a
 * camera change under the same image size and strip the context keeps its
 * lists and plan instead: DESIGN.md "Moving camera").
 */
int xrt_set_fill_plan(xrt_context* ctx, int mode);

/* Diagnostics: regions the last enqueued BINNED frame rendered through the fill plan. */
int xrt_debug_fill_regions(xrt_context* ctx, uint32_t* regions);

/*
 * Diagnostics: BINNED frames by geometry path since the context was created --
 * counters[0] frames whose lists were sized synchronously (a new frame
 * geometry), [1] frames rendered over lists sized for another camera of the
 * same region grid (a moving camera), [2] frames k_prep flagged for a fill-plan
 * miss, [3] frames k_prep flagged for a list overflow.
 */
int xrt_debug_geometry_counters(xrt_context* ctx, uint64_t counters[4]);

/*
 * Diagnostics: counters[0] = host-buffer frames (xrt_render_rows) of a geometry
 * seen for the first time that were sized on the device (the count pass, one
 * 32-byte read-back of its pair
 * total, the lists carved and filled by k_size_lists / k_scatter_pairs; no
 * host plan, no second k_prep; XRT_DEVICE_FIRST=0 turns it off), [1] = those
 * whose pool was too small for the pair total, grown and counted again, [2] /
 * [3] = the last such frame's pair total and the pool its count pass had.
 */
int xrt_debug_first_frames(xrt_context* ctx, uint64_t counters[4]);

/*
 * Diagnostics: the frame pipeline since the context was created --
 * counters[0] frames rendered from a preparation made ahead of their call
 * (xrt_render_rows_device repeating its frame geometry), [1] preparations made
 * ahead and dropped (the next call's geometry or settings differed), [2]
 * renders launched with their preparation already complete (no wait), [3]
 * renders launched after the host read k_prep's check (sizing / validation).
 */
int xrt_debug_pipeline_counters(xrt_context* ctx, uint64_t counters[4]);

/*
 * Diagnostics: copies the last render's statistics records (32 bytes each, one
 * per workgroup -- per tile wave for BINNED: u32 rays, hit rays, odd rays,
 * overflow rays, hits, wave-level triangle tests, candidates, max hits)
 * into `dst`, at most `capacity` bytes; `*n_records` receives the number of
 * records.
 */
int xrt_debug_block_records(xrt_context* ctx, void* dst, uint64_t capacity, uint64_t* n_records);

/*
 * Diagnostics: the timing records of the render `frames_back` frames before
 * the last (0 = the last; up to XRT_FRAME_SETS - 1 = 3; after a timed region too), one per statistics
 * record (u32 s_memrealtime start, u32 end; 100 MHz, low 32 bits), into `dst`,
 * at most `capacity` records; `*n_records` receives their number.
 */
int xrt_debug_wave_times(xrt_context* ctx, uint32_t frames_back, uint32_t* dst, uint64_t capacity,
                         uint64_t* n_records);


/*
 * Test hook (host code, no device): for each i, the culled render's
 * division-free reject mt_may_hit(det, a, b, tnum) and the exact remainder of
 * Ray::intersect from the same numerators (hit with t > 1e-7, and t).
 */
void xrt_host_mt_check(const float* det, const float* a, const float* b, const float* tnum, uint64_t n,
                       uint8_t* may_hit, uint8_t* hit, float* t);

/*
 * Diagnostics: host time of the last xrt_render_rows call (host buffers), ms:
 * ms[0] device planes (allocated once per size), [1] enqueue (preparation,
 * list sizing of a new geometry, launch), [2] wait for the render, [3] D2H of
 * the planes (DMA into the context's pinned ring, overlapped with its copy
 * threads moving the pieces into the caller's pages), [4] copy threads (a
 * count), [5] MB copied, [6] statistics, [7] total; within them [8] the time
 * in hipMalloc, [9] a new frame geometry's list sizing, [10] synchronisations
 * before a launch layout's upload (only when frames in flight may read it) --
 * [13] of which the prep stream's, [14] the buffer sets' render events',
 * [15] the last stream's --, [11] host waits for the preparation (k_prep),
 * [12] kernel launches.
 */
int xrt_debug_host_call_ms(xrt_context* ctx, double ms[16]);

/*
 * Diagnostics: [0] binned frames rendered with a tile plan (tiles that had no
 * survivor in an earlier frame of the same geometry store their misses without
 * reading the region's list), [1] tile plans taken.
 * The plan is OFF by default (it reuses an earlier frame's cull results, so
 * it only helps a loop of identical frames); XRT_TILE_PLAN=1 in the
 * environment at xrt_create, or xrt_debug_set_tile_plan, turns it on.
 */
int xrt_debug_tile_plan(xrt_context* ctx, uint64_t counters[2]);

/*
 * Host code (no device): the cull's direction grid of `camera` (DESIGN.md
 * section 5, step 0) as the library computes it -- grids[0], a bisection per
 * axis -- and by a scan of every row or column, grids[1].  Equal for every
 * camera (the test's claim).  An axis on which up and right are both nonzero
 * has no scan: both take its O(1) lower bound, which tests/test_camera_cpu.py
 * holds against every pixel's direction instead.
 */
int xrt_debug_direction_grid(const xrt_camera* camera, int grids[2]);

/*
 * Test hook (host code, no device): the tile cull's footprints of n triangles
 * (tris[9*i] = p1, p2, p3) under `camera` -- the records as k_prep forms
 * them, the cull parameters as the library forms them, compute_footprint
 * compiled for the host -- in xrt_probe_prep's layout: footprint16[16*i] = box
 * (xmin, xmax, ymin, ymax) and the three relaxed edges (a, b, c, .).  The
 * device's reciprocal square root differs from the host's by an ulp, so the
 * edges of the two agree closely, not bit for bit.
 */
int xrt_host_footprints(const xrt_camera* camera, const float* tris, uint64_t n, float* footprint16);

/* Turns the tile plan on (1) or off (0) for later frames. */
int xrt_debug_set_tile_plan(xrt_context* ctx, int on);

/*
 * The ray table ("Ray table"): an attenuation BINNED
 * frame that repeats the previous one's camera, image size and strip has the
 * camera's ray directions tabulated once on the device, and the frames after
 * it read them instead of generating them (bit for bit the same rays).  On by
 * default within XRT_RAY_CACHE_MB megabytes (256; 0 = never), read from the
 * environment at xrt_create.  xrt_debug_set_ray_table turns it off (0) or on
 * (1) for later frames.  counters: [0] fills launched, [1] frames rendered
 * from the table, [2] frames in its scope that computed their rays (no fill
 * yet, a fill postponed behind renders in flight, over the budget, or off),
 * [3] bytes held.
 */
int xrt_debug_set_ray_table(xrt_context* ctx, int on);
int xrt_debug_ray_table_counters(xrt_context* ctx, uint64_t counters[4]);

/*
 * Host code (no device): where the table of a width x height image's strip
 * [row_begin, row_end) keeps dx of pixel (row, col), in floats -- dy and dz lie
 * 64 and 128 floats further --, by the function the two kernels use; *floats
 * (may be NULL) receives the table's size in floats.
 */
int xrt_debug_ray_table_index(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t row,
                              uint32_t col, uint64_t* index, uint64_t* floats);

/*
 * The valid table's contents: waits on the host for its fill and copies the
 * whole table -- xrt_debug_ray_table_index's *floats for its key, padding
 * included -- into dst; dims (may be NULL) = the key's width, height,
 * row_begin, row_end.  XRT_ERR_NO_MESH while no table is valid (none filled
 * yet, or a frame of another key came since); XRT_ERR_ARGUMENT for a NULL dst
 * or `floats` below the table's size ([3] bytes held / 4 always suffices).
 * Changes nothing that decides how later frames take their rays.
 */
int xrt_debug_ray_table_read(xrt_context* ctx, float* dst, uint64_t floats, uint32_t dims[4]);

/*
 * Diagnostics: k_prep's per-wave timestamps.  enable 1 / 0 turns the records
 * on / off for later launches (-1 leaves it); *n_waves = the waves of the last
 * recorded launch; with dst, waits for the context's work and copies up to
 * `capacity` records of 8 u32 (s_memrealtime, 100 MHz, low 32 bits): the
 * wave's start, its triangle's record formed, its footprint, the binning's LDS
 * staging and scan, the union of its rectangles, small then large rectangles'
 * cells tested, its end.
 */
int xrt_debug_prep_times(xrt_context* ctx, int enable, uint32_t* dst, uint64_t capacity, uint64_t* n_waves);

/*
 * Diagnostics: the phases of the last xrt_destroy, ms: [0] waiting for the
 * context's own work, [1] device frees, [2] pinned host frees, [3] streams and
 * events destroyed.
 */
int xrt_debug_destroy_ms(double ms[4]);

/*
 * The soup the next render would read (xrt_set_pose): runs k_pose if one is
 * due, waits for it and copies the scene's 9 floats per triangle into dst.
 * *n_floats = the soup's size; dst NULL only asks for it, a capacity below it
 * is XRT_ERR_ARGUMENT.
 */
int xrt_debug_posed_triangles(xrt_context* ctx, float* dst, uint64_t capacity_floats, uint64_t* n_floats);

/*
 * Diagnostics: the whole posed soup written `launches` times back to back
 * (every mesh marked due each time), by device events on the prep stream:
 * microseconds per writing.  Needs a pose; waits for the context's work.
 */
int xrt_debug_pose_span(xrt_context* ctx, uint32_t launches, double* us_per_write);

/* Diagnostics: [0] k_pose launches so far, [1] the triangles they wrote. */
int xrt_debug_pose_counters(xrt_context* ctx, uint64_t counters[2]);

/*
 * Test hook (host code, no device): xrt_detector_response's arithmetic over
 * whole planes, by the function k_lsf runs per tap (lsf_chunk, host-compiled).
 * Arguments and checks as xrt_detector_response's, host buffers.
 */
int xrt_host_lsf(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, const float* lsf_x,
                 uint32_t taps_x, const float* lsf_y, uint32_t taps_y, float* out, uint8_t* out_u8);

/*
 * Test hooks (host code, no device) of the line-integral projections:
 * xrt_host_logf_batch is the device logf restatement compiled for the host
 * (against libm and tests/logf_ref.py on a machine without a GPU);
 * xrt_host_log_projection is xrt_log_projection's pixel function over whole
 * buffers, arguments and checks as xrt_log_projection's, host buffers.
 */
void xrt_host_logf_batch(const float* in, float* out, uint64_t n);
int xrt_host_log_projection(uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                            const float* flat, const float* dark, float flat_value, float t_min, int order,
                            float* out);

/*
 * Test hooks of the photon noise.  Host code, no device: xrt_host_philox4x32
 * is the generator on one counter and key (the published known answers);
 * xrt_host_poisson_batch is the device's sampler compiled for the host, out[i]
 * = the count N (f64; NaN and +inf as the contract has them) of the mean
 * lam[i] under the word words[i]; xrt_host_photon_noise is xrt_photon_noise's
 * pixel function over whole buffers, arguments and checks as
 * xrt_photon_noise's, host buffers.  xrt_debug_poisson_batch is
 * xrt_host_poisson_batch on the device, by a small kernel of its own.
 */
void xrt_host_philox4x32(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
void xrt_host_poisson_batch(const double* lam, const uint32_t* words, uint64_t n, double* out);
int xrt_host_photon_noise(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, float gain,
                          uint64_t seed, uint64_t first_index, int mode, float* out);
int xrt_debug_poisson_batch(xrt_context* ctx, const double* lam, const uint32_t* words, uint64_t n, double* out);

/*
 * Test hooks of the scatter model.  Host code, no device: the arithmetic of
 * k_scatter_source and k_scatter_add -- the pixel functions the kernels call,
 * the source's two-level sum in the contract's order -- over whole planes,
 * arguments and checks as xrt_scatter_source's and xrt_scatter_add's, host
 * buffers.
 */
int xrt_host_scatter_source(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes, const float* paths,
                            const uint16_t* open, const float* weight, const float* mu, const float* sigma,
                            uint32_t num_bins, uint32_t bin, float* lbuffer, float* source);
int xrt_host_scatter_add(uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin, const float* blurred,
                         uint32_t num_kernels, const float* amp, const float* primary, float* out, float* out_scatter,
                         uint8_t* out_u8);

/*
 * Test hook of the area sampling.  Host code, no device: xrt_area_integrate's
 * pixel function -- the one k_area_integrate calls -- over whole buffers,
 * arguments and checks as xrt_area_integrate's, host buffers.
 */
int xrt_host_area_integrate(uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y, uint32_t num_sources,
                            uint32_t num_planes, const float* weight, const float* image, float* out, uint8_t* out_u8);

/*
 * Test hook of the spectral detector.  Host code, no device:
 * xrt_spectral_detector's pixel function -- the one k_spectral_detector calls,
 * compiled for the host -- over whole buffers, arguments and checks as
 * xrt_spectral_detector's, host buffers.
 */
int xrt_host_spectral_detector(uint64_t num_pixels, uint32_t num_meshes, const float* paths, const uint16_t* open,
                               const float* weight, const float* mu, uint32_t num_bins, const float* response,
                               uint32_t num_channels, float gain, float read_noise, uint64_t seed, uint64_t first_index,
                               int draw_mode, int out_mode, float* out);

/*
 * Test hook of the voxel trace.  Host code, no device: xrt_volume_paths' ray
 * function -- volume_ray, the one k_volume_paths calls, compiled for the host
 * -- over whole host buffers.  The volume's arrays are taken directly
 * (arguments and checks as xrt_upload_volume's), the camera, strip and planes
 * as xrt_volume_paths'.
 */
int xrt_host_volume_paths(const xrt_camera* camera, uint32_t row_begin, uint32_t row_end, const uint8_t* labels,
                          const float* density, const uint32_t dims[3], const float origin[3], const float spacing[3],
                          uint32_t num_labels, float* paths);

/*
 * The shape of k_volume_paths' waves, for the A/B its layout rests on
 * (tools/volume_timing.py): rows = 0, the default, 8 x 8 pixel tiles; rows != 0,
 * 64 x 1 row segments.  The planes are the same bit for bit.
 */
int xrt_debug_volume_wave_shape(xrt_context* ctx, int rows);

/*
 * Test hooks of FDK reconstruction.  Host code, no device: xrt_fdk_filter's
 * contract as include/xrt.h writes it, and xrt_backproject's per-plane
 * arithmetic -- backproject_term, the one k_backproject calls, compiled for
 * the host -- over whole host buffers.  Arguments and checks as the host
 * forms'.
 */
int xrt_host_fdk_filter(uint32_t width, uint32_t height, uint32_t num_planes, const float* image, const float* weight,
                        const float* taps, uint32_t num_taps, float* out);
int xrt_host_backproject(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                         const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end, double scale, int accumulate,
                         float* volume);

/*
 * Test hooks of SIRT / OS-SART.  Host code, no device: forward_pixel and
 * volume_update_voxel -- the functions k_forward_project and k_volume_update
 * call, compiled for the host -- over whole host buffers, and xrt_sirt's
 * algorithm over them and xrt_host_backproject.  Arguments and checks as the
 * host forms'.
 */
int xrt_host_forward_project(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                             const uint32_t dims[3], const float spacing[3], const double* rays, int mode,
                             const float* meas, float* out);
int xrt_host_volume_update(uint64_t n, float* x, const float* corr, const float* norm, double relax, float lo, float hi);
int xrt_host_sirt(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                  const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets, double relax,
                  float lo, float hi, float* volume);

/*
 * Test hooks of TV-regularised SIRT.  Host code, no device: tv_quotients,
 * tv_voxel, sumsq_entry and tv_step_voxel -- the functions k_tv_gradient,
 * k_sumsq_first and k_tv_step call, compiled for the host -- over whole host
 * buffers, the sum's order as written, and xrt_sirt_tv's algorithm over
 * them and xrt_host_sirt's pieces.  Arguments and checks as the host forms'.
 */
int xrt_host_tv_gradient(const float* volume, const uint32_t dims[3], double eps, float* out);
int xrt_host_volume_sumsq(uint64_t n, const float* a, const float* b, double* out);
int xrt_host_tv_descend(float* volume, const uint32_t dims[3], double eps, uint32_t steps, double length, float lo, float hi);
int xrt_host_sirt_tv(uint32_t width, uint32_t height, uint32_t num_planes, const float* proj, const double* matrices,
                     const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets, double relax,
                     float lo, float hi, const xrt_tv_params* tv, float* volume);

/*
 * Test hooks of OS-MLTR.  Host code, no device: poisson_pixel,
 * backproject_pair_term and volume_update_voxel -- the functions
 * k_poisson_project and k_backproject_update call, compiled for the host --
 * over whole host buffers, and xrt_mltr's algorithm over them and
 * xrt_host_sirt_tv's descent.  Arguments and checks as the host forms'.
 */
int xrt_host_poisson_project(uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                             const uint32_t dims[3], const float spacing[3], const double* rays, const float* counts,
                             const float* flat, const float* background, float* pairs);
int xrt_host_backproject_update(uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs,
                                const double* matrices, const uint32_t dims[3], double relax, float lo, float hi,
                                float* volume);
int xrt_host_mltr(uint32_t width, uint32_t height, uint32_t num_planes, const float* counts, const float* flat,
                  const float* background, const double* matrices, const uint32_t dims[3], const float spacing[3],
                  uint32_t iterations, uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv,
                  float* volume);

/*
 * Test hook of the voxeliser.  Host code, no device: xrt_voxelize's crossing
 * and voxel functions -- voxel_footprint, voxel_crossing, voxel_label and
 * voxel_value, the ones the kernels call, compiled for the host -- over whole
 * host buffers.  The soup (the num_meshes meshes' triangles one after
 * another, 9 f32 each, already posed) and mesh_triangles are taken directly;
 * the grid, value and outputs and their checks are xrt_voxelize's.
 */
int xrt_host_voxelize(const float* soup, const uint64_t* mesh_triangles, uint32_t num_meshes, const uint32_t dims[3],
                      const float origin[3], const float spacing[3], const float* value, uint16_t* mask, uint8_t* labels,
                      float* volume, uint64_t* odd_columns);

/*
 * The scatter's schedule, for the A/B its threshold rests on
 * (tools/voxelize_timing.py): a triangle whose footprint box holds at least
 * `columns` grid columns is queued for the tile waves, a smaller one is
 * covered by its own lane; 0 restores the default, 0xFFFFFFFF queues none.
 * The outputs are the same bit for bit.
 */
int xrt_debug_voxelize_threshold(xrt_context* ctx, uint32_t columns);

/*
 * Diagnostics, timing only: the steps the next voxelisations enqueue, a sum of
 * 1 (the scatter and the tile waves), 2 (the scan) and 4 (clearing the flip
 * volume); 7 is the default.  With a step left out the outputs mean nothing.
 * Adding 8 keeps the scan from splitting a small grid's slices into runs: the
 * outputs are the same bit for bit.
 */
int xrt_debug_voxelize_stages(xrt_context* ctx, uint32_t stages);

/*
 * Diagnostics: the last voxelisation's triangles, [0] covered by their own
 * lane, [1] queued for the tile waves, [2] the queue entries they reserved,
 * [3] of [0] those that found the queue full.  Waits for that call;
 * XRT_ERR_ARGUMENT once another user of the working set has run.
 */
int xrt_debug_voxelize_counters(xrt_context* ctx, uint64_t counters[4]);

/*
 * Test hook of material decomposition.  Host code, no device: xrt_decompose's
 * pixel function -- decompose_pixel, the one k_decompose calls, compiled for
 * the host -- over whole buffers, arguments and checks as xrt_decompose's, host
 * buffers.
 */
int xrt_host_decompose(uint64_t num_pixels, const float* channels, const uint16_t* open, const float* weight, const float* mu,
                       uint32_t num_basis, uint32_t num_bins, const float* response, uint32_t num_channels, float gain,
                       int in_mode, const double* guess, uint32_t max_iter, double tol, double damping, float* out,
                       uint8_t* iters);

/*
 * Diagnostics of a multi context's transit (xrt_multi_set_transit): [0]
 * frames whose strips travelled in the hit layout, [1] frames that travelled
 * packed, [2] bytes the last frame sent into device 0, [3] 1 when a received
 * hit mask disagreed with its sender's plan (waits for the last gather).
 */
int xrt_multi_transit_stats(xrt_multi* m, uint64_t out[4]);

/*
 * Diagnostics of a multi context's balanced split (xrt_multi_set_split): [0]
 * balanced plans made (each from the strips' own records of an earlier
 * frame -- no extra render), [1] frames split equally because no such model
 * existed yet (the first frame), [2] link probes run (at most one per gather
 * path), [3] strip models collected (one per new camera).
 */
int xrt_multi_plan_stats(xrt_multi* m, uint64_t out[4]);

/*
 * Test hook: the expected hit count of the first tile of the first sender's
 * hit plan plus one, so the next hit frame's receive disagrees with its plan
 * (the mismatch path: the frame's call fails, the plans are made again).
 */
int xrt_multi_debug_corrupt_hit_plan(xrt_multi* m);

#ifdef __cplusplus
}
#endif

#endif /* XRT_DEBUG_H */
