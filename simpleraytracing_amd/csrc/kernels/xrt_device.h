// xrt_device.h -- device-side arithmetic of the X-ray render path (gfx950).
//
// Every function here reproduces the reference's f32/f64 rounding sequence
// exactly, so the GPU image is bit-identical to src/main.cxx's.  The numerical
// contract (DESIGN.md "Numerical contract"):
//   * no FMA contraction on the f32 path (built with -ffp-contract=off, and the
//     pragma below); the only fused ops are the explicit fma() calls of
//     glibc's expf, which are part of that function's definition;
//   * f32 sqrt is correctly rounded (HIP's default
//     -fhip-fp32-correctly-rounded-divide-sqrt); src/Ray.cxx:99's
//     (float)(1.0/(double)det) is the correctly rounded f32 1.0f/det for
//     every det (inv_det_of);
//   * f32 denormals are preserved (no -fgpu-flush-denormals-to-zero).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

// Variant builds (tools/build_variants.sh) get their own kernel namespace so
// several can be loaded side by side without kernel-name collisions.
#ifndef XRT_KERNEL_NS
#define XRT_KERNEL_NS xrt
#endif

// Tuning constants (overridable with -D for A/B builds, tools/build_variants.sh);
// the defaults are the measured-faster choices.
#ifndef XRT_TILE_WAVES
#define XRT_TILE_WAVES 2  // binned render: tile waves per workgroup (2: 2048^2 step -4 %, 1.12M-tri -5 % vs 4)
#endif
#ifndef XRT_RENDER_WAVES
#define XRT_RENDER_WAVES 8   // binned render: minimum waves per SIMD (8 = 64 VGPRs)
#endif
#ifndef XRT_STAGE
#define XRT_STAGE 64      // binned render: candidates a tile wave culls per round -- one footprint per lane, read into registers (64..256); only survivors' records go to the wave's 4-KB LDS stage
#endif
#ifndef XRT_PREP_THREADS
#define XRT_PREP_THREADS 64  // k_prep workgroup size (64: single-wave groups fill the render's holes)
#endif

namespace XRT_KERNEL_NS {

// Per-render triangle record: the ray-independent part of Ray::intersect
// (src/Ray.cxx:86-122) for the shared ray origin.  64 bytes, read
// wave-uniformly (one s_load_dwordx16 per triangle).
struct alignas(16) TriRec {
    float e1x, e1y, e1z;    // edge1 = P2 - P1                 Ray.cxx:86
    float e2x, e2y, e2z;    // edge2 = P3 - P1                 Ray.cxx:87
    float tvx, tvy, tvz;    // tvec  = origin - P1             Ray.cxx:102
    float qvx, qvy, qvz;    // qvec  = tvec x edge1            Ray.cxx:112
    float tnum;             // edge2 . qvec  (t * det)          Ray.cxx:122
    float pad0, pad1, pad2;
};
static_assert(sizeof(TriRec) == 64, "TriRec must be 64 bytes");

// Conservative screen-space footprint of a triangle (DESIGN.md "Tile cull"),
// stored structure-of-arrays as four float4 planes of length T:
//   plane 0  bbox  = (xmin, xmax, ymin, ymax) in pixel-centre coordinates
//   plane 1..3 edge k = (a, b, c, 0):  a*col + b*row + c >= 0 holds at every
//   pixel whose ray the reference's Ray::intersect can report as a hit with
//   t > 1e-7.
constexpr int kCullPlanes = 4;

// Camera + strip parameters, passed by value.
struct RenderParams {
    float ox, oy, oz;       // RayTracerInfo::origin
    float cx, cy, cz;       // RayTracerInfo::detector_position
    float ux, uy, uz;       // RayTracerInfo::up
    float rx, ry, rz;       // RayTracerInfo::right
    float spacing;          // pixel_spacing, main.cxx:639-641
    uint32_t width, height; // full image
    uint32_t row_begin, row_end;
    uint32_t num_triangles;
    uint32_t hit_capacity;  // <= XRT_MAX_HITS
    uint32_t prep_tris;     // triangles per k_prep wave (prep_tris_for)
    uint32_t model;         // kModelAttenuation (main.cxx), kModelSigned (the L-buffer fork), kModelMaterials, kModelSpectrum or kModelPaths
};

// What a render computes per ray.
constexpr uint32_t kModelAttenuation = 0;   // renderLoop, src/main.cxx:626-743
constexpr uint32_t kModelSigned = 1;        // renderLoopCallBack, src/main-pthreads-lbuffer.cxx:733-813
constexpr uint32_t kModelMaterials = 2;     // the fork's loop over every mesh, each with its own coefficient

// The materials model's scene: mesh m holds the triangle ids [end of mesh
// m - 1, end) of the scene soup and attenuates with mu (at most kMaxMeshes).
constexpr uint32_t kMaxMeshes = 16;
struct MeshMaterial {
    uint32_t end;
    float mu;
};

// The spectrum model: num_bins energy bins over the materials
// model's scene, I = sum_e weight[e] * exp(-sum_m mu[m * num_bins + e] * d_m).
// One device table: the meshes' id-range ends, the bins' weights, the f32 a
// ray without a hit gets (the host's weight chain, spectrum_miss) and the
// coefficients, mesh-major.
constexpr uint32_t kModelSpectrum = 3;
constexpr uint32_t kMaxBins = 32;
struct SpectrumTable {
    uint32_t end[kMaxMeshes];
    float weight[kMaxBins];
    float miss;
    uint32_t num_bins;
    float mu[kMaxMeshes * kMaxBins];   // [m * num_bins + e]
};

// The paths model: the render stores the per-mesh sums themselves
// -- one f32 plane of signed path lengths per mesh and a 16-bit plane whose
// bit m says that mesh m's signs do not cancel on the ray -- for
// k_apply_spectrum to integrate under any spectrum table afterwards.
constexpr uint32_t kModelPaths = 4;
static_assert(kMaxMeshes <= 16u, "a ray's open mask is 16 bits");

// Mesh poses: a pose is a row-major 3x4 [R | t]; k_pose writes
// the posed soup from the rest soup (what was uploaded), mesh by mesh.  The
// table travels by value in k_pose's kernel arguments: the poses, the meshes'
// id-range ends (0xFFFFFFFF past the scene's last mesh) and a bit per mesh
// whose pose is bitwise the identity (its vertices are copied, not computed).
constexpr uint32_t kPoseFloats = 12;
struct PoseTable {
    float pose[kMaxMeshes][kPoseFloats];
    uint32_t end[kMaxMeshes];
    uint32_t identity;
};

// One vertex under one pose: the fork's transformMatrix product
// (src/main-pthreads-lbuffer.cxx:561-564), three f32 products summed left to
// right, p_i = (r_i0 * x + r_i1 * y) + r_i2 * z, every product and sum rounded
// on its own (__fmul_rn / __fadd_rn on the device, no contraction on the
// host).  The translation is added only when some t_j is not +-0: with t = 0
// the result is the fork's expression bit for bit (p_i + 0.0f would turn a
// -0.0f into +0.0f).  The identity is the caller's business (PoseTable).
__host__ __device__ __forceinline__ float pose_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

__host__ __device__ __forceinline__ float pose_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

__host__ __device__ __forceinline__ void pose_vertex(const float* pose, float x, float y, float z, float& ox,
                                                     float& oy, float& oz)
{
    float p[3];
    for (int i = 0; i < 3; ++i) {
        const float* r = pose + 4 * i;
        p[i] = pose_add(pose_add(pose_mul(r[0], x), pose_mul(r[1], y)), pose_mul(r[2], z));
    }
    if (pose[3] != 0.0f || pose[7] != 0.0f || pose[11] != 0.0f)
        for (int i = 0; i < 3; ++i) p[i] = pose_add(p[i], pose[4 * i + 3]);
    ox = p[0];
    oy = p[1];
    oz = p[2];
}

// Register hit list per ray.  Each slot costs every exact test one
// v_med3_f32; a ray with more hits is recomputed exactly by its wave
// (finish_ray's fix-up, tens of microseconds for that wave).  dragon.ply rays
// have at most 12 hits (2048^2: 102 rays above 8): 12 slots render it 3 %
// faster than 16 with no fix-up; 8 slots would send those 102 rays through
// it and run 5x slower (DESIGN.md "Hit list").
#ifndef XRT_MAX_HITS
#define XRT_MAX_HITS 12
#endif
constexpr int kMaxHits = XRT_MAX_HITS;

// ---------------------------------------------------------------------------
// Ray generation: src/main.cxx:652-661 and the Ray ctor, include/Ray.inl:74-85.
// ---------------------------------------------------------------------------
// :655-656  float * (0.5 + unsigned - unsigned / 2.0) in double, narrowed once.
// A function of one pixel index: k_prep tabulates it per frame (pixel_offsets)
// for the render kernels.
__host__ __device__ __forceinline__ float pixel_offset(float spacing, uint32_t i, uint32_t n)
{
    return (float)((double)spacing * ((0.5 + (double)i) - (double)n / 2.0));
}

// The frame's pixel offsets: v_off of every image row, then u_off of every
// column (H + W floats, written by k_prep next to the frame's RenderParams).
struct PixelOffsets {
    const float* __restrict__ v;   // [height]
    const float* __restrict__ u;   // [width]
};

// P: RenderParams in any address space (kernel argument or constant memory).
// Callable from host code too (xrt_host_volume_paths): the same f32 sequence,
// with the host's correctly rounded sqrtf and division.
template <typename P>
__host__ __device__ __forceinline__ void make_ray(const P& p, uint32_t row, uint32_t col, float& dx, float& dy,
                                                  float& dz);

template <typename P>
__host__ __device__ __forceinline__ void make_ray_from(const P& p, float v_off, float u_off, float& dx, float& dy,
                                                       float& dz, float& sx, float& sy, float& sz);

template <typename P>
__host__ __device__ __forceinline__ void make_ray_from(const P& p, float v_off, float u_off, float& dx, float& dy,
                                                       float& dz)
{
    float sx, sy, sz;
    make_ray_from(p, v_off, u_off, dx, dy, dz, sx, sy, sz);
}

template <typename P>
__host__ __device__ __forceinline__ void make_ray(const P& p, uint32_t row, uint32_t col, float& dx, float& dy,
                                                  float& dz)
{
    make_ray_from(p, pixel_offset(p.spacing, row, p.height), pixel_offset(p.spacing, col, p.width), dx,
                  dy, dz);
}

// The same ray with the offsets read from the frame's tables.
template <typename P>
__host__ __device__ __forceinline__ void make_ray(const P& p, const PixelOffsets& off, uint32_t row, uint32_t col,
                                                  float& dx, float& dy, float& dz)
{
    make_ray_from(p, off.v[row], off.u[col], dx, dy, dz);
}

// Also returns the direction after the first normalisation (sx, sy, sz): the
// L-buffer fork takes sign(direction . normal) with it, not with the Ray's
// twice-normalised copy (main-pthreads-lbuffer.cxx:761-762, :791).
template <typename P>
__host__ __device__ __forceinline__ void make_ray_from(const P& p, float v_off, float u_off, float& dx, float& dy,
                                                       float& dz, float& sx, float& sy, float& sz)
{
    // :659  detector + up*v + right*u - origin  (Vec3 ops left to right, f32)
    float X = ((p.cx + p.ux * v_off) + p.rx * u_off) - p.ox;
    float Y = ((p.cy + p.uy * v_off) + p.ry * u_off) - p.oy;
    float Z = ((p.cz + p.uz * v_off) + p.rz * u_off) - p.oz;
    // :660  Vec3::normalise (Vec3.inl:469-476)
    const float len = sqrtf((X * X + Y * Y) + Z * Z);
    X = X / len;
    Y = Y / len;
    Z = Z / len;
    sx = X;
    sy = Y;
    sz = Z;
    // Ray ctor normalises again; a zero length keeps the default (0,0,0).
    const float len2 = sqrtf((X * X + Y * Y) + Z * Z);
    if (len2 != 0.0f) {
        dx = X / len2;
        dy = Y / len2;
        dz = Z / len2;
    } else {
        dx = 0.0f;
        dy = 0.0f;
        dz = 0.0f;
    }
}

// ---------------------------------------------------------------------------
// Ray::intersect, src/Ray.cxx:72-124, with the ray-independent terms taken
// from the TriRec.  A conservative pre-test rejects only when the reference's
// `u < 0 || u > 1` test (Ray.cxx:106) provably rejects, so the f64 division
// runs only for candidates (DESIGN.md "Early reject").
// ---------------------------------------------------------------------------
// Ray.cxx:99 computes (float)(1.0 / (double)det).  For every f32 det that is
// the correctly rounded f32 quotient 1.0f / det: 1/det is never within 2^-49
// (relative) of an f32 rounding midpoint, so the f64 rounding cannot move it
// across one.  Checked on all 2^32 inputs (tools/check_fp_identities.c,
// tests/test_abi.py); the f32 division sequence is about half the f64 one.
__host__ __device__ __forceinline__ float inv_det_of(float det) { return 1.0f / det; }


// v_rcp_f32 (within 1 ulp) and one FMA Newton step give the correctly rounded
// 1.0f / d for every d with biased exponent in [1, 252], i.e. 2^-126 <= |d| <
// 2^126: checked on all 2^32 inputs on the GPU (tools/probes/rcp_probe.hip,
// profiles/r01_rcp_exhaustive.txt; the XRT_PROBE_RCP_FAST sweep of
// tests/test_gpu_parity.py).  Three VALU ops instead of the ten of the IEEE
// division sequence (div_scale / rcp / 4 fma / div_fmas / div_fixup).
__device__ __forceinline__ float rcp_newton(float d)
{
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ bool rcp_newton_exact_for(float d)
{
    const float a = fabsf(d);
    return a >= 0x1p-126f && a < 0x1p126f;       // false for NaN
}

// Branch-free Ray::intersect for the culled kernels, whose survivors almost
// always have a hitting lane (so the early reject would not skip the wave's
// division): the same comparisons as mt_intersect, combined with no control
// flow so two tests can be interleaved.  `hit` includes accept_t.
__device__ __forceinline__ float mt_exact(float dx, float dy, float dz, float e1x, float e1y,
                                         float e1z, float e2x, float e2y, float e2z, float tvx,
                                         float tvy, float tvz, float qvx, float qvy, float qvz,
                                         float tnum, bool& hit);

__device__ __forceinline__ bool mt_intersect(float dx, float dy, float dz,
                                             float e1x, float e1y, float e1z,
                                             float e2x, float e2y, float e2z,
                                             float tvx, float tvy, float tvz,
                                             float qvx, float qvy, float qvz,
                                             float tnum, float& t)
{
    // pvec = direction x edge2               Ray.cxx:90 (Vec3.inl:321-329)
    float px = dy * e2z - dz * e2y;
    float py = dz * e2x - dx * e2z;
    float pz = dx * e2y - dy * e2x;
    // det = edge1 . pvec                     Ray.cxx:93
    float det = (e1x * px + e1y * py) + e1z * pz;
    // tvec . pvec (u * det)                  Ray.cxx:105
    float a = (tvx * px + tvy * py) + tvz * pz;

    // Early reject.  With D = |det|, A = a*sign(det): u = RN(A * RN(1/D)).
    //   A < -2^-20 D       =>  u <= -2^-20 (1 - 2^-21) < 0        (reference rejects)
    //   A > RN(D (1+2^-20)) =>  u >= RN(1 + 2^-22 - tiny) > 1      (reference rejects)
    // NaNs fail both compares and fall through to the exact test; det == +-0
    // with a != 0 rejects here, as the reference does at Ray.cxx:94.
    float D = fabsf(det);
    float A = __int_as_float(__float_as_int(a) ^ (__float_as_int(det) & 0x80000000));
    if (A < D * -0x1p-20f || A > D * 0x1.00001p0f) return false;

    if (det == 0.0f) return false;                        // Ray.cxx:94 (fpclassify FP_ZERO)
    float inv_det = inv_det_of(det);                      // Ray.cxx:99
    float u = a * inv_det;                                // Ray.cxx:105
    if (u < 0.0f || u > 1.0f) return false;               // Ray.cxx:106
    float v = ((dx * qvx + dy * qvy) + dz * qvz) * inv_det;   // Ray.cxx:115
    if (v < 0.0f || u + v > 1.0f) return false;           // Ray.cxx:116
    t = tnum * inv_det;                                   // Ray.cxx:122
    return true;
}

// main.cxx:687: (double)t > 0.0000001.  For f32 t that is t > 0x1.ad7f28p-24f,
// the largest float not above 1e-7 (all 2^32 inputs: tools/check_fp_identities.c).
__host__ __device__ __forceinline__ bool accept_t(float t) { return t > 0x1.ad7f28p-24f; }

// The division-free part of Ray::intersect: det (Ray.cxx:93) and the
// numerators of u (:105, tvec . pvec) and v (:115, dir . qvec), with the
// reference's operation order.
__device__ __forceinline__ void mt_numerators(float dx, float dy, float dz, float e1x, float e1y,
                                              float e1z, float e2x, float e2y, float e2z,
                                              float tvx, float tvy, float tvz, float qvx,
                                              float qvy, float qvz, float& det, float& a, float& b)
{
    const float px = dy * e2z - dz * e2y;                 // Ray.cxx:90
    const float py = dz * e2x - dx * e2z;
    const float pz = dx * e2y - dy * e2x;
    det = (e1x * px + e1y * py) + e1z * pz;               // Ray.cxx:93
    a = (tvx * px + tvy * py) + tvz * pz;                 // Ray.cxx:105 (u * det)
    b = (dx * qvx + dy * qvy) + dz * qvz;                 // Ray.cxx:115 (v * det)
}

// False only when the reference provably rejects (no division needed): with
// D = |det| and A, B, T the numerators of u, v, t carrying det's sign,
//   det == +-0                        Ray.cxx:94
//   A < -2^-20 D or A > (1+2^-20) D   u < 0 or u > 1   (mt_intersect's bounds)
//   B < -2^-20 D                      v < 0            (same argument as for u)
//   A + B > (1+2^-18) D, D normal     u + v > 1: u and v each lose at most 2 ulps
//                                     to their two roundings, the f32 sum one (for
//                                     denormal det, 1/det may overflow and u = 0 * inf
//                                     is NaN, which the reference lets through)
//   T <= 0                            t <= 0 (t = tnum * RN(1/det), same sign)
// NaNs fail every compare and are kept.  Used wave-wide: a triangle that
// every lane rejects skips the division and the hit-list insertion.
__host__ __device__ __forceinline__ float xrt_flip_sign(float x, uint32_t sgn)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    u ^= sgn;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

__host__ __device__ __forceinline__ bool mt_may_hit(float det, float a, float b, float tnum)
{
    uint32_t bits;
    __builtin_memcpy(&bits, &det, 4);
    const uint32_t sgn = bits & 0x80000000u;
    const float D = fabsf(det);
    const float A = xrt_flip_sign(a, sgn);
    const float B = xrt_flip_sign(b, sgn);
    const float T = xrt_flip_sign(tnum, sgn);
    const float lo = D * -0x1p-20f;
    return !(det == 0.0f || A < lo || A > D * 0x1.00001p0f || B < lo ||
             (D >= 0x1p-126f && A + B > D * 0x1.00004p0f) || T <= 0.0f);
}

// The rest of Ray::intersect from mt_numerators' values; `hit` includes accept_t.
__host__ __device__ __forceinline__ float mt_finish_inv(float det, float inv_det, float a, float b,
                                                       float tnum, bool& hit)
{
    const float u = a * inv_det;                          // Ray.cxx:105
    const float v = b * inv_det;                          // Ray.cxx:115
    const float t = tnum * inv_det;                       // Ray.cxx:122
    // Ray.cxx:106 and :116 with two compares: !(u < 0) && !(v < 0) is
    // !(min(u, v) < 0), and !(u > 1) && !(u + v > 1) is !(max(u, u + v) > 1),
    // because IEEE minNum / maxNum return the other operand when one is a
    // (quiet) NaN -- and a NaN passes the reference's tests -- and a NaN only
    // when both are.
    // (bitwise &: evaluated without branches)
    hit = (det != 0.0f) & !(fminf(u, v) < 0.0f) & !(fmaxf(u, u + v) > 1.0f) & accept_t(t);
    return t;
}

__host__ __device__ __forceinline__ float mt_finish(float det, float a, float b, float tnum, bool& hit)
{
    return mt_finish_inv(det, inv_det_of(det), a, b, tnum, hit);   // Ray.cxx:99
}

__device__ __forceinline__ float mt_exact(float dx, float dy, float dz, float e1x, float e1y,
                                         float e1z, float e2x, float e2y, float e2z, float tvx,
                                         float tvy, float tvz, float qvx, float qvy, float qvz,
                                         float tnum, bool& hit)
{
    float det, a, b;
    mt_numerators(dx, dy, dz, e1x, e1y, e1z, e2x, e2y, e2z, tvx, tvy, tvz, qvx, qvy, qvz, det, a, b);
    return mt_finish_inv(det, inv_det_of(det), a, b, tnum, hit);   // Ray.cxx:99
}

// ---------------------------------------------------------------------------
// Per-ray sorted hit list in registers (static indices only).  Replaces the
// per-pixel std::vector + std::sort of main.cxx:666-704.
// ---------------------------------------------------------------------------
struct HitList {
    float h[kMaxHits];
    uint32_t n;

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int k = 0; k < kMaxHits; ++k) h[k] = __builtin_inff();
        n = 0;
    }

    // Keeps h ascending with +inf sentinels.  With h sorted, inserting x gives
    // h'[k] = max(h[k-1], min(h[k], x)) = med3(h[k-1], h[k], x) (old values):
    // one independent v_med3_f32 per slot instead of a compare-exchange chain.
    // A miss inserts +inf, which leaves h unchanged.  hit == false or x > 0.
    __device__ __forceinline__ void push_if(bool hit, float t)
    {
        const float x = hit ? t : __builtin_inff();
        // top slot first: each slot's new value is its last reader's, so the
        // list is updated in place
#pragma unroll
        for (int k = kMaxHits - 1; k >= 1; --k) h[k] = __builtin_amdgcn_fmed3f(h[k - 1], h[k], x);
        // min(h[0], x): the values are never NaN, so one plain v_min_f32 (the
        // compiler's fminnum adds a canonicalising v_max of the loop-carried h[0])
        asm("v_min_f32 %0, %1, %2" : "=v"(h[0]) : "v"(h[0]), "v"(x));
        n += hit ? 1u : 0u;
    }

    __device__ __forceinline__ void push(float t) { push_if(true, t); }

    // main.cxx:703-708: pairwise sum of the sorted list, sequential f32.
    __device__ __forceinline__ float path_length() const
    {
        float distance = 0.0f;
#pragma unroll
        for (int k = 0; k < kMaxHits / 2; ++k)
            if (2u * k + 1u < n) distance += h[2 * k + 1] - h[2 * k];
        return distance;
    }
};

// ---------------------------------------------------------------------------
// Signed hit list of the L-buffer fork (main-pthreads-lbuffer.cxx:778-795):
// the per-hit terms sign(direction . normal) * t kept in triangle order --
// the f32 sum runs in that order -- and the sum of the signs.  Slots hold
// (triangle id, term) ascending by id, 0xFFFFFFFF past the end; n and
// sign_sum count every hit, so a ray with more hits than slots knows it and
// its flag is exact (finish_ray_signed recomputes the sum).
// ---------------------------------------------------------------------------
struct SignedHits {
    uint32_t id[kMaxHits];
    float v[kMaxHits];
    uint32_t n;
    int sign_sum;

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int k = 0; k < kMaxHits; ++k) {
            id[k] = 0xFFFFFFFFu;
            v[k] = 0.0f;
        }
        n = 0;
        sign_sum = 0;
    }

    // :791-793  sign = signum(direction . normal), distance += sign * t
    __device__ __forceinline__ void push_if(bool hit, float t, uint32_t tid, int sign)
    {
        if (!hit) return;
        ++n;
        sign_sum += sign;
        uint32_t cid = tid;
        float cv = (float)sign * t;
#pragma unroll
        for (int k = 0; k < kMaxHits; ++k) {   // sorted insert by id (ids are distinct)
            const bool lt = cid < id[k];
            const uint32_t oid = id[k];
            const float ov = v[k];
            id[k] = lt ? cid : oid;
            v[k] = lt ? cv : ov;
            cid = lt ? oid : cid;
            cv = lt ? ov : cv;
        }
    }

    // :778, :792: 0.0f plus the terms in triangle order, sequential f32
    __device__ __forceinline__ float distance() const
    {
        float d = 0.0f;
#pragma unroll
        for (int k = 0; k < kMaxHits; ++k)
            if ((uint32_t)k < n) d += v[k];
        return d;
    }
};

// signum(direction . normal) of the fork (:729-731, :791), Vec3::dotProduct's order.
__host__ __device__ __forceinline__ int hit_sign(float sx, float sy, float sz, float nx, float ny, float nz)
{
    const float dp = (sx * nx + sy * ny) + sz * nz;
    return (int)(0.0f < dp) - (int)(dp < 0.0f);
}

// ---------------------------------------------------------------------------
// glibc 2.35 expf (sysdeps/ieee754/flt-32/e_expf.c with e_exp2f_data.c,
// EXP2F_TABLE_BITS = 5), as x86-64 glibc dispatches it on FMA hardware
// (e_expf-fma.c: the compiler fuses InvLn2N*x into both uses and the
// polynomial).  This is the function std::exp(float) binds to in
// src/main.cxx:739.  Bit-identical to the system libm on all 2^32 inputs
// (tools/gen_expf_table.py; tests/test_abi.py::test_host_expf_restatement_matches_libm on
// the host build, tests/test_gpu_parity.py::test_probe_expf_matches_libm on the device).
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ double xrt_u64_as_double(uint64_t u)
{
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

__host__ __device__ __forceinline__ uint64_t xrt_double_as_u64(double d)
{
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    return u;
}

__host__ __device__ __forceinline__ uint64_t xrt_exp2f_tab(uint32_t i)
{
    // tab[i] = asuint64(RN(2^(i/32))) - (i << 47)
    constexpr uint64_t tab[32] = {
        0x3ff0000000000000ULL, 0x3fefd9b0d3158574ULL, 0x3fefb5586cf9890fULL, 0x3fef9301d0125b51ULL,
        0x3fef72b83c7d517bULL, 0x3fef54873168b9aaULL, 0x3fef387a6e756238ULL, 0x3fef1e9df51fdee1ULL,
        0x3fef06fe0a31b715ULL, 0x3feef1a7373aa9cbULL, 0x3feedea64c123422ULL, 0x3feece086061892dULL,
        0x3feebfdad5362a27ULL, 0x3feeb42b569d4f82ULL, 0x3feeab07dd485429ULL, 0x3feea47eb03a5585ULL,
        0x3feea09e667f3bcdULL, 0x3fee9f75e8ec5f74ULL, 0x3feea11473eb0187ULL, 0x3feea589994cce13ULL,
        0x3feeace5422aa0dbULL, 0x3feeb737b0cdc5e5ULL, 0x3feec49182a3f090ULL, 0x3feed503b23e255dULL,
        0x3feee89f995ad3adULL, 0x3feeff76f2fb5e47ULL, 0x3fef199bdd85529cULL, 0x3fef3720dcef9069ULL,
        0x3fef5818dcfba487ULL, 0x3fef7c97337b9b5fULL, 0x3fefa4afa2a490daULL, 0x3fefd0765b6e4540ULL,
    };
    return tab[i & 31];
}

__host__ __device__ __forceinline__ float xrt_expf(float x)
{
    constexpr double kInvLn2N = 0x1.71547652b82fep+0 * 32;
    constexpr double kShift = 0x1.8p+52;
    constexpr double kC0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32;
    constexpr double kC1 = 0x1.ebfce50fac4f3p-3 / 32 / 32;
    constexpr double kC2 = 0x1.62e42ff0c52d6p-1 / 32;

    uint32_t ix;
    __builtin_memcpy(&ix, &x, 4);
    uint32_t abstop = (ix >> 20) & 0x7ff;
    double xd = (double)x;
    double kd = __builtin_fma(kInvLn2N, xd, kShift);
    uint64_t ki = xrt_double_as_u64(kd);
    kd -= kShift;
    double r = __builtin_fma(kInvLn2N, xd, -kd);
    uint64_t t = xrt_exp2f_tab((uint32_t)(ki % 32)) + (ki << 47);
    double s = xrt_u64_as_double(t);
    double z = __builtin_fma(kC0, r, kC1);
    double r2 = r * r;
    double y = __builtin_fma(kC2, r, 1.0);
    y = __builtin_fma(z, r2, y);
    y = y * s;
    // the special cases as selects over the main path's value (which is
    // computed, and discarded, for them too): no divergent branches
    float out = (float)y;
    if (abstop >= 0x42b) {
        out = x < -0x1.9fe368p6f ? 0.0f : out;                   // underflow
        out = x > 0x1.62e42ep6f ? __builtin_inff() : out;        // overflow
        out = abstop >= 0x7f8 ? x + x : out;                     // +inf or NaN
        out = ix == 0xff800000u ? 0.0f : out;                    // -inf
    }
    return out;
}

// ---------------------------------------------------------------------------
// glibc 2.35 exp (sysdeps/ieee754/dbl-64/e_exp.c with exp_data.c,
// EXP_TABLE_BITS = 7, EXP_POLY_ORDER = 5) as x86-64 glibc dispatches it on FMA
// hardware (e_exp-fma.c: the compiler fuses kd = InvLn2N*x + Shift, the two
// steps of r, the polynomial's multiply-adds and scale + scale*tmp, except in
// the special case's k < 0 branch -- found by the exhaustive check).  The
// function std::exp(double) binds to in src/main-pthreads-lbuffer.cxx:808.
// Table: tools/gen_exp_table.py (equal to the one inside the system libm);
// the function: tests/test_abi.py::test_host_exp_restatement_matches_libm
// (every exponent the signed L-buffer can produce) and the device probe.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t xrt_exp_tab(uint32_t i)
{
    constexpr uint64_t tab[256] = {
        0x0000000000000000ULL, 0x3ff0000000000000ULL, 0x3c9b3b4f1a88bf6eULL, 0x3feff63da9fb3335ULL,
        0xbc7160139cd8dc5dULL, 0x3fefec9a3e778061ULL, 0xbc905e7a108766d1ULL, 0x3fefe315e86e7f85ULL,
        0x3c8cd2523567f613ULL, 0x3fefd9b0d3158574ULL, 0xbc8bce8023f98efaULL, 0x3fefd06b29ddf6deULL,
        0x3c60f74e61e6c861ULL, 0x3fefc74518759bc8ULL, 0x3c90a3e45b33d399ULL, 0x3fefbe3ecac6f383ULL,
        0x3c979aa65d837b6dULL, 0x3fefb5586cf9890fULL, 0x3c8eb51a92fdeffcULL, 0x3fefac922b7247f7ULL,
        0x3c3ebe3d702f9cd1ULL, 0x3fefa3ec32d3d1a2ULL, 0xbc6a033489906e0bULL, 0x3fef9b66affed31bULL,
        0xbc9556522a2fbd0eULL, 0x3fef9301d0125b51ULL, 0xbc5080ef8c4eea55ULL, 0x3fef8abdc06c31ccULL,
        0xbc91c923b9d5f416ULL, 0x3fef829aaea92de0ULL, 0x3c80d3e3e95c55afULL, 0x3fef7a98c8a58e51ULL,
        0xbc801b15eaa59348ULL, 0x3fef72b83c7d517bULL, 0xbc8f1ff055de323dULL, 0x3fef6af9388c8deaULL,
        0x3c8b898c3f1353bfULL, 0x3fef635beb6fcb75ULL, 0xbc96d99c7611eb26ULL, 0x3fef5be084045cd4ULL,
        0x3c9aecf73e3a2f60ULL, 0x3fef54873168b9aaULL, 0xbc8fe782cb86389dULL, 0x3fef4d5022fcd91dULL,
        0x3c8a6f4144a6c38dULL, 0x3fef463b88628cd6ULL, 0x3c807a05b0e4047dULL, 0x3fef3f49917ddc96ULL,
        0x3c968efde3a8a894ULL, 0x3fef387a6e756238ULL, 0x3c875e18f274487dULL, 0x3fef31ce4fb2a63fULL,
        0x3c80472b981fe7f2ULL, 0x3fef2b4565e27cddULL, 0xbc96b87b3f71085eULL, 0x3fef24dfe1f56381ULL,
        0x3c82f7e16d09ab31ULL, 0x3fef1e9df51fdee1ULL, 0xbc3d219b1a6fbffaULL, 0x3fef187fd0dad990ULL,
        0x3c8b3782720c0ab4ULL, 0x3fef1285a6e4030bULL, 0x3c6e149289cecb8fULL, 0x3fef0cafa93e2f56ULL,
        0x3c834d754db0abb6ULL, 0x3fef06fe0a31b715ULL, 0x3c864201e2ac744cULL, 0x3fef0170fc4cd831ULL,
        0x3c8fdd395dd3f84aULL, 0x3feefc08b26416ffULL, 0xbc86a3803b8e5b04ULL, 0x3feef6c55f929ff1ULL,
        0xbc924aedcc4b5068ULL, 0x3feef1a7373aa9cbULL, 0xbc9907f81b512d8eULL, 0x3feeecae6d05d866ULL,
        0xbc71d1e83e9436d2ULL, 0x3feee7db34e59ff7ULL, 0xbc991919b3ce1b15ULL, 0x3feee32dc313a8e5ULL,
        0x3c859f48a72a4c6dULL, 0x3feedea64c123422ULL, 0xbc9312607a28698aULL, 0x3feeda4504ac801cULL,
        0xbc58a78f4817895bULL, 0x3feed60a21f72e2aULL, 0xbc7c2c9b67499a1bULL, 0x3feed1f5d950a897ULL,
        0x3c4363ed60c2ac11ULL, 0x3feece086061892dULL, 0x3c9666093b0664efULL, 0x3feeca41ed1d0057ULL,
        0x3c6ecce1daa10379ULL, 0x3feec6a2b5c13cd0ULL, 0x3c93ff8e3f0f1230ULL, 0x3feec32af0d7d3deULL,
        0x3c7690cebb7aafb0ULL, 0x3feebfdad5362a27ULL, 0x3c931dbdeb54e077ULL, 0x3feebcb299fddd0dULL,
        0xbc8f94340071a38eULL, 0x3feeb9b2769d2ca7ULL, 0xbc87deccdc93a349ULL, 0x3feeb6daa2cf6642ULL,
        0xbc78dec6bd0f385fULL, 0x3feeb42b569d4f82ULL, 0xbc861246ec7b5cf6ULL, 0x3feeb1a4ca5d920fULL,
        0x3c93350518fdd78eULL, 0x3feeaf4736b527daULL, 0x3c7b98b72f8a9b05ULL, 0x3feead12d497c7fdULL,
        0x3c9063e1e21c5409ULL, 0x3feeab07dd485429ULL, 0x3c34c7855019c6eaULL, 0x3feea9268a5946b7ULL,
        0x3c9432e62b64c035ULL, 0x3feea76f15ad2148ULL, 0xbc8ce44a6199769fULL, 0x3feea5e1b976dc09ULL,
        0xbc8c33c53bef4da8ULL, 0x3feea47eb03a5585ULL, 0xbc845378892be9aeULL, 0x3feea34634ccc320ULL,
        0xbc93cedd78565858ULL, 0x3feea23882552225ULL, 0x3c5710aa807e1964ULL, 0x3feea155d44ca973ULL,
        0xbc93b3efbf5e2228ULL, 0x3feea09e667f3bcdULL, 0xbc6a12ad8734b982ULL, 0x3feea012750bdabfULL,
        0xbc6367efb86da9eeULL, 0x3fee9fb23c651a2fULL, 0xbc80dc3d54e08851ULL, 0x3fee9f7df9519484ULL,
        0xbc781f647e5a3ecfULL, 0x3fee9f75e8ec5f74ULL, 0xbc86ee4ac08b7db0ULL, 0x3fee9f9a48a58174ULL,
        0xbc8619321e55e68aULL, 0x3fee9feb564267c9ULL, 0x3c909ccb5e09d4d3ULL, 0x3feea0694fde5d3fULL,
        0xbc7b32dcb94da51dULL, 0x3feea11473eb0187ULL, 0x3c94ecfd5467c06bULL, 0x3feea1ed0130c132ULL,
        0x3c65ebe1abd66c55ULL, 0x3feea2f336cf4e62ULL, 0xbc88a1c52fb3cf42ULL, 0x3feea427543e1a12ULL,
        0xbc9369b6f13b3734ULL, 0x3feea589994cce13ULL, 0xbc805e843a19ff1eULL, 0x3feea71a4623c7adULL,
        0xbc94d450d872576eULL, 0x3feea8d99b4492edULL, 0x3c90ad675b0e8a00ULL, 0x3feeaac7d98a6699ULL,
        0x3c8db72fc1f0eab4ULL, 0x3feeace5422aa0dbULL, 0xbc65b6609cc5e7ffULL, 0x3feeaf3216b5448cULL,
        0x3c7bf68359f35f44ULL, 0x3feeb1ae99157736ULL, 0xbc93091fa71e3d83ULL, 0x3feeb45b0b91ffc6ULL,
        0xbc5da9b88b6c1e29ULL, 0x3feeb737b0cdc5e5ULL, 0xbc6c23f97c90b959ULL, 0x3feeba44cbc8520fULL,
        0xbc92434322f4f9aaULL, 0x3feebd829fde4e50ULL, 0xbc85ca6cd7668e4bULL, 0x3feec0f170ca07baULL,
        0x3c71affc2b91ce27ULL, 0x3feec49182a3f090ULL, 0x3c6dd235e10a73bbULL, 0x3feec86319e32323ULL,
        0xbc87c50422622263ULL, 0x3feecc667b5de565ULL, 0x3c8b1c86e3e231d5ULL, 0x3feed09bec4a2d33ULL,
        0xbc91bbd1d3bcbb15ULL, 0x3feed503b23e255dULL, 0x3c90cc319cee31d2ULL, 0x3feed99e1330b358ULL,
        0x3c8469846e735ab3ULL, 0x3feede6b5579fdbfULL, 0xbc82dfcd978e9db4ULL, 0x3feee36bbfd3f37aULL,
        0x3c8c1a7792cb3387ULL, 0x3feee89f995ad3adULL, 0xbc907b8f4ad1d9faULL, 0x3feeee07298db666ULL,
        0xbc55c3d956dcaebaULL, 0x3feef3a2b84f15fbULL, 0xbc90a40e3da6f640ULL, 0x3feef9728de5593aULL,
        0xbc68d6f438ad9334ULL, 0x3feeff76f2fb5e47ULL, 0xbc91eee26b588a35ULL, 0x3fef05b030a1064aULL,
        0x3c74ffd70a5fddcdULL, 0x3fef0c1e904bc1d2ULL, 0xbc91bdfbfa9298acULL, 0x3fef12c25bd71e09ULL,
        0x3c736eae30af0cb3ULL, 0x3fef199bdd85529cULL, 0x3c8ee3325c9ffd94ULL, 0x3fef20ab5fffd07aULL,
        0x3c84e08fd10959acULL, 0x3fef27f12e57d14bULL, 0x3c63cdaf384e1a67ULL, 0x3fef2f6d9406e7b5ULL,
        0x3c676b2c6c921968ULL, 0x3fef3720dcef9069ULL, 0xbc808a1883ccb5d2ULL, 0x3fef3f0b555dc3faULL,
        0xbc8fad5d3ffffa6fULL, 0x3fef472d4a07897cULL, 0xbc900dae3875a949ULL, 0x3fef4f87080d89f2ULL,
        0x3c74a385a63d07a7ULL, 0x3fef5818dcfba487ULL, 0xbc82919e2040220fULL, 0x3fef60e316c98398ULL,
        0x3c8e5a50d5c192acULL, 0x3fef69e603db3285ULL, 0x3c843a59ac016b4bULL, 0x3fef7321f301b460ULL,
        0xbc82d52107b43e1fULL, 0x3fef7c97337b9b5fULL, 0xbc892ab93b470dc9ULL, 0x3fef864614f5a129ULL,
        0x3c74b604603a88d3ULL, 0x3fef902ee78b3ff6ULL, 0x3c83c5ec519d7271ULL, 0x3fef9a51fbc74c83ULL,
        0xbc8ff7128fd391f0ULL, 0x3fefa4afa2a490daULL, 0xbc8dae98e223747dULL, 0x3fefaf482d8e67f1ULL,
        0x3c8ec3bc41aa2008ULL, 0x3fefba1bee615a27ULL, 0x3c842b94c3a9eb32ULL, 0x3fefc52b376bba97ULL,
        0x3c8a64a931d185eeULL, 0x3fefd0765b6e4540ULL, 0xbc8e37bae43be3edULL, 0x3fefdbfdad9cbe14ULL,
        0x3c77893b4d91cd9dULL, 0x3fefe7c1819e90d8ULL, 0x3c5305c14160cc89ULL, 0x3feff3c22b8f71f1ULL,
    };
    return tab[i & 255u];
}

__host__ __device__ __forceinline__ double xrt_exp_special(double tmp, uint64_t sbits, uint64_t ki)
{
    if ((ki & 0x80000000u) == 0) {              // k > 0: the scale's exponent may have overflowed
        sbits -= 1009ull << 52;
        const double scale = xrt_u64_as_double(sbits);
        return 0x1p1009 * __builtin_fma(scale, tmp, scale);
    }
    sbits += 1022ull << 52;                     // k < 0: subnormal range
    const double scale = xrt_u64_as_double(sbits);
    double y = scale + scale * tmp;
    if (y < 1.0) {
        double lo = scale - y + scale * tmp;
        const double hi = 1.0 + y;
        lo = 1.0 - hi + y + lo;
        y = (hi + lo) - 1.0;
        if (y == 0.0) y = 0.0;                  // no -0.0
    }
    return 0x1p-1022 * y;
}

__host__ __device__ __forceinline__ double xrt_exp(double x)
{
    constexpr double kInvLn2N = 0x1.71547652b82fep0 * 128;
    constexpr double kNegLn2hiN = -0x1.62e42fefa0000p-8;
    constexpr double kNegLn2loN = -0x1.cf79abc9e3b3ap-47;
    constexpr double kShift = 0x1.8p52;
    constexpr double kC2 = 0x1.ffffffffffdbdp-2;
    constexpr double kC3 = 0x1.555555555543cp-3;
    constexpr double kC4 = 0x1.55555cf172b91p-5;
    constexpr double kC5 = 0x1.1111167a4d017p-7;

    const uint64_t ix = xrt_double_as_u64(x);
    uint32_t abstop = (uint32_t)(ix >> 52) & 0x7ffu;
    if (abstop - 0x3c9u >= 0x408u - 0x3c9u) {   // |x| < 2^-54, |x| >= 512, inf or NaN
        if (abstop - 0x3c9u >= 0x80000000u) return 1.0 + x;
        if (abstop >= 0x409u) {                 // |x| >= 1024
            if (ix == 0xfff0000000000000ull) return 0.0;
            if (abstop >= 0x7ffu) return 1.0 + x;
            return (ix >> 63) ? 0.0 : __builtin_inf();
        }
        abstop = 0;                             // large |x|: the special case below
    }
    double kd = __builtin_fma(kInvLn2N, x, kShift);
    const uint64_t ki = xrt_double_as_u64(kd);
    kd -= kShift;
    const double r = __builtin_fma(kd, kNegLn2loN, __builtin_fma(kd, kNegLn2hiN, x));
    const uint32_t idx = 2u * (uint32_t)(ki & 127u);
    const uint64_t top = ki << 45;
    const double tail = xrt_u64_as_double(xrt_exp_tab(idx));
    const uint64_t sbits = xrt_exp_tab(idx + 1u) + top;
    const double r2 = r * r;
    const double tmp = __builtin_fma(r2 * r2, __builtin_fma(r, kC5, kC4),
                                     __builtin_fma(r2, __builtin_fma(r, kC3, kC2), tail + r));
    if (abstop == 0) return xrt_exp_special(tmp, sbits, ki);
    const double scale = xrt_u64_as_double(sbits);
    return __builtin_fma(scale, tmp, scale);
}

__host__ __device__ __forceinline__ float xrt_f32_from_bits(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// ---------------------------------------------------------------------------
// glibc 2.35 logf (sysdeps/ieee754/flt-32/e_logf.c with e_logf_data.c,
// LOGF_TABLE_BITS = 4, LOGF_POLY_ORDER = 4): x = 2^k * z with z in
// [0x1.66p-1, 0x1.66p0), c the centre of z's sixteenth of that range,
// log(x) = log1p(z/c - 1) + log(c) + k * Ln2 in f64, rounded once to f32.
// Every f64 operation is rounded on its own (this file's fp contract(off)).
// x86-64 glibc dispatches a build with fused steps on FMA hardware, yet no
// input's f32 result differs: this form equals the system libm on all 2^32
// inputs (tools/check_logf.c), so -- unlike xrt_expf -- a numpy
// restatement, which cannot fuse, is exact (tests/logf_ref.py).  A returned NaN's sign and
// payload are not part of the contract.  The table -- 16 pairs (1/c, log c),
// 256 bytes -- is indexed per lane: cached global loads, as xrt_exp's.
// ---------------------------------------------------------------------------
struct LogfEntry {
    double invc, logc;
};

__host__ __device__ __forceinline__ LogfEntry xrt_logf_tab(uint32_t i)
{
    constexpr LogfEntry tab[16] = {
        {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
        {0x1.49539f0f010b0p+0, -0x1.01eae7f513a67p-2}, {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
        {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8ea0p+0, -0x1.1aa2bc79c8100p-3},
        {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
        {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
        {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aa0p-1, 0x1.c5e53aa362eb4p-4},
        {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d224770p-3},
        {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2},
    };
    return tab[i & 15u];
}

// The inputs of the main path: positive, finite and normal.
__host__ __device__ __forceinline__ bool xrt_logf_is_regular(uint32_t ix)
{
    return ix - 0x00800000u < 0x7f800000u - 0x00800000u;       // (u32 arithmetic)
}

// The main path, from the bits of a regular x (or of a subnormal scaled by
// 2^23 with 23 taken off its exponent field again, which may wrap: every step
// below is u32 arithmetic).  log(1) needs no case of its own: r = 0 gives
// y = A2 * 0 + (0 + 0) = -0 + +0 = +0.0 in round-to-nearest, as the contract's
// first line returns.
__host__ __device__ __forceinline__ float xrt_logf_regular(uint32_t ix)
{
    constexpr double kLn2 = 0x1.62e42fefa39efp-1;
    constexpr double kA0 = -0x1.00ea348b88334p-2;
    constexpr double kA1 = 0x1.5575b0be00b6ap-2;
    constexpr double kA2 = -0x1.ffffef20a4123p-2;
    const uint32_t tmp = ix - 0x3f330000u;
    const LogfEntry e = xrt_logf_tab(tmp >> 19);
    const int32_t k = (int32_t)tmp >> 23;                       // arithmetic
    const double z = (double)xrt_f32_from_bits(ix - (tmp & 0xff800000u));
    const double r = z * e.invc - 1.0;
    const double y0 = e.logc + (double)k * kLn2;
    const double r2 = r * r;
    double y = kA1 * r + kA2;
    y = kA0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

// Every input.  The special cases are branches: a caller with several values
// can test them together first (k_log_projection does, xrt_logf_is_regular).
__host__ __device__ __forceinline__ float xrt_logf(float x)
{
    uint32_t ix;
    __builtin_memcpy(&ix, &x, 4);
    if (xrt_logf_is_regular(ix)) return xrt_logf_regular(ix);
    if (ix * 2u == 0u) return -__builtin_inff();                // +-0
    if (ix == 0x7f800000u) return x;                            // +inf
    if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return xrt_f32_from_bits(0x7fc00000u);   // x < 0, NaN
    const float scaled = x * 0x1p23f;                           // subnormal: normalised (exact)
    __builtin_memcpy(&ix, &scaled, 4);
    return xrt_logf_regular(ix - (23u << 23));
}

// ---------------------------------------------------------------------------
// Photon noise (the contract is include/xrt.h's): a counter-based
// generator and a Poisson sampler whose every step is a rounded f64 or f32
// operation, sqrt and / IEEE-correct, nothing fused (this file's fp
// contract(off)) -- so that a numpy restatement is the exact reference
// (tests/noise_ref.py) and host and device agree bit for bit.
// ---------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., Random123): ten rounds over the counter
// c[0..3] under the key (k0, k1), the key bumped between rounds.
__host__ __device__ __forceinline__ void xrt_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                           uint32_t k0, uint32_t k1, uint32_t (&w)[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// The four words of the pixels with global indices 4 j .. 4 j + 3 under `seed`.
__host__ __device__ __forceinline__ void xrt_noise_words(uint64_t j, uint64_t seed, uint32_t (&w)[4])
{
    xrt_philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// u = (w + 0.5) 2^-32: exact in f64, never 0 or 1.
__host__ __device__ __forceinline__ double xrt_uniform_from_word(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// The standard normal deviate at u(w): Wichura's AS241, PPND7.  Its third
// branch (sqrt(-ln t) > 5) is unreachable -- the smallest t is 2^-33 and
// sqrt(-ln 2^-33) < 4.79 -- and is left out; t lies in [2^-33, 0.075], so
// xrt_logf's main path is the whole of it.
__host__ __device__ __forceinline__ double xrt_normal_from_word(uint32_t w)
{
    const double u = xrt_uniform_from_word(w);
    const double q = u - 0.5;
    if (__builtin_fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = ((59.109374720 * r + 159.29113202) * r + 50.434271938) * r + 3.3871327179;
        const double den = ((67.187563600 * r + 78.757757664) * r + 17.895169469) * r + 1.0;
        return (q * num) / den;
    }
    const double t = q < 0.0 ? u : 1.0 - u;
    const float tf = (float)t;
    uint32_t it;
    __builtin_memcpy(&it, &tf, 4);
    const double r = ::sqrt(-(double)xrt_logf_regular(it)) - 1.6;
    const double num = ((0.17023821103 * r + 1.3067284816) * r + 2.7568153900) * r + 1.4234372777;
    const double den = (0.12021132975 * r + 0.73700164250) * r + 1.0;
    const double z = num / den;
    return q < 0.0 ? -z : z;
}

constexpr double kNoiseSmallMean = 64.0;
constexpr uint32_t kNoiseSearchCap = 255;

// lam < 64 (and not below 0): inversion by sequential search from exp(-lam).
__host__ __device__ __forceinline__ double xrt_poisson_search(double lam, double u)
{
    double p = xrt_exp(-lam), s = p;
    uint32_t N = 0;
    while (u > s && N < kNoiseSearchCap) {
        N += 1;
        p = (p * lam) / (double)N;
        s = s + p;
    }
    return (double)N;
}

// lam >= 64 and finite: the normal deviate with the second-order
// Cornish-Fisher term, rounded to the nearest count.
__host__ __device__ __forceinline__ double xrt_poisson_normal(double lam, uint32_t w)
{
    const double z = xrt_normal_from_word(w);
    const double x = lam + ::sqrt(lam) * z + (z * z - 1.0) / 6.0;
    const double v = __builtin_floor(x + 0.5);
    return v > 0.0 ? v : 0.0;
}

// The count N of one pixel, as f64: NaN for a NaN or negative mean (-0.0 is
// not negative), +inf for +inf.
__host__ __device__ __forceinline__ double xrt_poisson_from_word(double lam, uint32_t w)
{
    if (!(lam >= 0.0)) return __builtin_nan("");
    if (lam < kNoiseSmallMean) return xrt_poisson_search(lam, xrt_uniform_from_word(w));
    if (lam == __builtin_inf()) return lam;
    return xrt_poisson_normal(lam, w);
}

// One pixel's output from its count: XRT_NOISE_COUNTS or XRT_NOISE_INTENSITY.
__host__ __device__ __forceinline__ float xrt_noise_output(double N, float gain, bool counts)
{
    const float c = (float)N;
    return counts ? c : c / gain;
}

// The lanes of k_photon_noise: the Philox counters that n pixels from
// first_index on touch (n >= 1, first_index + n <= 2^64 - 1: the host's check).
__host__ __device__ constexpr uint64_t photon_noise_lanes(uint64_t first_index, uint64_t n)
{
    return ((first_index + (n - 1u)) >> 2) - (first_index >> 2) + 1u;
}
constexpr uint32_t kNoiseThreads = 256;

// NaN path lengths.  The only NaN the reference's pair sum can produce is
// inf - inf (two t = +inf "hits", which Ray.cxx records when 1/det overflows,
// DESIGN.md "Tile cull" step 0); x86 SSE returns its default NaN for it
// (0xFFC00000) and every later add propagates that operand.  The device's NaN
// encodings differ, so the kernels store the x86 bits explicitly.
constexpr uint32_t kX86DefaultNaN = 0xFFC00000u;
// shade() of that NaN on x86: (double) and * 0.1 keep it, the negation in
// -(0.3971f * cm) flips its sign, expf(x) returns x + x and 80 * x keeps it.
constexpr uint32_t kX86ShadeNaN = 0x7FC00000u;

// Beer-Lambert shade, main.cxx:725 and :739.
__host__ __device__ __forceinline__ float shade(float distance)
{
    if (distance != distance) return xrt_f32_from_bits(kX86ShadeNaN);
    float cm = (float)((double)distance * 0.1);
    return 80.000f * xrt_expf(-(0.3971f * cm));
}

// The fork's L-buffer update for mesh 0 (main-pthreads-lbuffer.cxx:805-808):
// L = 80 (its initial value, :314) times exp(-(mu * (distance * 0.1))) in f64,
// rounded to f32; -1 when the signs do not cancel.  A NaN distance (x86's
// default NaN from inf - inf or 0 * inf) gives 0x7FC00000 there: the f64
// negation flips its sign before exp returns it.
constexpr uint32_t kX86SignedNaN = 0x7FC00000u;
__host__ __device__ __forceinline__ float signed_lbuffer(float distance, int sign_sum, float mu)
{
    if (sign_sum != 0) return -1.0f;
    if (distance != distance) return xrt_f32_from_bits(kX86SignedNaN);
    return (float)((double)80.000f * xrt_exp(-((double)mu * ((double)distance * 0.1))));
}

// The materials model's update of L by one mesh the ray hit (the fork's
// :772 and :805-808 with the mesh filter lifted): a flagged ray stays -1, a
// mesh whose signs do not cancel flags it, otherwise L is multiplied by
// exp(-(mu * (distance * 0.1))) in f64 and rounded to f32.  Non-finite values
// as x86 evaluates them: a NaN exponent (a NaN distance, or mu == 0 with an
// infinite one) comes back from exp with its sign cleared by the negation and
// replaces a number; a NaN L keeps its bits; inf * 0 is x86's default NaN.
__host__ __device__ __forceinline__ float materials_update(float L, float distance, int sign_sum, float mu)
{
    if (L == -1.0f) return L;
    if (sign_sum != 0) return -1.0f;
    if (L != L) return L;
    const double x = (double)mu * ((double)distance * 0.1);
    if (x != x) return xrt_f32_from_bits(kX86SignedNaN);
    const float f = (float)((double)L * xrt_exp(-x));
    return f != f ? xrt_f32_from_bits(kX86DefaultNaN) : f;
}

// The spectrum model's L of one ray from its per-mesh sums: -1
// when some mesh's signs do not cancel, otherwise, in f64, left to right and
// without contraction,
//   E = 0; for each bin e: x = 0; for each mesh j: x = x + mu(j, e) * (dist(j) * 0.1);
//          E = E + weight(e) * exp(-x)
// rounded to f32.  The n meshes are whichever the caller lists, in scene order:
// a mesh the ray did not hit has distance +0.0f and adds +0.0 to an x that is
// never -0.0, so leaving it out is exact.  dist(j), sign(j), mu(j, e) and
// weight(e) are callables: the host reads arrays, the render kernels the lane's
// parked distances and the device table.  With weight > 0 and mu >= 0 every
// NaN x86 can reach here (x86's default NaN as a distance, 0 * inf, inf - inf
// in x) is negative in x, positive after the negation, and stays E: it is
// stored as 0x7FC00000 explicitly, as materials_update stores its.
template <typename Dist, typename Sign, typename Mu, typename Weight>
__host__ __device__ __forceinline__ float spectrum_lbuffer(uint32_t n, uint32_t num_bins, Dist dist, Sign sign,
                                                           Mu mu, Weight weight)
{
    bool flagged = false;
    for (uint32_t j = 0; j < n; ++j) flagged |= sign(j) != 0;
    if (flagged) return -1.0f;
    double E = 0.0;
    for (uint32_t e = 0; e < num_bins; ++e) {
        double x = 0.0;
        for (uint32_t j = 0; j < n; ++j) x = x + (double)mu(j, e) * ((double)dist(j) * 0.1);
        E = E + (double)weight(e) * xrt_exp(-x);
    }
    const float f = (float)E;
    return f != f ? xrt_f32_from_bits(kX86SignedNaN) : f;
}

// The same for a ray that hits nothing: every exp(-0.0) is 1.
__host__ __device__ __forceinline__ float spectrum_miss(const float* weight, uint32_t num_bins)
{
    double E = 0.0;
    for (uint32_t e = 0; e < num_bins; ++e) E = E + (double)weight[e] * 1.0;
    return (float)E;
}

// 8-bit image: Image::applyLUT's per-pixel formula (include/Image.inl:195-211)
// with vmin = 0, vmax = 80; NaN (undefined in the reference) maps to 0.
__host__ __device__ __forceinline__ uint8_t lut_u8(float v)
{
    const float vmin = 0.0f, vmax = 80.0f;
    // 255.0 * v / 80.0 == v * 3.1875 exactly (below); for x = v * 3.1875 >= 0
    // (at most 30 significant bits, < 256) x + 0.5 is exact, so round-half-
    // away-from-zero is floor(x + 0.5).  Selects instead of branches; the
    // product is computed, and discarded, for out-of-range v and NaN.
    const uint32_t r = (uint32_t)__builtin_floor((double)v * 3.1875 + 0.5);
    return v > vmax ? (uint8_t)255u : v >= vmin ? (uint8_t)r : (uint8_t)0u;
}

// ---------------------------------------------------------------------------
// The detector response: a separable line-spread function over an
// image plane, taps applied as written (a correlation), edges replicated, each
// pass summed in f64 in tap order and rounded once to f32.  The taps travel by
// value in k_lsf's kernel arguments, already widened to f64 (exact) -- scalar
// loads put them where v_fma_f64 reads them, with no conversion per tap -- and
// zero-padded to whole chunks of kLsfChunk, so that the next chunk's taps can
// be fetched ahead unconditionally (a pad meets no value).
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxLsfTaps = 129;
constexpr uint32_t kLsfChunk = 8;       // outputs a thread carries along the axis of its pass
constexpr uint32_t kLsfTapsPadded = (kMaxLsfTaps + kLsfChunk - 1) / kLsfChunk * kLsfChunk;
struct LsfTable {
    double hx[kLsfTapsPadded];
    double hy[kLsfTapsPadded];
    uint32_t nx, ny;
};

inline void lsf_table_set(LsfTable& tab, const float* lsf_x, uint32_t taps_x, const float* lsf_y, uint32_t taps_y)
{
    for (uint32_t k = 0; k < kLsfTapsPadded; ++k) {
        tab.hx[k] = k < taps_x ? (double)lsf_x[k] : 0.0;
        tab.hy[k] = k < taps_y ? (double)lsf_y[k] : 0.0;
    }
    tab.nx = taps_x;
    tab.ny = taps_y;
}

// acc + h * v in f64.  The product of two f32 values is exact in f64 (48
// significand bits, exponents in range), so the fused and the separate form
// round identically: the device takes v_fma_f64, the host the plain expression.
__host__ __device__ __forceinline__ double lsf_step(double h, double v, double acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma(h, v, acc);
#else
    return acc + h * v;
#endif
}

// kLsfChunk neighbouring outputs of one pass: acc[r] = sum over k = 0..n-1, in
// this order, of h[k] * (double)v(r + k), where h is a table's padded taps and
// v(i) the i-th value of the line through the outputs, v(0) the first output's
// leftmost (topmost) neighbour.  The values slide through a register window -- one new
// value a tap, kLsfChunk sums -- whose rotation is static with the tap loop
// unrolled by kLsfChunk.  The next chunk's values are fetched before the
// current chunk's sums and the taps half a chunk ahead, so their latency hides
// behind the FMAs.  That reads v ahead of need, up to index n + 2 kLsfChunk -
// 2: what lies past n + kLsfChunk - 2 meets no tap, and only has to be
// readable (k_lsf lays its LDS images out accordingly).  An
// accumulator starts at -0.0, which gives the k = 0 product bit for bit once
// that is added: x + -0.0 == x for every x, -0.0 and +0.0 included.
template <class Value>
__host__ __device__ __forceinline__ void lsf_chunk(const double* h, uint32_t n, Value v, double (&acc)[kLsfChunk])
{
    constexpr uint32_t kHalf = kLsfChunk / 2u;
    double win[kLsfChunk], ha[kHalf], hb[kHalf];      // ha: a chunk's first taps, hb: its last
    float raw[kLsfChunk];
#pragma unroll
    for (uint32_t r = 0; r < kLsfChunk; ++r) {
        win[r] = (double)v(r);
        acc[r] = -0.0;
        raw[r] = v(kLsfChunk + r);
    }
#pragma unroll
    for (uint32_t u = 0; u < kHalf; ++u) ha[u] = h[u];
    uint32_t k = 0;
    for (; k + kLsfChunk <= n; k += kLsfChunk) {
        float raw_next[kLsfChunk];
#pragma unroll
        for (uint32_t u = 0; u < kLsfChunk; ++u) raw_next[u] = v(k + 2u * kLsfChunk + u);
#pragma unroll
        for (uint32_t u = 0; u < kHalf; ++u) hb[u] = h[k + kHalf + u];
#pragma unroll
        for (uint32_t u = 0; u < kHalf; ++u) {
#pragma unroll
            for (uint32_t r = 0; r < kLsfChunk; ++r) acc[r] = lsf_step(ha[u], win[(u + r) % kLsfChunk], acc[r]);
            win[u] = (double)raw[u];
        }
#pragma unroll
        for (uint32_t u = 0; u < kHalf; ++u) ha[u] = h[k + kLsfChunk + u];   // (below kLsfTapsPadded: k + kLsfChunk <= n)
#pragma unroll
        for (uint32_t u = kHalf; u < kLsfChunk; ++u) {
#pragma unroll
            for (uint32_t r = 0; r < kLsfChunk; ++r) acc[r] = lsf_step(hb[u - kHalf], win[(u + r) % kLsfChunk], acc[r]);
            win[u] = (double)raw[u];
        }
#pragma unroll
        for (uint32_t u = 0; u < kLsfChunk; ++u) raw[u] = raw_next[u];
    }
    if (k < n) {                                          // the last n % kLsfChunk taps
#pragma unroll
        for (uint32_t u = 0; u < kHalf; ++u) hb[u] = h[k + kHalf + u];
#pragma unroll
        for (uint32_t u = 0; u + 1 < kLsfChunk; ++u) {
            if (k + u < n) {
                const double hk = u < kHalf ? ha[u % kHalf] : hb[u % kHalf];
#pragma unroll
                for (uint32_t r = 0; r < kLsfChunk; ++r) acc[r] = lsf_step(hk, win[(u + r) % kLsfChunk], acc[r]);
                win[u] = (double)raw[u];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Line-integral projections: one pixel of xrt_log_projection,
// p = -ln((I - dark) / (flat - dark)), every step a separately rounded f32
// operation.  `flat` is the flat plane's pixel, or flat_value where there is no
// plane; `dark` is read only with has_dark.  A transmission below t_min > 0 is
// raised to it (a NaN compares false and stays); t = 1 gives +0.0, t = 0
// +inf, t < 0 NaN.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ float log_projection_transmission(float image, float flat, float dark, bool has_dark,
                                                                      float t_min)
{
    const float num = has_dark ? image - dark : image;
    const float den = has_dark ? flat - dark : flat;
    const float t = num / den;
    return t_min > 0.0f && t < t_min ? t_min : t;
}

__host__ __device__ __forceinline__ float log_projection_pixel(float image, float flat, float dark, bool has_dark,
                                                               float t_min)
{
    return 0.0f - xrt_logf(log_projection_transmission(image, flat, dark, has_dark, t_min));
}

// The launch geometry of k_log_projection (kernels/xrt_kernels.h), formed on the host.
constexpr uint32_t kProjThreads = 256;
constexpr uint32_t kProjThreadsLog2 = 8;

struct LogProjectionPlan {
    uint32_t lanes_log2;                // a row's share of the workgroup: 2^lanes_log2 lanes, a quad each
    uint32_t chunks;                    // workgroups along a row
    uint64_t blocks;                    // the whole launch
};

// Quads that cover a row of W pixels under any misalignment 0..3: ceil((W + 3) / 4).
__host__ __device__ constexpr uint32_t log_projection_quads(uint32_t W) { return (uint32_t)(((uint64_t)W + 6u) / 4u); }

inline LogProjectionPlan log_projection_plan(uint32_t W, uint64_t rows)
{
    LogProjectionPlan plan;
    const uint32_t quads = log_projection_quads(W);
    plan.lanes_log2 = 0;
    while (plan.lanes_log2 < kProjThreadsLog2 && (1u << plan.lanes_log2) < quads) ++plan.lanes_log2;
    const uint32_t span = 1u << plan.lanes_log2, rows_per = kProjThreads >> plan.lanes_log2;
    plan.chunks = (quads + span - 1u) / span;
    plan.blocks = (rows + rows_per - 1u) / rows_per * plan.chunks;
    return plan;
}

// ---------------------------------------------------------------------------
// Area sampling: one output pixel of xrt_area_integrate, the
// weighted mean over S sub-sources and a bin_y x bin_x block of the finer
// plane, summed in f64 in the order (s, dy, dx) from -0.0 and divided once.
// weight[s] * value is exact in f64 (two f32 factors), so lsf_step's fused and
// separate forms round identically here too.  The weights travel by value in
// k_area_integrate's kernel arguments, already widened to f64, with the
// divisor wsum = bin_x bin_y sum(weight), formed on the host.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxAreaSources = 64;
constexpr uint32_t kMaxAreaBin = 8;
struct AreaWeights {
    double w[kMaxAreaSources];
    double wsum;
};

inline void area_weights_set(AreaWeights& tab, const float* weight, uint32_t num_sources, uint32_t bin_x, uint32_t bin_y)
{
    double sum = 0.0;
    for (uint32_t s = 0; s < kMaxAreaSources; ++s) {
        tab.w[s] = s < num_sources ? (double)weight[s] : 0.0;
        if (s < num_sources) sum = sum + tab.w[s];
    }
    tab.wsum = (double)(bin_x * bin_y) * sum;
}

__host__ __device__ __forceinline__ float area_finish(double acc, double wsum) { return (float)(acc / wsum); }

// `v(s, dy, dx)` is the sample of sub-source s at the block's row dy and column dx.
template <typename Value>
__host__ __device__ __forceinline__ float area_pixel(const AreaWeights& tab, uint32_t num_sources, uint32_t bin_x,
                                                     uint32_t bin_y, Value v)
{
    double acc = -0.0;
    for (uint32_t s = 0; s < num_sources; ++s) {
        const double w = tab.w[s];
        for (uint32_t dy = 0; dy < bin_y; ++dy)
            for (uint32_t dx = 0; dx < bin_x; ++dx) acc = lsf_step(w, (double)v(s, dy, dx), acc);
    }
    return area_finish(acc, tab.wsum);
}

// The launch geometry of k_area_integrate (kernels/xrt_kernels.h), formed on
// the host as log_projection_plan's: a row's share of the workgroup is the
// power of two of lanes that covers its units, so narrow planes fill their
// waves.  A unit is what one lane owns of an output row: with bin_x 1, 2 or 4
// the outputs whose inputs are one 16-byte quad of an input row (4, 2, 1), with
// bin_x 8 one output (two quads), otherwise -- `vector` 0 -- one output moved
// pixel by pixel.  `uniform`: every input row of one output row starts at the
// same address modulo 16 bytes (a row pitch and, past one source, a plane pitch
// of whole quads, or a single row), which is what lets the quads be cut at the
// addresses' multiples of 16 bytes.
constexpr uint32_t kAreaThreads = 256;
constexpr uint32_t kAreaThreadsLog2 = 8;

struct AreaPlan {
    uint32_t vector;                    // bin_x where the vector kernel serves (1, 2, 4, 8), else 0
    uint32_t lanes_log2;
    uint32_t chunks;
    uint64_t blocks;
};

inline AreaPlan area_plan(uint32_t W, uint64_t rows, uint32_t bin_x, uint32_t bin_y, uint32_t num_sources, uint32_t H)
{
    AreaPlan plan;
    const uint64_t Wb = (uint64_t)W * bin_x, plane = Wb * ((uint64_t)H * bin_y);
    const bool uniform = ((Wb & 3u) == 0u || bin_y == 1u) && ((plane & 3u) == 0u || num_sources == 1u);
    plan.vector = uniform && (bin_x == 1u || bin_x == 2u || bin_x == 4u || bin_x == 8u) ? bin_x : 0u;
    // units that cover a row under any misalignment the kernel vectorises: ceil((Wb + 3) / 4) quads, Wb / 8 pairs
    const uint64_t units = plan.vector == 0u ? W : plan.vector == 8u ? W : (Wb + 6u) / 4u;
    plan.lanes_log2 = 0;
    while (plan.lanes_log2 < kAreaThreadsLog2 && (1u << plan.lanes_log2) < units) ++plan.lanes_log2;
    const uint32_t span = 1u << plan.lanes_log2, rows_per = kAreaThreads >> plan.lanes_log2;
    plan.chunks = (uint32_t)((units + span - 1u) / span);
    plan.blocks = (rows + rows_per - 1u) / rows_per * plan.chunks;
    return plan;
}

// ---------------------------------------------------------------------------
// The spectral detector (the contract is include/xrt.h's): per
// pixel and energy bin a count of mean gain * weight * exp(-x), then a
// channels x bins response matrix into channel sums, in f64, every step rounded
// on its own.  The bins go a quad at a time: one Philox evaluation gives a
// quad's four words, and a quad's four exp run side by side.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxChannels = 8;
constexpr uint32_t kDetectorThreads = 256;

// What k_spectral_detector takes by value (a launch owns its tables).  The
// spectrum, quad by quad -- the coefficients of mesh m for the four bins of
// quad q are neighbours, mu[(q * kMaxMeshes + m) * 4 + r] for bin 4 q + r:
// one 16-byte scalar load at an offset known at compile time, used up by the
// mesh's four sums before the next mesh's is needed -- and +0.0f past the
// scene's meshes and past num_bins; weight +0.0f past num_bins.  The response
// with a row stride of kMaxBins (rows past num_channels and bins past num_bins
// are +0.0f), the scalars, and what every channel of a pixel without a hit
// gets under XRT_DETECT_EXPECTED (the host's own run of detector_pixel over
// zero distances).
struct DetectorSpectrum {
    float weight[kMaxBins];
    float mu[kMaxBins * kMaxMeshes];           // [detector_mu_index(m, e)]
    uint32_t num_bins;
};
__host__ __device__ constexpr uint32_t detector_mu_index(uint32_t m, uint32_t e)
{
    return ((e >> 2) * kMaxMeshes + m) * 4u + (e & 3u);
}
struct DetectorTable {
    float response[kMaxChannels * kMaxBins];   // [c * kMaxBins + e]
    float miss[kMaxChannels];
    float gain;
    float read_noise;
    uint32_t num_channels;
    uint32_t counts;                           // XRT_DETECT_COUNTS: 1
    // what the kernel needs only behind its bin loop, read from the argument segment there and so in no register
    // across the loop: the masks again, the output planes, their stride in pixels, and the seed again for the
    // read noise
    const uint16_t* open;
    float* out;
    uint64_t plane;
    uint64_t seed;
};
static_assert(sizeof(DetectorSpectrum) + sizeof(DetectorTable) + 64u <= 4096u, "k_spectral_detector's argument segment");

// Four xrt_exp at once, bit for bit xrt_exp of each: the main path of all four
// first and without a branch -- the table index is masked, so it is formed and
// loaded for any argument, and the four pairs of loads are in flight together
// --, then each value's class picks its result as xrt_exp's branches do: below
// 2^-54 in magnitude 1 + x, from 512 on the special case, from 1024 on the
// limits (0 for a negative argument, -inf included; +inf for a positive one;
// 1 + x for a NaN).
__host__ __device__ __forceinline__ void xrt_exp_quad(const double (&x)[4], double (&y)[4])
{
    constexpr double kInvLn2N = 0x1.71547652b82fep0 * 128;
    constexpr double kNegLn2hiN = -0x1.62e42fefa0000p-8;
    constexpr double kNegLn2loN = -0x1.cf79abc9e3b3ap-47;
    constexpr double kShift = 0x1.8p52;
    constexpr double kC2 = 0x1.ffffffffffdbdp-2;
    constexpr double kC3 = 0x1.555555555543cp-3;
    constexpr double kC4 = 0x1.55555cf172b91p-5;
    constexpr double kC5 = 0x1.1111167a4d017p-7;
    uint64_t ki[4], top[4], tail_bits[4], scale_bits[4];
    double r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double kd = __builtin_fma(kInvLn2N, x[j], kShift);
        ki[j] = xrt_double_as_u64(kd);
        kd -= kShift;
        r[j] = __builtin_fma(kd, kNegLn2loN, __builtin_fma(kd, kNegLn2hiN, x[j]));
        top[j] = ki[j] << 45;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t idx = 2u * (uint32_t)(ki[j] & 127u);
        tail_bits[j] = xrt_exp_tab(idx);
        scale_bits[j] = xrt_exp_tab(idx + 1u);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t sbits = scale_bits[j] + top[j];
        const double r2 = r[j] * r[j];
        const double tmp = __builtin_fma(r2 * r2, __builtin_fma(r[j], kC5, kC4),
                                         __builtin_fma(r2, __builtin_fma(r[j], kC3, kC2), xrt_u64_as_double(tail_bits[j]) + r[j]));
        const double scale = xrt_u64_as_double(sbits);
        double v = __builtin_fma(scale, tmp, scale);
        // the class by t = the exponent field less 0x3c9, against 0, 63 and 64 alone: below 0 |x| < 2^-54, from
        // 63 on |x| >= 512, from 64 on |x| >= 1024, inf or NaN (few constants: they sit in scalar registers)
        const int32_t t = (int32_t)((uint32_t)(xrt_double_as_u64(x[j]) >> 52) & 0x7ffu) - 0x3c9;
        v = t < 0 ? 1.0 + x[j] : v;
        if (t >= 63) {
            if (t >= 64)                               // xrt_exp's limits: 0 below, +inf above, 1 + x for a NaN
                v = x[j] < 0.0 ? 0.0 : x[j] != x[j] ? 1.0 + x[j] : __builtin_inf();
            else
                v = xrt_exp_special(tmp, sbits, ki[j]);
        }
        y[j] = v;
    }
}

// Four counts at once, each xrt_poisson_from_word of its mean and word: the
// means of 64 and above go through the normal branch one after another, those
// below 64 through ONE search loop stepped together as k_photon_noise steps its
// four pixels -- step k divides by the same (double)k for each and a mean drops
// out where the contract's loop ends --, their four exp(-lam) side by side.
__host__ __device__ __forceinline__ void xrt_poisson_quad(const double (&lam)[4], const uint32_t (&w)[4], double (&N)[4])
{
    bool small[4], any_small = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        small[e] = lam[e] >= 0.0 && lam[e] < kNoiseSmallMean;
        any_small |= small[e];
        N[e] = lam[e] >= 0.0 ? lam[e] : __builtin_nan("");              // +inf stays; a finite mean's is set below
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (lam[e] >= kNoiseSmallMean && lam[e] != __builtin_inf()) N[e] = xrt_poisson_normal(lam[e], w[e]);
    if (any_small) {
        // a mean that takes no part searches under u = 0, which no sum is below: whether a mean is still in the
        // search is u > s, formed where it is asked and kept in no register between the steps
        double u[4], p[4], s[4], neg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) neg[e] = small[e] ? -lam[e] : 0.0;
        xrt_exp_quad(neg, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u[e] = small[e] ? xrt_uniform_from_word(w[e]) : 0.0;
            s[e] = p[e];
            if (small[e]) N[e] = 0.0;
        }
        for (uint32_t k = 1; k <= kNoiseSearchCap; ++k) {
            if (!((u[0] > s[0]) | (u[1] > s[1]) | (u[2] > s[2]) | (u[3] > s[3]))) break;
            const double kd = (double)k;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(u[e] > s[e])) continue;
                p[e] = (p[e] * lam[e]) / kd;
                s[e] = s[e] + p[e];
                N[e] = kd;
            }
        }
    }
}

// One pixel's channel sums acc[0 .. kC) before the output conversion, for the
// pixel of global index g whose mask is clear.  quad_x(q, x) adds to x[0..3]
// (+0.0 on entry) the path sums of the bins 4 q .. 4 q + 3, each bin's meshes
// in ascending order: x[r] = x[r] + (double)mu * ((double)distance * 0.1), one
// mesh after another -- the caller knows where its distances are (registers,
// LDS, host arrays); a mesh of distance +0.0f may be left out (exact, as
// apply_bins').  kC >= the channels is a compile-time bound, so that the sums
// keep static indices: resp(c, e) is +0.0f past the channels and bins (acc
// starts at +0.0 and +0.0 * N = +0.0 leaves it as it is), weight(e) +0.0f for a
// bin past num_bins in the last quad: its x is dropped (an infinite path makes
// it 0 * inf), its mean and its count are 0.  read_noise() and tail_seed() are
// asked after the bins, where they are needed.
template <uint32_t kC, bool kNoisy, typename QuadX, typename Weight, typename Resp, typename ReadNoise, typename TailSeed>
__host__ __device__ __forceinline__ void detector_pixel(uint32_t num_bins, QuadX quad_x, Weight weight, Resp resp, float gain,
                                                        uint64_t seed, uint64_t g, ReadNoise read_noise, TailSeed tail_seed,
                                                        double (&acc)[kC])
{
    const double gd = (double)gain;
#pragma unroll
    for (uint32_t c = 0; c < kC; ++c) acc[c] = 0.0;
    for (uint32_t q = 0; 4u * q < num_bins; ++q) {
        double nx[4], y[4], N[4];
        double x[4] = {0.0, 0.0, 0.0, 0.0};
        quad_x(q, x);
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) nx[r] = 4u * q + r < num_bins ? -x[r] : -0.0;   // (0 * inf past num_bins)
        xrt_exp_quad(nx, y);
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) N[r] = ((double)weight(4u * q + r) * y[r]) * gd;
        if (kNoisy) {
            uint32_t w[4];
            xrt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), q, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
            double lam[4];
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) lam[r] = N[r];
            xrt_poisson_quad(lam, w, N);
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
#pragma unroll
            for (uint32_t c = 0; c < kC; ++c) acc[c] = acc[c] + (double)resp(c, 4u * q + r) * N[r];
        }
    }
    if (kNoisy) {
        const float rn = read_noise();
        if (rn > 0.0f) {
            const uint64_t s2 = tail_seed();
#pragma unroll
            for (uint32_t c4 = 0; 4u * c4 < kC; ++c4) {
                uint32_t v[4];
                xrt_philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), c4, 2u, (uint32_t)s2, (uint32_t)(s2 >> 32), v);
#pragma unroll
                for (uint32_t r = 0; r < 4 && 4u * c4 + r < kC; ++r)
                    acc[4u * c4 + r] = acc[4u * c4 + r] + (double)rn * xrt_normal_from_word(v[r]);
            }
        }
    }
}

// One channel's output from its sum: XRT_DETECT_COUNTS or XRT_DETECT_INTENSITY.
__host__ __device__ __forceinline__ float xrt_detector_output(double acc, float gain, bool counts)
{
    return counts ? (float)acc : (float)(acc / (double)gain);
}

// ---------------------------------------------------------------------------
// Material decomposition (the contract is include/xrt.h's): the
// inverse of the spectral detector under XRT_DETECT_EXPECTED.  Per pixel the
// line integrals A[0 .. kB) of kB basis materials whose expected channels
// match the measured ones, by Fisher scoring on the channels' Poisson
// likelihood: per iteration the detector's bin chain with the Jacobian beside
// it, a kB x kB normal matrix, an LDL^T solve.  All of it f64, every operation
// rounded on its own, exp and division only.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxBasis = 3;
constexpr uint32_t kDecomposeThreads = 256;
constexpr uint32_t kDecomposeMaxIter = 200;
constexpr uint32_t kDecomposeMasked = 254;
constexpr uint32_t kDecomposeFailed = 255;

// What k_decompose takes by value (a launch owns its tables).  mu quad by quad
// as DetectorSpectrum's, with kMaxBasis rows a quad: the coefficients of basis
// b for the four bins of quad q are one 16-byte scalar load.  weight, mu and
// response are +0.0f past num_bins, num_basis and num_channels.  guess[b *
// kMaxChannels + c] and y0[c] (the expected channels at A = 0) are the host's;
// without a guess has_guess is 0 and neither is read.
struct DecomposeTable {
    float weight[kMaxBins];
    float mu[kMaxBins * kMaxBasis];            // [decompose_mu_index(b, e)]
    float response[kMaxChannels * kMaxBins];   // [c * kMaxBins + e]
    double guess[kMaxBasis * kMaxChannels];
    double y0[kMaxChannels];
    double tol;
    double damping;
    float gain;
    uint32_t num_bins;
    uint32_t num_channels;
    uint32_t max_iter;
    uint32_t intensity;                        // XRT_DETECT_INTENSITY: 1
    uint32_t has_guess;
    const float* channels;
    const uint16_t* open;
    float* out;
    uint8_t* iters;
    uint64_t plane;
};
__host__ __device__ constexpr uint32_t decompose_mu_index(uint32_t b, uint32_t e)
{
    return ((e >> 2) * kMaxBasis + b) * 4u + (e & 3u);
}
static_assert(sizeof(DecomposeTable) + 64u <= 4096u, "k_decompose's argument segment");

// H d = g for the upper triangle H of a symmetric kB x kB matrix by LDL^T
// without pivoting, in the contract's order (kB = 1, 2 are its leading
// blocks); false, with x untouched, when a pivot is not > 0.
template <uint32_t kB>
__host__ __device__ __forceinline__ bool decompose_solve(const double (&H)[kMaxBasis][kMaxBasis], const double (&g)[kMaxBasis],
                                                         double (&x)[kMaxBasis])
{
    static_assert(kB >= 1 && kB <= kMaxBasis, "1 to 3 basis materials");
    const double d0 = H[0][0];
    if (kB == 1) {
        if (!(d0 > 0.0)) return false;
        x[0] = g[0] / d0;
        return true;
    }
    const double l10 = H[0][1] / d0;
    const double d1 = H[1][1] - l10 * H[0][1];
    const double z0 = g[0];
    const double z1 = g[1] - l10 * z0;
    if (kB == 2) {
        if (!(d0 > 0.0) || !(d1 > 0.0)) return false;
        x[1] = z1 / d1;
        x[0] = z0 / d0 - l10 * x[1];
        return true;
    }
    const double l20 = H[0][2] / d0;
    const double l21 = (H[1][2] - l20 * H[0][1]) / d1;
    const double d2 = (H[2][2] - l20 * H[0][2]) - l21 * (l21 * d1);
    const double z2 = (g[2] - l20 * z0) - l21 * z1;
    if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) return false;
    x[2] = z2 / d2;
    x[1] = z1 / d1 - l21 * x[2];
    x[0] = (z0 / d0 - l10 * x[1]) - l20 * x[2];
    return true;
}

// One unmasked pixel: A[0 .. kB) from its counts y[0 .. kC) (intensities
// already times gain), and the status its iters entry gets -- the iterations
// run, or kDecomposeFailed.  kC >= num_channels is a compile-time bound, so
// that every sum keeps a static index: resp(c, e) is +0.0f for a row past
// num_channels, whose ybar is then +0.0 or a NaN and which the contract's
// !(ybar > 0) leaves out as it leaves out a zero row; the start reads only the
// rows below num_channels.  mu(b, e), weight(e) and resp(c, e) are +0.0f for
// a bin past num_bins in the last quad: its x is dropped, its lam is +0.0 and
// adds +0.0 to sums that are never -0.0.  guess(b, c) and y0(c) are asked only
// when has_guess.
template <uint32_t kB, uint32_t kC, typename Mu, typename Weight, typename Resp, typename Guess, typename Y0>
__host__ __device__ __forceinline__ uint32_t decompose_pixel(uint32_t num_bins, uint32_t num_channels, Mu mu, Weight weight,
                                                             Resp resp, float gain, const double (&y)[kC], bool has_guess,
                                                             Guess guess, Y0 y0, uint32_t max_iter, double tol, double damping,
                                                             double (&A)[kB])
{
    const double gd = (double)gain;
#pragma unroll
    for (uint32_t b = 0; b < kB; ++b) A[b] = 0.0;
    if (has_guess) {
        double p[kC];
#pragma unroll
        for (uint32_t c = 0; c < kC; ++c) {
            p[c] = 0.0;
            if (c < num_channels) {
                float t = (float)(y[c] / y0(c));
                if (!(t >= 1e-30f)) t = 1e-30f;                 // zero, negative and NaN counts start at the floor
                p[c] = -(double)xrt_logf(t);
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) {
#pragma unroll
            for (uint32_t c = 0; c < kC; ++c)
                if (c < num_channels) A[b] = A[b] + guess(b, c) * p[c];
        }
    }
    uint32_t it = 0;
    while (it < max_iter) {
        double ybar[kC], J[kC][kB];
#pragma unroll
        for (uint32_t c = 0; c < kC; ++c) {
            ybar[c] = 0.0;
#pragma unroll
            for (uint32_t b = 0; b < kB; ++b) J[c][b] = 0.0;
        }
        double a01[kB];
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) a01[b] = A[b] * 0.1;
        for (uint32_t q = 0; 4u * q < num_bins; ++q) {
            double x[4] = {0.0, 0.0, 0.0, 0.0}, nx[4], ex[4];
#pragma unroll
            for (uint32_t b = 0; b < kB; ++b) {
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) x[r] = x[r] + (double)mu(b, 4u * q + r) * a01[b];
            }
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) nx[r] = 4u * q + r < num_bins ? -x[r] : -0.0;
            xrt_exp_quad(nx, ex);
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                const double lam = ((double)weight(4u * q + r) * ex[r]) * gd;
#pragma unroll
                for (uint32_t c = 0; c < kC; ++c) {
                    const double t = (double)resp(c, 4u * q + r) * lam;
                    ybar[c] = ybar[c] + t;
#pragma unroll
                    for (uint32_t b = 0; b < kB; ++b) J[c][b] = J[c][b] + (double)mu(b, 4u * q + r) * t;
                }
            }
        }
        double g[kMaxBasis] = {0.0, 0.0, 0.0}, H[kMaxBasis][kMaxBasis] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
        for (uint32_t c = 0; c < kC; ++c) {
            if (!(ybar[c] > 0.0)) continue;                     // a zero response row, or underflow
            const double qc = y[c] / ybar[c];
            const double rc = 1.0 - qc;
            const double v = 1.0 / ybar[c];
#pragma unroll
            for (uint32_t b = 0; b < kB; ++b) g[b] = g[b] + J[c][b] * rc;
#pragma unroll
            for (uint32_t b = 0; b < kB; ++b) {
#pragma unroll
                for (uint32_t b2 = b; b2 < kB; ++b2) H[b][b2] = H[b][b2] + (J[c][b] * J[c][b2]) * v;
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) H[b][b] = H[b][b] + H[b][b] * damping;
        double d[kMaxBasis] = {0.0, 0.0, 0.0};
        if (!decompose_solve<kB>(H, g, d)) return kDecomposeFailed;
        bool done = true;
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) {
            const double s = d[b] / 0.1;
            A[b] = A[b] + s;
            done = done && s <= tol && -s <= tol;
        }
        ++it;
        if (done) break;
    }
    return it;
}

// ---------------------------------------------------------------------------
// Voxel phantoms: a labelled, axis-aligned volume traced into
// paths planes.  volume_ray is the contract: k_volume_paths calls it on the
// device and xrt_host_volume_paths compiled for the host, and
// tests/volume_ref.py restates it.  All of it is f64, every operation rounded
// on its own (no FMA), every min or max the written select (no fmin / fmax:
// a NaN takes the same branch on both sides), no register array with a
// dynamic index.
// ---------------------------------------------------------------------------
// The volume, by value in k_volume_paths' arguments.  labels[(z * ny + y) * nx
// + x], label 0 empty, label L in 1..num_labels into plane L - 1; density of
// the same shape or null (1).
struct VolumeDesc {
    const uint8_t* __restrict__ labels;
    const float* __restrict__ density;
    uint32_t n[3];          // nx, ny, nz
    uint32_t num_labels;
    float origin[3];        // the minimum corner of voxel (0, 0, 0)
    float spacing[3];       // > 0
};

constexpr uint32_t kMaxVolumeDim = 2048;

// Grid plane i of an axis: from the index every time, so nothing drifts.
__host__ __device__ __forceinline__ double volume_plane(double lo, double s, uint32_t i) { return lo + (double)i * s; }

// One axis of the slab test against [p0, pn): narrows [te, tx]; false when a
// ray parallel to the axis lies outside the slab.
__host__ __device__ __forceinline__ bool volume_slab(double O, double d, double p0, double pn, double& inv, double& te,
                                                     double& tx)
{
    inv = 0.0;
    if (d == 0.0) return O >= p0 && O < pn;
    inv = 1.0 / d;
    const double t0 = (p0 - O) * inv, t1 = (pn - O) * inv;
    const double mn = t0 < t1 ? t0 : t1, mx = t0 < t1 ? t1 : t0;
    te = mn > te ? mn : te;
    tx = mx < tx ? mx : tx;
    return true;
}

// The voxel index of the entry point on one axis, clamped into the volume (a
// NaN goes to 0).
__host__ __device__ __forceinline__ int32_t volume_start(double O, double te, double d, double lo, double s, uint32_t n)
{
    double f = floor(((O + te * d) - lo) / s);
    const double top = (double)(n - 1u);
    f = f >= 0.0 ? f : 0.0;
    f = f <= top ? f : top;
    return (int32_t)f;
}

// The ray O + t d through the volume: add(m, run) is called once per run of
// consecutive steps in label m + 1 with the run's f64 sum of segment lengths
// (times the voxel's density), in ray order -- the association of the plane's
// sum.  A ray that misses calls nothing.  At most nx + ny + nz + 3 steps.
template <typename Add>
__host__ __device__ __forceinline__ void volume_ray(const VolumeDesc& v, double Ox, double Oy, double Oz, double dx,
                                                    double dy, double dz, Add&& add)
{
    const double inf = __builtin_huge_val();
    const uint32_t nx = v.n[0], ny = v.n[1], nz = v.n[2];
    const double lox = (double)v.origin[0], loy = (double)v.origin[1], loz = (double)v.origin[2];
    const double sx = (double)v.spacing[0], sy = (double)v.spacing[1], sz = (double)v.spacing[2];
    double te = 0.0, tx = inf, ivx, ivy, ivz;
    if (!volume_slab(Ox, dx, volume_plane(lox, sx, 0u), volume_plane(lox, sx, nx), ivx, te, tx)) return;
    if (!volume_slab(Oy, dy, volume_plane(loy, sy, 0u), volume_plane(loy, sy, ny), ivy, te, tx)) return;
    if (!volume_slab(Oz, dz, volume_plane(loz, sz, 0u), volume_plane(loz, sz, nz), ivz, te, tx)) return;
    if (!(te < tx)) return;
    int32_t ix = volume_start(Ox, te, dx, lox, sx, nx);
    int32_t iy = volume_start(Oy, te, dy, loy, sy, ny);
    int32_t iz = volume_start(Oz, te, dz, loz, sz, nz);
    const int32_t stx = dx > 0.0 ? 1 : -1, sty = dy > 0.0 ? 1 : -1, stz = dz > 0.0 ? 1 : -1;
    const int32_t upx = dx > 0.0 ? 1 : 0, upy = dy > 0.0 ? 1 : 0, upz = dz > 0.0 ? 1 : 0;
    double tc = te, run = 0.0;
    uint32_t cur = 0;
    const uint32_t limit = nx + ny + nz + 3u;
    for (uint32_t k = 0; k < limit; ++k) {
        const double tnx = dx == 0.0 ? inf : (volume_plane(lox, sx, (uint32_t)(ix + upx)) - Ox) * ivx;
        const double tny = dy == 0.0 ? inf : (volume_plane(loy, sy, (uint32_t)(iy + upy)) - Oy) * ivy;
        const double tnz = dz == 0.0 ? inf : (volume_plane(loz, sz, (uint32_t)(iz + upz)) - Oz) * ivz;
        double t = tnx;                 // ties: the lower axis first
        int32_t a = 0;
        if (tny < t) { t = tny; a = 1; }
        if (tnz < t) { t = tnz; a = 2; }
        const double tend = t < tx ? t : tx;
        const double seg = tend - tc;
        const uint64_t vox = ((uint64_t)(uint32_t)iz * ny + (uint32_t)iy) * nx + (uint32_t)ix;
        const uint32_t L = v.labels[vox];
        if (L != cur) {
            if (cur) add(cur - 1u, run);
            run = 0.0;
            cur = L;
        }
        if (L != 0u && seg > 0.0) run = run + (v.density ? seg * (double)v.density[vox] : seg);
        if (seg > 0.0) tc = tend;
        if (!(t < tx)) break;
        ix += a == 0 ? stx : 0;
        iy += a == 1 ? sty : 0;
        iz += a == 2 ? stz : 0;
        if ((uint32_t)ix >= nx || (uint32_t)iy >= ny || (uint32_t)iz >= nz) break;
    }
    if (cur) add(cur - 1u, run);
}

// ---------------------------------------------------------------------------
// FDK reconstruction: the arithmetic that k_backproject and its
// host restatement (xrt_host_backproject) share.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxRampWidth = 4096;            // XRT_MAX_RAMP_WIDTH

// The (j, k) part of one line of a projection matrix, A = that line's four
// entries: a voxel's homogeneous coordinate is A[0] * i + backproject_bracket.
__host__ __device__ __forceinline__ double backproject_bracket(const double* A, double j, double k)
{
    return (A[1] * j + A[2] * k) + A[3];
}

// A projection sample: the pixel inside the plane, +0.0f outside (W and H are at most 2^31 - 1: the
// callers' argument check).
__host__ __device__ __forceinline__ float backproject_sample(const float* plane, uint32_t W, uint32_t H, int32_t y,
                                                             int32_t x)
{
    return x >= 0 && y >= 0 && (uint32_t)x < W && (uint32_t)y < H ? plane[(size_t)y * W + (size_t)x] : 0.0f;
}

// One plane's contribution to one voxel whose homogeneous detector
// coordinates are (a, b, c): nothing unless c > 0 and the point lies within
// one pixel of the plane; else the bilinear sample (f32, every operation
// rounded on its own) times 1 / c^2, added to acc in f64.
__host__ __device__ __forceinline__ void backproject_term(const float* plane, uint32_t W, uint32_t H, double a, double b,
                                                          double c, double& acc)
{
    if (!(c > 0.0)) return;                          // (a NaN compares false)
    const double w = 1.0 / c;
    const double col = a * w, row = b * w;
    if (!(col > -1.0 && col < (double)W && row > -1.0 && row < (double)H)) return;
    const double fc = floor(col), fr = floor(row);
    const float fx = (float)(col - fc), fy = (float)(row - fr);
    const int32_t x0 = (int32_t)fc, y0 = (int32_t)fr;          // -1 .. W - 1 and -1 .. H - 1
    const float s00 = backproject_sample(plane, W, H, y0, x0), s01 = backproject_sample(plane, W, H, y0, x0 + 1);
    const float s10 = backproject_sample(plane, W, H, y0 + 1, x0), s11 = backproject_sample(plane, W, H, y0 + 1, x0 + 1);
    const float top = s00 + fx * (s01 - s00);
    const float bot = s10 + fx * (s11 - s10);
    const float v = top + fy * (bot - top);
    acc = acc + (double)v * (w * w);
}

// What a voxel's sum becomes in the volume.
__host__ __device__ __forceinline__ float backproject_output(double acc, double scale, bool accumulate, float old)
{
    return accumulate ? (float)((double)old + acc * scale) : (float)(acc * scale);
}

// ---------------------------------------------------------------------------
// SIRT / OS-SART: the forward projector of a f32 volume under
// the backprojector's matrices, and the voxel update.  forward_ray is the
// contract: k_forward_project calls it on the device and
// xrt_host_forward_project compiled for the host, and tests/sirt_ref.py
// restates it.  volume_ray's rules (f64, no FMA, written selects, planes from
// the index every time) over the grid lo = -0.5, s = 1 of centre-index
// coordinates; no labels, no runs.
// ---------------------------------------------------------------------------
constexpr int kForwardProject = 0;                  // XRT_FP_PROJECT
constexpr int kForwardResidual = 1;                 // XRT_FP_RESIDUAL

// One component of pixel (row, col)'s ray direction under the ray matrix R
// (xrt_ray_matrix), Ra = that line's four entries; Ra[3] is the source's.
__host__ __device__ __forceinline__ double forward_direction(const double* Ra, double row, double col)
{
    return Ra[0] * col + (Ra[1] * row + Ra[2]);
}

// The ray O + t d, t > 0, through the grid of n voxels (voxel i occupies
// [i - 0.5, i + 0.5]): false for a miss; else acc = the sum over the steps
// with seg > 0 of seg * vol[voxel], in ray order, and span = tx - te, both in
// units of t.  At most nx + ny + nz + 3 steps.  Only the stepped axis' tnext
// is formed again after a step: the others' indices have not changed, so
// their values would be the same.
__host__ __device__ __forceinline__ bool forward_ray(const float* __restrict__ vol, uint32_t nx, uint32_t ny, uint32_t nz,
                                                     double Ox, double Oy, double Oz, double dx, double dy, double dz,
                                                     double& acc, double& span)
{
    const double inf = __builtin_huge_val();
    const double lo = -0.5, s = 1.0;
    double te = 0.0, tx = inf, ivx, ivy, ivz;
    if (!volume_slab(Ox, dx, volume_plane(lo, s, 0u), volume_plane(lo, s, nx), ivx, te, tx)) return false;
    if (!volume_slab(Oy, dy, volume_plane(lo, s, 0u), volume_plane(lo, s, ny), ivy, te, tx)) return false;
    if (!volume_slab(Oz, dz, volume_plane(lo, s, 0u), volume_plane(lo, s, nz), ivz, te, tx)) return false;
    if (!(te < tx)) return false;
    int32_t ix = volume_start(Ox, te, dx, lo, s, nx);
    int32_t iy = volume_start(Oy, te, dy, lo, s, ny);
    int32_t iz = volume_start(Oz, te, dz, lo, s, nz);
    const int32_t stx = dx > 0.0 ? 1 : -1, sty = dy > 0.0 ? 1 : -1, stz = dz > 0.0 ? 1 : -1;
    const int32_t upx = dx > 0.0 ? 1 : 0, upy = dy > 0.0 ? 1 : 0, upz = dz > 0.0 ? 1 : 0;
    double tnx = dx == 0.0 ? inf : (volume_plane(lo, s, (uint32_t)(ix + upx)) - Ox) * ivx;
    double tny = dy == 0.0 ? inf : (volume_plane(lo, s, (uint32_t)(iy + upy)) - Oy) * ivy;
    double tnz = dz == 0.0 ? inf : (volume_plane(lo, s, (uint32_t)(iz + upz)) - Oz) * ivz;
    double tc = te, sum = 0.0;
    const uint32_t limit = nx + ny + nz + 3u;
    for (uint32_t k = 0; k < limit; ++k) {
        double t = tnx;                 // ties: the lower axis first
        int32_t a = 0;
        if (tny < t) { t = tny; a = 1; }
        if (tnz < t) { t = tnz; a = 2; }
        const double tend = t < tx ? t : tx;
        const double seg = tend - tc;
        const uint64_t vox = ((uint64_t)(uint32_t)iz * ny + (uint32_t)iy) * nx + (uint32_t)ix;
        if (seg > 0.0) {
            sum = sum + seg * (double)vol[vox];
            tc = tend;
        }
        if (!(t < tx)) break;
        if (a == 0) {
            ix += stx;
            if ((uint32_t)ix >= nx) break;
            tnx = (volume_plane(lo, s, (uint32_t)(ix + upx)) - Ox) * ivx;
        } else if (a == 1) {
            iy += sty;
            if ((uint32_t)iy >= ny) break;
            tny = (volume_plane(lo, s, (uint32_t)(iy + upy)) - Oy) * ivy;
        } else {
            iz += stz;
            if ((uint32_t)iz >= nz) break;
            tnz = (volume_plane(lo, s, (uint32_t)(iz + upz)) - Oz) * ivz;
        }
    }
    acc = sum;
    span = tx - te;
    return true;
}

// The length of the direction in the scene's unit: what a step of 1 in t is worth.
__host__ __device__ __forceinline__ double forward_ell(double sx, double sy, double sz, double dx, double dy, double dz)
{
    return ::sqrt(((sx * dx) * (sx * dx) + (sy * dy) * (sy * dy)) + (sz * dz) * (sz * dz));
}

// A pixel of xrt_forward_project: the ray of (row, col) under R through the
// volume, as the mode has it (meas: the pixel's measurement, read by the
// residual mode only).
__host__ __device__ __forceinline__ float forward_pixel(const float* __restrict__ vol, uint32_t nx, uint32_t ny,
                                                        uint32_t nz, double sx, double sy, double sz, const double* R,
                                                        uint32_t row, uint32_t col, int mode, float meas)
{
    const double dr = (double)row, dc = (double)col;
    const double dx = forward_direction(R, dr, dc), dy = forward_direction(R + 4, dr, dc),
                 dz = forward_direction(R + 8, dr, dc);
    double acc, span;
    if (!forward_ray(vol, nx, ny, nz, R[3], R[7], R[11], dx, dy, dz, acc, span)) return 0.0f;
    const double ell = forward_ell(sx, sy, sz, dx, dy, dz);
    if (mode == kForwardProject) return (float)(acc * ell);
    const double L = span * ell;
    return L > 0.0 ? (float)(((double)meas - acc * ell) / L) : 0.0f;
}

// A voxel of xrt_volume_update.
__host__ __device__ __forceinline__ float volume_update_voxel(float x, float corr, float norm, double relax, float lo,
                                                              float hi)
{
    if (!(norm > 0.0f)) return x;
    float v = (float)((double)x + relax * ((double)corr / (double)norm));
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return v;
}

// ---------------------------------------------------------------------------
// OS-MLTR: the Poisson likelihood's pixel stage over
// forward_ray, and the backprojector's term over a plane of (num, den) pairs.
// poisson_pixel and backproject_pair_term are the contract: k_poisson_project
// and k_backproject_update call them on the device,
// xrt_host_poisson_project and xrt_host_backproject_update compiled for the
// host, and tests/mltr_ref.py restates them.
// ---------------------------------------------------------------------------

// A pixel of xrt_poisson_project: y the measured counts, flat the expected
// counts without the object, bg the expected counts that did not come through
// it (with_bg false: +0.0).  (num, den) = (+0.0f, +0.0f) for a miss, a ray
// without length and an expectation that is not above zero.
__host__ __device__ __forceinline__ void poisson_pixel(const float* __restrict__ vol, uint32_t nx, uint32_t ny, uint32_t nz,
                                                       double sx, double sy, double sz, const double* R, uint32_t row,
                                                       uint32_t col, float y, float flat, bool with_bg, float bg, float& num,
                                                       float& den)
{
    num = den = 0.0f;
    const double dr = (double)row, dc = (double)col;
    const double dx = forward_direction(R, dr, dc), dy = forward_direction(R + 4, dr, dc),
                 dz = forward_direction(R + 8, dr, dc);
    double acc, span;
    if (!forward_ray(vol, nx, ny, nz, R[3], R[7], R[11], dx, dy, dz, acc, span)) return;
    const double ell = forward_ell(sx, sy, sz, dx, dy, dz);
    const double l = acc * ell, L = span * ell;
    const double psi = (double)flat * xrt_exp(-l);
    const double r = with_bg ? (double)bg : 0.0;
    const double yh = psi + r;
    if (!(L > 0.0) || !(yh > 0.0)) return;           // (a NaN compares false)
    const double q = psi / yh;
    num = (float)(psi - (double)y * q);
    den = (float)((L * psi) * q);
}

// A sample of a plane of pairs: the pixel's (num, den) inside, (+0.0f, +0.0f)
// outside.  A pair is one 8-byte load or store (the entries check the
// planes' alignment).
struct alignas(8) FloatPair {
    float n, d;
};

__host__ __device__ __forceinline__ void backproject_pair_sample(const FloatPair* plane, uint32_t W, uint32_t H, int32_t y,
                                                                 int32_t x, float& n, float& d)
{
    n = 0.0f;
    d = 0.0f;
    if (x >= 0 && y >= 0 && (uint32_t)x < W && (uint32_t)y < H) {
        const FloatPair s = plane[(size_t)y * W + (size_t)x];
        n = s.n;
        d = s.d;
    }
}

// backproject_term over a plane of pairs: its coordinates, acceptance tests
// and weights once, its three f32 expressions per component.
__host__ __device__ __forceinline__ void backproject_pair_term(const FloatPair* plane, uint32_t W, uint32_t H, double a,
                                                               double b, double c, double& accn, double& accd)
{
    if (!(c > 0.0)) return;                          // (a NaN compares false)
    const double w = 1.0 / c;
    const double col = a * w, row = b * w;
    if (!(col > -1.0 && col < (double)W && row > -1.0 && row < (double)H)) return;
    const double fc = floor(col), fr = floor(row);
    const float fx = (float)(col - fc), fy = (float)(row - fr);
    const int32_t x0 = (int32_t)fc, y0 = (int32_t)fr;          // -1 .. W - 1 and -1 .. H - 1
    float n00, n01, n10, n11, d00, d01, d10, d11;
    backproject_pair_sample(plane, W, H, y0, x0, n00, d00);
    backproject_pair_sample(plane, W, H, y0, x0 + 1, n01, d01);
    backproject_pair_sample(plane, W, H, y0 + 1, x0, n10, d10);
    backproject_pair_sample(plane, W, H, y0 + 1, x0 + 1, n11, d11);
    const float topn = n00 + fx * (n01 - n00);
    const float botn = n10 + fx * (n11 - n10);
    const float vn = topn + fy * (botn - topn);
    const float topd = d00 + fx * (d01 - d00);
    const float botd = d10 + fx * (d11 - d10);
    const float vd = topd + fy * (botd - topd);
    const double ww = w * w;
    accn = accn + (double)vn * ww;
    accd = accd + (double)vd * ww;
}

// ---------------------------------------------------------------------------
// TV-regularised SIRT: the gradient of the smoothed isotropic
// total variation, the sum of squares' chunk order and the descent step.
// tv_quotients and tv_voxel are the gradient's contract: k_tv_gradient calls
// them on the device and xrt_host_tv_gradient compiled for the host, and
// tests/tv_ref.py restates them.  f64, no FMA, written selects.
// ---------------------------------------------------------------------------

// The forward differences of a voxel of value v over its norm: vx, vy, vz are
// its upper neighbours' values, read only where hx, hy, hz say that there is
// one (no difference across the border).
__host__ __device__ __forceinline__ void tv_quotients(double v, double vx, double vy, double vz, bool hx, bool hy, bool hz,
                                                      double eps, double& qx, double& qy, double& qz)
{
    const double dx = hx ? vx - v : 0.0;
    const double dy = hy ? vy - v : 0.0;
    const double dz = hz ? vz - v : 0.0;
    const double n = ::sqrt(((dx * dx + dy * dy) + dz * dz) + eps);
    qx = dx / n;
    qy = dy / n;
    qz = dz / n;
}

// A voxel of xrt_tv_gradient from its own quotients and its lower neighbours'
// (bx: qx of (i - 1, j, k), +0.0 where i = 0; by, bz likewise).
__host__ __device__ __forceinline__ float tv_voxel(double bx, double by, double bz, double qx, double qy, double qz)
{
    return (float)(((bx + by) + bz) - ((qx + qy) + qz));
}

// The quotients of voxel (i, j, k) of the volume x read where it lies.
__host__ __device__ __forceinline__ void tv_quotients_at(const float* __restrict__ x, uint32_t nx, uint32_t ny, uint32_t nz,
                                                         uint32_t i, uint32_t j, uint32_t k, double eps, double& qx,
                                                         double& qy, double& qz)
{
    const uint64_t row = nx, plane = (uint64_t)nx * ny;
    const uint64_t at = ((uint64_t)k * ny + j) * nx + i;
    const bool hx = i + 1u < nx, hy = j + 1u < ny, hz = k + 1u < nz;
    tv_quotients((double)x[at], hx ? (double)x[at + 1u] : 0.0, hy ? (double)x[at + row] : 0.0,
                 hz ? (double)x[at + plane] : 0.0, hx, hy, hz, eps, qx, qy, qz);
}

// xrt_volume_sumsq's order (include/xrt.h): chunks of kSumsqChunk entries, a
// chunk's kSumsqLanes accumulators each over kSumsqRounds entries a
// kSumsqLanes apart, then the halving tree.
constexpr uint32_t kSumsqLanes = 256;
constexpr uint32_t kSumsqRounds = 16;
constexpr uint32_t kSumsqChunk = kSumsqLanes * kSumsqRounds;   // 4096

// An entry of the first level: the square of a[i], or of a[i] - b[i].
__host__ __device__ __forceinline__ double sumsq_entry(const float* __restrict__ a, const float* __restrict__ b, uint64_t i)
{
    const double e = b ? (double)a[i] - (double)b[i] : (double)a[i];
    return e * e;
}

// The descent's step length from the resident sums: scale, or scale *
// sqrt(*moved) where the solver ties it to the data step.
__host__ __device__ __forceinline__ double tv_step_length(double scale, const double* moved)
{
    return moved ? scale * ::sqrt(*moved) : scale;
}

// A voxel of a descent step under c = length / gn.
__host__ __device__ __forceinline__ float tv_step_voxel(float x, float g, double c, float lo, float hi)
{
    float v = (float)((double)x - c * (double)g);
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return v;
}

// ---------------------------------------------------------------------------
// Voxelisation (include/xrt.h "voxelise the scene"): the
// crossing of one triangle with one grid column and the outputs of one voxel,
// shared by k_voxel_scatter, k_voxel_tiles, k_voxel_scan and
// xrt_host_voxelize.  All f64, every operation rounded on its own (the build
// contracts nothing).
// ---------------------------------------------------------------------------
struct VoxelGrid {
    uint32_t nx, ny, nz;
    float ox, oy, oz;                  // the minimum corner
    float sx, sy, sz;                  // the voxel spacing
};

// The centre of voxel i along an axis of origin o and spacing s (f32 widened).
__host__ __device__ __forceinline__ double voxel_centre(float o, float s, uint32_t i)
{
    return (double)o + ((double)i + 0.5) * (double)s;
}

// The least i in [0, n] with voxel_centre(i) >= v (kStrict: > v), n when none
// is: an estimate by division, then settled by the comparisons themselves
// (the centres never decrease with i, every operation being monotone).
template <bool kStrict>
__host__ __device__ inline uint32_t voxel_first_index(float o, float s, uint32_t n, double v)
{
    const double e = (v - (double)o) / (double)s;          // about i + 0.5
    uint32_t i = e > 0.0 ? (e < (double)n ? (uint32_t)e : n) : 0u;   // (a NaN starts at 0)
    auto before = [&](uint32_t q) {
        const double c = voxel_centre(o, s, q);
        return kStrict ? c <= v : c < v;
    };
    while (i > 0u && !before(i - 1u)) --i;
    while (i < n && before(i)) ++i;
    return i;
}

// A triangle's vertices widened and its normal n = e1 x e2, each component two
// products and a difference.
struct VoxelTriangle {
    double x0, y0, z0, x1, y1, z1, x2, y2, z2;
    double nx, ny, nz;
};

__host__ __device__ inline VoxelTriangle voxel_triangle(const float* __restrict__ t)
{
    VoxelTriangle v;
    v.x0 = (double)t[0]; v.y0 = (double)t[1]; v.z0 = (double)t[2];
    v.x1 = (double)t[3]; v.y1 = (double)t[4]; v.z1 = (double)t[5];
    v.x2 = (double)t[6]; v.y2 = (double)t[7]; v.z2 = (double)t[8];
    const double ax = v.x1 - v.x0, ay = v.y1 - v.y0, az = v.z1 - v.z0;
    const double bx = v.x2 - v.x0, by = v.y2 - v.y0, bz = v.z2 - v.z0;
    v.nx = ay * bz - az * by;
    v.ny = az * bx - ax * bz;
    v.nz = ax * by - ay * bx;
    return v;
}

// Whether the edge between two vertices counts for the column at (px, py): the
// endpoints ordered by y first, so that the two triangles of a shared edge
// evaluate one expression on the same operands.
__host__ __device__ __forceinline__ bool voxel_edge_counts(double ax, double ay, double bx, double by, double px, double py)
{
    if (ay == by) return false;
    if (by < ay) {
        const double tx = ax, ty = ay;
        ax = bx; ay = by;
        bx = tx; by = ty;
    }
    const bool straddle = (ay <= py) != (by <= py);
    const double w = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    return straddle && w > 0.0;
}

// Whether the triangle crosses the column at (px, py), and then the crossing's
// slice: the least k in [0, nz] with centre_z(k) >= z.
__host__ __device__ inline bool voxel_crossing(const VoxelTriangle& t, const VoxelGrid& g, double px, double py, uint32_t& k)
{
    if (t.nz == 0.0) return false;
    const bool e01 = voxel_edge_counts(t.x0, t.y0, t.x1, t.y1, px, py);
    const bool e12 = voxel_edge_counts(t.x1, t.y1, t.x2, t.y2, px, py);
    const bool e20 = voxel_edge_counts(t.x2, t.y2, t.x0, t.y0, px, py);
    if (!(e01 ^ e12 ^ e20)) return false;
    const double z = t.z0 - (t.nx * (px - t.x0) + t.ny * (py - t.y0)) / t.nz;
    k = voxel_first_index<false>(g.oz, g.sz, g.nz, z);
    return true;
}

// The columns [i0, i1) x [j0, j1) outside which the triangle crosses nothing:
// an optimisation that leaves no crossing out.  An edge can count only with
// a.y <= py < b.y -- exact comparisons --, so py lies in [ymin, ymax).  To the
// right of xmax every straddled edge has w <= 0 whatever the rounding (the
// products round monotonically).  To the left of xmin the exact w is positive
// for every straddled edge, and the rounded one can only fail to be within
// 2^-51 (xmax - xmin) of xmin: the box keeps 2^-40 (xmax - xmin) there.
struct VoxelBox {
    uint32_t i0, i1, j0, j1;
};

__host__ __device__ inline VoxelBox voxel_footprint(const VoxelTriangle& t, const VoxelGrid& g)
{
    VoxelBox b = {0u, 0u, 0u, 0u};
    if (t.nz == 0.0) return b;
    const double xmin = ::fmin(t.x0, ::fmin(t.x1, t.x2)), xmax = ::fmax(t.x0, ::fmax(t.x1, t.x2));
    const double ymin = ::fmin(t.y0, ::fmin(t.y1, t.y2)), ymax = ::fmax(t.y0, ::fmax(t.y1, t.y2));
    b.i0 = voxel_first_index<false>(g.ox, g.sx, g.nx, xmin - (xmax - xmin) * 0x1p-40);
    b.i1 = voxel_first_index<true>(g.ox, g.sx, g.nx, xmax);
    b.j0 = voxel_first_index<false>(g.oy, g.sy, g.ny, ymin);
    b.j1 = voxel_first_index<false>(g.oy, g.sy, g.ny, ymax);
    if (b.i1 < b.i0) b.i1 = b.i0;
    return b;
}

// A voxel's label: 0 for an empty mask, else 1 + its highest set bit.
__host__ __device__ __forceinline__ uint8_t voxel_label(uint32_t mask)
{
    uint32_t l = 0u;
    while (mask) {
        ++l;
        mask >>= 1;
    }
    return (uint8_t)l;
}

// A voxel's value: the f64 sum, from 0 and in mesh order, of the values of the
// meshes it lies in, as f32.
template <typename Value>
__host__ __device__ __forceinline__ float voxel_value(uint32_t mask, uint32_t num_meshes, Value value)
{
    double sum = 0.0;
    for (uint32_t m = 0; m < num_meshes; ++m)
        if (mask >> m & 1u) sum = sum + (double)value(m);
    return (float)sum;
}

// The entry of voxel (i, j, k) in a [nz (+ 1)][ny][nx] array.
__host__ __device__ __forceinline__ uint64_t voxel_index(const VoxelGrid& g, uint32_t i, uint32_t j, uint32_t k)
{
    return ((uint64_t)k * g.ny + j) * g.nx + i;
}

// ---------------------------------------------------------------------------
// The scatter model: a kernel-superposition estimate from the
// paths model's planes.  The tables travel by value in the kernels' arguments:
// the spectrum's weights and coefficients as SpectrumTable holds them and,
// in the same layout, the part of each coefficient that scatters.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxScatterBin = 64;
constexpr uint32_t kMaxScatterKernels = 4;
struct ScatterTable {
    float weight[kMaxBins];
    uint32_t num_bins;
    float miss;                           // spectrum_miss of the weights: the L-buffer of a pixel that hits nothing
    float mu[kMaxBins * kMaxMeshes];      // [e * kMaxMeshes + m], 0 past the meshes: a bin's row is one scalar load
    float sigma[kMaxBins * kMaxMeshes];   // [e * kMaxMeshes + m]
};
struct ScatterAmps {
    float amp[kMaxScatterKernels];
    uint32_t num;
};

// One pixel's primary E and scatter source Q from its n per-mesh lengths
// dist(j) = (double)path * 0.1, in f64, left to right, every operation rounded
// on its own (no contraction):
//   E = 0; Q = 0
//   for each bin e: xe = 0; se = 0
//       for each mesh j: xe = xe + mu(j, e) * dist(j); se = se + sigma(j, e) * dist(j)
//       t = weight(e) * exp(-xe); E = E + t; Q = Q + t * se
// E's chain is spectrum_lbuffer's, so scatter_lbuffer(E) is its L bit for bit.
// A mesh with dist = +0.0 may be left out or listed under any finite row: it
// adds +0.0 to sums that are never -0.0.
template <typename Dist, typename Mu, typename Sigma, typename Weight>
__host__ __device__ __forceinline__ void scatter_pixel(uint32_t n, uint32_t num_bins, Dist dist, Mu mu, Sigma sigma,
                                                       Weight weight, double& E, double& Q)
{
    E = 0.0;
    Q = 0.0;
#pragma unroll 1
    for (uint32_t e = 0; e < num_bins; ++e) {       // (one bin's coefficients in scalar registers at a time)
        double xe = 0.0, se = 0.0;
        for (uint32_t j = 0; j < n; ++j) {
            const double d = dist(j);
            xe = xe + (double)mu(j, e) * d;
            se = se + (double)sigma(j, e) * d;
        }
        const double t = (double)weight(e) * xrt_exp(-xe);
        E = E + t;
        Q = Q + t * se;
    }
}

// The L-buffer value of scatter_pixel's E: spectrum_lbuffer's rounding and its
// explicit NaN.
__host__ __device__ __forceinline__ float scatter_lbuffer(double E)
{
    const float f = (float)E;
    return f != f ? xrt_f32_from_bits(kX86SignedNaN) : f;
}

// Where fine pixel x of a detector binned by 2^bin_log2 falls on the coarse
// axis of nc samples: u = (x + 0.5) / D - 0.5 clamped to [0, nc - 1], its two
// neighbours and the weight of the second.  (x + 0.5) * (1 / D) is the
// quotient exactly: D is a power of two.
struct ScatterAxis {
    uint32_t i0, i1;
    double f;
};
__host__ __device__ __forceinline__ ScatterAxis scatter_axis(uint32_t x, uint32_t bin_log2, uint32_t nc)
{
    const double inv = 1.0 / (double)(1u << bin_log2);
    double u = ((double)x + 0.5) * inv - 0.5;
    const double hi = (double)(nc - 1u);
    u = u < 0.0 ? 0.0 : u;
    u = u > hi ? hi : u;
    const double u0 = __builtin_floor(u);
    ScatterAxis a;
    a.i0 = (uint32_t)u0;
    a.i1 = a.i0 + 1u < nc ? a.i0 + 1u : nc - 1u;
    a.f = u - u0;
    return a;
}

// One fine pixel's scatter S from the G blurred coarse planes, coarse(g, y, x)
// their f32 values: per plane the bilinear sample in the c + f * (c' - c) form
// (a constant plane comes back exactly; f == 0 selects c whatever c' holds),
// times the plane's amplitude, summed from 0.0 in plane order.  f64, nothing
// fused.
template <typename Coarse, typename Amp>
__host__ __device__ __forceinline__ double scatter_sample(const ScatterAxis& ax, const ScatterAxis& ay, uint32_t num_kernels,
                                                          Amp amp, Coarse coarse)
{
    double S = 0.0;
    for (uint32_t g = 0; g < num_kernels; ++g) {
        const double c00 = (double)coarse(g, ay.i0, ax.i0), c01 = (double)coarse(g, ay.i0, ax.i1);
        const double c10 = (double)coarse(g, ay.i1, ax.i0), c11 = (double)coarse(g, ay.i1, ax.i1);
        const double a = ax.f == 0.0 ? c00 : c00 + ax.f * (c01 - c00);
        const double b = ax.f == 0.0 ? c10 : c10 + ax.f * (c11 - c10);
        const double v = ay.f == 0.0 ? a : a + ay.f * (b - a);
        S = S + (double)amp(g) * v;
    }
    return S;
}

// The fine tile a workgroup of k_scatter_source owns: 64 columns by
// max(D, 4) rows, whole blocks for every allowed D.
constexpr uint32_t kScatterTile = 64;
constexpr uint32_t kScatterThreads = 256;
constexpr uint32_t kScatterBatchRows = kScatterThreads / kScatterTile;
__host__ __device__ __forceinline__ uint32_t scatter_tile_rows(uint32_t bin_log2)
{
    return (1u << bin_log2) > kScatterBatchRows ? (1u << bin_log2) : kScatterBatchRows;
}

}  // namespace XRT_KERNEL_NS
