// xrt_cull_host.inc -- the host side of the tile cull: a camera's render and
// cull parameters (make_params, make_cull_params and the direction grid of
// DESIGN.md section 5, step 0) and the footprints themselves, by
// compute_footprint compiled for the host (host_footprints).  No HIP call:
// included by xrt_abi.hip, and by tools/cull_san.cpp for a host sanitizer
// build, after kernels/xrt_kernels.h.

RenderParams make_params(const xrt_camera& c, uint32_t row_begin, uint32_t row_end, uint64_t T,
                         uint32_t capacity)
{
    RenderParams p;
    p.ox = c.origin[0]; p.oy = c.origin[1]; p.oz = c.origin[2];
    p.cx = c.detector[0]; p.cy = c.detector[1]; p.cz = c.detector[2];
    p.ux = c.up[0]; p.uy = c.up[1]; p.uz = c.up[2];
    p.rx = c.right[0]; p.ry = c.right[1]; p.rz = c.right[2];
    p.spacing = c.pixel_spacing;
    p.width = c.width;
    p.height = c.height;
    p.row_begin = row_begin;
    p.row_end = row_end;
    p.num_triangles = (uint32_t)T;
    p.hit_capacity = capacity;
    p.prep_tris = prep_tris_for(T);
    return p;
}

// Grid exponent shared by every float of magnitude >= m > 0 (their ulps are
// at least 2^(floor(log2 m) - 23); 2^-149 at worst).
inline int grid_floor(double m)
{
    if (!(m > 0.0) || !std::isfinite(m)) return -149;
    return std::max(std::ilogb(m) - 23, -149);
}

// The f32 pixel offset of make_ray (main.cxx:655-656).
inline float pixel_offset(float spacing, uint32_t i, uint32_t n)
{
    return (float)((double)spacing * ((0.5 + (double)i) - (double)n / 2.0));
}

// Smallest nonzero |X_k| over the image, X_k = ((detector_k + up_k v) +
// right_k u) - origin_k in f32 as make_ray forms it (main.cxx:659): exact over
// the rows (right_k == 0) or the columns (up_k == 0) it varies with.  When it
// varies with both (a rolled, skewed or otherwise general camera), a lower
// bound in O(1): the magnitudes and grids of the four f32 operations carried
// through them (ValueRange below), every nonzero offset being >= spacing / 2.
// It proves that a nonzero X_k is at least about 2^-24 of the smaller of
// |detector_k|, |origin_k| and half a pixel's step along up_k or right_k --
// not the sum of the lowest set bits of up_k, right_k and the offset, which
// is 40 to 100 binades smaller and made step 0 of compute_footprint give up
// on ordinary triangles.  0 when X_k is 0 at every pixel.
// Smallest nonzero |x(i)| over i < n of a monotone sequence (non-decreasing or
// non-increasing; NaN-free): the last element below 0 and the first above 0,
// found by bisection -- O(log n) instead of a scan.
template <typename F>
double min_nonzero_monotone(uint32_t n, F x)
{
    double best = std::numeric_limits<double>::infinity();
    if (n == 0) return best;
    const bool up = x(0) <= x(n - 1);
    // first index whose value is past 0 in the sequence's direction (n if none)
    auto first = [&](auto past) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (past(x(mid))) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    // up: the first x > 0, and the last x < 0 (one before the first x >= 0)
    const uint32_t i_pos = up ? first([](float v) { return v > 0.0f; }) : first([](float v) { return v <= 0.0f; });
    const uint32_t i_neg = up ? first([](float v) { return v >= 0.0f; }) : first([](float v) { return v < 0.0f; });
    if (up) {
        if (i_pos < n) best = std::min(best, (double)std::fabs(x(i_pos)));
        if (i_neg > 0) best = std::min(best, (double)std::fabs(x(i_neg - 1)));
    } else {                                           // positives first, then zeros, then negatives
        if (i_pos > 0) best = std::min(best, (double)std::fabs(x(i_pos - 1)));
        if (i_neg < n) best = std::min(best, (double)std::fabs(x(i_neg)));
    }
    return best;
}

// What is known of one f32 intermediate of X_k over the whole image: every
// value is 0 (only if `zero`) or has lo <= |x| <= hi, and is a multiple of
// 2^grid.  Two rules carry it through a rounded operation:
//   (1) a rounded sum or product of multiples of 2^g is a multiple of 2^g;
//   (2) a nonzero float of magnitude >= m is a multiple of 2^(ilogb(m) - 23)
//       (grid_floor) -- so a rounded product is on the grid of its own
//       magnitude however fine its factors' grids are, and a sum that cannot
//       cancel (|a| > |b| throughout: fl(a + tiny) is near a) on that of |a| - |b|.
// Both hold; the larger grid is kept.  Magnitudes are f64 bounds of f32
// values, kept a factor (1 +- 2^-20) on the safe side of every rounding.
struct ValueRange {
    double lo, hi;
    int grid;
    bool zero;
};
constexpr double kRangeDown = 1.0 - 0x1p-20, kRangeUp = 1.0 + 0x1p-20;

inline ValueRange range_always_zero() { return {std::numeric_limits<double>::infinity(), 0.0, kNoGrid, true}; }
inline bool range_is_zero(const ValueRange& a) { return !(a.hi > 0.0); }
inline ValueRange range_of(float x)
{
    if (x == 0.0f) return range_always_zero();
    return {std::fabs((double)x), std::fabs((double)x), grid_exp(x), false};
}

// fl(x * v), x a constant.
inline ValueRange range_times(float x, const ValueRange& v)
{
    if (x == 0.0f || range_is_zero(v)) return range_always_zero();
    ValueRange p;
    const double ax = std::fabs((double)x);
    p.lo = ax * v.lo * kRangeDown;
    p.hi = ax * v.hi * kRangeUp;
    p.zero = v.zero;
    p.grid = std::max(grid_exp(x) + v.grid, -149);             // (1)
    if (p.lo < 0x1p-126) {                                     // may round to a denormal or to 0
        p.lo = 0x1p-149;
        p.zero = true;
    }
    p.grid = std::max(p.grid, grid_floor(p.lo));               // (2)
    p.lo = std::max(p.lo, std::ldexp(1.0, p.grid));
    return p;
}

// fl(a + b) (or fl(a - b): the ranges are of magnitudes).
inline ValueRange range_sum(const ValueRange& a, const ValueRange& b)
{
    if (range_is_zero(a)) return b;
    if (range_is_zero(b)) return a;
    // both terms nonzero
    ValueRange s;
    s.grid = std::min(a.grid, b.grid);                         // (1)
    s.zero = true;
    const double apart = a.lo > b.hi ? a.lo - b.hi : b.lo > a.hi ? b.lo - a.hi : 0.0;
    if (apart > 0.0) {                                         // no cancellation: |a + b| >= apart
        s.zero = false;
        s.grid = std::max(s.grid, grid_floor(apart * kRangeDown));   // (2)
        s.lo = apart * kRangeDown;
    } else {
        s.lo = 0.0;
    }
    s.lo = std::max(s.lo, std::ldexp(1.0, std::max(s.grid, -149)));
    s.hi = (a.hi + b.hi) * kRangeUp;
    // one term 0: the sum is the other term
    if (a.zero) {
        s.lo = std::min(s.lo, b.lo);
        s.grid = std::min(s.grid, b.grid);
        s.zero = s.zero || b.zero;
    }
    if (b.zero) {
        s.lo = std::min(s.lo, a.lo);
        s.grid = std::min(s.grid, a.grid);
        s.zero = s.zero || a.zero;
    }
    return s;
}

// A pixel offset of n pixels: 0 (the centre of an odd side) or at least half
// a pixel, a float of that magnitude.
inline ValueRange range_of_offsets(double ps, uint32_t n)
{
    if (!(ps > 0.0) || n == 0) return range_always_zero();
    ValueRange v;
    v.lo = 0.5 * ps * (1.0 - 0x1p-23);
    v.hi = ps * (0.5 * (double)n + 1.0) * kRangeUp;
    v.grid = grid_floor(v.lo);
    v.zero = true;
    return v;
}

double min_nonzero_x(const xrt_camera& c, int k, bool scan = false)
{
    const float cu = c.up[k], cr = c.right[k], cc = c.detector[k], co = c.origin[k];
    auto x_of = [&](float v, float u) { return ((cc + cu * v) + cr * u) - co; };
    const uint32_t kMaxScan = 1u << 20;
    double best = std::numeric_limits<double>::infinity();
    auto take = [&](float x) {
        if (x != 0.0f) best = std::min(best, (double)std::fabs(x));
    };
    // Along one axis x is monotone in the pixel index (pixel_offset and each
    // rounded f32 operation are monotone), so its smallest nonzero magnitude is
    // next to its sign change: a bisection per camera instead of a scan of
    // every row or column (xrt_debug_direction_grid compares the two).
    const bool finite = std::isfinite(cu) && std::isfinite(cr) && std::isfinite(cc) && std::isfinite(co) &&
                        std::isfinite(c.pixel_spacing);
    if (cr == 0.0f && c.height <= kMaxScan) {
        const float u0 = pixel_offset(c.pixel_spacing, 0, c.width);
        auto xr = [&](uint32_t row) { return x_of(pixel_offset(c.pixel_spacing, row, c.height), u0); };
        if (!scan && finite) best = min_nonzero_monotone(c.height, xr);
        else for (uint32_t row = 0; row < c.height; ++row) take(xr(row));
    } else if (cu == 0.0f && c.width <= kMaxScan) {
        const float v0 = pixel_offset(c.pixel_spacing, 0, c.height);
        auto xc = [&](uint32_t col) { return x_of(v0, pixel_offset(c.pixel_spacing, col, c.width)); };
        if (!scan && finite) best = min_nonzero_monotone(c.width, xc);
        else for (uint32_t col = 0; col < c.width; ++col) take(xc(col));
    } else {
        const double ps = std::fabs((double)c.pixel_spacing);
        const int goff = ps > 0.0 ? grid_floor(0.5 * ps * (1.0 - 0x1p-23)) : kNoGrid;
        int gx = std::min(grid_exp(cc), grid_exp(co));
        if (cu != 0.0f && goff != kNoGrid) gx = std::min(gx, std::max(grid_exp(cu) + goff, -149));
        if (cr != 0.0f && goff != kNoGrid) gx = std::min(gx, std::max(grid_exp(cr) + goff, -149));
        if (gx != kNoGrid) best = std::ldexp(1.0, gx);
        // The same four operations with the magnitudes carried along (ValueRange):
        // the grid of each intermediate is that of its own magnitude where
        // that is coarser than its terms' -- cu * v of a full-mantissa cu, or
        // cc + cu * v where the product is absorbed.
        if (finite) {
            const ValueRange x = range_sum(range_sum(range_sum(range_of(cc), range_times(cu, range_of_offsets(ps, c.height))),
                                                     range_times(cr, range_of_offsets(ps, c.width))),
                                           range_of(co));
            if (range_is_zero(x)) best = std::numeric_limits<double>::infinity();
            else if (x.hi < (double)std::numeric_limits<float>::max()) best = std::max(best, x.lo);
        }
    }
    return std::isfinite(best) ? best : 0.0;
}

// A grid 2^g such that every nonzero component of every ray direction of the
// image (make_ray: main.cxx:652-661 and Ray.inl:80-84) is a multiple of it:
// the two normalisations divide X_k by |X| <= dmax and by ~1, so a nonzero
// component is >= min|X_k| / (1.001 dmax), a float whose ulp is the grid.
int direction_grid(const xrt_camera& c, double dmax, bool scan = false)
{
    int g = kNoGrid;
    for (int k = 0; k < 3; ++k) {
        const double xmin = min_nonzero_x(c, k, scan);
        if (xmin > 0.0) g = std::min(g, grid_floor(xmin / (1.001 * dmax)));
    }
    return g;
}

// Bounds used by the cull derivation (DESIGN.md "Tile cull"): over every pixel
// of the image, |D| <= dmax and the terms summed into D are <= mag.
CullParams make_cull_params(const xrt_camera& c)
{
    double ps = std::fabs((double)c.pixel_spacing);
    double vmax = ps * ((double)c.height / 2.0 + 1.0);
    double umax = ps * ((double)c.width / 2.0 + 1.0);
    double d2 = 0.0, mag = 0.0;
    for (int k = 0; k < 3; ++k) {
        double cterm = std::fabs((double)c.detector[k] - (double)c.origin[k]);
        double spread = std::fabs((double)c.up[k]) * vmax + std::fabs((double)c.right[k]) * umax;
        d2 += (cterm + spread) * (cterm + spread);
        mag = std::max(mag, std::fabs((double)c.detector[k]) + spread + std::fabs((double)c.origin[k]));
    }
    CullParams cp;
    cp.dmax = std::sqrt(d2) * (1.0 + 1e-6);
    cp.mag = mag;
    cp.width = c.width;
    cp.height = c.height;
    cp.dir_grid = direction_grid(c, cp.dmax);
    cp.pad = 0;
    for (int k = 0; k < 3; ++k) {
        cp.cvec[k] = (double)c.detector[k] - (double)c.origin[k];
        cp.up[k] = c.up[k];
        cp.rt[k] = c.right[k];
    }
    cp.ps = c.pixel_spacing;
    cp.cv = cp.ps * (0.5 - cp.height / 2.0);
    cp.cu = cp.ps * (0.5 - cp.width / 2.0);
    return cp;
}

// The footprints of n triangles under `camera` on the host: each record as
// k_prep forms it (the reference's f32 operations, Ray.cxx:86-87, 102, 112,
// 122; restated here so that k_prep's own code stays as it is), then
// compute_footprint with the library's cull parameters.  footprint16 as
// xrt_probe_prep lays it out: box, then the three relaxed edges.
inline void host_footprints(const xrt_camera& camera, const float* tris, uint64_t n, float* footprint16)
{
    RenderParams p = make_params(camera, 0, camera.height, n, 0);
    p.model = kModelAttenuation;
    const CullParams cp = make_cull_params(camera);
    for (uint64_t i = 0; i < n; ++i) {
        const float* P = tris + 9 * i;
        TriRec r = {};
        r.e1x = P[3] - P[0]; r.e1y = P[4] - P[1]; r.e1z = P[5] - P[2];
        r.e2x = P[6] - P[0]; r.e2y = P[7] - P[1]; r.e2z = P[8] - P[2];
        r.tvx = p.ox - P[0]; r.tvy = p.oy - P[1]; r.tvz = p.oz - P[2];
        r.qvx = r.tvy * r.e1z - r.tvz * r.e1y;
        r.qvy = r.tvz * r.e1x - r.tvx * r.e1z;
        r.qvz = r.tvx * r.e1y - r.tvy * r.e1x;
        r.tnum = (r.e2x * r.qvx + r.e2y * r.qvy) + r.e2z * r.qvz;
        const Footprint fp = compute_footprint(r, p, cp);
        const float4 planes[4] = {fp.bbox, make_float4(fp.e0.x, fp.e0.y, fp.e0.z, 0.0f), fp.e1, fp.e2};
        std::memcpy(footprint16 + 16 * i, planes, sizeof planes);
    }
}
