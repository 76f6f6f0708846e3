// xrt_multi.inc -- single-process multi-GPU render (include/xrt.h, "multi-GPU"),
// included at the end of xrt_abi.hip (it drives the contexts' prepare_frame /
// launch_frame).
//
// The image is split into contiguous row strips.  XRT_SPLIT_EQUAL: rows_per =
// H / n with the remainder going to the first strips (the rule of the
// reference's row-range renderer, src/main-pthreads-rows.cxx:311-334).
// XRT_SPLIT_BALANCED (the default): the gather, not the render, bounds a
// multi-GPU frame -- a sender's rows cost their transfer over its one link
// into device 0, the root's only their render -- so device 0 takes ONE run of
// 32-row bands anywhere in the frame (the dense middle of the object) and the
// senders split the bands above and below it, from a model of the frame
// (per-band render cost from one full-frame render's wave timing records,
// per-band packed bytes from its fill plan) and the measured link rate
// (balanced_split; DESIGN.md "Multi-GPU").  Strip g renders on device g;
// device 0 renders its strip straight into the destination frame, the others
// into double-buffered L-buffer strips with misses coded XRT_MISS_TRANSIT
// (4 bytes per pixel instead of the 9 of three planes: the image and 8-bit
// planes are functions of the L-buffer), which one grouped ncclSend / ncclRecv
// moves into device 0's frame over xGMI -- the RCCL analogue of the reference's
// MPI root gather (src/main-mpi.cxx:855-881), one communicator per device from
// ncclCommInitAll.  Device 0 then expands the received rows into the image and
// 8-bit planes (k_expand, the same device functions as the render).  What
// travels (xrt_multi_set_transit): the 32x32 blocks of the regions a strip's
// fill plan leaves (packed), or -- XRT_TRANSIT_HITS, the default, once a
// strip geometry repeats -- per tile of those regions a 64-bit hit mask and
// the hit rays' L values, rendered straight into that layout (hit transit).  A frame's
// gather runs on each device's communication stream while the next frame
// renders into the other strip buffer.  A device listed twice (a one-GPU
// rehearsal of the strip logic) gathers with device copies instead of RCCL.
// The signed model (xrt_multi_set_model) gathers its L-buffer strips the same
// way -- no miss code is needed, a miss there is L = 80 -- and device 0 runs
// the hole fill over the assembled frame (it reads neighbouring rows, so it
// cannot run per strip).
#include <rccl/rccl.h>

#include <array>
#include <set>

struct xrt_multi {
    struct Strip {
        Owned<float> lbuffer;           // the strip's L-buffer, misses as XRT_MISS_TRANSIT
        Owned<float> packed;            // its unfilled regions, 1024 floats each (packed transit)
        Owned<float> msg;               // its hit-layout message (hit transit), 32-bit words
        Fence sent;                     // the gather that last read it
    };
    // Packed transit (DESIGN.md "Multi-GPU"): per device g > 0 its strip's region
    // map (the fill plan of its last frame; identity without one) on device g, and
    // on device 0 the unpack descriptors of every strip and the receive buffer.
    std::vector<std::vector<uint32_t>> map_host;   // per device: the map behind d_map
    std::vector<Owned<uint32_t>> d_map;
    std::vector<uint32_t> n_packed, block_base;
    Owned<uint32_t> d_desc;             // device 0: 4 u32 per region of strips 1 .. n-1
    size_t n_desc = 0;
    Owned<float> rbuf;                  // device 0: every strip's packed regions
    uint32_t desc_w = 0, desc_h = 0;    // frame the descriptors were built for
    std::vector<uint32_t> desc_b, desc_e;   // and its strips (the descriptors hold their rows)
    // Hit transit (XRT_TRANSIT_HITS): per sender the strip geometry of its last
    // frame and, once a geometry repeats, its hit plan (xrt_plan_hit_layout,
    // from that previous frame); on device 0 the hit descriptors of every
    // message and the mismatch flag.  A frame of a new geometry travels packed.
    int transit = XRT_TRANSIT_HITS;
    struct HitKey {
        xrt_camera cam = {};
        uint32_t b = 0, e = 0;
        uint64_t gen = 0;
        int kernel = 0;
        bool valid = false;
        bool same(const HitKey& o) const
        {
            return valid && o.valid && std::memcmp(&cam, &o.cam, sizeof cam) == 0 && b == o.b && e == o.e &&
                   gen == o.gen && kernel == o.kernel;
        }
    };
    std::vector<HitKey> seen, planned;  // per device: its last frame's key, its hit plan's key
    std::vector<uint64_t> hit_words;    // per device: its message's words (>= 4)
    std::vector<uint32_t> hit_base;     // per device: its message's first word in rbuf
    std::vector<std::vector<uint32_t>> tile_hits;
    Owned<uint32_t> d_hdesc;            // device 0: 4 u32 per region of strips 1 .. n-1
    Owned<uint32_t> d_tdesc;            // device 0: 4 u32 per planned tile
    size_t n_hdesc = 0;
    Owned<uint32_t> d_bad;              // device 0: a mask disagreed with its plan
    bool hits_failed = false;           // the last planning attempt failed (retried on a new geometry)
    bool maps_current = false;          // the last frame travelled packed: map_host is its geometry's
    uint64_t frames_hits = 0, frames_packed = 0, last_bytes = 0;
    std::vector<int> devices;
    std::vector<xrt_context*> ctx;
    // RCCL communicators: one per device (distinct devices), or one rank on
    // the single device of a repeated list (xrt_multi_set_gather); empty when
    // gathering with copies.  rank[g] = the rank of strip g's device.
    std::vector<ncclComm_t> comm;
    std::vector<int> rank;
    bool self_comm = false;             // one rank, strips sent to itself
    std::vector<hipStream_t> compute;   // per device render stream (device 0: the caller's, else its own)
    std::vector<hipStream_t> comms;     // per device gather stream
    std::vector<std::array<Strip, 2>> strips;
    std::vector<PlainEvent> rendered;   // per device: its strip's render is complete
    PlainEvent gathered;                // device 0: the frame is assembled
    PlainEvent caller_ready;            // device 0: the caller's stream reached the call
    hipStream_t own0 = nullptr;         // device 0 stream of the host-buffer entry point
    uint64_t frame = 0;
    Owned<float> d_image;               // device-0 frame of the host-buffer entry point
    Owned<float> d_lbuffer;
    Owned<uint8_t> d_u8;
    Owned<float> scratch_l;             // device-0 L-buffer when the caller wants none
    // Strip split (xrt_multi_set_split): the mode, the caller's link rate
    // (bytes per microsecond one sender delivers into device 0; 0 = measured
    // once, link_measured), and the plan of the last frame geometry.
    int split = XRT_SPLIT_BALANCED;
    double link_set = 0.0, link_measured = 0.0;
    // The balanced split's model, from the strips' own renders of an earlier
    // frame (k_band_model behind each strip's render of a new camera, its
    // per-band sums copied into pinned memory): per 32-row band of the frame
    // its render cost (us) and the bytes its strip would send.  No extra
    // render: the first frame of a multi context splits equally.
    struct StripModel {
        Owned<BandModel> d;             // ry + 1 entries: the bands, then the span (x = first start, y = last end)
        Pinned<BandModel> h;            // pinned copy
        Fence copied;                   // the copy is complete
        uint32_t b = 0, e = 0, ry = 0;  // the strip's rows and bands
    };
    std::vector<StripModel> smodel;
    bool model_pending = false;         // strip records of `pending_cam` on their way
    bool collected = false;             // pending_cam's strips were modelled (pending or harvested)
    xrt_camera pending_cam = {};
    uint64_t pending_gen = 0;
    bool model_valid = false;           // cost / bytes below describe a frame of this size and mesh
    uint32_t model_w = 0, model_h = 0;
    uint64_t model_gen = 0;
    std::vector<double> model_cost, model_bytes;
    double model_span_us = 0.0;
    // counters (xrt_multi_plan_stats): balanced plans made, frames split
    // equally for want of a model, link probes, strip models collected
    uint64_t n_plans = 0, n_equal_no_model = 0, n_link_probes = 0, n_models = 0;
    Pinned<uint32_t> h_bad;             // pinned: device 0's d_bad after each hit gather
    struct Plan {
        bool valid = false;
        xrt_camera cam = {};
        uint64_t gen = 0;
        int kernel = 0, model = 0, split = 0;
        double link_set = 0.0;
        std::vector<uint32_t> b, e;     // strip g = rows [b[g], e[g])
        double info[3] = {0.0, 0.0, 0.0};   // link bytes/us, frame span us, predicted step us
    } plan;
    std::string error;
};

static std::string& g_multi_create_error = *new std::string();   // never destroyed (g_create_error)

// The balanced split's allowance for device 0's unpack of the gathered blocks
// (one k_unpack_blocks launch per frame), us.
constexpr double kUnpackUs = 5.0;

namespace {

int mfail(xrt_multi* m, int code, const std::string& msg)
{
    if (m) m->error = msg;
    else g_multi_create_error = msg;
    return code;
}

#define XRT_MHIP(m, expr)                                                                     \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return mfail((m), XRT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define XRT_MNCCL(m, expr)                                                                    \
    do {                                                                                      \
        ncclResult_t _r = (expr);                                                             \
        if (_r != ncclSuccess)                                                                \
            return mfail((m), XRT_ERR_DEVICE, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
    } while (0)

// Strip g of n over `height` rows: [begin, end).
inline void strip_rows(uint32_t height, uint32_t n, uint32_t g, uint32_t& begin, uint32_t& end)
{
    const uint32_t per = height / n, rem = height % n;
    begin = g * per + std::min(g, rem);
    end = begin + per + (g < rem ? 1u : 0u);
}

// The balanced row split (DESIGN.md "Multi-GPU"): from per-band render costs
// (us) and per-band bytes a sender's packed strip sends to device 0, and the
// bytes per microsecond one sender delivers over its link, strips for n
// devices -- bounds[2g], bounds[2g+1] = [begin, end) rows of strip g; strip 0
// is the root's ONE run of bands anywhere in the frame, strips 1 .. n-1 the
// senders' pieces above it, then below it, in frame order.  Frame k's gather
// overlaps frame k+1's render, so the step is the largest of the root's
// render (+ the unpack) and each sender's max(render, bytes / link); the
// split minimises it: a bisection over the step with a greedy feasibility
// test (the root's run from each start band as long as the step allows, the
// fewest senders covering the rest), then the senders' pieces are split until
// every device has one.  Every device keeps at least one band; false when
// there are fewer bands than devices.  bench.py's strips use the same
// function (simpleraytracing_amd/strips.py -> xrt_balanced_bounds).
bool balanced_split(const double* cost, const double* byts, uint32_t nb, uint32_t n, double link, uint32_t height,
                    uint32_t band_rows, double unpack_us, std::vector<uint32_t>& bounds, double& step_out)
{
    std::vector<double> pc(nb + 1, 0.0), pb(nb + 1, 0.0);
    for (uint32_t i = 0; i < nb; ++i) {
        pc[i + 1] = pc[i] + cost[i];
        pb[i + 1] = pb[i] + byts[i];
    }
    if (n <= 1) {
        bounds.assign({0u, height});
        step_out = pc[nb] + unpack_us;
        return true;
    }
    if (nb < n || nb == 0) return false;
    link = std::max(link, 1e-9);
    auto sender = [&](uint32_t a, uint32_t b) { return std::max(pc[b] - pc[a], (pb[b] - pb[a]) / link); };
    // fewest senders covering bands [i, j) within `step` (greedy); -1: impossible
    auto pieces = [&](uint32_t i, uint32_t j, double step) -> long {
        long k = 0;
        for (uint32_t a = i; a < j;) {
            uint32_t b = a + 1;
            if (sender(a, b) > step) return -1;
            while (b < j && sender(a, b + 1) <= step) ++b;
            ++k;
            a = b;
        }
        return k;
    };
    // the root's run [ra, rb) of a feasible layout within `step`
    auto plan = [&](double step, uint32_t& ra, uint32_t& rb) -> bool {
        for (uint32_t a = 0; a < nb; ++a) {
            uint32_t b = 0;                    // the longest run from a within the step leaving a band per sender
            for (uint32_t e = nb; e > a; --e)
                if (a + (nb - e) >= n - 1 && pc[e] - pc[a] + unpack_us <= step) {
                    b = e;
                    break;
                }
            if (!b) continue;
            const long ka = pieces(0, a, step), kb = pieces(b, nb, step);
            if (ka >= 0 && kb >= 0 && ka + kb <= (long)n - 1) {
                ra = a;
                rb = b;
                return true;
            }
        }
        return false;
    };
    double lo = 0.0, hi = pc[nb] + unpack_us + pb[nb] / link;
    uint32_t ra = 0, rb = 0;
    if (!plan(hi, ra, rb)) return false;
    for (int it = 0; it < 60; ++it) {
        const double mid = 0.5 * (lo + hi);
        uint32_t a, b;
        if (plan(mid, a, b)) {
            hi = mid;
            ra = a;
            rb = b;
        } else {
            lo = mid;
        }
    }
    const double step = hi;
    auto split = [&](uint32_t i, uint32_t j) {
        std::vector<std::array<uint32_t, 2>> out;
        for (uint32_t s0 = i; s0 < j;) {
            uint32_t e = s0 + 1;
            while (e < j && sender(s0, e + 1) <= step) ++e;
            out.push_back({s0, e});
            s0 = e;
        }
        return out;
    };
    std::vector<std::array<uint32_t, 2>> side[2] = {split(0, ra), split(rb, nb)};
    while (side[0].size() + side[1].size() < n - 1) {
        // the costliest piece of two bands or more (ties: the later piece, the side below)
        double best = -1.0;
        int bs = -1;
        size_t bk = 0;
        for (int sd = 0; sd < 2; ++sd)
            for (size_t k = 0; k < side[sd].size(); ++k) {
                const uint32_t x = side[sd][k][0], y = side[sd][k][1];
                if (y - x < 2) continue;
                const double c = sender(x, y);
                if (bs < 0 || c > best || (c == best && (k > bk || (k == bk && sd > bs)))) {
                    best = c;
                    bs = sd;
                    bk = k;
                }
            }
        if (bs < 0) return false;
        const uint32_t x = side[bs][bk][0], y = side[bs][bk][1], mid = (x + y) / 2;
        side[bs][bk] = {x, mid};
        side[bs].insert(side[bs].begin() + (long)bk + 1, std::array<uint32_t, 2>{mid, y});
    }
    auto rows = [&](uint32_t band) { return (uint32_t)std::min<uint64_t>((uint64_t)band * band_rows, height); };
    bounds.clear();
    bounds.push_back(rows(ra));
    bounds.push_back(rows(rb));
    for (int sd = 0; sd < 2; ++sd)
        for (const auto& pz : side[sd]) {
            bounds.push_back(rows(pz[0]));
            bounds.push_back(rows(pz[1]));
        }
    // the step these bounds imply under the model
    double st = pc[rb] - pc[ra] + unpack_us;
    for (int sd = 0; sd < 2; ++sd)
        for (const auto& pz : side[sd]) st = std::max(st, sender(pz[0], pz[1]));
    step_out = st;
    return true;
}

// buf holds at least n (Owned::reserve); a HIP error goes to m->error.
template <typename T, typename Mem>
int mensure(xrt_multi* m, Owned<T, Mem>& buf, size_t n)
{
    XRT_MHIP(m, buf.reserve(n));
    return XRT_OK;
}

int check_ctx(xrt_multi* m, size_t g, int rc)
{
    if (rc == XRT_OK) return XRT_OK;
    return mfail(m, rc, "device " + std::to_string(m->devices[g]) + ": " + m->ctx[g]->error);
}

// The region map of device g's strip after its frame was enqueued: its fill
// plan (regions it filled travel as nothing) or the identity.
void strip_map(xrt_multi* m, uint32_t g, uint32_t W, uint32_t rows, std::vector<uint32_t>& map, uint32_t& packed)
{
    const uint32_t rx = (W + kRegion - 1) / kRegion, ry = (rows + kRegion - 1) / kRegion;
    map.assign((size_t)rx * ry, 0u);
    uint32_t k = 0;
    (void)xrt_plan_region_map(m->ctx[g], W, rows, map.data(), map.size(), &k);
    packed = k;
}

// Packed transit state for this frame's maps: per-device maps on the devices,
// device 0's descriptors and receive buffer.  Rebuilt (synchronously) only when
// a map, a strip or the frame changes -- once per geometry.  (A strip can move
// under an equal map: a 64-row frame's two strips swap when the balanced split
// follows the equal one, each one row of unfilled regions.)
int refresh_transit(xrt_multi* m, uint32_t W, uint32_t H, const std::vector<uint32_t>& b,
                    const std::vector<uint32_t>& e, bool& changed)
{
    const uint32_t n = (uint32_t)m->devices.size();
    changed = m->desc_w != W || m->desc_h != H || m->desc_b != b || m->desc_e != e;
    std::vector<std::vector<uint32_t>> maps(n);
    std::vector<uint32_t> packed(n, 0);
    for (uint32_t g = 1; g < n; ++g) {
        strip_map(m, g, W, e[g] - b[g], maps[g], packed[g]);
        changed = changed || maps[g] != m->map_host[g];
    }
    if (!changed) return XRT_OK;
    int rc;
    for (uint32_t g = 0; g < n; ++g) {                 // frames in flight read the old state
        XRT_MHIP(m, hipSetDevice(m->devices[g]));
        XRT_MHIP(m, hipDeviceSynchronize());
    }
    std::vector<uint32_t> desc;
    uint32_t base = 0;
    const uint32_t rx = (W + kRegion - 1) / kRegion;
    for (uint32_t g = 1; g < n; ++g) {
        XRT_MHIP(m, hipSetDevice(m->devices[g]));
        if ((rc = mensure(m, m->d_map[g], maps[g].size()))) return rc;
        XRT_MHIP(m, hipMemcpy(m->d_map[g].get(), maps[g].data(), maps[g].size() * 4, hipMemcpyHostToDevice));
        for (auto& st : m->strips[g]) {
            const size_t need = (size_t)std::max<uint32_t>(packed[g], 1u) * kPackBlock;
            if ((rc = mensure(m, st.packed, need))) return rc;
        }
        const uint32_t rows = e[g] - b[g];
        for (size_t r = 0; r < maps[g].size(); ++r) {
            const uint32_t y = (uint32_t)(r / rx), x = (uint32_t)(r % rx);
            desc.push_back(b[g] + kRegion * y);
            desc.push_back(std::min(kRegion, rows - kRegion * y));
            desc.push_back(kRegion * x);
            desc.push_back(maps[g][r] == kEmpty ? kEmpty : base + maps[g][r]);
        }
        m->block_base[g] = base;
        m->n_packed[g] = packed[g];
        base += std::max<uint32_t>(packed[g], 1u);
        m->map_host[g] = maps[g];
    }
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    if ((rc = mensure(m, m->d_desc, std::max<size_t>(desc.size(), 4)))) return rc;
    if (!desc.empty())
        XRT_MHIP(m, hipMemcpy(m->d_desc.get(), desc.data(), desc.size() * 4, hipMemcpyHostToDevice));
    m->n_desc = desc.size() / 4;
    if ((rc = mensure(m, m->rbuf, (size_t)base * kPackBlock))) return rc;
    m->desc_w = W;
    m->desc_h = H;
    m->desc_b = b;
    m->desc_e = e;
    return XRT_OK;
}

// The senders' strip geometry of this frame (hit transit's key).
xrt_multi::HitKey hit_key(xrt_multi* m, uint32_t g, const xrt_camera* camera, uint32_t b, uint32_t e)
{
    xrt_multi::HitKey k;
    k.cam = *camera;
    k.b = b;
    k.e = e;
    k.gen = soup_gen(m->ctx[g]);
    k.kernel = m->ctx[g]->kernel;
    k.valid = true;
    return k;
}

// Hit plans of every sender from its previous frame (this frame's geometry,
// packed), the message buffers, and device 0's hit descriptors over the maps
// that frame left (map_host).  Synchronous, once per geometry.  Returns false
// (hit transit not used for this geometry) where a sender has no plan.
bool plan_hits(xrt_multi* m, uint32_t W, const std::vector<uint32_t>& b, const std::vector<uint32_t>& e)
{
    const uint32_t n = (uint32_t)m->devices.size();
    const uint32_t rx = (W + kRegion - 1) / kRegion;
    for (uint32_t g = 0; g < n; ++g)                   // frames in flight read the old buffers
        if (hipSetDevice(m->devices[g]) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    std::vector<uint32_t> desc, tdesc;
    uint64_t base = 0, tbase = 0;
    for (uint32_t g = 1; g < n; ++g) {
        xrt_context* c = m->ctx[g];
        uint64_t tiles = 0, words = 0;
        if (hipSetDevice(m->devices[g]) != hipSuccess || xrt_plan_hit_layout(c, nullptr, 0, &tiles, &words) != XRT_OK)
            return false;
        std::vector<uint32_t>& th = m->tile_hits[g];
        th.assign(tiles, 0u);
        if (xrt_plan_hit_layout(c, th.data(), tiles, &tiles, &words) != XRT_OK) return false;
        const std::vector<uint32_t>& map = m->map_host[g];
        const uint32_t rows = e[g] - b[g];
        uint32_t n_slots = 0;
        for (uint32_t v : map) n_slots += v != kEmpty ? 1u : 0u;
        if (map.size() != (size_t)rx * ((rows + kRegion - 1) / kRegion) || tiles != (uint64_t)kWavesPerRegion * n_slots)
            return false;                              // the map is not this plan's
        const uint64_t msg = std::max<uint64_t>(words, 4u);
        for (auto& st : m->strips[g]) {                // the message, and room for one tile's overrun
            if (st.msg.reserve((size_t)msg + 64u) != hipSuccess) return false;
        }
        std::vector<uint64_t> off(tiles + 1u, 0u);
        for (uint64_t i = 0; i < tiles; ++i) off[i + 1] = off[i] + th[i];
        for (size_t r = 0; r < map.size(); ++r) {
            const uint32_t y = (uint32_t)(r / rx), x = (uint32_t)(r % rx);
            desc.push_back(b[g] + kRegion * y);
            desc.push_back(std::min(kRegion, rows - kRegion * y));
            desc.push_back(kRegion * x);
            desc.push_back(map[r] == kEmpty ? kEmpty : (uint32_t)(tbase + (uint64_t)kWavesPerRegion * map[r]));
        }
        for (uint64_t i = 0; i < tiles; ++i) {
            tdesc.push_back((uint32_t)(base + 2 * i));
            tdesc.push_back((uint32_t)(base + 2 * tiles + off[i]));
            tdesc.push_back(th[i]);
            tdesc.push_back(0u);
        }
        m->hit_words[g] = msg;
        m->hit_base[g] = (uint32_t)base;
        base += (msg + 3u) / 4u * 4u;
        tbase += tiles;
        if (base > 0xFFFFFFFFull) return false;
    }
    if (tdesc.empty()) tdesc.assign(4, 0u);
    if (hipSetDevice(m->devices[0]) != hipSuccess) return false;
    if (mensure(m, m->d_hdesc, std::max<size_t>(desc.size(), 4)) || mensure(m, m->d_tdesc, tdesc.size()) ||
        mensure(m, m->d_bad, 4))
        return false;
    if ((!desc.empty() && hipMemcpy(m->d_hdesc.get(), desc.data(), desc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(m->d_tdesc.get(), tdesc.data(), tdesc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(m->d_bad.get(), 0, 4) != hipSuccess)
        return false;
    m->n_hdesc = desc.size() / 4;
    if (mensure(m, m->rbuf, base)) return false;
    for (uint32_t g = 1; g < n; ++g)
        if (xrt_set_transit_hits(m->ctx[g], m->strips[g][0].msg.cap()) != XRT_OK) return false;
    return true;
}

// Bytes per microsecond one sender delivers into device 0 while every sender
// sends at once (the gather's pattern), through the gather this multi context
// uses (RCCL, or device copies on a repeated device list): 4 MB from each of
// devices 1 .. n-1, one untimed round, then the mean of five.
int measure_link(xrt_multi* m, double& rate)
{
    const uint32_t n = (uint32_t)m->devices.size();
    rate = 0.0;
    if (n < 2) return XRT_OK;
    const size_t count = (size_t)1 << 20;         // floats: 4 MB
    std::vector<float*> src(n, nullptr);
    float* dst = nullptr;
    int rc = XRT_OK;
    auto release = [&]() {
        for (uint32_t g = 1; g < n; ++g) {
            (void)hipSetDevice(m->devices[g]);
            (void)hipFree(src[g]);
        }
        (void)hipSetDevice(m->devices[0]);
        (void)hipFree(dst);
    };
    auto one_round = [&]() -> int {
        if (!m->comm.empty()) {
            XRT_MNCCL(m, ncclGroupStart());
            for (uint32_t g = 1; g < n; ++g) {
                ncclComm_t cs = m->comm[m->self_comm ? 0 : g];
                XRT_MNCCL(m, ncclSend(src[g], count, ncclFloat32, 0, cs, m->self_comm ? m->comms[0] : m->comms[g]));
                XRT_MNCCL(m, ncclRecv(dst + (size_t)(g - 1) * count, count, ncclFloat32, m->rank[g], m->comm[0],
                                      m->comms[0]));
            }
            XRT_MNCCL(m, ncclGroupEnd());
        } else {
            XRT_MHIP(m, hipSetDevice(m->devices[0]));
            for (uint32_t g = 1; g < n; ++g)
                XRT_MHIP(m, hipMemcpyAsync(dst + (size_t)(g - 1) * count, src[g], count * 4, hipMemcpyDefault,
                                           m->comms[0]));
        }
        for (uint32_t g = 0; g < n; ++g) {
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            XRT_MHIP(m, hipStreamSynchronize(m->comms[g]));
        }
        return XRT_OK;
    };
    for (uint32_t g = 1; g < n && rc == XRT_OK; ++g) {
        if (hipSetDevice(m->devices[g]) != hipSuccess || hipMalloc(&src[g], count * 4) != hipSuccess ||
            hipMemset(src[g], 0, count * 4) != hipSuccess)
            rc = mfail(m, XRT_ERR_DEVICE, "link probe allocation failed");
    }
    if (rc == XRT_OK && (hipSetDevice(m->devices[0]) != hipSuccess ||
                         hipMalloc(&dst, (size_t)(n - 1) * count * 4) != hipSuccess))
        rc = mfail(m, XRT_ERR_DEVICE, "link probe allocation failed");
    if (rc == XRT_OK) rc = one_round();
    const int reps = 5;
    const auto t0 = HostClock::now();
    for (int r = 0; r < reps && rc == XRT_OK; ++r) rc = one_round();
    const double us = std::chrono::duration<double, std::micro>(HostClock::now() - t0).count() / reps;
    release();
    if (rc == XRT_OK) rate = (double)(count * 4) / std::max(us, 1e-3);
    return rc;
}

// The strip models of the last frame that collected one (k_band_model behind
// each strip's render), once every device's copy is complete, into the
// frame's model: per 32-row band of the frame its render cost in us (each
// strip's wave time per band scaled to that strip's span; a strip band that
// straddles two frame bands is shared by its rows) and the bytes it would
// send -- packed: a 32x32 block of 4 B per tile region; hits: per tile region
// 16 masks of 8 B and 4 B per hit ray.  Never waits: records still in flight
// leave the previous model in place.
void harvest_model(xrt_multi* m)
{
    if (!m->model_pending) return;
    const uint32_t n = (uint32_t)m->devices.size();
    for (uint32_t g = 0; g < n; ++g) {
        (void)hipSetDevice(m->devices[g]);
        if (m->smodel[g].copied.passed() != hipSuccess) return;
    }
    m->model_pending = false;
    const uint32_t W = m->pending_cam.width, H = m->pending_cam.height;
    const uint32_t nb = (H + kRegion - 1) / kRegion;
    std::vector<double> cost(nb, 0.0), byts(nb, 0.0);
    double span_max = 0.0;
    for (uint32_t g = 0; g < n; ++g) {
        const xrt_multi::StripModel& sm = m->smodel[g];
        const BandModel* const h = sm.h.get();
        const uint32_t s_lo = h[sm.ry].ticks, s_hi = h[sm.ry].hits;         // the span entry
        const double span_us = s_hi > s_lo ? (double)(s_hi - s_lo) / (kTicksPerMs * 1e-3) : 0.0;
        uint64_t total = 0;
        for (uint32_t j = 0; j < sm.ry; ++j) total += h[j].ticks;
        if (!(span_us > 0.0) || total == 0) return;            // not a usable record: keep the old model
        span_max = std::max(span_max, span_us);
        for (uint32_t j = 0; j < sm.ry; ++j) {
            const double c = (double)h[j].ticks / (double)total * span_us;
            const double by = m->transit == XRT_TRANSIT_HITS ? 8.0 * kWavesPerRegion * h[j].tiles + 4.0 * h[j].hits
                                                             : 4.0 * kPackBlock * h[j].tiles;
            const uint32_t r0 = sm.b + j * kRegion, r1 = std::min(sm.e, r0 + kRegion);
            for (uint32_t fb = r0 / kRegion; fb * kRegion < r1 && fb < nb; ++fb) {
                const uint32_t o0 = std::max(r0, fb * kRegion), o1 = std::min(r1, (fb + 1) * kRegion);
                const double w = (double)(o1 - o0) / (double)(r1 - r0);
                cost[fb] += w * c;
                byts[fb] += w * by;
            }
        }
    }
    m->model_cost.swap(cost);
    m->model_bytes.swap(byts);
    m->model_span_us = span_max;
    m->model_w = W;
    m->model_h = H;
    m->model_gen = m->pending_gen;
    m->model_valid = true;
    ++m->n_models;
}

// Behind every strip's render of frame `camera` (launched): its band model
// (k_band_model) into pinned memory.  The set's completion event is recorded
// again after it, so the set's records and the layout it reads are not
// rewritten under it.  Frames of a camera already modelled, or whose strips
// did not all render binned, collect nothing.
int collect_model(xrt_multi* m, const xrt_camera* camera, const std::vector<uint32_t>& b,
                  const std::vector<uint32_t>& e, const std::vector<PendingFrame>& pf, hipStream_t s0)
{
    const uint32_t n = (uint32_t)m->devices.size();
    if (m->collected && std::memcmp(&m->pending_cam, camera, sizeof *camera) == 0 &&
        m->pending_gen == soup_gen(m->ctx[0]))
        return XRT_OK;                                 // this camera's strips were modelled already
    for (uint32_t g = 0; g < n; ++g)
        if (!pf[g].binned || pf[g].rows == 0 || !m->ctx[g]->last_set || !m->ctx[g]->last_set->binned) return XRT_OK;
    if (m->model_pending) {                            // an older frame's records: wait for their copies
        for (uint32_t g = 0; g < n; ++g) {
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            XRT_MHIP(m, m->smodel[g].copied.wait());
        }
        // ... and take them: a host that runs ahead of the caller's stream never finds them complete in
        // plan_strips, and the records below would overwrite every model unread
        harvest_model(m);
    }
    for (uint32_t g = 0; g < n; ++g) {
        xrt_context* c = m->ctx[g];
        FrameSet& fs = *c->last_set;
        xrt_multi::StripModel& sm = m->smodel[g];
        hipStream_t sg = g == 0 ? s0 : m->compute[g];
        XRT_MHIP(m, hipSetDevice(m->devices[g]));
        const uint32_t ry = pf[g].ry, n_slots = pf[g].rx * pf[g].ry;
        if (std::min(sm.d.cap(), sm.h.cap()) < (size_t)ry + 1u) {
            XRT_MHIP(m, hipStreamSynchronize(sg));
            if (int rc = mensure(m, sm.d, (size_t)ry + 1u)) return rc;
            if (int rc = mensure(m, sm.h, (size_t)ry + 1u)) return rc;
        }
        BandModel* const d = sm.d.get();
        XRT_MHIP(m, hipMemsetAsync(d, 0, (size_t)ry * sizeof(BandModel), sg));
        XRT_MHIP(m, hipMemsetAsync(d + ry, 0xFF, sizeof(uint32_t), sg));             // span start: ~0
        XRT_MHIP(m, hipMemsetAsync(reinterpret_cast<uint32_t*>(d + ry) + 1, 0, 3 * sizeof(uint32_t), sg));
        const uint32_t tile_slots = n_slots - c->last_fill_regions;
        hipLaunchKernelGGL(k_band_model, dim3((n_slots + 255) / 256), dim3(256), 0, sg, fs.block_stats.get(),
                           fs.last_times, pf[g].bins.desc, n_slots, tile_slots, d, reinterpret_cast<uint32_t*>(d + ry));
        XRT_MHIP(m, hipGetLastError());
        XRT_MHIP(m, hipMemcpyAsync(sm.h.get(), d, ((size_t)ry + 1u) * sizeof(BandModel), hipMemcpyDeviceToHost, sg));
        XRT_MHIP(m, sm.copied.record(sg));
        XRT_MHIP(m, hipEventRecord(fs.done.get(), sg));      // the set is reused after the model read it
        fs.done_ev = fs.done.get();
        sm.b = b[g];
        sm.e = e[g];
        sm.ry = ry;
    }
    m->model_pending = true;
    m->collected = true;
    m->pending_cam = *camera;
    m->pending_gen = soup_gen(m->ctx[0]);
    return XRT_OK;
}

// The strips of this frame: equal (the reference's rule) or balanced (a plan
// per frame geometry: camera, mesh, kernel, model and link setting).
int plan_strips(xrt_multi* m, const xrt_camera* camera, std::vector<uint32_t>& b, std::vector<uint32_t>& e)
{
    const uint32_t n = (uint32_t)m->devices.size(), H = camera->height;
    b.assign(n, 0u);
    e.assign(n, 0u);
    auto equal = [&]() {
        for (uint32_t g = 0; g < n; ++g) strip_rows(H, n, g, b[g], e[g]);
    };
    const xrt_context* c0 = m->ctx[0];
    const uint32_t bands = (H + kRegion - 1) / kRegion;
    if (n < 2 || m->split == XRT_SPLIT_EQUAL || c0->model != kModelAttenuation || bands < n) {
        equal();
        return XRT_OK;
    }
    xrt_multi::Plan& P = m->plan;
    if (P.valid && std::memcmp(&P.cam, camera, sizeof *camera) == 0 && P.gen == soup_gen(c0) &&
        P.kernel == c0->kernel && P.model == (int)c0->model && P.split == m->split && P.link_set == m->link_set) {
        b = P.b;
        e = P.e;
        return XRT_OK;
    }
    // the model of an earlier frame of this size and mesh (any camera: a
    // projection sweep moves little between frames); none yet -- the multi
    // context's first frame -- splits equally (not a plan: the next frame of
    // this camera plans from the first one's strips)
    harvest_model(m);
    if (!m->model_valid || m->model_w != camera->width || m->model_h != H || m->model_gen != soup_gen(c0) ||
        m->model_cost.size() != bands) {
        equal();
        ++m->n_equal_no_model;
        return XRT_OK;
    }
    int rc;
    double link = m->link_set;
    if (!(link > 0.0)) {                               // measured once per multi context (and gather path)
        if (!(m->link_measured > 0.0)) {
            ++m->n_link_probes;
            if ((rc = measure_link(m, m->link_measured))) return rc;
        }
        link = m->link_measured;
    }
    const double span_us = m->model_span_us;
    double step = 0.0;
    std::vector<uint32_t> bounds;
    if (!balanced_split(m->model_cost.data(), m->model_bytes.data(), bands, n, link, H, kRegion, kUnpackUs, bounds,
                        step)) {
        equal();
        return XRT_OK;
    }
    ++m->n_plans;
    for (uint32_t g = 0; g < n; ++g) {
        b[g] = bounds[2 * g];
        e[g] = bounds[2 * g + 1];
    }
    P.valid = true;
    P.cam = *camera;
    P.gen = soup_gen(c0);
    P.kernel = c0->kernel;
    P.model = (int)c0->model;
    P.split = m->split;
    P.link_set = m->link_set;
    P.b = b;
    P.e = e;
    P.info[0] = link;
    P.info[1] = span_us;
    P.info[2] = step;
    return XRT_OK;
}

// A hit mask that disagreed with its sender's plan (k_unpack_hits sets d_bad;
// the flag reaches h_bad behind each hit gather): that frame's values were not
// its plan's.  Every hit plan is dropped (the next frame of each geometry
// travels packed, the one after plans again) and the error is reported.
bool hit_mismatch(xrt_multi* m) { return m->h_bad.get() && *(volatile uint32_t*)m->h_bad.get() != 0u; }

int report_hit_mismatch(xrt_multi* m)
{
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    XRT_MHIP(m, hipStreamSynchronize(m->comms[0]));
    if (m->d_bad.get()) XRT_MHIP(m, hipMemset(m->d_bad.get(), 0, 4));
    *m->h_bad.get() = 0u;
    for (auto& k : m->planned) k = xrt_multi::HitKey();
    m->hits_failed = false;
    return mfail(m, XRT_ERR_DEVICE, "hit transit: a received hit mask disagreed with its sender's plan (that frame's "
                                    "gathered rows are wrong); the hit plans were dropped and are made again");
}

}  // namespace

extern "C" {

int xrt_balanced_bounds(const double* band_cost, const double* band_bytes, uint32_t n_bands, uint32_t n,
                        double link_bytes_per_us, uint32_t height, uint32_t band_rows, double unpack_us,
                        uint32_t* bounds, double* step_us)
{
    if (!band_cost || !band_bytes || !bounds || n < 1 || band_rows < 1) return XRT_ERR_ARGUMENT;
    std::vector<uint32_t> b;
    double step = 0.0;
    if (!balanced_split(band_cost, band_bytes, n_bands, n, link_bytes_per_us, height, band_rows, unpack_us, b, step))
        return XRT_ERR_ARGUMENT;
    std::copy(b.begin(), b.end(), bounds);
    if (step_us) *step_us = step;
    return XRT_OK;
}

int xrt_multi_set_split(xrt_multi* m, int mode, double link_bytes_per_us)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    if (mode != XRT_SPLIT_EQUAL && mode != XRT_SPLIT_BALANCED)
        return mfail(m, XRT_ERR_ARGUMENT, "unknown split mode");
    if (!(link_bytes_per_us >= 0.0)) return mfail(m, XRT_ERR_ARGUMENT, "link rate must be >= 0");
    m->split = mode;
    m->link_set = link_bytes_per_us;
    m->plan.valid = false;
    return XRT_OK;
}

int xrt_multi_plan(xrt_multi* m, const xrt_camera* camera, uint32_t* bounds, double* info)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    int rc = check_camera(m->ctx[0], camera, 0, camera ? camera->height : 0);
    if (rc) return mfail(m, rc, m->ctx[0]->error);
    std::vector<uint32_t> b, e;
    if ((rc = plan_strips(m, camera, b, e))) return rc;
    for (size_t g = 0; g < b.size(); ++g) {
        if (bounds) {
            bounds[2 * g] = b[g];
            bounds[2 * g + 1] = e[g];
        }
    }
    const bool planned = m->plan.valid && std::memcmp(&m->plan.cam, camera, sizeof *camera) == 0 && m->plan.b == b;
    if (info)
        for (int k = 0; k < 3; ++k) info[k] = planned ? m->plan.info[k] : 0.0;
    return XRT_OK;
}

int xrt_multi_create(const int* devices, int num_devices, xrt_multi** out)
{
    if (!out) return mfail(nullptr, XRT_ERR_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!devices || num_devices < 1) return mfail(nullptr, XRT_ERR_ARGUMENT, "no devices");
    xrt_multi* m = new xrt_multi();
    m->devices.assign(devices, devices + num_devices);
    const size_t n = m->devices.size();
    m->ctx.assign(n, nullptr);
    m->compute.assign(n, nullptr);
    m->comms.assign(n, nullptr);
    m->strips.resize(n);
    m->rendered.resize(n);
    m->map_host.resize(n);
    m->d_map.resize(n);
    m->n_packed.assign(n, 0);
    m->block_base.assign(n, 0);
    m->seen.assign(n, xrt_multi::HitKey());
    m->planned.assign(n, xrt_multi::HitKey());
    m->hit_words.assign(n, 0);
    m->hit_base.assign(n, 0);
    m->tile_hits.resize(n);
    m->smodel.resize(n);
    int rc = XRT_OK;
    for (size_t g = 0; g < n && rc == XRT_OK; ++g) {
        rc = xrt_create(m->devices[g], &m->ctx[g]);
        if (rc != XRT_OK) {
            rc = mfail(m, rc, std::string("xrt_create: ") + xrt_last_error(nullptr));
            break;
        }
        // every camera sized for itself: the per-device maps and the root's
        // receive descriptors then change only with the geometry
        m->ctx[g]->reuse_cameras = false;
        (void)hipSetDevice(m->devices[g]);
        bool ok = hipStreamCreateWithFlags(&m->comms[g], hipStreamNonBlocking) == hipSuccess &&
                  m->rendered[g].create() == hipSuccess;
        if (g > 0) ok = ok && hipStreamCreateWithFlags(&m->compute[g], hipStreamNonBlocking) == hipSuccess;
        if (g == 0)
            ok = ok && m->h_bad.reserve(1) == hipSuccess && (*m->h_bad.get() = 0u, true) &&
                 m->gathered.create() == hipSuccess && m->caller_ready.create() == hipSuccess &&
                 hipStreamCreateWithFlags(&m->own0, hipStreamNonBlocking) == hipSuccess;
        if (!ok) rc = mfail(m, XRT_ERR_DEVICE, "stream / event creation failed");
        else if (g > 0 && xrt_set_miss_code(m->ctx[g], XRT_MISS_TRANSIT) != XRT_OK)
            rc = mfail(m, XRT_ERR_DEVICE, "xrt_set_miss_code failed");
    }
    if (rc == XRT_OK) rc = xrt_multi_set_gather(m, XRT_GATHER_AUTO);
    if (rc != XRT_OK) {
        g_multi_create_error = m->error;
        xrt_multi_destroy(m);
        return rc;
    }
    *out = m;
    return XRT_OK;
}

void xrt_multi_destroy(xrt_multi* m)
{
    if (!m) return;
    for (size_t g = 0; g < m->devices.size(); ++g) {
        (void)hipSetDevice(m->devices[g]);
        if (m->comms[g]) (void)hipStreamSynchronize(m->comms[g]);
        if (m->compute[g]) (void)hipStreamSynchronize(m->compute[g]);
    }
    for (ncclComm_t c : m->comm)
        if (c) (void)ncclCommDestroy(c);
    for (size_t g = 0; g < m->devices.size(); ++g) {
        (void)hipSetDevice(m->devices[g]);
        if (g < m->d_map.size()) m->d_map[g].reset();
        m->strips[g] = {};                             // the strip buffers and their fences
        m->rendered[g].reset();
        if (g < m->smodel.size()) m->smodel[g] = xrt_multi::StripModel();
        if (m->comms[g]) (void)hipStreamDestroy(m->comms[g]);
        if (m->compute[g]) (void)hipStreamDestroy(m->compute[g]);
        if (g == 0) {
            release(m->gathered, m->caller_ready);
            if (m->own0) (void)hipStreamDestroy(m->own0);
            release(m->d_image, m->d_lbuffer, m->d_u8, m->scratch_l, m->d_desc, m->d_hdesc, m->d_tdesc, m->d_bad,
                    m->h_bad, m->rbuf);
        }
        xrt_destroy(m->ctx[g]);
    }
    delete m;
}

const char* xrt_multi_last_error(const xrt_multi* m) { return m ? m->error.c_str() : g_multi_create_error.c_str(); }

int xrt_multi_num_devices(const xrt_multi* m) { return m ? (int)m->devices.size() : 0; }

int xrt_multi_upload_mesh(xrt_multi* m, const float* triangles, uint64_t num_triangles)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    for (size_t g = 0; g < m->ctx.size(); ++g) {   // the mesh is replicated (40 MB at 1.12M triangles)
        int rc = check_ctx(m, g, xrt_upload_mesh(m->ctx[g], triangles, num_triangles));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_upload_scene(xrt_multi* m, const float* triangles, const uint64_t* mesh_triangles,
                           uint32_t num_meshes)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    for (size_t g = 0; g < m->ctx.size(); ++g) {   // replicated, as the mesh is
        int rc = check_ctx(m, g, xrt_upload_scene(m->ctx[g], triangles, mesh_triangles, num_meshes));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_set_kernel(xrt_multi* m, int kernel)
{
    if (!m) return XRT_ERR_ARGUMENT;
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        int rc = check_ctx(m, g, xrt_set_kernel(m->ctx[g], kernel));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_set_model(xrt_multi* m, int model, float mu)
{
    if (!m) return XRT_ERR_ARGUMENT;
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        int rc = check_ctx(m, g, xrt_set_model(m->ctx[g], model, mu));
        if (rc) return rc;
        // a signed strip in transit needs no miss code (a miss is L = 80)
        rc = check_ctx(m, g, xrt_set_miss_code(m->ctx[g], g > 0 && model != XRT_MODEL_SIGNED ? XRT_MISS_TRANSIT : 0u));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_set_materials(xrt_multi* m, const float* mu, uint32_t num_meshes)
{
    if (!m) return XRT_ERR_ARGUMENT;
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        int rc = check_ctx(m, g, xrt_set_materials(m->ctx[g], mu, num_meshes));
        if (rc) return rc;
        rc = check_ctx(m, g, xrt_set_miss_code(m->ctx[g], 0u));   // as for the signed model: a miss is L = 80
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_set_spectrum(xrt_multi* m, const float* weight, const float* mu, uint32_t num_meshes,
                           uint32_t num_bins)
{
    if (!m) return XRT_ERR_ARGUMENT;
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        int rc = check_ctx(m, g, xrt_set_spectrum(m->ctx[g], weight, mu, num_meshes, num_bins));
        if (rc) return rc;
        rc = check_ctx(m, g, xrt_set_miss_code(m->ctx[g], 0u));   // a miss is the table's miss value: no transit code
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_set_pose(xrt_multi* m, uint32_t mesh, const float pose[12])
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    for (size_t g = 0; g < m->ctx.size(); ++g) {   // every device poses its own copy of the scene
        int rc = check_ctx(m, g, xrt_set_pose(m->ctx[g], mesh, pose));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_multi_reset_poses(xrt_multi* m)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        int rc = check_ctx(m, g, xrt_reset_poses(m->ctx[g]));
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_render_rows_multi_device(xrt_multi* m, const xrt_camera* camera, float* d_image, float* d_lbuffer,
                                 uint8_t* d_u8, void* stream)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    int rc = check_camera(m->ctx[0], camera, 0, camera ? camera->height : 0);
    if (rc) return mfail(m, rc, m->ctx[0]->error);
    if (hit_mismatch(m)) return report_hit_mismatch(m);          // an earlier frame's gather
    const uint32_t n = (uint32_t)m->devices.size(), W = camera->width, H = camera->height;
    const size_t buf = m->frame & 1u;
    hipStream_t s0 = (hipStream_t)stream;
    std::vector<PendingFrame> pf(n);
    std::vector<uint32_t> b, e;
    if ((rc = plan_strips(m, camera, b, e))) return rc;
    const bool planes = d_image || d_lbuffer || d_u8;
    const bool sgn = m->ctx[0]->model != kModelAttenuation;   // signed, materials or spectrum: L-buffer strips, hole fill
    // device 0's L-buffer receives the other strips (a scratch frame when the caller wants none)
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    float* lroot = d_lbuffer;
    if (!lroot && planes && (n > 1 || sgn)) {
        if (m->scratch_l.cap() < (size_t)W * H) {
            XRT_MHIP(m, hipDeviceSynchronize());
            if ((rc = mensure(m, m->scratch_l, (size_t)W * H))) return rc;
        }
        lroot = m->scratch_l.get();
    }
    // Hit transit: every sender's strip geometry repeats one its plan was made
    // for (or its previous, packed frame can give that plan now)
    const bool packed = n > 1 && planes && !sgn;
    bool hits = packed && m->transit == XRT_TRANSIT_HITS;
    for (uint32_t g = 1; g < n && hits; ++g) hits = m->planned[g].same(hit_key(m, g, camera, b[g], e[g]));
    if (packed && m->transit == XRT_TRANSIT_HITS && !hits && !m->hits_failed && m->maps_current) {
        bool again = true;                             // each sender's previous frame was this geometry's
        for (uint32_t g = 1; g < n && again; ++g) again = m->seen[g].same(hit_key(m, g, camera, b[g], e[g]));
        if (again) {
            hits = plan_hits(m, W, b, e);
            for (uint32_t g = 1; g < n; ++g) {
                m->planned[g] = hits ? m->seen[g] : xrt_multi::HitKey();
                m->ctx[g]->error.clear();
            }
            m->hits_failed = !hits;
        }
    }
    for (uint32_t g = 1; g < n; ++g)                   // a packed frame renders its senders row-major
        if (!hits && m->ctx[g]->hits_cap && (rc = check_ctx(m, g, xrt_set_transit_hits(m->ctx[g], 0)))) return rc;
    // the gather into the caller's planes comes after the caller's earlier work on them
    XRT_MHIP(m, hipEventRecord(m->caller_ready.get(), s0));
    XRT_MHIP(m, hipStreamWaitEvent(m->comms[0], m->caller_ready.get(), 0));
    // every device's preparation first, then the renders
    for (uint32_t g = 0; g < n; ++g) {
        const size_t px = (size_t)(e[g] - b[g]) * W;
        float *img = nullptr, *lb = nullptr;
        uint8_t* u8 = nullptr;
        hipStream_t sg = g == 0 ? s0 : m->compute[g];
        if (g == 0) {                                  // device 0 renders in place
            const size_t o = (size_t)b[0] * W;
            img = d_image && !sgn ? d_image + o : nullptr;
            lb = sgn ? (planes ? lroot + o : nullptr) : d_lbuffer ? d_lbuffer + o : nullptr;
            u8 = d_u8 && !sgn ? d_u8 + o : nullptr;
        } else if (planes) {
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            xrt_multi::Strip& st = m->strips[g][buf];
            if (st.sent.pending()) {                   // the gather two frames ago still reads it
                XRT_MHIP(m, st.sent.order(sg));
                st.sent.forget();
            }
            if (hits) {
                if (!m->ctx[g]->hits_cap &&
                    (rc = check_ctx(m, g, xrt_set_transit_hits(m->ctx[g], st.msg.cap()))))
                    return rc;
                lb = st.msg.get();
            } else {
                if (st.lbuffer.cap() < px) {
                    XRT_MHIP(m, hipStreamSynchronize(sg));
                    if ((rc = mensure(m, st.lbuffer, px))) return rc;
                }
                lb = st.lbuffer.get();
            }
        }
        if ((rc = check_ctx(m, g, prepare_frame(m->ctx[g], camera, b[g], e[g], img, lb, u8, sg, pf[g]))))
            return rc;
    }
    for (uint32_t g = 0; g < n; ++g) {
        if ((rc = check_ctx(m, g, launch_frame(m->ctx[g], pf[g])))) return rc;
        if (g == 0 && sgn && planes) {                 // the hole fill reads device 0's rows too
            XRT_MHIP(m, hipSetDevice(m->devices[0]));
            XRT_MHIP(m, hipEventRecord(m->rendered[0].get(), s0));
            XRT_MHIP(m, hipStreamWaitEvent(m->comms[0], m->rendered[0].get(), 0));
        }
        if (g > 0) {
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            XRT_MHIP(m, hipEventRecord(m->rendered[g].get(), m->compute[g]));
            XRT_MHIP(m, hipStreamWaitEvent(m->comms[g], m->rendered[g].get(), 0));
        }
    }
    // the balanced split's model from this frame's strips (a new camera)
    if (n > 1 && m->split == XRT_SPLIT_BALANCED && !sgn && (rc = collect_model(m, camera, b, e, pf, s0))) return rc;
    // Packed transit for the attenuation model: only the regions each strip's
    // fill plan did not fill travel (the maps change once per geometry).
    if (packed && !hits) {
        bool changed = false;
        if ((rc = refresh_transit(m, W, H, b, e, changed))) return rc;
        for (uint32_t g = 1; g < n; ++g) {             // pack on the strip's device, after its render
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            if ((rc = check_ctx(m, g, xrt_pack_regions_device(m->ctx[g], W, e[g] - b[g], m->d_map[g].get(),
                                                              m->strips[g][buf].lbuffer.get(), m->strips[g][buf].packed.get(),
                                                              m->comms[g]))))
                return rc;
        }
    }
    if (packed) {
        ++(hits ? m->frames_hits : m->frames_packed);
        m->maps_current = !hits;
        for (uint32_t g = 1; g < n; ++g) {             // each sender's last frame geometry
            const xrt_multi::HitKey k = hit_key(m, g, camera, b[g], e[g]);
            if (!m->seen[g].same(k)) m->hits_failed = false;   // a new geometry may plan
            m->seen[g] = k;
        }
    } else {                                           // (the senders' frames hold no transit)
        m->maps_current = false;
        for (auto& k : m->seen) k = xrt_multi::HitKey();
    }
    if (n > 1 && planes) {
        // the root gather: device g's strip (packed regions, or its L-buffer rows
        // [b_g, e_g)) to device 0
        auto src = [&](uint32_t g) -> const float* {
            return hits ? m->strips[g][buf].msg.get() : packed ? m->strips[g][buf].packed.get() : m->strips[g][buf].lbuffer.get();
        };
        auto dst = [&](uint32_t g) -> float* {
            return hits     ? m->rbuf.get() + m->hit_base[g]
                   : packed ? m->rbuf.get() + (size_t)m->block_base[g] * kPackBlock
                            : lroot + (size_t)b[g] * W;
        };
        auto count = [&](uint32_t g) -> size_t {
            return hits     ? (size_t)m->hit_words[g]
                   : packed ? (size_t)std::max<uint32_t>(m->n_packed[g], 1u) * kPackBlock
                            : (size_t)(e[g] - b[g]) * W;
        };
        m->last_bytes = 0;
        for (uint32_t g = 1; g < n; ++g) m->last_bytes += 4u * count(g);
        const bool send_on_root = m->comm.empty() || m->self_comm;   // the strips live on device 0
        if (send_on_root) {                            // the root's gather stream follows each strip's pack
            for (uint32_t g = 1; g < n; ++g) {
                XRT_MHIP(m, hipSetDevice(m->devices[g]));
                XRT_MHIP(m, hipEventRecord(m->rendered[g].get(), m->comms[g]));
            }
            XRT_MHIP(m, hipSetDevice(m->devices[0]));
            for (uint32_t g = 1; g < n; ++g) XRT_MHIP(m, hipStreamWaitEvent(m->comms[0], m->rendered[g].get(), 0));
        }
        if (!m->comm.empty()) {
            XRT_MNCCL(m, ncclGroupStart());
            for (uint32_t g = 1; g < n; ++g) {
                const int r = m->rank[g];
                ncclComm_t cs = m->comm[m->self_comm ? 0 : g];
                XRT_MNCCL(m, ncclSend(src(g), count(g), ncclFloat32, 0, cs, m->self_comm ? m->comms[0] : m->comms[g]));
                XRT_MNCCL(m, ncclRecv(dst(g), count(g), ncclFloat32, r, m->comm[0], m->comms[0]));
            }
            XRT_MNCCL(m, ncclGroupEnd());
        } else {                                       // a device listed twice: device copies
            for (uint32_t g = 1; g < n; ++g)
                XRT_MHIP(m, hipMemcpyAsync(dst(g), src(g), count(g) * 4, hipMemcpyDefault, m->comms[0]));
        }
        for (uint32_t g = 1; g < n; ++g) {
            XRT_MHIP(m, hipSetDevice(m->devices[g]));
            xrt_multi::Strip& st = m->strips[g][buf];
            XRT_MHIP(m, st.sent.record(send_on_root ? m->comms[0] : m->comms[g]));
        }
        // the received rows into the image and 8-bit planes (and the miss codes back to +inf)
        if (hits) {
            if ((rc = check_ctx(m, 0, xrt_unpack_hits_device(m->ctx[0], W, m->n_hdesc, m->d_hdesc.get(), m->d_tdesc.get(),
                                                             reinterpret_cast<const uint32_t*>(m->rbuf.get()), lroot,
                                                             d_image, d_u8, m->d_bad.get(), m->comms[0]))))
                return rc;
            XRT_MHIP(m, hipMemcpyAsync(m->h_bad.get(), m->d_bad.get(), 4, hipMemcpyDeviceToHost, m->comms[0]));
        } else if (packed) {
            if ((rc = check_ctx(m, 0, xrt_unpack_blocks_device(m->ctx[0], W, m->n_desc, m->d_desc.get(), m->rbuf.get(), lroot,
                                                               d_image, d_u8, m->comms[0]))))
                return rc;
        } else if (!sgn) {                             // the rows above and below the root's strip
            const uint32_t spans[2][2] = {{0u, b[0]}, {e[0], H}};
            for (const auto& sp : spans) {
                if (sp[1] <= sp[0]) continue;
                const size_t o = (size_t)sp[0] * W;
                if ((rc = check_ctx(m, 0, xrt_expand_rows_device(m->ctx[0], (size_t)(sp[1] - sp[0]) * W, lroot + o,
                                                                 d_image ? d_image + o : nullptr,
                                                                 d_u8 ? d_u8 + o : nullptr, m->comms[0]))))
                    return rc;
            }
        }
    }
    if (sgn && (d_image || d_u8)) {                    // the fork's hole fill over the whole frame
        if ((rc = check_ctx(m, 0, xrt_hole_fill_device(m->ctx[0], W, H, lroot, d_image, d_u8, m->comms[0]))))
            return rc;
    }
    // the caller's stream sees the assembled frame
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    XRT_MHIP(m, hipEventRecord(m->gathered.get(), m->comms[0]));
    XRT_MHIP(m, hipStreamWaitEvent(s0, m->gathered.get(), 0));
    ++m->frame;
    return XRT_OK;
}

int xrt_multi_set_transit(xrt_multi* m, int mode)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    if (mode != XRT_TRANSIT_PACKED && mode != XRT_TRANSIT_HITS) return mfail(m, XRT_ERR_ARGUMENT, "unknown transit mode");
    m->transit = mode;
    m->hits_failed = false;
    for (auto& k : m->planned) k = xrt_multi::HitKey();   // the next repeat of a geometry plans again
    return XRT_OK;
}

int xrt_multi_transit_stats(xrt_multi* m, uint64_t out[4])
{
    if (!m || !out) return XRT_ERR_ARGUMENT;
    out[0] = m->frames_hits;
    out[1] = m->frames_packed;
    out[2] = m->last_bytes;
    uint32_t bad = 0;
    if (m->d_bad.get()) {
        XRT_MHIP(m, hipSetDevice(m->devices[0]));
        XRT_MHIP(m, hipStreamSynchronize(m->comms[0]));
        XRT_MHIP(m, hipMemcpy(&bad, m->d_bad.get(), 4, hipMemcpyDeviceToHost));
    }
    out[3] = bad;
    return XRT_OK;
}

int xrt_multi_plan_stats(xrt_multi* m, uint64_t out[4])
{
    if (!m || !out) return XRT_ERR_ARGUMENT;
    out[0] = m->n_plans;
    out[1] = m->n_equal_no_model;
    out[2] = m->n_link_probes;
    out[3] = m->n_models;
    return XRT_OK;
}

int xrt_multi_debug_corrupt_hit_plan(xrt_multi* m)
{
    if (!m) return XRT_ERR_ARGUMENT;
    if (!m->d_tdesc.get()) return mfail(m, XRT_ERR_ARGUMENT, "no hit plan");
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    XRT_MHIP(m, hipDeviceSynchronize());
    uint32_t td[4];
    XRT_MHIP(m, hipMemcpy(td, m->d_tdesc.get(), sizeof td, hipMemcpyDeviceToHost));
    td[2] += 1u;                                      // tile 0 of the first sender expects one more hit
    XRT_MHIP(m, hipMemcpy(m->d_tdesc.get(), td, sizeof td, hipMemcpyHostToDevice));
    return XRT_OK;
}

int xrt_multi_set_gather(xrt_multi* m, int mode)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    if (mode != XRT_GATHER_AUTO && mode != XRT_GATHER_COPY && mode != XRT_GATHER_RCCL)
        return mfail(m, XRT_ERR_ARGUMENT, "unknown gather mode");
    const size_t n = m->devices.size();
    const std::set<int> distinct(m->devices.begin(), m->devices.end());
    const bool all_distinct = distinct.size() == n, one_device = distinct.size() == 1;
    if (mode == XRT_GATHER_RCCL && !all_distinct && !one_device)
        return mfail(m, XRT_ERR_ARGUMENT, "an RCCL gather needs distinct devices or one device listed n times");
    const bool rccl = n > 1 && (mode == XRT_GATHER_RCCL || (mode == XRT_GATHER_AUTO && all_distinct));
    for (size_t g = 0; g < n; ++g) {                  // frames in flight may gather over the old state
        XRT_MHIP(m, hipSetDevice(m->devices[g]));
        XRT_MHIP(m, hipDeviceSynchronize());
    }
    // a link rate measured through the other gather path, and the split and
    // hit plans made with it, are not this path's
    m->link_measured = 0.0;
    m->plan.valid = false;
    for (auto& k : m->planned) k = xrt_multi::HitKey();
    m->hits_failed = false;
    for (ncclComm_t c : m->comm)
        if (c) (void)ncclCommDestroy(c);
    m->comm.clear();
    m->rank.assign(n, 0);
    m->self_comm = false;
    if (!rccl) return XRT_OK;
    if (all_distinct) {                                // one communicator per device
        m->comm.assign(n, nullptr);
        for (size_t g = 0; g < n; ++g) m->rank[g] = (int)g;
        ncclResult_t r = ncclCommInitAll(m->comm.data(), (int)n, m->devices.data());
        if (r != ncclSuccess) {
            m->comm.clear();
            return mfail(m, XRT_ERR_DEVICE, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
        }
    } else {                                           // one rank on the single device
        m->comm.assign(1, nullptr);
        ncclResult_t r = ncclCommInitAll(m->comm.data(), 1, m->devices.data());
        if (r != ncclSuccess) {
            m->comm.clear();
            return mfail(m, XRT_ERR_DEVICE, std::string("ncclCommInitAll (one rank): ") + ncclGetErrorString(r));
        }
        m->self_comm = true;
    }
    return XRT_OK;
}

int xrt_multi_read_stats(xrt_multi* m, xrt_stats* stats)
{
    if (!m || !stats) return XRT_ERR_ARGUMENT;
    std::memset(stats, 0, sizeof *stats);
    for (size_t g = 0; g < m->ctx.size(); ++g) {
        xrt_stats s;
        int rc = check_ctx(m, g, xrt_read_stats(m->ctx[g], &s));
        if (rc) return rc;
        stats->rays += s.rays;
        stats->hit_rays += s.hit_rays;
        stats->odd_rays += s.odd_rays;
        stats->overflow_rays += s.overflow_rays;
        stats->hits += s.hits;
        stats->max_hits = std::max(stats->max_hits, s.max_hits);
        stats->kernel = s.kernel;
        stats->kernel_ms = std::max(stats->kernel_ms, s.kernel_ms);
        stats->candidates += s.candidates;
        stats->tile_tests += s.tile_tests;
        stats->global_triangles = std::max(stats->global_triangles, s.global_triangles);
    }
    for (size_t g = 0; g < m->devices.size(); ++g) {
        XRT_MHIP(m, hipSetDevice(m->devices[g]));
        XRT_MHIP(m, hipStreamSynchronize(m->comms[g]));
    }
    return XRT_OK;
}

int xrt_render_rows_multi(xrt_multi* m, const xrt_camera* camera, float* image, float* lbuffer,
                          uint8_t* image_u8, xrt_stats* stats)
{
    if (!m) return mfail(nullptr, XRT_ERR_ARGUMENT, "multi context is NULL");
    int rc = check_camera(m->ctx[0], camera, 0, camera ? camera->height : 0);
    if (rc) return mfail(m, rc, m->ctx[0]->error);
    const size_t px = (size_t)camera->width * camera->height;
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    if (std::min({m->d_image.cap(), m->d_lbuffer.cap(), m->d_u8.cap()}) < px) {
        XRT_MHIP(m, hipDeviceSynchronize());
        if ((rc = mensure(m, m->d_image, px)) || (rc = mensure(m, m->d_lbuffer, px)) || (rc = mensure(m, m->d_u8, px)))
            return rc;
    }
    rc = xrt_render_rows_multi_device(m, camera, image ? m->d_image.get() : nullptr, lbuffer ? m->d_lbuffer.get() : nullptr,
                                      image_u8 ? m->d_u8.get() : nullptr, m->own0);
    if (rc) return rc;
    XRT_MHIP(m, hipSetDevice(m->devices[0]));
    // (through device 0's pinned ring and copy threads)
    const std::vector<D2HCopy> copies = plane_copies(px, image, m->d_image.get(), lbuffer, m->d_lbuffer.get(), image_u8, m->d_u8.get());
    if ((rc = check_ctx(m, 0, d2h_copy(m->ctx[0], m->own0, copies)))) return rc;
    XRT_MHIP(m, hipStreamSynchronize(m->own0));
    if (hit_mismatch(m)) return report_hit_mismatch(m);          // this frame's gather
    xrt_stats local;
    return xrt_multi_read_stats(m, stats ? stats : &local);
}

}  // extern "C"
