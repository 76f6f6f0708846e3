// xrt_plan_host.inc -- how a binned frame's region lists are sized: the frame
// geometry's key (BinKey), the state a context keeps about it (GeometryState),
// the one decision per frame (choose_list_mode), the base launch order of a
// region grid (centre_first_order) and the compact lists and fill plan a
// host-sized frame computes from its counts (plan_lists).  No HIP call and no
// xrt_context: included by xrt_abi.hip, and by tools/plan_san.cpp for a host
// sanitizer build, after xrt.h (xrt_camera) and the standard headers.

// Split tiles (DESIGN.md "Split tiles"): in a frame whose tile waves are at
// most kSplitFillFactor x the GPU's wave slots (its span is its heaviest tiles'),
// the regions with at least kSplitHeavyFrac of the heaviest region's candidates
// (and at least kSplitFloor) render each tile with two waves.  Larger frames
// split nothing (their heavy regions start first and others cover the tail).
// XRT_SPLIT_MIN=n instead splits every region of at least n candidates in any
// frame (0: never).
constexpr double kSplitFillFactor = 2.0;
constexpr double kSplitHeavyFrac = 0.6;
constexpr uint32_t kSplitFloor = 64;
constexpr uint32_t kSplitAuto = 0xFFFFFFFFu;
// A camera that stays put this many frames over lists sized for another
// camera is sized for itself.
constexpr uint32_t kStillFrames = 2;

// Binned list sizing: the region lists are sized by a synchronous count
// whenever the frame geometry changes (mesh, camera, strip); later frames
// of the same geometry reuse the size without a host round trip.
struct BinKey {
    xrt_camera cam;
    uint32_t row_begin, row_end;
    uint64_t T, gen;
    uint64_t pose_gen;             // the meshes' poses (xrt_set_pose)
    // field by field (the struct has padding; the camera's floats by bits)
    bool same(const BinKey& o) const
    {
        return std::memcmp(&cam, &o.cam, sizeof cam) == 0 && row_begin == o.row_begin &&
               row_end == o.row_end && T == o.T && gen == o.gen && pose_gen == o.pose_gen;
    }
    // the same region grid and mesh: only the camera's or the meshes' pose differs
    bool same_layout(const BinKey& o) const
    {
        return cam.width == o.cam.width && cam.height == o.cam.height && row_begin == o.row_begin &&
               row_end == o.row_end && T == o.T && gen == o.gen;
    }
};
static_assert(sizeof(xrt_camera) == 15 * 4, "xrt_camera has no padding (compared bytewise)");

// How a frame's region lists are sized (DESIGN.md "List modes").
enum class ListMode {
    None,          // not binned, or no rows: no lists
    Fixed,         // a forced capacity (xrt_set_bin_capacity), or no better lists known
    Compact,       // bin_key's compact lists, already sized
    HostSized,     // count pass, read-back, plan_lists, second k_prep into the compact lists
    DeviceMoving,  // a new camera over bin_key's region grid: sized on the device
    DeviceFirst,   // a geometry's first host-buffer frame: sized on the device, its pool checked
};

// What a context knows about the geometry its lists were sized for.
struct GeometryState {
    BinKey bin_key = {};
    bool bin_key_valid = false;
    bool compact = false;              // the compact layout is valid for bin_key
    bool dev_geometry = false;         // bin_key's only frame was sized on the device (no compact lists)
    // The last frame rendered over lists sized for another camera (DESIGN.md
    // "Moving camera"): a sizing then plans for motion (roomier lists, no
    // fill plan).
    bool moving = false;
    BinKey last_key = {};              // the last frame's geometry
    uint32_t still_frames = 0;         // frames in a row on one camera over reused lists
    void resize_next_frame() { bin_key_valid = false; }
};

struct FrameFacts {
    BinKey key;
    bool binned;                       // BINNED, with rows and triangles
    bool attenuation;                  // the fill plan's model (the other models' renders fill nothing)
    bool forced_cap;                   // xrt_set_bin_capacity in force
    bool transit;                      // xrt_set_transit_layout / _hits in force
    bool reuse_cameras;                // false for xrt_render_rows_multi's contexts
    bool device_first;                 // XRT_DEVICE_FIRST
    bool host_stream;                  // a host-buffer call (on the context's host stream)
};

// The frame's list mode, and the state's transitions for it.
inline ListMode choose_list_mode(GeometryState& g, const FrameFacts& f)
{
    const BinKey& key = f.key;
    // A new camera over the same region grid (a projection sweep) reuses the
    // lists sized for an earlier camera instead of the synchronous sizing
    // (DESIGN.md "Moving camera"), without a fill plan: k_prep flags a region
    // count past its list's capacity, that region renders from the whole mesh
    // (exact) and the next frame re-sizes.  A camera that then stays put for
    // kStillFrames frames is sized for itself (tight lists and a fill plan).
    // Contexts of xrt_render_rows_multi size every camera (reuse_cameras).
    g.still_frames = key.same(g.last_key) ? g.still_frames + 1u : 0u;
    g.last_key = key;
    bool reuse = false;
    if (f.binned && f.attenuation && g.bin_key_valid && (g.compact || g.dev_geometry) && !f.forced_cap && !f.transit) {
        if (f.reuse_cameras && !key.same(g.bin_key) && key.same_layout(g.bin_key) && g.still_frames < kStillFrames) {
            reuse = true;
            g.moving = true;
        } else if (g.moving && g.still_frames >= kStillFrames) {
            g.moving = false;              // the camera stopped: sized for it below
            g.bin_key_valid = false;
        }
    }
    if (!key.same_layout(g.bin_key)) g.moving = false;
    if (!f.binned) return ListMode::None;
    if (reuse) return ListMode::DeviceMoving;
    // (a geometry whose only frame was sized on the device has no compact
    // lists: the same camera again is sized on the host)
    if (g.bin_key_valid && key.same(g.bin_key) && !g.dev_geometry)
        return g.compact && !f.forced_cap ? ListMode::Compact : ListMode::Fixed;
    g.compact = false;                     // a new geometry
    g.dev_geometry = false;
    if (f.forced_cap) return ListMode::Fixed;
    // A frame geometry seen for the first time -- a context's first frame, the
    // reference's whole workload -- is sized on the device as a moving camera's
    // frame is (one 32-byte read-back for the pool, no host plan and no
    // second k_prep); the same geometry again is sized on the host (compact
    // lists, fill plan, heaviest regions first) for the frames that follow.
    // Host-buffer calls only (xrt_render_rows: the drop-in renderLoop's one
    // frame into an Image): device-pointer callers -- pipelines, and strips
    // whose transit plans (xrt_plan_region_map, xrt_plan_hit_layout) describe
    // the host-sized layout of the frame before -- keep the host sizing.
    if (f.device_first && g.still_frames == 0u && f.attenuation && !f.transit && f.reuse_cameras && f.host_stream) {
        g.dev_geometry = true;             // later cameras over its region grid take the moving path
        g.bin_key = key;
        g.bin_key_valid = true;
        return ListMode::DeviceFirst;
    }
    // A new geometry's first k_prep only counts its pairs (no lists): the
    // compact lists are sized from the counts and k_prep runs again into them.
    return ListMode::HostSized;
}

// The base launch order of a region grid: centre first (regions by the
// distance of their centre from the image centre), so the dense middle of a
// centred object does not start last and set the tail.
inline std::vector<uint32_t> centre_first_order(uint32_t rx, uint32_t ry)
{
    // by squared distance from the grid's centre, ties in region order: keys
    // (4 x the squared distance, exact in integers) beside the indices, sorted
    // once (a comparator recomputing the distances took 0.37 ms at 64 x 64)
    const size_t n = (size_t)rx * ry;
    std::vector<std::pair<uint64_t, uint32_t>> key(n);
    for (uint32_t y = 0; y < ry; ++y)
        for (uint32_t x = 0; x < rx; ++x) {
            const int64_t dx = 2 * (int64_t)x - ((int64_t)rx - 1), dy = 2 * (int64_t)y - ((int64_t)ry - 1);
            const size_t r = (size_t)y * rx + x;
            key[r] = {(uint64_t)(dx * dx + dy * dy), (uint32_t)r};
        }
    std::sort(key.begin(), key.end());
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = key[k].second;
    return order;
}

// A host-sized geometry's compact layout: slot s renders region slot_region[s]
// from list[base[s] .. base[s] + cap[s]) of `pool` entries; slots
// [tile_slots, regions) are the fill plan's, the first split_slots split.
struct ListPlan {
    std::vector<uint32_t> slot_region, base, cap;
    uint32_t tile_slots = 0, split_slots = 0;
    uint64_t pool = 0;
};

// The plan from a count pass: counts[s * stride] pairs in launch slot s of the
// fixed layout, whose slot s is region fixed_region[s].  fill_plan is
// xrt_set_fill_plan's mode, split_min XRT_SPLIT_MIN's (or kSplitAuto),
// wave_slots the render waves the GPU holds, waves_per_region a region's tile
// waves.  False, with `plan` untouched, when the lists exceed 2^32 entries.
inline bool plan_lists(const uint32_t* counts, size_t stride, const std::vector<uint32_t>& fixed_region,
                       uint32_t global_count, int fill_plan, bool moving, uint32_t split_min, uint32_t wave_slots,
                       uint32_t waves_per_region, ListPlan& plan)
{
    const uint32_t n_regions = (uint32_t)fixed_region.size();
    std::vector<uint32_t> count_of(n_regions);     // by region
    for (uint32_t s = 0; s < n_regions; ++s) count_of[fixed_region[s]] = counts[(size_t)s * stride];
    // The fill plan (not for a moving camera, whose next pose would miss it):
    // the regions this frame counted empty (with an empty global list) go to
    // the end of the launch order, one workgroup each; the tile regions by
    // candidate count, heaviest first (their long tiles start first instead
    // of setting the tail: render 2048^2 -6 %, 1024^2 -10 %).
    std::vector<uint32_t> slot_region = fixed_region;
    uint32_t tile_slots = n_regions, split_slots = 0;
    if (fill_plan != 0 && global_count == 0u && !moving) {
        std::vector<uint32_t> full, empty;
        for (uint32_t r : fixed_region) (count_of[r] != 0u && fill_plan != 2 ? full : empty).push_back(r);
        std::stable_sort(full.begin(), full.end(), [&](uint32_t a, uint32_t b) { return count_of[a] > count_of[b]; });
        tile_slots = (uint32_t)full.size();
        // the heaviest regions (the first slots): two waves per tile
        if (split_min == kSplitAuto) {
            const bool small = (double)tile_slots * waves_per_region <= kSplitFillFactor * wave_slots;
            const uint32_t heaviest = tile_slots ? count_of[full[0]] : 0u;
            split_min = small ? std::max<uint32_t>(kSplitFloor, (uint32_t)std::ceil(kSplitHeavyFrac * heaviest))
                              : 0u;
        }
        while (split_min && split_slots < tile_slots && count_of[full[split_slots]] >= split_min)
            ++split_slots;
        full.insert(full.end(), empty.begin(), empty.end());
        slot_region.swap(full);
    }
    std::vector<uint32_t> base(n_regions), cap(n_regions);
    uint64_t run = 0;
    for (uint32_t s = 0; s < n_regions; ++s) {
        const uint64_t c = count_of[slot_region[s]];
        // a moving camera: room for the counts of the next poses (2c + 64)
        const uint64_t room = moving ? 2u * c + 64u : c + c / 8u + 4u;
        base[s] = (uint32_t)run;
        cap[s] = (uint32_t)std::min<uint64_t>(room, 0xFFFFFFFFull);
        run += room;
    }
    if (run > 0xFFFFFFFFull) return false;
    plan = ListPlan{std::move(slot_region), std::move(base), std::move(cap), tile_slots, split_slots, run};
    return true;
}
