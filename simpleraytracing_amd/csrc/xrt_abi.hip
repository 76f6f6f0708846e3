// xrt_abi.hip -- the C ABI of include/xrt.h: device/context management,
// launches and the host-side camera arithmetic.  Built into libxrt.so by
// simpleraytracing_amd/csrc/Makefile (hipcc --offload-arch=gfx950).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "xrt_debug.h"
#include "kernels/xrt_kernels.h"

using namespace XRT_KERNEL_NS;

// Region lists: the first frame of a geometry (xrt_context::BinKey) bins into
// lists of kInitialRegionCap entries per region, reads every region's count
// back once, and re-bins into compact lists sized from them (the counts of
// every later frame of the geometry are the same): the sum of the counts plus
// 1/8 + 4 per region, instead of the largest count times the regions.
constexpr uint32_t kInitialRegionCap = 256;
// Timed regions (xrt_timing_begin/end) keep the timing records of every
// frame (Outputs::wave_times: each wave's s_memrealtime start and end), up to
// kTimingRecords of them (8 B each) per region, and put a HIP start/stop event
// pair on the render dispatch of every kEventStride-th frame, a cross-check of
// the in-kernel spans (a start event costs the frame a few microseconds).
// xrt_timing_begin allocates the region's record space (one chunk: room for
// kTimingFrames frames of the context's last frame size, at most
// kTimingRecords = 1 GB, 128 frames of 8192^2) and its events up front: an allocation inside the region
// stalls the host for long enough that the GPU idles, and an idle GPU drops
// its clocks and takes ~30 ms of load to ramp them back (DESIGN.md
// "Measurement").  Frames past the record space are not sampled.
constexpr size_t kTimingRecords = (size_t)1 << 27;
constexpr size_t kTimingFrames = 256;
// After a timed region a context keeps one chunk of at most this many bytes
// for the next region; larger ones are freed (xrt_timing_end).
constexpr size_t kKeptTimingBytes = (size_t)64 << 20;
constexpr uint64_t kEventStride = 16;
constexpr size_t kTimingEvents = 256;          // start/stop pairs created by xrt_timing_begin
// s_memrealtime ticks per millisecond (100 MHz on gfx950)
constexpr double kTicksPerMs = 1e5;
// Buffer sets in rotation: frame N's preparation reuses the set of frame
// N - kFrameSets, whose render the host has seen complete by then.
#ifndef XRT_FRAME_SETS
#define XRT_FRAME_SETS 4
#endif
constexpr int kFrameSets = XRT_FRAME_SETS;
// LDS a k_prep workgroup holds (its own + dynamic padding): the CU's LDS left
// beside a render at full occupancy (XRT_RENDER_WAVES waves per SIMD, each
// with its record stage), split over kPrepPerCu workgroups, so no more of
// them share a CU with the render (round 3: three beside the render, 1.12
// M-triangle frame 1,224 -> 1,143 us, 4096^2 -1.5 %, 2048^2 equal; one or two
// per CU starve the preparation, DESIGN.md "Pipelining").  LDS is allocated
// in 512-B granules.
#ifndef XRT_PREP_PER_CU
#define XRT_PREP_PER_CU 3
#endif
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kLdsGranule = 512;
constexpr size_t kRenderLdsPerCu = (size_t)XRT_RENDER_WAVES * 4 * kRenderLdsPerWave;
static_assert(kRenderLdsPerCu < kLdsPerCu, "the render's stages fit a CU at full occupancy");
constexpr size_t kPrepLds = (kLdsPerCu - kRenderLdsPerCu) / XRT_PREP_PER_CU / kLdsGranule * kLdsGranule;
// Frames prepared ahead of their call when a device-pointer render repeats
// its geometry (xrt_context::ahead); with kFrameSets sets, two renders can be
// in flight beside them.
#ifndef XRT_AHEAD_FRAMES
#define XRT_AHEAD_FRAMES 2
#endif
constexpr size_t kAheadFrames = XRT_AHEAD_FRAMES;
static_assert(kAheadFrames + 2 <= (size_t)kFrameSets, "sets for the renders in flight and the frames ahead");


// Everything one frame's preparation writes and its render reads or writes.
// kFrameSets sets rotate, so frame N+1's preparation (k_prep, binning) runs on
// the context's prep stream while frame N renders on the caller's stream.
// Ordering is kept by the host, not by cross-queue waits on the device
// (each costs the render queue several microseconds per frame, DESIGN.md
// "Pipelining"): the host waits for the preparation's completion event before
// it launches the render, and for the completion event of the render that
// last used the set before it prepares into the set again.
constexpr uint32_t kDirtyAll = 0xFFFFFFFFu;
constexpr int kHostCallFields = 16;    // xrt_debug_host_call_ms
constexpr int kAccFields = 8;          // running sums behind host_call_ms[8..15]
// D2H of the host-buffer entry points (xrt_render_rows, ...): the planes are
// DMAed in pieces of at most kStageChunk into a pinned staging ring of
// kStageSlots pieces (allocated with the context), and the context's copy
// threads move each piece into the caller's pages while the DMA of the next
// pieces runs.  A pageable hipMemcpy stages through one thread at 12.7 GB/s
// into fresh pages (tools/probes/d2h_probe.hip); the DMA into pinned memory
// runs at ~54 GB/s and the page faults of fresh caller pages are taken by
// several threads at once.  Pieces end at 2-MB boundaries of the caller's
// buffer (a transparent huge page is faulted in by one thread: 512-KB parts of
// one page on several threads measured 3.7-4.9 ms for 37.7 MB of fresh pages
// against 1.5-1.8 ms).  XRT_D2H_THREADS overrides the thread count (0:
// pageable hipMemcpy).
constexpr size_t kStageChunk = (size_t)2 << 20;
constexpr size_t kStageSlots = 16;
constexpr int kD2HThreads = 8;
// Pinned scratch of the list sizing (the count read-back) and of the launch
// layouts' uploads, allocated with the context and grown on demand: pageable
// copies there stage or pin the caller-side memory inside the HIP call, and a
// fresh context's first sizing right after a long frame loop once waited
// 10-22 ms in them (DESIGN.md "Measurement").
constexpr size_t kSizingScratch = (size_t)1 << 20;

#include "xrt_owned_host.inc"

struct FrameSet {
    Owned<TriRec> recs;            // per-render records
    Owned<float4> cull;            // per-render cull planes (4 x T float4)
    Owned<RenderParams> frame;           // the frame's parameters (k_prep writes, make_ray reads)
    Owned<float> offsets;                // the frame's pixel offsets, rows then columns (k_prep)
    Owned<BlockStats> block_stats;       // the render's per-workgroup / per-wave records
    Owned<uint2> times;                  // their timing records (Outputs::wave_times), frames not sampled
    // where the set's last render stored its timing records: `times`, or a
    // timed region's chunk (copied back into `times` by xrt_timing_end)
    const uint2* last_times = nullptr;
    uint32_t rendered_blocks = 0;        // records of the set's last render (n_blocks of its frame)
    uint32_t n_blocks = 0;         // records of the set's last render
    bool binned = false;           // the set's last frame was binned (BinState valid)

    // binning (XRT_KERNEL_BINNED)
    // Two halves (parities), each [BinState line | line-padded region counts].
    // A frame counts into one half while its k_prep clears the other, which
    // the set's previous frame used (its render is complete: the host waited
    // for it before reusing the set) -- no memset on the per-frame path.
    Owned<uint32_t> bin_counts;        // words, both halves
    size_t bin_half_words = 0;         // words per half
    uint32_t half = 0;                 // half of the set's last frame
    // Per half: the counters past dirty[h] are zero, and so is its BinState
    // when dirty[h] == 0; kDirtyAll = unknown (fresh allocation).
    uint32_t dirty[2] = {kDirtyAll, kDirtyAll};
    BinState* last_state = nullptr;    // BinState of the set's last binned frame
    Owned<RegionEntry> bin_list;       // regions x capacity footprint entries
    Owned<RegionEntry> global_list;

    // Completion events ride on the kernel dispatches themselves
    // (hipExtLaunchKernel stop events): no separate event packets.
    Owned<SlotDesc> dyn_desc;          // a device-sized frame's launch layout (k_size_lists)
    Owned<uint4> pairs;                // its (slot, index, triangle) pairs (k_prep's count pass)
    Owned<SlotDesc> plan_desc;         // its render layout under the device fill plan (tiles first, then fills)
    Owned<uint32_t> plan_counts;       // and its counter lines in that order
    bool lazy_flags = false;           // plan_flag armed for a frame launched without reading it
    TimedEvent ready;                  // k_prep complete (prep stream)
    TimedEvent done;                   // render end (a stop event on the render's dispatch)
    hipEvent_t done_ev = nullptr;      // the event that marks the set's last render complete: done, or a region's (tev)
    bool done_valid = false;
    bool ray_reader = false;           // the set's last render reads the context's ray table
    // k_prep's flags (BinBuffers::plan_miss): [0] the fill plan did not hold,
    // [1] a list overflowed.  Host-mapped, cleared by the host before k_prep,
    // read after the host has waited for k_prep's completion.
    Owned<volatile uint32_t, PinnedMem<hipHostMallocCoherent>> plan_flag;
};

using HostClock = std::chrono::steady_clock;

// A fixed set of host threads that run the pieces of one job at a time
// (start: tasks 0 .. count-1 claimed in order; wait: until every piece ran).
class CopyPool {
public:
    explicit CopyPool(int n)
    {
        for (int i = 0; i < n; ++i) threads_.emplace_back([this] { loop(); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    int size() const { return (int)threads_.size(); }
    void start(size_t count, std::function<void(size_t)> task)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            task_ = std::move(task);
            count_ = count;
            next_.store(0);
            active_ = threads_.size();
            ++gen_;
        }
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return active_ == 0; });
    }

private:
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            const size_t count = count_;
            lk.unlock();
            for (size_t i; (i = next_.fetch_add(1)) < count;) task_(i);
            lk.lock();
            if (--active_ == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::function<void(size_t)> task_;
    size_t count_ = 0, active_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// A launch layout of a region grid: launch slot -> region and list
// (SlotDesc, device), region -> slot (k_prep's binning), and the host copy of
// slot -> region (row-major over the strip).
struct SlotLayout {
    Owned<SlotDesc> d_desc;
    Owned<uint32_t> d_rank;
    std::vector<uint32_t> slot_region;
    uint32_t rx = 0, ry = 0, cap = 0;  // the fixed-capacity layout's key
};

// A frame between its preparation (enqueued) and its render launch.  Split so
// that a multi-device render can enqueue every device's preparation before it
// waits for any (xrt_render_rows_multi).
struct PendingFrame {
    FrameSet* fs = nullptr;
    // the frame renders the current geometry (bin_key) over its compact
    // layout and fill plan: its records can give the tile plan
    bool plan_source = false;
    bool hit_plan_ok = false;          // hit layout: the context's hit plan is this frame's geometry's
    hipStream_t stream = nullptr;
    hipEvent_t prep_done = nullptr;    // k_prep complete (prep stream)
    // The host waits for prep_done and reads k_prep's check before the launch
    // (a sizing frame, a frame with the check armed); otherwise the render's
    // queue waits for prep_done on the device and the host runs ahead.
    bool host_wait = false;
    bool ahead = false;                // prepared ahead of its call (xrt_context::ahead)
    int kernel = XRT_KERNEL_AUTO;
    bool binned = false;
    uint32_t rows = 0, rx = 0, ry = 0;
    dim3 grid;
    RenderParams p;
    Outputs out;
    BinBuffers bins = {};
    BinState* bin_ctl = nullptr;
    HostClock::time_point t_call;
};

#include "xrt_plan_host.inc"           // (here: the context carries its GeometryState)

struct xrt_context {
    int device = 0;
    std::string error;

    Owned<float> d_tris;           // raw triangle soup, 9 f32 per triangle
    uint64_t num_tris = 0;
    FrameSet sets[kFrameSets];
    int next_set = 0;
    FrameSet* last_set = nullptr;      // set of the last enqueued frame
    hipStream_t prep_stream = nullptr;    // the device's, shared with its other contexts (acquire_streams)
    bool owns_streams = false;         // holds a reference to them
    size_t prep_lds = 0;               // dynamic LDS of a k_prep launch (kPrepLds in all)

    // Launch layouts of the region grid (SlotLayout): the fixed-capacity one
    // the first frame of a geometry bins into (centre-first order), and the
    // compact one sized from its counts (the fill plan's order when there is
    // a plan).
    SlotLayout fixed;
    SlotLayout compact_layout;
    uint64_t slot_pool = 0;            // entries of the compact lists
    uint64_t motion_pool = 0;          // entries of a device-sized (moving camera) frame's lists
    uint64_t motion_pool_forced = 0;   // test hook XRT_MOTION_POOL: that many entries, never grown
    bool device_fill = true;           // moving frames render over the device fill plan (XRT_DEVICE_FILL=0: off)
    bool device_first = true;          // a geometry's first frame sized on the device (XRT_DEVICE_FIRST=0: off)
    // Box tile masks (BinBuffers::box_masks; XRT_BOX_MASKS): 0 (default)
    // never, 1 in the host-sized frames of meshes under kPrepBigMesh
    // triangles, 2 in every binned frame.  Exact either way; measured a wash
    // (DESIGN.md "Box tile masks"): the renders' dispatches shrink, k_prep's
    // grow by about as much, and the step does not move beyond box-to-box noise.
    int box_masks = 0;
    size_t bin_force_cap = 0;          // test hook (xrt_set_bin_capacity)
    // Fill plan of the current geometry (bin_key): the compact layout's
    // slots [plan_tile_slots, regions) are the regions its sizing frame
    // counted empty, one workgroup each (DESIGN.md "Fill plan").  fill_plan:
    // 1 on (xrt_set_fill_plan 0 turns it off); 2 plans EVERY region as empty
    // (tests of the exact fallback).
    int fill_plan = 1;
    uint32_t plan_tile_slots = 0;
    // the plan's heaviest regions render each tile with two waves (BinBuffers::
    // split_slots): the leading tile slots whose candidate count is at least
    // split_min (XRT_SPLIT_MIN; 0 = never)
    uint32_t plan_split_slots = 0;
    uint32_t split_min = kSplitAuto;   // kSplitAuto: the rule above
    uint32_t wave_slots = 0;           // the device's CUs x 32 (render waves resident at full occupancy)
    bool plan_valid = false;
    // Tile plan (SlotDesc::live): 0 = the compact layout's tiles all live (as
    // uploaded), 1 = k_tile_plan ran after a render of the current geometry
    // (bin_key) with its fill plan.  Off by default: it reuses an earlier
    // frame's cull results, so it helps only a loop of identical frames
    // (XRT_TILE_PLAN=1 or xrt_debug_set_tile_plan turn it on).
    bool tile_plan_enabled = false;
    // xrt_debug_prep_times: k_prep's per-wave timestamps of the last launch
    bool prep_times_on = false;
    Owned<uint4> d_prep_times;
    size_t prep_times_n = 0;
    int tile_plan_state = 0;
    uint64_t hp_tile_plan_frames = 0, hp_tile_plans = 0;
    uint32_t last_fill_regions = 0;    // regions the last enqueued frame filled (diagnostics)
    uint64_t packed_cap = 0;           // xrt_set_transit_layout: the packed L-buffer's floats (0: row-major)

    // staging for the host-pointer entry point
    Owned<float> d_image;
    Owned<float> d_lbuffer;
    Owned<uint8_t> d_u8;
    // The host-buffer entry points run on this context-owned non-blocking
    // stream (never the null stream, whose legacy semantics order it against
    // every blocking stream of the device), and copy back through the pinned
    // ring h_stage (kStageSlots x kStageChunk) with the copy threads of `pool`.
    hipStream_t host_stream = nullptr;
    Pinned<uint8_t> h_stage;
    PlainEvent stage_ev[kStageSlots];
    Pinned<uint8_t> h_sizing;          // pinned scratch of the sizing path (kSizingScratch, grown on demand)
    Fence sizing_done;                 // the last upload from h_sizing (prep stream)
    PlainEvent host_render_done;
    std::unique_ptr<CopyPool> pool;
    // the preparation stream holds work that reads a launch layout (k_prep)
    // since it was last synchronised (upload_layout needs it idle)
    bool prep_reads_layout = false;
    // XRT_SIZING_PROFILE=1: a new geometry's preparation step by step, each
    // step synchronised and timed on the host (stderr) -- diagnostics only
    int sizing_profile = 0;
    HostClock::time_point prof_t{};

    TimedEvent ev_begin, ev_end;
    // xrt_read_stats: the last render's records summed on the device
    // (k_reduce_stats) into one record, read through pinned memory
    Owned<StatsSum> d_stats_partial;       // [kReduceMaxBlocks]
    Owned<unsigned int> d_stats_done;      // the last-block counter (reset by that block)
    Owned<StatsSum> d_stats_out;
    Pinned<StatsSum> h_stats;
    // host time of the last host-buffer call (xrt_render_rows), ms:
    // [0] device planes, [1] enqueue (preparation, sizing, launch), [2] wait for
    // the render, [3] D2H of the planes (DMA into the pinned ring overlapped with
    // the copy threads), [4] copy threads, [5] MB copied, [6] statistics,
    // [7] total; within them: [8] every hipMalloc of the call, [9] a new
    // geometry's list sizing (count read-back, layout upload), [10] the
    // synchronisations before a launch layout's upload -- [13] of them the prep
    // stream's, [14] the sets' render events', [15] the last stream's --,
    // [11] host waits for k_prep, [12] kernel launches (k_prep and render)
    double host_call_ms[kHostCallFields] = {};
    double acc_ms[kAccFields] = {};                  // running sums of [8..15]
    // region timing (xrt_timing_begin/end)
    bool timing = false;
    std::vector<TimedEvent> tev;      // pairs: [2i] start, [2i+1] stop of a sampled render dispatch
    size_t tev_used = 0;
    uint64_t timed_frames = 0;        // frames enqueued since xrt_timing_begin
    size_t timed_records = 0;         // their timing records kept
    size_t timing_space = 0;          // records the region's chunk holds (xrt_timing_begin)
    // the sampled frames' timing records: chunks of device memory (a chunk is
    // never moved while kernels may write it), and where each frame's are
    struct TimesChunk {
        Owned<uint2> p;
        size_t used = 0;
    };
    std::vector<TimesChunk> tchunks;
    struct TimesSample {              // a frame's records: where they are (chunks never move) and how many
        const uint2* p;
        size_t n;
    };
    std::vector<TimesSample> tsamples;
    double event_ms = 0.0;            // the last timed region's HIP-event samples
    uint64_t event_launches = 0;
    hipStream_t last_stream = nullptr;
    bool pending = false;
    int kernel = XRT_KERNEL_AUTO;
    uint64_t mesh_gen = 0;             // bumped by every upload
    using BinKey = ::BinKey;
    GeometryState geo;                 // the geometry the region lists were sized for (choose_list_mode)
    bool reuse_cameras = true;         // false for xrt_render_rows_multi's contexts
    // Hit transit (xrt_set_transit_hits): the message buffer's capacity in
    // 32-bit words (0: off), and the hit plan of geometry hit_key
    // (xrt_plan_hit_layout): per tile of its fill plan the exclusive scan of
    // the tiles' hit counts, n_tiles + 1 entries on the device.
    uint64_t hits_cap = 0;
    bool hit_valid = false;
    BinKey hit_key = {};
    uint32_t hit_tiles = 0;
    uint64_t hit_words = 0;
    Owned<uint32_t> d_hit_off;
    // Prepare-ahead (DESIGN.md "Pipelining"): when a device-pointer render
    // repeats the previous call's frame geometry, the preparations of the next
    // kAheadFrames frames of that geometry are enqueued at once on the prep
    // stream; a later call whose geometry and settings match takes the oldest
    // (its k_prep then ran beside earlier renders and is complete: the render
    // is launched with no wait at all).  Any mismatch drops them (their k_prep
    // runs, on the prep stream, before any newer one).  state_gen counts the
    // setting changes a prepared frame depends on.
    struct AheadFrame {
        PendingFrame pf;
        BinKey key;
        uint64_t state_gen;
        uint32_t outs;                 // which output planes (image 1, L-buffer 2, u8 4)
    };
    std::deque<AheadFrame> ahead;
    uint64_t state_gen = 0;
    BinKey call_key = {};              // the last device-pointer call's geometry
    uint64_t call_state_gen = ~0ull;
    uint64_t hp_ahead_used = 0, hp_ahead_dropped = 0, hp_launch_nowait = 0, hp_host_waits = 0;
    uint64_t hp_dev_first = 0, hp_dev_first_recounts = 0;   // first frames sized on the device; pools regrown
    uint64_t dev_first_pairs = 0, dev_first_pool = 0;       // the last one's pair total and first pool
    uint32_t miss_code = 0;            // L-buffer bits of a miss (0: +inf; xrt_set_miss_code)
    uint32_t model = kModelAttenuation;   // xrt_set_model
    float mu = 0.1037f;                // kModelSigned: mesh 0's attenuation coefficient
    // The scene (xrt_upload_scene; xrt_upload_mesh uploads one mesh): mesh m
    // holds mesh_tris[m] of d_tris' num_tris triangles, one after another.
    std::vector<uint64_t> mesh_tris;
    // kModelMaterials (xrt_set_materials): one coefficient per mesh, and the
    // device table of the scene's id ranges with them (upload_materials)
    std::vector<float> materials_mu;
    Owned<MeshMaterial> d_materials;
    // kModelSpectrum (xrt_set_spectrum): the bins' weights, the coefficients
    // (mesh-major, spectrum_meshes x weights.size()) and their device table
    // (upload_spectrum)
    std::vector<float> spectrum_weight, spectrum_mu;
    uint32_t spectrum_meshes = 0;
    Owned<SpectrumTable> d_spectrum;
    // kModelPaths (xrt_set_paths): the scene's id-range ends, kMaxMeshes words,
    // kept with every scene upload (upload_path_ends)
    Owned<uint32_t> d_path_ends;
    xrt_camera cull_cam = {};          // camera of the cached cull parameters
    CullParams cull = {};
    bool cull_valid = false;
    int last_kernel = XRT_KERNEL_BINNED;
    uint32_t hit_capacity = kMaxHits;
    // XRT_HOST_PROFILE=1: host time per enqueue, split by wait (printed at destroy)
    bool host_profile = false;
    double hp_total = 0, hp_done = 0, hp_prep = 0, hp_lprep = 0, hp_lrender = 0, hp_gap = 0;
    uint64_t hp_calls = 0;
    uint64_t hp_sizings = 0, hp_reused = 0, hp_plan_miss = 0, hp_overflow = 0;   // frames by geometry path
    HostClock::time_point hp_last_end{};

    // Mesh poses (xrt_set_pose): d_tris stays the rest soup.
    // `poses` is empty while every mesh is at the identity: no posed soup, no
    // kernel, every reader takes d_tris (render_soup).  Otherwise it holds one
    // pose per mesh, readers take d_tris_posed, and `posed_written` the pose
    // each mesh's range of it was last written with (empty: never written
    // since the upload): the next render's k_pose rewrites the meshes that
    // differ, on the prep stream ahead of its k_prep.
    using Pose = std::array<float, kPoseFloats>;
    Owned<float> d_tris_posed;
    std::vector<Pose> poses;
    std::vector<Pose> posed_written;
    uint64_t pose_gen = 0;             // bumped by every pose change
    uint64_t hp_pose_launches = 0, hp_pose_tris = 0;   // k_pose launches and the triangles they wrote

    // The voxel volume (xrt_upload_volume): apart from the
    // meshes, the model and the frames.  vol.labels is null while there is
    // none; it and vol.density point into vol_labels and vol_density.
    // vol_traced marks the last trace enqueued (on the caller's stream): the
    // next upload waits for it before it frees the arrays.
    VolumeDesc vol = {};
    Owned<uint8_t> vol_labels;
    Owned<float> vol_density;
    Fence vol_traced;
    uint32_t vol_tile_shift = kVolumeTileShift;        // xrt_debug_volume_wave_shape

    // The working set of xrt_sirt[_device]: one allocation
    // holding the gathered matrices (A then R, f64), the residual planes of
    // the largest subset, the correction volume and the norm volumes -- with
    // TV also the sums' partials and x0; xrt_volume_sumsq and
    // xrt_tv_descend lay their partials and gradient volume in it --, kept
    // between calls.  sirt_mats is the upload's source (it must outlive the
    // copy); sirt_done marks the last call's end on its stream: the next call
    // waits for it before it touches either.
    Owned<uint8_t> d_sirt;
    std::vector<double> sirt_mats;
    Fence sirt_done;

    // The voxeliser (xrt_voxelize[_device]) lays its control
    // words, queue and flip volume in that working set.  vox_scattered marks the
    // last scatter enqueued on the caller's stream, the soup's only reader
    // there: sync_context waits for it, so an upload or a pose change does not
    // replace the soup under it.  vox_counters: the set still holds the last
    // call's control words (xrt_debug_voxelize_counters), laid there by
    // work on vox_stream: a next voxelisation on that stream is ordered
    // behind it by the stream and need not wait for the set on the host.
    Fence vox_scattered;
    PlainEvent vox_pose_ev;
    hipStream_t vox_stream = nullptr;
    bool vox_counters = false;
    uint32_t vox_threshold = kVoxelQueueColumns;       // xrt_debug_voxelize_threshold
    uint32_t vox_stages = 7u;                          // xrt_debug_voxelize_stages: 1 scatter, 2 scan, 4 clear, 8 the scan in one run

    // Ray table (DESIGN.md "Ray table"): the ray directions of one camera and
    // strip, filled by k_ray_table on the prep stream when an attenuation
    // BINNED frame repeats the previous one's RayKey, and read by
    // k_render_binned_rays in place of make_ray_from while the key stays.  The
    // rays depend on nothing else: the mesh, the poses and the lists may change
    // under a valid table.
    struct RayKey {
        float cam[13];                 // RenderParams' camera floats
        uint32_t width, height, row_begin, row_end;
        bool same(const RayKey& o) const   // field by field, the floats by bits
        {
            return std::memcmp(cam, o.cam, sizeof cam) == 0 && width == o.width && height == o.height &&
                   row_begin == o.row_begin && row_end == o.row_end;
        }
    };
    Owned<float> d_rays;
    RayKey ray_key = {};               // the table's, while ray_valid
    bool ray_valid = false;            // a fill for ray_key is enqueued (or complete)
    Fence ray_filled;                  // that fill's end (prep stream); once it has passed, readers need no wait
    std::vector<hipStream_t> ray_waited;   // the streams already ordered after the fill
    RayKey ray_call_key = {};          // the previous eligible frame's key
    bool ray_call_valid = false;
    bool ray_enabled = true;           // xrt_debug_set_ray_table
    size_t ray_budget = (size_t)256 << 20;   // XRT_RAY_CACHE_MB (0: no table)
    uint64_t hp_ray_fills = 0, hp_ray_frames = 0, hp_ray_computed = 0;
};

inline double seconds_since(HostClock::time_point t)
{
    return std::chrono::duration<double>(HostClock::now() - t).count();
}

// XRT_SIZING_PROFILE: synchronise the prep stream and print the time since the
// last mark (the step's enqueue + execution).
void prof_mark(xrt_context* ctx, const char* what)
{
    if (!ctx->sizing_profile) return;
    const auto t_enq = HostClock::now();
    // XRT_SIZING_PROFILE=2: host time per step only, no synchronisation
    const hipError_t e = ctx->sizing_profile == 2 ? hipSuccess : hipStreamSynchronize(ctx->prep_stream);
    const auto now = HostClock::now();
    std::fprintf(stderr, "xrt sizing profile: %-34s %9.3f ms (of which sync %8.3f ms)%s\n", what,
                 std::chrono::duration<double, std::milli>(now - ctx->prof_t).count(),
                 std::chrono::duration<double, std::milli>(now - t_enq).count(), e == hipSuccess ? "" : " ERROR");
    ctx->prof_t = HostClock::now();
}

// No static object of libxrt has a destructor: process exit runs the shared
// libraries' finalizers (__cxa_finalize) in an order libxrt does not control,
// the HIP runtime's among them, and contexts a caller leaks (RayTracer.cpp's
// per-device slots) are reclaimed by the process's end, not torn down.  The
// error strings of a failed create are heap objects that are never freed.
static std::string& g_create_error = *new std::string();
// xrt_destroy's phases, ms (xrt_debug_destroy_ms): [0] waiting for the
// context's work, [1] device frees, [2] pinned host frees, [3] streams and events
static double g_destroy_ms[4] = {};

// The prep and host streams are shared by every context of one device in the
// process (reference-counted; the last context's destroy destroys them).  A
// process gets GPU_MAX_HW_QUEUES hardware queues (4 by default) and HIP shares
// one between streams past that: a second context with streams of its own
// beside a caller's two render streams put its prep stream on a render
// stream's queue, where a frame's k_prep waits for the render queued before it
// and the next render for that k_prep -- preparation and render serialised
// (2048^2: 32 -> 58 us a still frame, 51 -> 69 us a moving one; DESIGN.md
// "Moving camera").  Shared, contexts add no queue: their k_preps serialise on
// the device's prep stream, which they would on one queue anyway.
struct DeviceStreams {
    hipStream_t prep = nullptr, host = nullptr;
    int refs = 0;
};
static std::mutex& g_streams_mu = *new std::mutex();
static std::vector<DeviceStreams>& g_streams = *new std::vector<DeviceStreams>();

bool acquire_streams(int device, hipStream_t& prep, hipStream_t& host)
{
    std::lock_guard<std::mutex> lock(g_streams_mu);
    if ((size_t)device >= g_streams.size()) g_streams.resize((size_t)device + 1);
    DeviceStreams& d = g_streams[(size_t)device];
    if (d.refs == 0) {
        if (hipStreamCreateWithFlags(&d.prep, hipStreamNonBlocking) != hipSuccess) return false;
        if (hipStreamCreateWithFlags(&d.host, hipStreamNonBlocking) != hipSuccess) {
            (void)hipStreamDestroy(d.prep);
            d.prep = nullptr;
            return false;
        }
    }
    ++d.refs;
    prep = d.prep;
    host = d.host;
    return true;
}

void release_streams(int device)
{
    std::lock_guard<std::mutex> lock(g_streams_mu);
    DeviceStreams& d = g_streams[(size_t)device];
    if (--d.refs == 0) {
        (void)hipStreamDestroy(d.prep);
        (void)hipStreamDestroy(d.host);
        d.prep = d.host = nullptr;
    }
}

// AUTO switches from TILED to BINNED past this many footprint-box tests
// (T x regions) per frame (DESIGN.md "Kernels").
constexpr uint64_t kAutoSweep = 20000000ull;

namespace {

int fail(xrt_context* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->error = msg;
    else g_create_error = msg;
    return code;
}

#define XRT_HIP(ctx, expr)                                                                    \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail((ctx), XRT_ERR_DEVICE,                                                \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                   \
    } while (0)

// buf holds at least need_elems (Owned::reserve); a HIP error goes to ctx->error,
// the allocation's time to acc_ms[0] (host_call_ms[8]).
template <typename T, typename Mem>
int ensure(xrt_context* ctx, Owned<T, Mem>& buf, size_t need_elems)
{
    if (need_elems <= buf.cap() && buf) return XRT_OK;
    buf.reset();                                   // (reserve's own test and free, here to keep the free out of the timed hipMalloc)
    const auto t = HostClock::now();
    XRT_HIP(ctx, buf.reserve(need_elems));
    if (ctx) ctx->acc_ms[0] += std::chrono::duration<double, std::milli>(HostClock::now() - t).count();
    return XRT_OK;
}

// The pinned sizing scratch, at least `bytes`, once no upload from it is still
// in flight (its last upload's event, long complete as a rule).
int sizing_scratch(xrt_context* ctx, size_t bytes, uint8_t*& out)
{
    XRT_HIP(ctx, ctx->sizing_done.wait());
    XRT_HIP(ctx, ctx->h_sizing.reserve(bytes));
    out = ctx->h_sizing.get();
    return XRT_OK;
}

// Waits for this context's own work: its preparations (prep stream), every
// render still marked in flight (the sets' completion events) and the last
// enqueue's stream (a statistics reduction behind the render).  Not the whole
// device: other contexts' and the caller's unrelated work are not this
// context's to wait for (a device-wide synchronise measured 21 ms once, in a
// process whose device was otherwise idle).
int sync_context(xrt_context* ctx)
{
    auto t = HostClock::now();
    auto lap = [&](int k) {
        const auto now = HostClock::now();
        ctx->acc_ms[k] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    };
    XRT_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    ctx->prep_reads_layout = false;
    lap(5);
    for (FrameSet& fs : ctx->sets)
        if (fs.done_valid) XRT_HIP(ctx, hipEventSynchronize(fs.done_ev));
    lap(6);
    if (ctx->pending) XRT_HIP(ctx, hipStreamSynchronize(ctx->last_stream));
    XRT_HIP(ctx, ctx->vox_scattered.wait());          // a scatter of xrt_voxelize_device reads the soup
    lap(7);
    return XRT_OK;
}

// True when a render or preparation of this context may still read its launch
// layouts (upload_layout must not overwrite them under it).
bool layouts_in_use(const xrt_context* ctx)
{
    if (ctx->prep_reads_layout || ctx->pending) return true;
    for (const FrameSet& fs : ctx->sets)
        if (fs.done_valid) return true;
    return false;
}

// The reference's stdmin / stdmax semantics (std::min(a,b) = b<a ? b : a).
inline float stdmin(float a, float b) { return (b < a) ? b : a; }
inline float stdmax(float a, float b) { return (a < b) ? b : a; }

inline void cross3(const float a[3], const float b[3], float o[3])
{
    float x = a[1] * b[2] - a[2] * b[1];
    float y = a[2] * b[0] - a[0] * b[2];
    float z = a[0] * b[1] - a[1] * b[0];
    o[0] = x;
    o[1] = y;
    o[2] = z;
}

inline float length3(const float a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

inline void normalise3(float a[3])
{
    float len = length3(a);
    a[0] /= len;
    a[1] /= len;
    a[2] /= len;
}

// The triangles the current model renders: the first of d_tris.  The
// attenuation and the signed model see mesh 0 only (src/main.cxx:687,
// main-pthreads-lbuffer.cxx:788), the materials model every mesh.
inline uint64_t render_tris(const xrt_context* ctx)
{
    if (ctx->model == kModelMaterials || ctx->model == kModelSpectrum || ctx->model == kModelPaths ||
        ctx->mesh_tris.empty())
        return ctx->num_tris;
    return ctx->mesh_tris[0];
}

// The identity pose, bit for bit (+0.0 zeros).
constexpr xrt_context::Pose kIdentityPose = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};

inline bool same_pose(const xrt_context::Pose& a, const xrt_context::Pose& b)
{
    return std::memcmp(a.data(), b.data(), sizeof(xrt_context::Pose)) == 0;
}

// Names the content of the soup the renders read: both counters only grow.
inline uint64_t soup_gen(const xrt_context* ctx) { return ctx->mesh_gen + ctx->pose_gen; }

// The soup a preparation reads (k_prep is the soup's only reader on the device:
// the renders and their fix-up walks read k_prep's records): d_tris while
// every pose is the identity, otherwise d_tris_posed -- after the k_pose
// launches, enqueued here on the prep stream, that rewrite the id ranges of
// the meshes whose pose differs from the one their range was last written
// with.  A run of such meshes is one launch (kPoseLaunchTris triangles at
// most).  Nothing on the device reads the posed soup while they are enqueued:
// poses change only in xrt_set_pose / xrt_reset_poses and the uploads, which
// wait for the context's work, and every reader is enqueued behind this on
// the prep stream.  The host does not wait.
int render_soup(xrt_context* ctx, const float*& soup)
{
    soup = ctx->d_tris.get();
    if (ctx->poses.empty()) return XRT_OK;
    const size_t M = ctx->mesh_tris.size();
    if (!ctx->d_tris_posed || ctx->d_tris_posed.cap() < 9 * ctx->num_tris) ctx->posed_written.clear();
    int rc = ensure(ctx, ctx->d_tris_posed, 9 * ctx->num_tris);
    if (rc) return rc;
    soup = ctx->d_tris_posed.get();
    const bool all = ctx->posed_written.size() != M;
    PoseTable tab;
    std::memset(&tab, 0, sizeof tab);
    uint64_t end = 0;
    bool due = false;
    for (size_t m = 0; m < kMaxMeshes; ++m) {
        if (m < M) {
            end += ctx->mesh_tris[m];
            std::memcpy(tab.pose[m], ctx->poses[m].data(), sizeof tab.pose[m]);
            if (same_pose(ctx->poses[m], kIdentityPose)) tab.identity |= 1u << m;
            due = due || all || !same_pose(ctx->poses[m], ctx->posed_written[m]);
        }
        tab.end[m] = m < M ? (uint32_t)end : 0xFFFFFFFFu;
    }
    if (!due) return XRT_OK;
    uint64_t first = 0;                            // of the run of meshes to write
    for (size_t m = 0; m < M;) {
        if (!all && same_pose(ctx->poses[m], ctx->posed_written[m])) {
            first = tab.end[m++];
            continue;
        }
        size_t last = m;
        while (last + 1 < M && (all || !same_pose(ctx->poses[last + 1], ctx->posed_written[last + 1]))) ++last;
        for (uint64_t t = first; t < tab.end[last]; t += kPoseLaunchTris) {
            const uint64_t n = std::min<uint64_t>(kPoseLaunchTris, tab.end[last] - t);
            hipLaunchKernelGGL(k_pose, dim3((unsigned)((3 * n + kPoseThreads - 1) / kPoseThreads)),
                               dim3(kPoseThreads), 0, ctx->prep_stream, ctx->d_tris.get() + 9 * t,
                               ctx->d_tris_posed.get() + 9 * t, (uint32_t)t, (uint32_t)(3 * n), tab);
            XRT_HIP(ctx, hipGetLastError());
            ++ctx->hp_pose_launches;
            ctx->hp_pose_tris += n;
        }
        first = tab.end[last];
        m = last + 1;
    }
    ctx->posed_written = ctx->poses;
    return XRT_OK;
}

#include "xrt_cull_host.inc"

int check_camera(xrt_context* ctx, const xrt_camera* cam, uint32_t row_begin, uint32_t row_end)
{
    if (!cam) return fail(ctx, XRT_ERR_ARGUMENT, "camera is NULL");
    if (cam->width == 0 || cam->height == 0)
        return fail(ctx, XRT_ERR_ARGUMENT, "image size must be non-zero");
    if (row_begin > row_end || row_end > cam->height)
        return fail(ctx, XRT_ERR_ARGUMENT,
                    "row range [" + std::to_string(row_begin) + ", " + std::to_string(row_end) +
                        ") outside image height " + std::to_string(cam->height));
    if ((uint64_t)cam->width * cam->height > (1ull << 32) - 1)
        return fail(ctx, XRT_ERR_ARGUMENT, "image larger than 2^32-1 pixels");
    return XRT_OK;
}

xrt_context::BinKey geometry_key(const xrt_context* ctx, const xrt_camera* cam, uint32_t row_begin,
                                 uint32_t row_end)
{
    xrt_context::BinKey key = {};
    key.cam = *cam;
    key.row_begin = row_begin;
    key.row_end = row_end;
    key.T = render_tris(ctx);
    key.gen = ctx->mesh_gen;
    key.pose_gen = ctx->pose_gen;
    return key;
}

inline uint32_t frame_regions(const PendingFrame& pf) { return pf.rows ? pf.rx * pf.ry : 0u; }

// k_prep: one thread per triangle, and at least one per image row and column
// (the pixel-offset tables).
int launch_prep(xrt_context* ctx, PendingFrame& pf)
{
    FrameSet& fs = *pf.fs;
    const RenderParams& p = pf.p;
    const BinBuffers& bins = pf.bins;
    const bool culled = pf.kernel != XRT_KERNEL_BRUTE;
    const uint64_t T = render_tris(ctx);
    // p.prep_tris triangles per wave; every thread covers a pixel-offset entry / counter
    const uint64_t threads = std::max<uint64_t>((uint64_t)p.height + p.width, bins.clear ? bins.clear_regions : 0u);
    const uint64_t per_block = (uint64_t)kPrepWaves * p.prep_tris;
    const uint64_t blocks = std::max<uint64_t>((T + per_block - 1) / per_block,
                                               (threads + kPrepThreads - 1) / kPrepThreads);
    uint4* ptimes = nullptr;                       // xrt_debug_prep_times
    if (ctx->prep_times_on) {
        int rc = ensure(ctx, ctx->d_prep_times, 2 * (size_t)blocks * kPrepWaves);
        if (rc) return rc;
        ptimes = ctx->d_prep_times.get();
        ctx->prep_times_n = (size_t)blocks * kPrepWaves;
    }
    const float* soup = nullptr;                   // (k_pose first when a pose changed, on the prep stream too)
    if (int rc = render_soup(ctx, soup)) return rc;
    const auto t_launch = HostClock::now();
    hipExtLaunchKernelGGL(k_prep, dim3((unsigned)blocks), dim3(kPrepThreads),
                          ctx->prep_lds, ctx->prep_stream, nullptr, pf.prep_done, 0u,
                          soup, (uint32_t)T, p, ctx->cull, fs.recs.get(), culled ? fs.cull.get() : nullptr, bins, pf.bin_ctl,
                          fs.frame.get(), fs.offsets.get(), ptimes);
    XRT_HIP(ctx, hipGetLastError());
    if (bins.counts) ctx->prep_reads_layout = true;
    ctx->acc_ms[4] += std::chrono::duration<double, std::milli>(HostClock::now() - t_launch).count();
    if (ctx->host_profile) ctx->hp_lprep += seconds_since(t_launch);
    return XRT_OK;
}

// Region buffers of a binned frame.  The frame counts into one half of the
// set's counters (FrameSet::bin_counts); k_prep clears the other half.  A half
// is cleared here, on the prep stream, only when it is not known clean for
// this many regions (the first frames, a larger region grid, a re-run).  The
// caller sets the launch layout (bins.desc / bins.rank).
int bin_buffers(xrt_context* ctx, PendingFrame& pf, uint64_t list_entries, bool rerun = false)
{
    FrameSet& fs = *pf.fs;
    BinBuffers& bins = pf.bins;
    const uint32_t n_regions = frame_regions(pf);
    const uint64_t T = render_tris(ctx);
    static_assert(sizeof(BinState) <= kCounterStride * sizeof(uint32_t), "BinState fits its line");
    int rc;
    // per half: control block padded to a line, then one line-padded counter per region
    const size_t half_words = kCounterStride + (size_t)kCounterStride * n_regions;
    if (!fs.bin_counts.get() || fs.bin_half_words < half_words) {
        if ((rc = ensure(ctx, fs.bin_counts, 2 * half_words))) return rc;
        fs.bin_half_words = half_words;
        fs.dirty[0] = fs.dirty[1] = kDirtyAll;
    }
    if ((rc = ensure(ctx, fs.bin_list, (size_t)list_entries))) return rc;
    if ((rc = ensure(ctx, fs.global_list, T))) return rc;
    const uint32_t q = rerun ? fs.half : fs.half ^ 1u;     // a re-run recounts into the same half
    uint32_t* mine = fs.bin_counts.get() + (size_t)q * fs.bin_half_words;
    uint32_t* other = fs.bin_counts.get() + (size_t)(q ^ 1u) * fs.bin_half_words;
    if (rerun || fs.dirty[q] != 0u)                         // (on k_prep's stream: it must not overtake it)
        XRT_HIP(ctx, hipMemsetAsync(mine, 0, half_words * sizeof(uint32_t), ctx->prep_stream));
    fs.half = q;
    fs.dirty[q] = n_regions;                                // this frame counts into it
    // k_prep clears the other half: its control block and its dirty counters
    const uint32_t alloc_regions = (uint32_t)((fs.bin_half_words - kCounterStride) / kCounterStride);
    bins.clear = other + kCounterStride;
    bins.clear_regions = fs.dirty[q ^ 1u] == kDirtyAll ? alloc_regions : fs.dirty[q ^ 1u];
    fs.dirty[q ^ 1u] = 0u;
    pf.bin_ctl = reinterpret_cast<BinState*>(mine);
    fs.last_state = pf.bin_ctl;
    bins.counts = mine + kCounterStride;
    bins.list = fs.bin_list.get();
    bins.global_list = fs.global_list.get();
    return XRT_OK;
}

// Uploads a launch layout: slot s renders region slot_region[s] from
// list[base[s] .. base[s] + cap[s]).  Frames in flight may read the previous
// one, so the device is synchronised first.
int upload_layout(xrt_context* ctx, SlotLayout& L, uint32_t rx, uint32_t ry, std::vector<uint32_t> slot_region,
                  const std::vector<uint32_t>& base, const std::vector<uint32_t>& cap)
{
    const size_t n = slot_region.size();
    std::vector<SlotDesc> desc(n);
    std::vector<uint32_t> rank(n);
    for (size_t s = 0; s < n; ++s) {
        const uint32_t r = slot_region[s];
        desc[s] = SlotDesc{base[s], cap[s], (r % rx) | ((r / rx) << 16), 0xFFFFu};   // every tile live
        rank[r] = (uint32_t)s;
    }
    // Frames in flight may read the old layout: wait for them, but only when
    // there are any (a fresh context's first frame waits for nothing).
    int rc;
    if (layouts_in_use(ctx)) {
        const auto t_sync = HostClock::now();
        if ((rc = sync_context(ctx))) return rc;
        ctx->acc_ms[2] += std::chrono::duration<double, std::milli>(HostClock::now() - t_sync).count();
    }
    if ((rc = ensure(ctx, L.d_desc, n))) return rc;
    if ((rc = ensure(ctx, L.d_rank, n))) return rc;
    // from the pinned scratch, on the prep stream, in order before the k_prep
    // that reads them
    uint8_t* h = nullptr;
    if ((rc = sizing_scratch(ctx, n * (sizeof(SlotDesc) + sizeof(uint32_t)), h))) return rc;
    std::memcpy(h, desc.data(), n * sizeof(SlotDesc));
    std::memcpy(h + n * sizeof(SlotDesc), rank.data(), n * sizeof(uint32_t));
    XRT_HIP(ctx, hipMemcpyAsync(L.d_desc.get(), h, n * sizeof(SlotDesc), hipMemcpyHostToDevice, ctx->prep_stream));
    XRT_HIP(ctx, hipMemcpyAsync(L.d_rank.get(), h + n * sizeof(SlotDesc), n * sizeof(uint32_t), hipMemcpyHostToDevice,
                                ctx->prep_stream));
    XRT_HIP(ctx, ctx->sizing_done.record(ctx->prep_stream));
    L.slot_region = std::move(slot_region);
    L.rx = rx;
    L.ry = ry;
    return XRT_OK;
}

// The fixed-capacity layout (centre-first order, `cap` entries per slot) of a
// region grid: the first frame of a geometry bins into it.
inline uint32_t fixed_region_cap(const xrt_context* ctx)
{
    return ctx->bin_force_cap ? (uint32_t)std::min<size_t>(kInitialRegionCap, ctx->bin_force_cap) : kInitialRegionCap;
}

int fixed_layout(xrt_context* ctx, PendingFrame& pf)
{
    const uint32_t rx = pf.rx, ry = pf.ry, cap = fixed_region_cap(ctx);
    SlotLayout& L = ctx->fixed;
    if (L.rx != rx || L.ry != ry || L.cap != cap || !L.d_desc.get()) {
        const size_t n = (size_t)rx * ry;
        std::vector<uint32_t> base(n), caps(n, cap);
        for (size_t s = 0; s < n; ++s) base[s] = (uint32_t)(s * cap);
        int rc = upload_layout(ctx, L, rx, ry, centre_first_order(rx, ry), base, caps);
        if (rc) return rc;
        L.cap = cap;
    }
    pf.bins.desc = L.d_desc.get();
    pf.bins.rank = L.d_rank.get();
    return XRT_OK;
}

// The current geometry's compact layout (its fill plan's order when there is
// a plan, DESIGN.md "Fill plan").  The signed model keeps the plan's order (the
// compact lists are sized by its slots) but renders every region as tiles.
void use_compact(xrt_context* ctx, uint32_t n_regions, BinBuffers& bins, bool fill)
{
    bins.desc = ctx->compact_layout.d_desc.get();
    bins.rank = ctx->compact_layout.d_rank.get();
    bins.tile_slots = fill && ctx->plan_valid ? ctx->plan_tile_slots : n_regions;
    bins.split_slots = fill && ctx->plan_valid && kCanSplit ? ctx->plan_split_slots : 0u;
}

// Arms the k_prep check of a frame whose fill plan k_prep's binning has not
// yet been seen to match: the first frame over a new plan (`validate`).
// The binning of a frame geometry (mesh, camera, strip) is deterministic --
// the same footprints join the same regions, only the order of a list's
// entries varies with the atomics -- so later frames of a validated geometry
// cannot miss it and are launched without the host reading the check
// (DESIGN.md "Pipelining").
void arm_plan_check(FrameSet& fs, uint32_t n_regions, BinBuffers& bins, bool validate)
{
    bins.plan_miss = nullptr;
    if (fs.plan_flag.get() && validate && bins.tile_slots < n_regions) {
        fs.plan_flag.get()[0] = 0u;
        fs.plan_flag.get()[1] = 0u;
        bins.plan_miss = const_cast<uint32_t*>(fs.plan_flag.get());
    }
}

// prepare_frame's stages, in its order; each fills its part of the
// PendingFrame.  First the arguments' checks and the kernel choice: pf's
// kernel, binned, rows and region grid.
int choose_kernel(xrt_context* ctx, const xrt_camera* cam, uint32_t row_begin, uint32_t row_end,
                  const float* d_image, const uint8_t* d_u8, PendingFrame& pf)
{
    int rc = check_camera(ctx, cam, row_begin, row_end);
    if (rc) return rc;
    if (!ctx->d_tris.get() && ctx->num_tris) return fail(ctx, XRT_ERR_NO_MESH, "no mesh uploaded");
    if (ctx->num_tris > 0xFFFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many triangles");
    XRT_HIP(ctx, hipSetDevice(ctx->device));

    const uint64_t T = render_tris(ctx);
    const uint32_t rows = row_end - row_begin;
    const uint32_t rx = (cam->width + kRegion - 1) / kRegion, ry = (rows + kRegion - 1) / kRegion;
    // AUTO: the per-region footprint sweep of TILED costs T x regions box
    // tests; past kAutoSweep of them binning once per frame is cheaper.
    const uint64_t sweep = T * (uint64_t)rx * ry;
    // (the signed and the materials model: one hit collection, L-buffer only)
    const bool signed_model = ctx->model != kModelAttenuation;
    if (ctx->model == kModelMaterials && ctx->materials_mu.size() != ctx->mesh_tris.size())
        return fail(ctx, XRT_ERR_ARGUMENT, "the scene's mesh count differs from xrt_set_materials'");
    if (ctx->model == kModelSpectrum && ctx->spectrum_meshes != ctx->mesh_tris.size())
        return fail(ctx, XRT_ERR_ARGUMENT, "the scene's mesh count differs from xrt_set_spectrum's");
    int kernel = ctx->kernel != XRT_KERNEL_AUTO ? ctx->kernel
                 : signed_model || sweep > kAutoSweep ? XRT_KERNEL_BINNED
                                                      : XRT_KERNEL_TILED;
    if (signed_model) {
        if (kernel == XRT_KERNEL_TILED)
            return fail(ctx, XRT_ERR_ARGUMENT, "the signed model renders with the BRUTE or BINNED kernel");
        // (the paths model's planes travel in d_lbuffer and d_u8: Outputs, xrt_render_paths_device)
        if (d_image || (d_u8 && ctx->model != kModelPaths))
            return fail(ctx, XRT_ERR_ARGUMENT,
                        "the signed model writes the L-buffer only (the image is xrt_hole_fill's)");
    }
    // k_prep packs a footprint's region rectangle in 16-bit fields: grids past
    // 65535 regions a side render TILED (exact, slower) -- BRUTE for the signed model.
    pf.binned = kernel == XRT_KERNEL_BINNED && rows > 0 && T > 0 && rx <= 0xFFFFu && ry <= 0xFFFFu;
    if (signed_model && !pf.binned) kernel = XRT_KERNEL_BRUTE;
    pf.kernel = kernel;
    pf.rows = rows;
    pf.rx = rx;
    pf.ry = ry;
    return XRT_OK;
}

// The frame's buffer set (pf.fs): the render that last used it (kFrameSets
// frames ago) must be complete before the set is prepared again.
int claim_set(xrt_context* ctx, const xrt_camera* cam, PendingFrame& pf)
{
    FrameSet& fs = *pf.fs;
    const uint64_t T = render_tris(ctx);
    int rc;
    if (fs.done_valid) {
        const auto t = HostClock::now();
        XRT_HIP(ctx, hipEventSynchronize(fs.done_ev));
        fs.done_valid = false;
        if (ctx->host_profile) ctx->hp_done += seconds_since(t);
    }
    if (fs.lazy_flags) {
        // the set's last frame was device-sized and launched without reading
        // k_prep's flags; its render is complete: a list past the pool there
        // (that region rendered from the whole mesh, exactly) grows the pool
        fs.lazy_flags = false;
        if (fs.plan_flag.get() && fs.plan_flag.get()[1] != 0u) {
            ++ctx->hp_overflow;
            ctx->motion_pool = std::min<uint64_t>(2 * ctx->motion_pool + 65536u, 0xFFFFFFFFull);
        }
    }
    if ((rc = ensure(ctx, fs.recs, T))) return rc;
    if (pf.kernel != XRT_KERNEL_BRUTE && (rc = ensure(ctx, fs.cull, (size_t)T * kCullPlanes))) return rc;
    return ensure(ctx, fs.offsets, (size_t)cam->height + cam->width);
}

// The render's Outputs (launch_frame adds the timing records and the rays).
int frame_outputs(xrt_context* ctx, const xrt_camera* cam, float* d_image, float* d_lbuffer, uint8_t* d_u8,
                  PendingFrame& pf)
{
    const FrameSet& fs = *pf.fs;
    Outputs& out = pf.out;
    out.image = d_image;
    out.lbuffer = d_lbuffer;
    out.image_u8 = d_u8;
    out.frame = (const __attribute__((address_space(4))) RenderParams*)fs.frame.get();
    out.off.v = fs.offsets.get();
    out.off.u = fs.offsets.get() + cam->height;
    const uint32_t miss_bits = ctx->miss_code ? ctx->miss_code : 0x7F800000u;   // +inf
    std::memcpy(&out.miss_l, &miss_bits, sizeof miss_bits);
    out.mu = ctx->mu;
    if (ctx->model == kModelSpectrum) {
        out.spectrum = (const __attribute__((address_space(4))) SpectrumTable*)ctx->d_spectrum.get();
        out.num_meshes = ctx->spectrum_meshes;
    } else if (ctx->model == kModelPaths) {
        out.path_ends = (const __attribute__((address_space(4))) uint32_t*)ctx->d_path_ends.get();
        out.num_meshes = (uint32_t)ctx->mesh_tris.size();
    } else {
        out.materials = (const __attribute__((address_space(4))) MeshMaterial*)ctx->d_materials.get();
        out.num_meshes = (uint32_t)ctx->materials_mu.size();
    }
    out.packed = 0u;
    out.wave_times = nullptr;          // launch_frame
    out.hit_tiles = 0u;
    out.hit_off = nullptr;
    out.rays = nullptr;                // launch_frame
    if (ctx->packed_cap || ctx->hits_cap) {        // xrt_set_transit_layout / _hits
        if (!pf.binned || ctx->model != kModelAttenuation || d_image || d_u8)
            return fail(ctx, XRT_ERR_ARGUMENT,
                        "the transit layouts are for BINNED attenuation renders of the L-buffer only");
        out.packed = ctx->hits_cap ? kLayoutHits : kLayoutPacked;
        out.hit_tiles = ctx->hit_tiles;
        out.hit_off = ctx->d_hit_off.get();
    }
    return XRT_OK;
}

// Lists already known (ListMode::Fixed, Compact) and a host-sized frame's
// count pass (no lists yet): the buffers, the layout, the tile-plan and
// box-mask bits and the plan check of the k_prep that follows.
int known_lists(xrt_context* ctx, PendingFrame& pf, ListMode mode)
{
    BinBuffers& bins = pf.bins;
    const uint32_t n_regions = frame_regions(pf);
    const bool fill_ok = pf.p.model == kModelAttenuation;
    const bool compact = mode == ListMode::Compact, counting = mode == ListMode::HostSized;
    int rc;
    const uint64_t entries = compact ? ctx->slot_pool : counting ? 0u : (uint64_t)n_regions * fixed_region_cap(ctx);
    if ((rc = bin_buffers(ctx, pf, entries))) return rc;
    if (counting) prof_mark(ctx, "bin buffers (counter memset)");
    if (counting) bins.list = nullptr;
    bins.tile_slots = n_regions;
    if (compact) use_compact(ctx, n_regions, bins, fill_ok);
    else if ((rc = fixed_layout(ctx, pf))) return rc;
    bins.tile_plan = compact && fill_ok && ctx->plan_valid && ctx->tile_plan_enabled && ctx->tile_plan_state == 1 ? 1u
                                                                                                                 : 0u;
    bins.box_masks = ctx->box_masks == 2 || (ctx->box_masks == 1 && render_tris(ctx) < kPrepBigMesh) ? 1u : 0u;
    if (counting) prof_mark(ctx, "fixed layout upload");
    // the fill plan's test hook (every region planned empty) is checked every frame
    arm_plan_check(*pf.fs, n_regions, bins, ctx->fill_plan == 2);
    return XRT_OK;
}

// Device sizing's count pass: k_prep counts the frame's pairs per slot of the
// region grid's base layout and appends them to the set's pairs, a pool of
// ctx->motion_pool entries.  `rerun`: again, into a pool regrown.
int count_pairs(xrt_context* ctx, PendingFrame& pf, bool dev_plan, bool mark, bool rerun)
{
    FrameSet& fs = *pf.fs;
    BinBuffers& bins = pf.bins;
    const uint32_t n_regions = frame_regions(pf);
    int rc;
    if ((rc = bin_buffers(ctx, pf, ctx->motion_pool, rerun))) return rc;   // (a re-run clears this frame's counters)
    if (mark) prof_mark(ctx, "device first: bin buffers");
    if ((rc = fixed_layout(ctx, pf))) return rc;
    if (mark) prof_mark(ctx, "device first: fixed layout");
    if ((rc = ensure(ctx, fs.dyn_desc, n_regions))) return rc;
    if ((rc = ensure(ctx, fs.pairs, ctx->motion_pool))) return rc;
    if (dev_plan && ((rc = ensure(ctx, fs.plan_desc, n_regions)) ||
                     (rc = ensure(ctx, fs.plan_counts, (size_t)n_regions * kCounterStride))))
        return rc;
    bins.tile_slots = n_regions;
    bins.split_slots = 0u;
    bins.tile_plan = 0u;
    bins.plan_miss = nullptr;
    bins.box_masks = ctx->box_masks == 2 ? 1u : 0u;
    bins.list = nullptr;                           // the count-only pass, appending its pairs
    bins.pairs = fs.pairs.get();
    bins.pairs_cap = (uint32_t)std::min<uint64_t>(ctx->motion_pool, 0xFFFFFFFFull);
    if ((rc = launch_prep(ctx, pf))) return rc;
    if (mark) prof_mark(ctx, "device first: count pass (buffers before it)");
    return XRT_OK;
}

// ListMode::DeviceMoving and DeviceFirst (DESIGN.md "Moving camera"): the
// lists sized on the device, no host round trip -- k_prep counts its pairs per
// slot of the region grid's base layout (centre first), k_size_lists carves
// each slot's list from the set's pool, k_scatter_pairs bins into them.  Every
// region renders as tiles (no fill plan: the host never sees the counts).
// k_prep's flags are read when the set is next used (lazy_flags).
int device_sized_lists(xrt_context* ctx, PendingFrame& pf, ListMode mode)
{
    FrameSet& fs = *pf.fs;
    BinBuffers& bins = pf.bins;
    const hipStream_t ps = ctx->prep_stream;
    const uint64_t T = render_tris(ctx);
    const uint32_t n_regions = frame_regions(pf);
    const bool first = mode == ListMode::DeviceFirst;
    int rc;
    // (a geometry's first frame: room for ~6 pairs a triangle, checked below)
    const uint64_t first_guess = first ? 6u * (uint64_t)T + 2u * n_regions : 0u;
    ctx->motion_pool = ctx->motion_pool_forced
                           ? ctx->motion_pool_forced
                           : std::max<uint64_t>(std::max<uint64_t>(ctx->motion_pool, first_guess),
                                                std::max<uint64_t>(2 * ctx->slot_pool, 65536u));
    // the device fill plan (not for the transit layouts, whose tiles follow a host plan)
    const bool dev_plan = ctx->device_fill && ctx->fill_plan != 0 && pf.out.packed == 0u;
    if ((rc = count_pairs(ctx, pf, dev_plan, first, false))) return rc;
    if (first) {
        // A first frame has no earlier pose to size its pool from: the count
        // pass's pair total (32 bytes read back) checks it, and a pool too
        // small grows and counts again -- never the whole-mesh fallback.
        ++ctx->hp_dev_first;
        uint8_t* hs = nullptr;
        if ((rc = sizing_scratch(ctx, sizeof(BinState), hs))) return rc;
        XRT_HIP(ctx, hipMemcpyAsync(hs, pf.bin_ctl, sizeof(BinState), hipMemcpyDeviceToHost, ps));
        XRT_HIP(ctx, hipStreamSynchronize(ps));
        BinState st;
        std::memcpy(&st, hs, sizeof st);
        prof_mark(ctx, "device first: pair total read back");
        ctx->dev_first_pairs = st.pairs;
        ctx->dev_first_pool = bins.pairs_cap;
        if (st.pairs > bins.pairs_cap && !ctx->motion_pool_forced) {
            ++ctx->hp_dev_first_recounts;
            ctx->motion_pool = std::min<uint64_t>((uint64_t)st.pairs + st.pairs / 4u + 65536u, 0xFFFFFFFFull);
            if ((rc = count_pairs(ctx, pf, dev_plan, false, true))) return rc;
        }
    }
    const uint32_t pool = bins.pairs_cap;
    uint32_t* const flag = fs.plan_flag.get() ? const_cast<uint32_t*>(fs.plan_flag.get()) : nullptr;
    if (flag) {                                    // [1]: a list past the pool, read lazily
        flag[0] = 0u;
        flag[1] = 0u;
        fs.lazy_flags = true;
    }
    // The lists of the frame: k_size_lists and k_scatter_pairs on the device's
    // host stream (idle in a device-pointer pipeline, no extra queue) after
    // the count pass's event, the preparation's event after them.  (Measured
    // and dropped: on the render's stream they queue behind that stream's
    // previous render, on the prep stream the next frame's k_prep queues
    // behind them -- 2048^2 moving frames 47.0 / 57.5 us against 41.1,
    // profiles/r06ac, r06ae.)
    uint32_t* const pass_counts = bins.counts;     // the count pass's counter lines (the base layout's order)
    const SlotDesc* const fixed = bins.desc;
    SlotDesc* const plan_desc = dev_plan ? fs.plan_desc.get() : nullptr;   // the device fill plan's layout (null: none)
    uint32_t* const plan_counts = dev_plan ? fs.plan_counts.get() : nullptr;
    bins.list = fs.bin_list.get();
    bins.desc = dev_plan ? fs.plan_desc.get() : fs.dyn_desc.get();
    if (dev_plan) {                                // the render reads the plan's order
        bins.counts = fs.plan_counts.get();
        bins.dev_plan = 1u;
    }
    bins.pairs = nullptr;
    bins.clear = nullptr;
    const hipStream_t ss = ctx->host_stream;
    if (ss != ps) XRT_HIP(ctx, hipStreamWaitEvent(ss, pf.prep_done, 0));
    hipLaunchKernelGGL(k_size_lists, dim3((n_regions + 255) / 256), dim3(256), 0, ss, pass_counts, fixed,
                       fs.dyn_desc.get(), n_regions, pool, pf.bin_ctl, plan_desc, plan_counts);
    XRT_HIP(ctx, hipGetLastError());
    const uint32_t scatter_blocks = (uint32_t)std::min<uint64_t>((pool + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(k_scatter_pairs, dim3(scatter_blocks), dim3(256), 0, ss, (const uint4*)fs.pairs.get(),
                       (const BinState*)pf.bin_ctl, pool, (const SlotDesc*)fs.dyn_desc.get(), (const float4*)fs.cull.get(),
                       (uint32_t)T, bins.list, flag);
    XRT_HIP(ctx, hipGetLastError());
    XRT_HIP(ctx, hipEventRecord(pf.prep_done, ss));
    return XRT_OK;
}

// ListMode::HostSized, after its count pass: the compact region lists sized
// once per frame geometry (mesh, camera, strip) -- a synchronous read of every
// region's count, the plan from them (plan_lists), its layout's upload, and a
// re-run of k_prep into the compact lists.
int host_sized_lists(xrt_context* ctx, PendingFrame& pf)
{
    const hipStream_t ps = ctx->prep_stream;
    const uint32_t n_regions = frame_regions(pf);
    int rc;
    ++ctx->hp_sizings;
    prof_mark(ctx, "k_prep count pass");
    const auto t_sizing = HostClock::now();
    // every region's count (line-padded) and the BinState, into the pinned scratch
    const size_t cbytes = (size_t)n_regions * kCounterStride * sizeof(uint32_t);
    uint8_t* hs = nullptr;
    if ((rc = sizing_scratch(ctx, cbytes + sizeof(BinState), hs))) return rc;
    XRT_HIP(ctx, hipMemcpyAsync(hs, pf.bins.counts, cbytes, hipMemcpyDeviceToHost, ps));
    prof_mark(ctx, "count read-back: counts enqueued");
    XRT_HIP(ctx, hipMemcpyAsync(hs + cbytes, pf.bin_ctl, sizeof(BinState), hipMemcpyDeviceToHost, ps));
    prof_mark(ctx, "count read-back: state enqueued");
    XRT_HIP(ctx, hipStreamSynchronize(ps));
    prof_mark(ctx, "count read-back");
    BinState st;
    std::memcpy(&st, hs + cbytes, sizeof st);
    ListPlan plan;
    if (!plan_lists(reinterpret_cast<const uint32_t*>(hs), kCounterStride, ctx->fixed.slot_region, st.global_count,
                    ctx->fill_plan, ctx->geo.moving, ctx->split_min, ctx->wave_slots, kWavesPerRegion, plan))
        return fail(ctx, XRT_ERR_OVERFLOW, "region lists exceed 2^32 entries");
    prof_mark(ctx, "plan (host)");
    if ((rc = upload_layout(ctx, ctx->compact_layout, pf.rx, pf.ry, std::move(plan.slot_region), plan.base, plan.cap)))
        return rc;
    ctx->tile_plan_state = 0;                  // the new layout's tiles are all live
    prof_mark(ctx, "compact layout upload");
    ctx->acc_ms[1] += std::chrono::duration<double, std::milli>(HostClock::now() - t_sizing).count();
    ctx->plan_tile_slots = plan.tile_slots;
    ctx->plan_split_slots = plan.split_slots;
    ctx->plan_valid = plan.tile_slots < n_regions;
    ctx->slot_pool = plan.pool;
    ctx->geo.compact = true;
    ctx->geo.bin_key = ctx->geo.last_key;      // this frame's
    ctx->geo.bin_key_valid = true;
    if ((rc = bin_buffers(ctx, pf, plan.pool, true))) return rc;   // clears
    pf.bins.tile_slots = n_regions;
    use_compact(ctx, n_regions, pf.bins, pf.p.model == kModelAttenuation);
    arm_plan_check(*pf.fs, n_regions, pf.bins, true);
    prof_mark(ctx, "counter memset (re-run)");
    if ((rc = launch_prep(ctx, pf))) return rc;
    prof_mark(ctx, "k_prep into the compact lists");
    return XRT_OK;
}

// The render's grid, the set's statistics records, and what launch_frame needs
// to know of the lists.
int finish_frame(xrt_context* ctx, const BinKey& key, ListMode mode, PendingFrame& pf)
{
    FrameSet& fs = *pf.fs;
    const BinBuffers& bins = pf.bins;
    const uint32_t n_regions = frame_regions(pf);
    int rc;
    // BINNED: one 8x8 tile per render wave, kTileWaves waves per workgroup, and
    // one workgroup per region of the fill plan
    pf.grid = pf.kernel == XRT_KERNEL_BRUTE ? dim3((pf.p.width + 15) / 16, (pf.rows + 15) / 16)
              : pf.binned ? dim3(kWavesPerRegion / kTileWaves * (bins.tile_slots + bins.split_slots) +
                                 (n_regions - bins.tile_slots))
                          : dim3(pf.rx, pf.ry);
    // stats records: one per workgroup; BINNED one per tile wave, 16 per fill region
    const uint32_t n_blocks = !pf.rows ? 0u : pf.binned ? kWavesPerRegion * n_regions : pf.grid.x * pf.grid.y;
    if ((rc = ensure(ctx, fs.block_stats, n_blocks))) return rc;
    if ((rc = ensure(ctx, fs.times, n_blocks))) return rc;
    fs.n_blocks = n_blocks;
    fs.binned = pf.binned;
    pf.out.block_stats = fs.block_stats.get();
    pf.plan_source = (mode == ListMode::Compact || mode == ListMode::HostSized) &&
                     pf.p.model == kModelAttenuation && ctx->plan_valid &&
                     bins.desc == ctx->compact_layout.d_desc.get() && bins.tile_slots == ctx->plan_tile_slots;
    pf.hit_plan_ok = ctx->hit_valid && key.same(ctx->hit_key);
    if (!pf.rows) pf.prep_done = nullptr;
    pf.host_wait = bins.plan_miss != nullptr;      // (never armed in a device-sized frame)
    return XRT_OK;
}

// A frame's preparation, enqueued on the context's prep stream beside the
// previous frame's render; the host waits for its completion before it
// launches the render (DESIGN.md "Pipelining": no cross-queue event on the
// render queue).
int prepare_frame(xrt_context* ctx, const xrt_camera* cam, uint32_t row_begin, uint32_t row_end,
                  float* d_image, float* d_lbuffer, uint8_t* d_u8, hipStream_t stream, PendingFrame& pf,
                  int set_index = -1)
{
    pf = PendingFrame{};
    int rc = choose_kernel(ctx, cam, row_begin, row_end, d_image, d_u8, pf);
    if (rc) return rc;
    pf.fs = &ctx->sets[set_index < 0 ? ctx->next_set : set_index];
    pf.stream = stream;
    pf.prep_done = pf.fs->ready.get();
    pf.t_call = HostClock::now();
    if ((rc = claim_set(ctx, cam, pf))) return rc;
    pf.p = make_params(*cam, row_begin, row_end, render_tris(ctx), ctx->hit_capacity);
    pf.p.model = ctx->model;
    if (!ctx->cull_valid || std::memcmp(&ctx->cull_cam, cam, sizeof *cam) != 0) {
        ctx->cull = make_cull_params(*cam);      // a scan over the rows / columns: once per camera
        ctx->cull_cam = *cam;
        ctx->cull_valid = true;
    }
    if ((rc = frame_outputs(ctx, cam, d_image, d_lbuffer, d_u8, pf))) return rc;
    const xrt_context::BinKey key = geometry_key(ctx, cam, row_begin, row_end);
    const ListMode mode = choose_list_mode(
        ctx->geo, FrameFacts{key, pf.binned, ctx->model == kModelAttenuation, ctx->bin_force_cap != 0,
                             ctx->packed_cap || ctx->hits_cap, ctx->reuse_cameras, ctx->device_first,
                             stream == ctx->host_stream});
    if (mode == ListMode::DeviceMoving) ++ctx->hp_reused;
    if ((mode == ListMode::HostSized || mode == ListMode::DeviceFirst) && ctx->sizing_profile) {
        ctx->prof_t = pf.t_call;
        prof_mark(ctx, "set wait + buffers");
    }
    if (pf.binned) {
        pf.bins.regions_x = pf.rx;
        pf.bins.regions_y = pf.ry;
    }
    if (mode == ListMode::DeviceMoving || mode == ListMode::DeviceFirst) {
        if ((rc = device_sized_lists(ctx, pf, mode))) return rc;
    } else {
        if (mode != ListMode::None && (rc = known_lists(ctx, pf, mode))) return rc;
        if (pf.rows > 0 && (rc = launch_prep(ctx, pf))) return rc;
        if (mode == ListMode::HostSized && (rc = host_sized_lists(ctx, pf))) return rc;
    }
    return finish_frame(ctx, key, mode, pf);
}

// The timed region's record space: one chunk of `space` records in place of
// every earlier one.
int region_chunk(xrt_context* ctx, size_t space)
{
    ctx->tchunks.clear();
    xrt_context::TimesChunk c;
    XRT_HIP(ctx, c.p.reserve(space));
    ctx->tchunks.push_back(std::move(c));
    ctx->timing_space = space;
    return XRT_OK;
}

// At least n timing-enabled events for the region's sampled dispatches.
int region_events(xrt_context* ctx, size_t n)
{
    while (ctx->tev.size() < n) {
        TimedEvent e;
        XRT_HIP(ctx, e.create());
        ctx->tev.push_back(std::move(e));
    }
    return XRT_OK;
}

// Room for n timing records of a sampled frame in the timed region's chunks
// (a new chunk, never a moved one, when the last is full).
int timing_slot(xrt_context* ctx, size_t n, uint2*& slot)
{
    if (ctx->tchunks.empty() || ctx->tchunks.back().p.cap() - ctx->tchunks.back().used < n) {
        size_t want = std::max<size_t>(n * 64, (size_t)1 << 16);
        // chunks of earlier regions are reused before new ones are allocated
        size_t k = 0;
        while (k < ctx->tchunks.size() && !(ctx->tchunks[k].used == 0 && ctx->tchunks[k].p.cap() >= n)) ++k;
        if (k < ctx->tchunks.size() && k + 1 < ctx->tchunks.size()) {
            // an unused chunk to the end (the samples hold device pointers, not indices)
            std::swap(ctx->tchunks[k], ctx->tchunks.back());
        } else if (k == ctx->tchunks.size()) {
            xrt_context::TimesChunk c;
            XRT_HIP(ctx, c.p.reserve(want));
            ctx->tchunks.push_back(std::move(c));
        }
    }
    xrt_context::TimesChunk& c = ctx->tchunks.back();
    slot = c.p.get() + c.used;
    ctx->tsamples.push_back({slot, n});
    c.used += n;
    return XRT_OK;
}

// A frame's kernel span from its waves' timing records: the last end minus
// the first start, in ms (32-bit tick differences: spans below 21 s).
double records_span_ms(const std::vector<uint2>& t)
{
    if (t.empty()) return 0.0;
    const uint32_t ref = t[0].x;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (const uint2& r : t) {
        lo = std::min<int64_t>(lo, (int32_t)(r.x - ref));
        hi = std::max<int64_t>(hi, (int32_t)(r.y - ref));
    }
    return hi > lo ? (double)(hi - lo) / kTicksPerMs : 0.0;
}

// The ray table for an attenuation BINNED frame about to be launched on
// `stream`, or null when the frame computes its rays (xrt_context::RayKey).
// A frame whose key repeats the previous frame's starts the fill (the trigger
// of prepare-ahead: an orbit or a one-shot frame never pays for one); the
// frames until then, a frame over the budget and a context with the table off
// compute.  The render is ordered after the fill on the device, one wait per
// stream and fill and none once the fill's event has passed; the host never
// waits.  A table that launched renders may still read is not refilled: the
// new key's frames compute until those renders' completion events have passed.
int frame_rays(xrt_context* ctx, const RenderParams& p, hipStream_t stream, const float*& rays)
{
    rays = nullptr;
    xrt_context::RayKey key = {};
    const float cam[13] = {p.ox, p.oy, p.oz, p.cx, p.cy, p.cz, p.ux, p.uy, p.uz, p.rx, p.ry, p.rz, p.spacing};
    std::memcpy(key.cam, cam, sizeof cam);
    key.width = p.width;
    key.height = p.height;
    key.row_begin = p.row_begin;
    key.row_end = p.row_end;
    const bool repeated = ctx->ray_call_valid && key.same(ctx->ray_call_key);
    ctx->ray_call_key = key;
    ctx->ray_call_valid = true;
    if (ctx->ray_valid && !key.same(ctx->ray_key)) ctx->ray_valid = false;
    const uint64_t floats = ray_table_floats(p.width, p.row_begin, p.row_end);
    if (!ctx->ray_enabled || floats * sizeof(float) > ctx->ray_budget) {
        ++ctx->hp_ray_computed;
        return XRT_OK;
    }
    if (!ctx->ray_valid && repeated) {
        // renders in flight over the old table (a set is reused only after its
        // last render is complete, so each set's last event speaks for it), and
        // an old fill still running before the buffer is freed for a larger one
        bool busy = false;
        for (FrameSet& fs : ctx->sets) {
            if (!fs.ray_reader) continue;
            if (!fs.done_valid || hipEventQuery(fs.done_ev) == hipSuccess) fs.ray_reader = false;
            else busy = true;
        }
        if (!busy && floats > ctx->d_rays.cap() && ctx->d_rays && ctx->ray_filled.passed() != hipSuccess) busy = true;
        if (!busy) {
            XRT_HIP(ctx, ctx->d_rays.reserve(floats));
            const uint32_t tiles = ray_table_tiles_x(p.width) * ray_table_tiles_y(p.row_begin, p.row_end);
            hipLaunchKernelGGL(k_ray_table, dim3((tiles + 3u) / 4u), dim3(256), 0, ctx->prep_stream, p, ctx->d_rays.get());
            XRT_HIP(ctx, hipGetLastError());
            XRT_HIP(ctx, ctx->ray_filled.record(ctx->prep_stream));
            ctx->ray_key = key;
            ctx->ray_valid = true;
            ctx->ray_waited.clear();
            ++ctx->hp_ray_fills;
        }
    }
    if (!ctx->ray_valid) {
        ++ctx->hp_ray_computed;
        return XRT_OK;
    }
    const hipError_t q = ctx->ray_filled.passed();
    if (q != hipErrorNotReady) XRT_HIP(ctx, q);
    else if (std::find(ctx->ray_waited.begin(), ctx->ray_waited.end(), stream) == ctx->ray_waited.end()) {
        XRT_HIP(ctx, ctx->ray_filled.order(stream));
        ctx->ray_waited.push_back(stream);
    }
    ++ctx->hp_ray_frames;
    rays = ctx->d_rays.get();
    return XRT_OK;
}

int launch_frame(xrt_context* ctx, PendingFrame& pf)
{
    FrameSet& fs = *pf.fs;
    hipStream_t stream = pf.stream;
    const int kernel = pf.kernel;
    const bool binned = pf.binned;
    const uint32_t rows = pf.rows, rx = pf.rx, ry = pf.ry;
    const RenderParams& p = pf.p;
    BinState* bin_ctl = pf.bin_ctl;
    const auto t_call = pf.t_call;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    // The render runs once its preparation is complete: the caller's queue
    // waits for it on the device (a barrier packet, ~2.4 us per frame), or --
    // when the host must read k_prep's check to choose the grid -- the host
    // waits for it before the launch.
    if (pf.prep_done && pf.host_wait) {
        const auto t = HostClock::now();
        XRT_HIP(ctx, hipEventSynchronize(pf.prep_done));
        ctx->acc_ms[3] += std::chrono::duration<double, std::milli>(HostClock::now() - t).count();
        ++ctx->hp_host_waits;
        if (ctx->host_profile) ctx->hp_prep += seconds_since(t);
    } else if (pf.prep_done) {
        // a preparation already complete needs no wait packet (a frame prepared
        // ahead usually is); hipErrorNotReady otherwise
        const hipError_t q = hipEventQuery(pf.prep_done);
        if (q == hipSuccess) ++ctx->hp_launch_nowait;
        else if (q == hipErrorNotReady) XRT_HIP(ctx, hipStreamWaitEvent(stream, pf.prep_done, 0));
        else XRT_HIP(ctx, q);
    }
    dim3 grid = pf.grid;
    BinBuffers bins = pf.bins;
    bool missed = false;
    if (binned && bins.plan_miss && pf.host_wait && (fs.plan_flag.get()[0] | fs.plan_flag.get()[1]) != 0u) {
        missed = true;
        // k_prep binned a pair into a region the plan fills, into the global
        // list or past a list's capacity: this frame renders every region as
        // tiles (an overflowed region from the whole mesh -- exact, slower), and
        // the next frame re-sizes its lists.
        ++(fs.plan_flag.get()[1] != 0u ? ctx->hp_overflow : ctx->hp_plan_miss);
        bins.tile_slots = rx * ry;
        bins.tile_plan = 0u;
        pf.plan_source = false;
        // an overflowed list renders its region from the whole mesh: as ordinary
        // tiles (split tiles only ever merge list-rendered halves)
        if (fs.plan_flag.get()[1] != 0u) bins.split_slots = 0u;
        grid = dim3(kWavesPerRegion / kTileWaves * (bins.tile_slots + bins.split_slots));
        ctx->geo.resize_next_frame();
    }
    ctx->last_fill_regions = binned ? rx * ry - bins.tile_slots : 0u;
    if (pf.out.packed == kLayoutPacked && rows > 0 &&
        (bins.tile_slots >= rx * ry || (uint64_t)bins.tile_slots * kPackBlock > ctx->packed_cap))
        return fail(ctx, XRT_ERR_OVERFLOW, "the packed layout needs this frame's fill plan (and room for its "
                                        "unfilled regions): the frame was not rendered");
    // the hit layout: the plan's tiles are exactly this frame's tile regions',
    // and the message has room for the plan's words plus one tile's hits (a
    // tile with more hits than its plan stays inside the buffer)
    if (pf.out.packed == kLayoutHits && rows > 0 &&
        (!pf.hit_plan_ok || missed || (uint64_t)bins.tile_slots * kWavesPerRegion != pf.out.hit_tiles ||
         ctx->hit_words + kWavesPerRegion * 4u > ctx->hits_cap))
        return fail(ctx, XRT_ERR_OVERFLOW, "the hit layout needs this geometry's hit plan (xrt_plan_hit_layout), "
                                        "its fill plan and room for its words: the frame was not rendered");

    // Every render dispatch carries the set's stop event (the host needs it
    // to reuse the set).  Its waves store their timing records beside their
    // statistics (the span of the set's last frame: xrt_read_stats); in a
    // timed region every frame keeps them apart (the mean span over the
    // region's frames: xrt_timing_end) and every kEventStride-th
    // dispatch also carries a start event (xrt_timing_events).
    Outputs out = pf.out;
    out.wave_times = fs.times.get();
    hipEvent_t t0 = nullptr, t1 = fs.done.get();
    const uint64_t frame_in_region = ctx->timing ? ctx->timed_frames++ : 0;
    if (ctx->timing && rows > 0 && frame_in_region == 0 &&
        ctx->timing_space < std::min(kTimingRecords, kTimingFrames * (size_t)fs.n_blocks)) {
        // the region's first frame is larger than the space xrt_timing_begin
        // sized from the context's previous frame (or there was none): room for
        // kTimingFrames of these, before any record of the region is kept
        const size_t space = std::min(kTimingRecords, kTimingFrames * (size_t)fs.n_blocks);
        XRT_HIP(ctx, hipStreamSynchronize(stream));
        if (int rc = region_chunk(ctx, space)) return rc;
    }
    if (ctx->timing && rows > 0 && ctx->timed_records + fs.n_blocks <= ctx->timing_space) {
        ctx->timed_records += fs.n_blocks;
        uint2* slot = nullptr;
        int rc = timing_slot(ctx, fs.n_blocks, slot);
        if (rc) return rc;
        out.wave_times = slot;
    }
    fs.last_times = out.wave_times;
    fs.rendered_blocks = fs.n_blocks;
    if (ctx->timing && rows > 0 && frame_in_region % kEventStride == 0) {
        if (ctx->tev_used + 2 > ctx->tev.size())
            if (int rc = region_events(ctx, ctx->tev.size() + 64)) return rc;
        t0 = ctx->tev[ctx->tev_used].get();
        t1 = ctx->tev[ctx->tev_used + 1].get();
        ctx->tev_used += 2;
    }
    if (rows > 0) {
        const bool sgn = p.model != kModelAttenuation;
        const bool mat = p.model == kModelMaterials;
        const bool spc = p.model == kModelSpectrum;
        const bool pth = p.model == kModelPaths;
        // the attenuation BINNED render takes its rays from the camera's table
        // when there is one for this frame (the other models need the
        // once-normalised direction, and the hit layout keeps its own kernel)
        const bool ray_scope = kernel != XRT_KERNEL_BRUTE && kernel != XRT_KERNEL_TILED && binned && !sgn &&
                               out.packed != kLayoutHits;
        if (ray_scope) {
            if (int rc = frame_rays(ctx, p, stream, out.rays)) return rc;
        }
        fs.ray_reader = out.rays != nullptr;
        const auto t_launch = HostClock::now();
        if (kernel == XRT_KERNEL_BRUTE)
            hipExtLaunchKernelGGL(pth   ? k_render_brute<kModelPaths>
                                  : spc ? k_render_brute<kModelSpectrum>
                                  : mat ? k_render_brute<kModelMaterials>
                                  : sgn ? k_render_brute<kModelSigned>
                                        : k_render_brute<kModelAttenuation>, grid, dim3(256), 0, stream,
                                  t0, t1, 0, fs.recs.get(), p, out);
        else if (kernel == XRT_KERNEL_TILED || !binned)
            hipExtLaunchKernelGGL(k_render_tiled, dim3(rx, ry), dim3(256), 0, stream, t0, t1, 0,
                                  fs.recs.get(), fs.cull.get(), p, out);
        else
            hipExtLaunchKernelGGL(pth   ? k_render_binned<kModelPaths>
                                  : spc ? k_render_binned<kModelSpectrum>
                                  : mat ? k_render_binned<kModelMaterials>
                                  : sgn ? k_render_binned<kModelSigned>
                                  : out.packed == kLayoutHits ? k_render_binned_hits
                                  : out.rays                  ? k_render_binned_rays
                                                              : k_render_binned<kModelAttenuation>, grid, dim3(64 * kTileWaves),
                                  0, stream, t0, t1, 0, fs.recs.get(), fs.cull.get(), p, out, bins, (const BinState*)bin_ctl);
        XRT_HIP(ctx, hipGetLastError());
        ctx->acc_ms[4] += std::chrono::duration<double, std::milli>(HostClock::now() - t_launch).count();
        if (ctx->host_profile) ctx->hp_lrender += seconds_since(t_launch);
        fs.done_ev = t1;
        fs.done_valid = true;
        if (binned && bins.tile_plan) ++ctx->hp_tile_plan_frames;
        // The geometry's tile plan from this render's records, once (behind
        // the render on its stream; frames in flight read either value, both
        // exact for the geometry).
        if (binned && !sgn && pf.plan_source && ctx->tile_plan_enabled && ctx->tile_plan_state == 0 &&
            bins.tile_slots > bins.split_slots) {
            const uint32_t n = bins.tile_slots - bins.split_slots;
            hipLaunchKernelGGL(k_tile_plan, dim3((n + 255) / 256), dim3(256), 0, stream, fs.block_stats.get(),
                               ctx->compact_layout.d_desc.get(), bins.split_slots, bins.tile_slots);
            XRT_HIP(ctx, hipGetLastError());
            // the set's completion event covers k_tile_plan too: the set's
            // statistics records and the layout's descriptions are not
            // rewritten while it reads / writes them
            XRT_HIP(ctx, hipEventRecord(fs.done.get(), stream));
            fs.done_ev = fs.done.get();
            ctx->tile_plan_state = 1;
            ++ctx->hp_tile_plans;
        }
    }
    if (ctx->host_profile) {
        ctx->hp_total += seconds_since(t_call);
        if (ctx->hp_calls) ctx->hp_gap += std::chrono::duration<double>(t_call - ctx->hp_last_end).count();
        ctx->hp_last_end = HostClock::now();
        ++ctx->hp_calls;
    }
    ctx->last_set = &fs;
    ctx->next_set = (int)((&fs - ctx->sets) + 1) % kFrameSets;
    ctx->last_stream = stream;
    ctx->pending = true;
    ctx->last_kernel = kernel;
    return XRT_OK;
}

// One frame: its preparation (or the one prepared ahead for it) and its
// render; `ahead` (the pipelined device-pointer entry) prepares the next
// frames of a repeated geometry ahead of their calls (xrt_context::ahead).
int enqueue_render(xrt_context* ctx, const xrt_camera* cam, uint32_t row_begin, uint32_t row_end,
                   float* d_image, float* d_lbuffer, uint8_t* d_u8, hipStream_t stream, bool ahead = false,
                   bool paths = false)
{
    int rc = check_camera(ctx, cam, row_begin, row_end);
    if (rc) return rc;
    // the paths model's planes are not the other entries' (`paths`: xrt_render_paths_device's call)
    if ((ctx->model == kModelPaths) != paths)
        return fail(ctx, XRT_ERR_ARGUMENT, paths ? "xrt_render_paths needs xrt_set_paths"
                                                 : "the paths model renders with xrt_render_paths");
    const xrt_context::BinKey key = geometry_key(ctx, cam, row_begin, row_end);
    const uint32_t outs = (d_image ? 1u : 0u) | (d_lbuffer ? 2u : 0u) | (d_u8 ? 4u : 0u);
    PendingFrame pf;
    bool taken = false;
    if (!ctx->ahead.empty()) {
        xrt_context::AheadFrame& a = ctx->ahead.front();
        if (ahead && a.key.same(key) && a.state_gen == ctx->state_gen && a.outs == outs) {
            pf = a.pf;
            ctx->ahead.pop_front();
            pf.stream = stream;
            pf.out.image = d_image;
            pf.out.lbuffer = d_lbuffer;
            pf.out.image_u8 = d_u8;
            pf.t_call = HostClock::now();
            taken = true;
            ++ctx->hp_ahead_used;
        } else {                       // their k_prep runs before any newer one (prep stream)
            ctx->hp_ahead_dropped += ctx->ahead.size();
            ctx->ahead.clear();
        }
    }
    if (!taken && (rc = prepare_frame(ctx, cam, row_begin, row_end, d_image, d_lbuffer, d_u8, stream, pf)))
        return rc;
    const bool repeated = ahead && key.same(ctx->call_key) && ctx->call_state_gen == ctx->state_gen;
    ctx->call_key = key;
    ctx->call_state_gen = ahead ? ctx->state_gen : ~0ull;
    if ((rc = launch_frame(ctx, pf))) return rc;
    // the next frames of a repeated geometry, prepared now (a steady frame:
    // no sizing, no check to read on the host)
    if (repeated && !pf.host_wait && pf.rows > 0) {
        while (ctx->ahead.size() < kAheadFrames) {
            xrt_context::AheadFrame a;
            a.key = key;
            a.state_gen = ctx->state_gen;
            a.outs = outs;
            const int set = (int)((ctx->next_set + ctx->ahead.size()) % kFrameSets);
            if ((rc = prepare_frame(ctx, cam, row_begin, row_end, d_image, d_lbuffer, d_u8, stream, a.pf, set))) {
                ctx->ahead.clear();
                return rc;
            }
            a.pf.ahead = true;
            ctx->ahead.push_back(a);
        }
    }
    return XRT_OK;
}

// One plane's device -> host copy of a host-buffer call.
struct D2HCopy {
    void* dst;
    const void* src;
    size_t bytes;
};

// Copies `copies` (device -> the caller's host pages) behind the work already
// on `stream`: kStageChunk pieces DMAed in order into the pinned ring on the
// stream, each moved into the caller's pages by a copy thread once its DMA is
// complete; a ring slot is reused once its previous piece has been moved.
// Without copy threads (XRT_D2H_THREADS=0): pageable copies + synchronise.
int d2h_copy(xrt_context* ctx, hipStream_t stream, const std::vector<D2HCopy>& copies)
{
    struct Piece {
        uint8_t* dst;
        const uint8_t* src;
        size_t bytes;
    };
    std::vector<Piece> pieces;                         // at most kStageChunk, ending at 2-MB boundaries of dst
    for (const D2HCopy& c : copies) {
        size_t o = 0;
        while (o < c.bytes) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(c.dst) + o;
            const size_t len = std::min(kStageChunk - (size_t)(a % kStageChunk), c.bytes - o);
            pieces.push_back({(uint8_t*)c.dst + o, (const uint8_t*)c.src + o, len});
            o += len;
        }
    }
    if (pieces.empty()) return XRT_OK;
    if (!ctx->pool) {
        for (const D2HCopy& c : copies)
            if (c.bytes) XRT_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream));
        XRT_HIP(ctx, hipStreamSynchronize(stream));
        return XRT_OK;
    }
    const size_t n = pieces.size();
    std::atomic<size_t> enqueued{0};                   // pieces whose DMA (and event) is enqueued
    std::unique_ptr<std::atomic<uint8_t>[]> moved(new std::atomic<uint8_t>[n]);
    for (size_t i = 0; i < n; ++i) moved[i].store(0);
    std::atomic<int> failed{0};
    ctx->pool->start(n, [&](size_t i) {
        while (enqueued.load(std::memory_order_acquire) <= i) {
            if (failed.load()) {
                moved[i].store(1, std::memory_order_release);
                return;
            }
            std::this_thread::yield();
        }
        if (hipEventSynchronize(ctx->stage_ev[i % kStageSlots].get()) != hipSuccess)
            failed.store(1);
        else
            std::memcpy(pieces[i].dst, ctx->h_stage.get() + (i % kStageSlots) * kStageChunk, pieces[i].bytes);
        moved[i].store(1, std::memory_order_release);
    });
    hipError_t err = hipSuccess;
    for (size_t i = 0; i < n; ++i) {
        if (i >= kStageSlots)                          // the slot's previous piece has been moved
            while (!moved[i - kStageSlots].load(std::memory_order_acquire)) std::this_thread::yield();
        uint8_t* slot = ctx->h_stage.get() + (i % kStageSlots) * kStageChunk;
        err = hipMemcpyAsync(slot, pieces[i].src, pieces[i].bytes, hipMemcpyDeviceToHost, stream);
        if (err == hipSuccess) err = hipEventRecord(ctx->stage_ev[i % kStageSlots].get(), stream);
        if (err != hipSuccess) {
            failed.store(1);
            break;
        }
        enqueued.store(i + 1, std::memory_order_release);
    }
    ctx->pool->wait();
    if (err != hipSuccess) return fail(ctx, XRT_ERR_DEVICE, std::string("D2H copy: ") + hipGetErrorString(err));
    if (failed.load()) return fail(ctx, XRT_ERR_DEVICE, "D2H copy: a staged piece failed");
    return XRT_OK;
}

// How a host buffer meets the device, one of two ways (DESIGN.md "Host entry
// points"): the renders and the hole fill go through the context's staging
// planes (stage_planes, plane_copies, d2h_copy); the operators and the probes
// through buffers of their own call (DeviceScratch).

// The context's staging planes (d_image, d_lbuffer, d_u8), each of at least
// `need` elements: a plane that is too small is replaced by one of `need`.
int stage_planes(xrt_context* ctx, size_t need)
{
    if (int rc = ensure(ctx, ctx->d_image, need)) return rc;
    if (int rc = ensure(ctx, ctx->d_lbuffer, need)) return rc;
    return ensure(ctx, ctx->d_u8, need);
}

// The copy-back list of a call's `n` pixels: the planes the caller asked for
// (a NULL host pointer: not asked for), each from its device plane.
std::vector<D2HCopy> plane_copies(size_t n, float* image, const float* d_image, float* lbuffer, const float* d_lbuffer,
                                  uint8_t* image_u8, const uint8_t* d_u8)
{
    std::vector<D2HCopy> copies;
    if (n) {
        if (image) copies.push_back({image, d_image, n * sizeof(float)});
        if (lbuffer) copies.push_back({lbuffer, d_lbuffer, n * sizeof(float)});
        if (image_u8) copies.push_back({image_u8, d_u8, n});
    }
    return copies;
}

// The device buffers of one call of a host-buffer operator or probe, all on
// `stream`: allocate (upload), launch, download, finish.  The first failure
// sticks (rc(), the context's error "<name> allocation / upload / kernel
// failed") and turns every later step into a no-op; the destructor waits for
// the stream and frees the buffers on every path.
class DeviceScratch {
public:
    DeviceScratch(xrt_context* ctx, hipStream_t stream, const char* name) : ctx_(ctx), stream_(stream), name_(name) {}
    DeviceScratch(const DeviceScratch&) = delete;
    DeviceScratch& operator=(const DeviceScratch&) = delete;
    ~DeviceScratch()
    {
        (void)hipStreamSynchronize(stream_);
        for (void* p : buffers_) (void)hipFree(p);
    }
    int rc() const { return rc_; }
    // `n` elements; nullptr when there are none or the buffer is not wanted
    template <typename T>
    T* alloc(size_t n, bool wanted = true)
    {
        void* p = nullptr;
        if (rc_ || !wanted || !n) return nullptr;
        if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return failed("allocation");
        buffers_.push_back(p);
        return static_cast<T*>(p);
    }
    // a buffer holding the `n` elements at `host` (NULL: no buffer)
    template <typename T>
    T* upload(const T* host, size_t n)
    {
        T* p = alloc<T>(n, host != nullptr);
        if (p && hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, stream_) != hipSuccess)
            return failed("upload");
        return p;
    }
    // after a bare hipLaunchKernelGGL
    void launched()
    {
        if (!rc_ && hipGetLastError() != hipSuccess) failed("kernel");
    }
    // behind the launch (`host` NULL: not asked for)
    template <typename T>
    void download(T* host, const T* device, size_t n)
    {
        if (!rc_ && host && hipMemcpyAsync(host, device, n * sizeof(T), hipMemcpyDeviceToHost, stream_) != hipSuccess)
            failed("kernel");
    }
    // the downloads are in the caller's buffers
    int finish()
    {
        if (!rc_ && hipStreamSynchronize(stream_) != hipSuccess) failed("kernel");
        return rc_;
    }

private:
    std::nullptr_t failed(const char* step)
    {
        rc_ = fail(ctx_, XRT_ERR_DEVICE, std::string(name_) + " " + step + " failed");
        return nullptr;
    }
    xrt_context* ctx_;
    hipStream_t stream_;
    const char* name_;
    int rc_ = XRT_OK;
    std::vector<void*> buffers_;
};

}  // namespace

extern "C" {

int xrt_debug_destroy_ms(double ms[4])
{
    if (!ms) return XRT_ERR_ARGUMENT;
    std::copy(g_destroy_ms, g_destroy_ms + 4, ms);
    return XRT_OK;
}

int xrt_abi_version(void) { return XRT_ABI_VERSION; }

int xrt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// XRT_SEGV_TRACE=1 (diagnostics): a fatal signal prints every frame of the
// faulting thread with the shared library it lies in (dladdr), then the
// signal is raised again with its default action.
namespace {
void fatal_signal_trace(int sig, siginfo_t* si, void*)
{
    void* frames[64];
    const int n = backtrace(frames, 64);
    char line[512];
    int k = std::snprintf(line, sizeof line, "xrt: signal %d (fault address %p), pid %d, %d frames:\n", sig,
                          si ? si->si_addr : nullptr, (int)getpid(), n);
    (void)!write(2, line, (size_t)std::max(k, 0));
    for (int i = 0; i < n; ++i) {
        Dl_info d = {};
        if (dladdr(frames[i], &d) && d.dli_fname)
            k = std::snprintf(line, sizeof line, "  #%-2d %p %s + %#lx (%s)\n", i, frames[i], d.dli_fname,
                              (unsigned long)((uintptr_t)frames[i] - (uintptr_t)d.dli_fbase),
                              d.dli_sname ? d.dli_sname : "?");
        else
            k = std::snprintf(line, sizeof line, "  #%-2d %p (no library)\n", i, frames[i]);
        (void)!write(2, line, (size_t)std::max(k, 0));
    }
    signal(sig, SIG_DFL);
    raise(sig);
}

void install_fatal_signal_trace()
{
    static std::once_flag once;
    std::call_once(once, [] {
        const char* v = std::getenv("XRT_SEGV_TRACE");
        if (!v || std::atoi(v) == 0) return;
        struct sigaction sa = {};
        sa.sa_sigaction = fatal_signal_trace;
        sa.sa_flags = SA_SIGINFO | SA_RESETHAND;
        sigemptyset(&sa.sa_mask);
        for (int sig : {SIGSEGV, SIGBUS, SIGABRT, SIGILL, SIGFPE}) sigaction(sig, &sa, nullptr);
    });
}
}  // namespace

int xrt_create(int device, xrt_context** out)
{
    install_fatal_signal_trace();
    if (!out) return fail(nullptr, XRT_ERR_ARGUMENT, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, XRT_ERR_DEVICE,
                    std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= n)
        return fail(nullptr, XRT_ERR_ARGUMENT, "device index out of range");
    if ((e = hipSetDevice(device)) != hipSuccess)
        return fail(nullptr, XRT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    xrt_context* ctx = new xrt_context();
    ctx->device = device;
    const char* hp = std::getenv("XRT_HOST_PROFILE");
    ctx->host_profile = hp && std::atoi(hp) != 0;
    if (const char* tp = std::getenv("XRT_TILE_PLAN")) ctx->tile_plan_enabled = std::atoi(tp) != 0;
    const char* sp = std::getenv("XRT_SIZING_PROFILE");
    ctx->sizing_profile = sp ? std::atoi(sp) : 0;
    if (const char* sm = std::getenv("XRT_SPLIT_MIN")) ctx->split_min = (uint32_t)std::strtoul(sm, nullptr, 10);
    if (const char* mp = std::getenv("XRT_MOTION_POOL")) ctx->motion_pool_forced = std::strtoull(mp, nullptr, 10);
    if (const char* bm = std::getenv("XRT_BOX_MASKS")) ctx->box_masks = std::atoi(bm);
    if (const char* df = std::getenv("XRT_DEVICE_FILL")) ctx->device_fill = std::atoi(df) != 0;
    if (const char* dq = std::getenv("XRT_DEVICE_FIRST")) ctx->device_first = std::atoi(dq) != 0;
    if (const char* rc = std::getenv("XRT_RAY_CACHE_MB")) ctx->ray_budget = (size_t)std::strtoull(rc, nullptr, 10) << 20;
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu <= 0)
        n_cu = 256;
    ctx->wave_slots = (uint32_t)n_cu * 32u;
    // The prep stream at the default queue priority: frames are prepared ahead
    // of their renders (the highest and the lowest priority measured the same).
    bool ok = ctx->ev_begin.create() == hipSuccess && ctx->ev_end.create() == hipSuccess;
    ok = ok && acquire_streams(device, ctx->prep_stream, ctx->host_stream);
    ctx->owns_streams = ok;
    hipFuncAttributes prep_attr = {};
    ok = ok && hipFuncGetAttributes(&prep_attr, reinterpret_cast<const void*>(k_prep)) == hipSuccess;
    // k_prep's own LDS must fit the cap (else more than XRT_PREP_PER_CU would not fit beside the render)
    ok = ok && prep_attr.sharedSizeBytes <= kPrepLds;
    ctx->prep_lds = ok ? kPrepLds - prep_attr.sharedSizeBytes : 0;
    ok = ok && ctx->d_stats_partial.reserve(kReduceMaxBlocks) == hipSuccess &&
         ctx->d_stats_done.reserve(1) == hipSuccess &&
         hipMemset(ctx->d_stats_done.get(), 0, sizeof(unsigned int)) == hipSuccess &&
         ctx->d_stats_out.reserve(1) == hipSuccess && ctx->h_stats.reserve(1) == hipSuccess;
    for (FrameSet& fs : ctx->sets)     // dispatch-attached events need timing enabled
        ok = ok && fs.frame.reserve(1) == hipSuccess && fs.ready.create() == hipSuccess &&
             fs.done.create() == hipSuccess && fs.plan_flag.reserve(2) == hipSuccess;
    // the host-buffer entry points' stream, pinned D2H ring and copy threads
    int threads = kD2HThreads;
    if (const char* th = std::getenv("XRT_D2H_THREADS")) threads = std::max(0, std::atoi(th));
    ok = ok && ctx->host_render_done.create() == hipSuccess && ctx->h_sizing.reserve(kSizingScratch) == hipSuccess;
    if (ok && threads > 0) {
        ok = ctx->h_stage.reserve(kStageSlots * kStageChunk) == hipSuccess;
        for (auto& e : ctx->stage_ev) ok = ok && e.create() == hipSuccess;
        if (ok) ctx->pool.reset(new CopyPool(threads));
    }
    if (!ok) {
        xrt_destroy(ctx);
        return fail(nullptr, XRT_ERR_DEVICE, "device allocation failed");
    }
    *out = ctx;
    return XRT_OK;
}

void xrt_destroy(xrt_context* ctx)
{
    if (!ctx) return;
    if (ctx->host_profile && ctx->hp_calls)
        std::fprintf(stderr, "xrt host profile: %llu enqueues, per call %.1f us (waiting: set reuse %.1f us, "
                     "preparation %.1f us; launching: k_prep %.1f us, render %.1f us; between calls %.1f us)\n",
                     (unsigned long long)ctx->hp_calls, ctx->hp_total / ctx->hp_calls * 1e6,
                     ctx->hp_done / ctx->hp_calls * 1e6, ctx->hp_prep / ctx->hp_calls * 1e6,
                     ctx->hp_lprep / ctx->hp_calls * 1e6, ctx->hp_lrender / ctx->hp_calls * 1e6,
                     ctx->hp_gap / ctx->hp_calls * 1e6);
    if (ctx->host_profile && ctx->hp_calls)
        std::fprintf(stderr, "xrt geometry: %llu sizings, %llu camera reuses; frames flagged by k_prep: %llu plan "
                     "misses, %llu list overflows; prepared ahead: %llu used, %llu dropped; renders launched "
                     "without a wait: %llu\n", (unsigned long long)ctx->hp_sizings,
                     (unsigned long long)ctx->hp_reused, (unsigned long long)ctx->hp_plan_miss,
                     (unsigned long long)ctx->hp_overflow, (unsigned long long)ctx->hp_ahead_used,
                     (unsigned long long)ctx->hp_ahead_dropped, (unsigned long long)ctx->hp_launch_nowait);
    (void)hipSetDevice(ctx->device);
    auto t = HostClock::now();
    auto lap = [&](int k) {
        const auto now = HostClock::now();
        g_destroy_ms[k] = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    };
    // [0] the context's work: its streams, its sets' renders, the last trace of
    // the volume and the last user of the working set
    (void)sync_context(ctx);
    if (ctx->host_stream) (void)hipStreamSynchronize(ctx->host_stream);
    (void)ctx->vol_traced.wait();
    (void)ctx->sirt_done.wait();
    lap(0);
    ctx->pool.reset();
    // [1] device memory (with the sets, their mapped flags and dispatch events)
    for (FrameSet& fs : ctx->sets) fs = FrameSet();
    ctx->fixed = SlotLayout();
    ctx->compact_layout = SlotLayout();
    ctx->tchunks.clear();
    release(ctx->d_tris, ctx->d_tris_posed, ctx->d_image, ctx->d_lbuffer, ctx->d_u8, ctx->d_stats_partial,
            ctx->d_stats_done, ctx->d_stats_out, ctx->d_hit_off, ctx->d_materials, ctx->d_spectrum, ctx->d_path_ends,
            ctx->d_prep_times, ctx->d_rays, ctx->vol_labels, ctx->vol_density, ctx->d_sirt);
    lap(1);
    // [2] pinned host memory
    release(ctx->h_stats, ctx->h_stage, ctx->h_sizing);
    lap(2);
    // [3] the device's shared streams, and the events
    if (ctx->owns_streams) release_streams(ctx->device);
    ctx->tev.clear();
    for (auto& e : ctx->stage_ev) e.reset();
    release(ctx->host_render_done, ctx->sizing_done, ctx->ev_begin, ctx->ev_end, ctx->ray_filled, ctx->vol_traced,
            ctx->sirt_done, ctx->vox_scattered, ctx->vox_pose_ev);
    lap(3);
    delete ctx;                        // (an owner not named above goes here, untimed)
}

const char* xrt_last_error(const xrt_context* ctx)
{
    return ctx ? ctx->error.c_str() : g_create_error.c_str();
}

// The materials model's device table from the scene's mesh sizes and the
// coefficients, when both are set for the same number of meshes (a render
// checks that they are).  No frame is in flight (the callers synchronise).
static int upload_materials(xrt_context* ctx)
{
    const size_t M = ctx->mesh_tris.size();
    if (M == 0 || ctx->materials_mu.size() != M) return XRT_OK;
    MeshMaterial tab[XRT_MAX_MESHES];
    uint64_t end = 0;
    for (size_t m = 0; m < M; ++m) {
        end += ctx->mesh_tris[m];
        tab[m].end = (uint32_t)end;
        tab[m].mu = ctx->materials_mu[m];
    }
    if (ctx->d_materials.reserve(XRT_MAX_MESHES) != hipSuccess)
        return fail(ctx, XRT_ERR_DEVICE, "materials table allocation failed");
    XRT_HIP(ctx, hipMemcpy(ctx->d_materials.get(), tab, M * sizeof(MeshMaterial), hipMemcpyHostToDevice));
    return XRT_OK;
}

// The spectrum model's device table, likewise: the id ranges, the weights,
// the miss value (the weight chain, in the kernels' order) and the coefficients.
static int upload_spectrum(xrt_context* ctx)
{
    const size_t M = ctx->mesh_tris.size(), K = ctx->spectrum_weight.size();
    if (M == 0 || K == 0 || ctx->spectrum_meshes != M) return XRT_OK;
    SpectrumTable tab = {};
    uint64_t end = 0;
    for (size_t m = 0; m < M; ++m) {
        end += ctx->mesh_tris[m];
        tab.end[m] = (uint32_t)end;
    }
    std::copy(ctx->spectrum_weight.begin(), ctx->spectrum_weight.end(), tab.weight);
    std::copy(ctx->spectrum_mu.begin(), ctx->spectrum_mu.end(), tab.mu);
    tab.num_bins = (uint32_t)K;
    tab.miss = spectrum_miss(tab.weight, tab.num_bins);
    if (ctx->d_spectrum.reserve(1) != hipSuccess)
        return fail(ctx, XRT_ERR_DEVICE, "spectrum table allocation failed");
    XRT_HIP(ctx, hipMemcpy(ctx->d_spectrum.get(), &tab, sizeof tab, hipMemcpyHostToDevice));
    return XRT_OK;
}

// The paths model's: the id-range ends alone, whichever model is selected, so
// that a scene uploaded after xrt_set_paths renders without another call.
static int upload_path_ends(xrt_context* ctx)
{
    const size_t M = ctx->mesh_tris.size();
    if (M == 0 || M > kMaxMeshes) return XRT_OK;
    uint32_t ends[kMaxMeshes] = {};
    uint64_t end = 0;
    for (size_t m = 0; m < M; ++m) {
        end += ctx->mesh_tris[m];
        ends[m] = (uint32_t)end;
    }
    if (ctx->d_path_ends.reserve(kMaxMeshes) != hipSuccess)
        return fail(ctx, XRT_ERR_DEVICE, "paths table allocation failed");
    XRT_HIP(ctx, hipMemcpy(ctx->d_path_ends.get(), ends, sizeof ends, hipMemcpyHostToDevice));
    return XRT_OK;
}

// Every model's table (a scene upload changes the id ranges of each).
static int upload_tables(xrt_context* ctx)
{
    int rc = upload_materials(ctx);
    if (!rc) rc = upload_spectrum(ctx);
    return rc ? rc : upload_path_ends(ctx);
}

int xrt_upload_scene(xrt_context* ctx, const float* triangles, const uint64_t* mesh_triangles,
                     uint32_t num_meshes)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_meshes < 1 || num_meshes > XRT_MAX_MESHES)
        return fail(ctx, XRT_ERR_ARGUMENT, "a scene has 1 to XRT_MAX_MESHES meshes");
    if (!mesh_triangles) return fail(ctx, XRT_ERR_ARGUMENT, "mesh_triangles is NULL");
    uint64_t num_triangles = 0;
    for (uint32_t m = 0; m < num_meshes; ++m) {
        if (mesh_triangles[m] > 0xFFFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many triangles");
        num_triangles += mesh_triangles[m];
    }
    if (num_triangles && !triangles) return fail(ctx, XRT_ERR_ARGUMENT, "triangles is NULL");
    // (ids are 32 bits, and 0xFFFFFFFF marks an empty hit slot)
    if (num_triangles >= 0xFFFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many triangles");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);                   // frames in flight read the mesh (prep stream)
    if (rc) return rc;
    rc = ensure(ctx, ctx->d_tris, 9 * num_triangles);
    if (rc) return rc;
    if (num_triangles)
        XRT_HIP(ctx, hipMemcpy(ctx->d_tris.get(), triangles, 9 * num_triangles * sizeof(float),
                               hipMemcpyHostToDevice));
    ctx->num_tris = num_triangles;
    ctx->mesh_tris.assign(mesh_triangles, mesh_triangles + num_meshes);
    ++ctx->mesh_gen;
    ++ctx->state_gen;
    ctx->poses.clear();                 // a new scene is at rest
    ctx->posed_written.clear();
    return upload_tables(ctx);
}

int xrt_upload_mesh(xrt_context* ctx, const float* triangles, uint64_t num_triangles)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_triangles && !triangles) return fail(ctx, XRT_ERR_ARGUMENT, "triangles is NULL");
    if (num_triangles > 0xFFFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many triangles");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);                   // frames in flight read the mesh (prep stream)
    if (rc) return rc;
    rc = ensure(ctx, ctx->d_tris, 9 * num_triangles);
    if (rc) return rc;
    if (num_triangles)
        XRT_HIP(ctx, hipMemcpy(ctx->d_tris.get(), triangles, 9 * num_triangles * sizeof(float),
                               hipMemcpyHostToDevice));
    ctx->num_tris = num_triangles;
    ctx->mesh_tris.assign(1, num_triangles);      // a one-mesh scene
    ++ctx->mesh_gen;
    ++ctx->state_gen;
    ctx->poses.clear();                 // a new scene is at rest
    ctx->posed_written.clear();
    return upload_tables(ctx);
}

int xrt_mesh_bbox(const float* tris, uint64_t n, float lower[3], float upper[3])
{
    if ((n && !tris) || !lower || !upper) return XRT_ERR_ARGUMENT;
    const float inf = std::numeric_limits<float>::infinity();
    for (int k = 0; k < 3; ++k) {
        lower[k] = inf;
        upper[k] = -inf;
    }
    // TriangleMesh::computeBoundingBox, src/TriangleMesh.cxx:200-227 (p1, p2, p3 in turn)
    for (uint64_t i = 0; i < n; ++i)
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                float x = tris[9 * i + 3 * v + k];
                lower[k] = stdmin(lower[k], x);
                upper[k] = stdmax(upper[k], x);
            }
    return XRT_OK;
}

int xrt_scene_bbox(const float* tris, const uint64_t* mesh_triangles, uint32_t num_meshes, float lower[3],
                   float upper[3])
{
    if ((num_meshes && !mesh_triangles) || !lower || !upper) return XRT_ERR_ARGUMENT;
    const float inf = std::numeric_limits<float>::infinity();
    for (int k = 0; k < 3; ++k) {
        lower[k] = inf;
        upper[k] = -inf;
    }
    // getBBox, src/main.cxx:545-562: the corners of each mesh's box in turn
    uint64_t first = 0;
    for (uint32_t m = 0; m < num_meshes; ++m) {
        float lo[3], hi[3];
        const uint64_t n = mesh_triangles[m];
        if (n && !tris) return XRT_ERR_ARGUMENT;
        xrt_mesh_bbox(n ? tris + 9 * first : nullptr, n, lo, hi);
        for (int k = 0; k < 3; ++k) {
            lower[k] = stdmin(lower[k], lo[k]);
            upper[k] = stdmax(upper[k], hi[k]);
        }
        first += n;
    }
    return XRT_OK;
}

int xrt_camera_from_bbox(const float lower[3], const float upper[3], uint32_t width,
                         uint32_t height, xrt_camera* out)
{
    if (!lower || !upper || !out || !width || !height) return XRT_ERR_ARGUMENT;
    // initialiseRayTracing, src/main.cxx:575-604
    float range[3] = {upper[0] - lower[0], upper[1] - lower[1], upper[2] - lower[2]};
    float centre[3];
    for (int k = 0; k < 3; ++k) centre[k] = lower[k] + (float)((double)range[k] / 2.0);
    float diagonal = length3(range);
    float up[3] = {0.0f, 0.0f, -1.0f};
    float origin[3] = {centre[0] - diagonal * 1, centre[1] - 0.0f, centre[2] - 0.0f};
    float xoff = (float)((double)diagonal * 0.6);
    float detector[3] = {centre[0] + xoff, centre[1] + 0.0f, centre[2] + 0.0f};
    float direction[3] = {detector[0] - origin[0], detector[1] - origin[1], detector[2] - origin[2]};
    normalise3(direction);
    normalise3(direction);
    float right[3];
    cross3(direction, up, right);
    // renderLoop prologue, src/main.cxx:637-641
    float res1 = range[2] / (float)width;
    float res2 = range[1] / (float)height;
    float spacing = 2 * stdmax(res1, res2);
    std::memcpy(out->origin, origin, sizeof origin);
    std::memcpy(out->detector, detector, sizeof detector);
    std::memcpy(out->up, up, sizeof up);
    std::memcpy(out->right, right, sizeof right);
    out->pixel_spacing = spacing;
    out->width = width;
    out->height = height;
    return XRT_OK;
}

int xrt_set_kernel(xrt_context* ctx, int kernel)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (kernel < XRT_KERNEL_AUTO || kernel > XRT_KERNEL_BINNED)
        return fail(ctx, XRT_ERR_ARGUMENT, "unknown kernel");
    ctx->kernel = kernel;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_set_model(xrt_context* ctx, int model, float mu)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (model != XRT_MODEL_ATTENUATION && model != XRT_MODEL_SIGNED)
        return fail(ctx, XRT_ERR_ARGUMENT, "unknown model");
    ctx->model = (uint32_t)model;
    ctx->mu = mu;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_set_materials(xrt_context* ctx, const float* mu, uint32_t num_meshes)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_meshes < 1 || num_meshes > XRT_MAX_MESHES)
        return fail(ctx, XRT_ERR_ARGUMENT, "1 to XRT_MAX_MESHES coefficients");
    if (!mu) return fail(ctx, XRT_ERR_ARGUMENT, "mu is NULL");
    for (uint32_t m = 0; m < num_meshes; ++m)
        if (!std::isfinite(mu[m]) || mu[m] < 0.0f)
            return fail(ctx, XRT_ERR_ARGUMENT, "a coefficient must be finite and >= 0");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);                   // frames in flight read the table
    if (rc) return rc;
    ctx->model = kModelMaterials;
    ctx->materials_mu.assign(mu, mu + num_meshes);
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return upload_materials(ctx);
}

// The argument checks of xrt_set_spectrum (spectrum_arguments; no device needed) and the host pieces of the
// spectral detector, which rest on them.
#include "xrt_detector_host.inc"

int xrt_set_spectrum(xrt_context* ctx, const float* weight, const float* mu, uint32_t num_meshes,
                     uint32_t num_bins)
{
    // (the table's checks first: they need no context, and without one their message is xrt_last_error(NULL)'s)
    if (const char* why = spectrum_arguments(weight, mu, num_meshes, num_bins))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);                   // frames in flight read the table
    if (rc) return rc;
    ctx->model = kModelSpectrum;
    ctx->spectrum_weight.assign(weight, weight + num_bins);
    ctx->spectrum_mu.assign(mu, mu + (size_t)num_meshes * num_bins);
    ctx->spectrum_meshes = num_meshes;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return upload_spectrum(ctx);
}

int xrt_set_paths(xrt_context* ctx)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    ctx->model = kModelPaths;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

// Records a pose change: waits for the frames in flight (their k_prep reads the
// soup the next k_pose rewrites) and drops the frames prepared ahead.  A pose
// whose bits do not change is no change: no wait, no new generation.
static int change_poses(xrt_context* ctx, std::vector<xrt_context::Pose> poses)
{
    bool rest = true;
    for (const xrt_context::Pose& q : poses) rest = rest && same_pose(q, kIdentityPose);
    if (rest) poses.clear();
    if (poses.size() == ctx->poses.size() &&
        std::equal(poses.begin(), poses.end(), ctx->poses.begin(), same_pose))
        return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);
    if (rc) return rc;
    ctx->poses.swap(poses);
    ++ctx->pose_gen;                    // BinKey::same: another geometry over the same layout
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_set_pose(xrt_context* ctx, uint32_t mesh, const float pose[12])
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (mesh >= ctx->mesh_tris.size())
        return fail(ctx, XRT_ERR_ARGUMENT, "mesh " + std::to_string(mesh) + " is not a mesh of the scene (" +
                                               std::to_string(ctx->mesh_tris.size()) + " meshes)");
    xrt_context::Pose q = kIdentityPose;
    if (pose) std::memcpy(q.data(), pose, sizeof q);
    for (float v : q)
        if (!std::isfinite(v)) return fail(ctx, XRT_ERR_ARGUMENT, "a pose value must be finite");
    std::vector<xrt_context::Pose> poses = ctx->poses;
    if (poses.empty()) poses.assign(ctx->mesh_tris.size(), kIdentityPose);
    poses[mesh] = q;
    return change_poses(ctx, std::move(poses));
}

int xrt_reset_poses(xrt_context* ctx)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    return change_poses(ctx, {});
}

#include "xrt_pose_host.inc"

int xrt_debug_posed_triangles(xrt_context* ctx, float* dst, uint64_t capacity_floats, uint64_t* n_floats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    const uint64_t n = 9 * ctx->num_tris;
    if (n_floats) *n_floats = n;
    if (!dst) return XRT_OK;
    if (capacity_floats < n) return fail(ctx, XRT_ERR_ARGUMENT, "dst is smaller than the soup");
    if (!n) return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const float* soup = nullptr;
    int rc = render_soup(ctx, soup);              // k_pose, if one is due
    if (rc) return rc;
    XRT_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    XRT_HIP(ctx, hipMemcpy(dst, soup, n * sizeof(float), hipMemcpyDeviceToHost));
    return XRT_OK;
}

int xrt_debug_pose_span(xrt_context* ctx, uint32_t launches, double* us_per_write)
{
    if (!ctx || !us_per_write || !launches) return XRT_ERR_ARGUMENT;
    if (ctx->poses.empty()) return fail(ctx, XRT_ERR_ARGUMENT, "no pose is set");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);
    if (rc) return rc;
    const float* soup = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    XRT_HIP(ctx, hipEventCreate(&t0));
    XRT_HIP(ctx, hipEventCreate(&t1));
    ctx->posed_written.clear();
    rc = render_soup(ctx, soup);                  // (allocation and first touch outside the span)
    if (!rc) rc = hipEventRecord(t0, ctx->prep_stream) == hipSuccess ? XRT_OK : XRT_ERR_DEVICE;
    for (uint32_t k = 0; k < launches && !rc; ++k) {
        ctx->posed_written.clear();               // every mesh due again
        rc = render_soup(ctx, soup);
    }
    float ms = 0.0f;
    if (!rc && (hipEventRecord(t1, ctx->prep_stream) != hipSuccess || hipEventSynchronize(t1) != hipSuccess ||
                hipEventElapsedTime(&ms, t0, t1) != hipSuccess))
        rc = fail(ctx, XRT_ERR_DEVICE, "pose span: events failed");
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    *us_per_write = (double)ms * 1e3 / launches;
    return rc;
}

int xrt_debug_pose_counters(xrt_context* ctx, uint64_t counters[2])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_pose_launches;
    counters[1] = ctx->hp_pose_tris;
    return XRT_OK;
}

// The checks both paths renders share.
static int paths_arguments(xrt_context* ctx, uint32_t num_meshes, const float* paths)
{
    if (ctx->model != kModelPaths) return fail(ctx, XRT_ERR_ARGUMENT, "xrt_render_paths needs xrt_set_paths");
    if (num_meshes == 0 || num_meshes != ctx->mesh_tris.size())
        return fail(ctx, XRT_ERR_ARGUMENT, "num_meshes differs from the scene's mesh count");
    if (!paths) return fail(ctx, XRT_ERR_ARGUMENT, "paths is NULL");
    return XRT_OK;
}

int xrt_render_paths_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                            uint32_t num_meshes, float* d_paths, uint16_t* d_open, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (int rc = paths_arguments(ctx, num_meshes, d_paths)) return rc;
    return enqueue_render(ctx, camera, row_begin, row_end, nullptr, d_paths, reinterpret_cast<uint8_t*>(d_open),
                          (hipStream_t)stream, true, true);
}

int xrt_render_paths(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                     uint32_t num_meshes, float* paths, uint16_t* open, xrt_stats* stats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    int rc = check_camera(ctx, camera, row_begin, row_end);
    if (rc) return rc;
    if ((rc = paths_arguments(ctx, num_meshes, paths))) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)(row_end - row_begin) * camera->width;
    // the planes in the context's L-buffer staging, the masks in its 8-bit one (2 bytes a pixel)
    if ((rc = stage_planes(ctx, n * std::max<size_t>(num_meshes, sizeof(uint16_t))))) return rc;
    uint16_t* d_open = open ? reinterpret_cast<uint16_t*>(ctx->d_u8.get()) : nullptr;
    // (not prepared ahead: a host-buffer call, as xrt_render_rows)
    if ((rc = enqueue_render(ctx, camera, row_begin, row_end, nullptr, ctx->d_lbuffer.get(),
                             reinterpret_cast<uint8_t*>(d_open), ctx->host_stream, false, true)))
        return rc;
    std::vector<D2HCopy> copies;
    if (n) {
        copies.push_back({paths, ctx->d_lbuffer.get(), n * num_meshes * sizeof(float)});
        if (open) copies.push_back({open, d_open, n * sizeof(uint16_t)});
    }
    if ((rc = d2h_copy(ctx, ctx->host_stream, copies))) return rc;
    xrt_stats local;
    return xrt_read_stats(ctx, stats ? stats : &local);
}

// The launch of k_apply_spectrum (validated arguments, device pointers).
static int launch_apply_spectrum(xrt_context* ctx, uint64_t n, uint32_t num_meshes, const float* d_paths,
                                 const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                                 float* d_lbuffer, hipStream_t stream)
{
    SpectrumTable tab = {};             // by value: the launch owns its copy (no context state, no wait)
    std::copy(weight, weight + num_bins, tab.weight);
    std::copy(mu, mu + (size_t)num_meshes * num_bins, tab.mu);
    tab.num_bins = num_bins;
    tab.miss = spectrum_miss(tab.weight, num_bins);
    hipLaunchKernelGGL(k_apply_spectrum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_paths, d_open,
                       (size_t)n, num_meshes, tab, d_lbuffer);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

// The checks both apply entries share, the table's first (no context needed).
static int apply_arguments(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* paths,
                           const float* weight, const float* mu, uint32_t num_bins, const float* lbuffer)
{
    if (const char* why = spectrum_arguments(weight, mu, num_meshes, num_bins))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_pixels > (1ull << 38)) return fail(ctx, XRT_ERR_ARGUMENT, "too many pixels");
    if (num_pixels && (!paths || !lbuffer)) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    return XRT_OK;
}

int xrt_apply_spectrum_device(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* d_paths,
                              const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                              float* d_lbuffer, void* stream)
{
    int rc = apply_arguments(ctx, num_pixels, num_meshes, d_paths, weight, mu, num_bins, d_lbuffer);
    if (rc || !num_pixels) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_apply_spectrum(ctx, num_pixels, num_meshes, d_paths, d_open, weight, mu, num_bins, d_lbuffer,
                                 (hipStream_t)stream);
}

int xrt_apply_spectrum(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* paths,
                       const uint16_t* open, const float* weight, const float* mu, uint32_t num_bins,
                       float* lbuffer)
{
    int rc = apply_arguments(ctx, num_pixels, num_meshes, paths, weight, mu, num_bins, lbuffer);
    if (rc || !num_pixels) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)num_pixels;
    DeviceScratch s(ctx, ctx->host_stream, "apply");
    const float* dp = s.upload(paths, n * num_meshes);
    const uint16_t* dopen = s.upload(open, n);
    float* dl = s.alloc<float>(n);
    if (s.rc()) return s.rc();
    if ((rc = launch_apply_spectrum(ctx, n, num_meshes, dp, dopen, weight, mu, num_bins, dl, ctx->host_stream))) return rc;
    s.download(lbuffer, dl, n);
    return s.finish();
}

// --- the spectral detector -----------------------------------

// The launch of k_spectral_detector (validated arguments, device pointers): the instantiation of the smallest
// mesh and channel bounds that hold num_meshes and num_channels, and of the draw mode.
static int launch_spectral_detector(xrt_context* ctx, uint64_t n, uint32_t num_meshes, const float* d_paths,
                                    const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                                    const float* response, uint32_t num_channels, float gain, float read_noise,
                                    uint64_t seed, uint64_t first_index, int draw_mode, int out_mode, float* d_out,
                                    hipStream_t stream)
{
    DetectorSpectrum tab;               // both tables by value: the launch owns its copies (no context state, no wait)
    DetectorTable det;
    detector_tables(weight, mu, num_meshes, num_bins, response, num_channels, gain, read_noise, draw_mode, out_mode, &tab,
                    &det);
    det.open = d_open;
    det.out = d_out;
    det.plane = n;
    det.seed = seed;
    const dim3 grid((unsigned)((n + kDetectorThreads - 1u) / kDetectorThreads)), block(kDetectorThreads);
    const bool noisy = draw_mode == XRT_DETECT_NOISY;
#define XRT_DETECT_LAUNCH(C, NOISY)                                                                              \
    do {                                                                                                         \
        if (num_meshes <= kDetectorFewMeshes)                                                                    \
            hipLaunchKernelGGL((k_spectral_detector<kDetectorFewMeshes, C, NOISY>), grid, block, 0, stream, d_paths, \
                               d_open, (size_t)n, num_meshes, tab, det, seed, first_index);                      \
        else                                                                                                     \
            hipLaunchKernelGGL((k_spectral_detector<kMaxMeshes, C, NOISY>), grid, block, 0, stream, d_paths, d_open, \
                               (size_t)n, num_meshes, tab, det, seed, first_index);                              \
    } while (0)
    if (num_channels <= 1u) {
        if (noisy) XRT_DETECT_LAUNCH(1, true); else XRT_DETECT_LAUNCH(1, false);
    } else if (num_channels <= 4u) {
        if (noisy) XRT_DETECT_LAUNCH(4, true); else XRT_DETECT_LAUNCH(4, false);
    } else {
        if (noisy) XRT_DETECT_LAUNCH(8, true); else XRT_DETECT_LAUNCH(8, false);
    }
#undef XRT_DETECT_LAUNCH
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_spectral_detector_device(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* d_paths,
                                 const uint16_t* d_open, const float* weight, const float* mu, uint32_t num_bins,
                                 const float* response, uint32_t num_channels, float gain, float read_noise,
                                 uint64_t seed, uint64_t first_index, int draw_mode, int out_mode, float* d_out,
                                 void* stream)
{
    if (const char* why = detector_arguments(num_pixels, num_meshes, d_paths, d_open, weight, mu, num_bins, response,
                                             num_channels, gain, read_noise, first_index, draw_mode, out_mode, d_out))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_spectral_detector(ctx, num_pixels, num_meshes, d_paths, d_open, weight, mu, num_bins, response,
                                    num_channels, gain, read_noise, seed, first_index, draw_mode, out_mode, d_out,
                                    (hipStream_t)stream);
}

int xrt_spectral_detector(xrt_context* ctx, uint64_t num_pixels, uint32_t num_meshes, const float* paths,
                          const uint16_t* open, const float* weight, const float* mu, uint32_t num_bins,
                          const float* response, uint32_t num_channels, float gain, float read_noise, uint64_t seed,
                          uint64_t first_index, int draw_mode, int out_mode, float* out)
{
    if (const char* why = detector_arguments(num_pixels, num_meshes, paths, open, weight, mu, num_bins, response,
                                             num_channels, gain, read_noise, first_index, draw_mode, out_mode, out))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)num_pixels;
    DeviceScratch s(ctx, ctx->host_stream, "spectral detector");
    const float* dp = s.upload(paths, n * num_meshes);
    const uint16_t* dopen = s.upload(open, n);
    float* dout = s.alloc<float>(n * num_channels);
    if (s.rc()) return s.rc();
    if (int rc = launch_spectral_detector(ctx, n, num_meshes, dp, dopen, weight, mu, num_bins, response, num_channels,
                                          gain, read_noise, seed, first_index, draw_mode, out_mode, dout,
                                          ctx->host_stream))
        return rc;
    s.download(out, dout, n * num_channels);
    return s.finish();
}

// --- voxel phantoms -----------------------------------------

#include "xrt_volume_host.inc"

// Frees the context's volume once its last trace is through.
static int free_volume(xrt_context* ctx)
{
    XRT_HIP(ctx, ctx->vol_traced.wait());
    ctx->vol_labels.reset();
    ctx->vol_density.reset();
    ctx->vol = VolumeDesc{};
    return XRT_OK;
}

int xrt_upload_volume(xrt_context* ctx, const uint8_t* labels, const float* density, const uint32_t dims[3],
                      const float origin[3], const float spacing[3], uint32_t num_labels)
{
    const bool release = !labels || num_labels == 0;
    if (!release) {
        const std::string why = volume_arguments(labels, density, dims, origin, spacing, num_labels);
        if (!why.empty()) return fail(ctx, XRT_ERR_ARGUMENT, why);
    }
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = free_volume(ctx)) return rc;
    if (release) return XRT_OK;
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    hipError_t e = ctx->vol_labels.reserve(n);
    if (e == hipSuccess && density) e = ctx->vol_density.reserve(n);
    if (e == hipSuccess) e = hipMemcpy(ctx->vol_labels.get(), labels, n, hipMemcpyHostToDevice);
    if (e == hipSuccess && density) e = hipMemcpy(ctx->vol_density.get(), density, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->vol_labels.reset();
        ctx->vol_density.reset();
        (void)hipGetLastError();
        return fail(ctx, XRT_ERR_DEVICE, std::string("xrt_upload_volume: ") + hipGetErrorString(e));
    }
    ctx->vol = volume_desc(ctx->vol_labels.get(), ctx->vol_density.get(), dims, origin, spacing, num_labels);
    return XRT_OK;
}

// The checks both traces share, the arguments' first (no context needed).
static int volume_paths_arguments(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                                  uint32_t num_labels, const float* paths)
{
    if (const char* why = volume_trace_arguments(camera, row_begin, row_end, num_labels, paths))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (!ctx->vol.labels) return fail(ctx, XRT_ERR_NO_MESH, "no volume uploaded (xrt_upload_volume)");
    if (num_labels != ctx->vol.num_labels)
        return fail(ctx, XRT_ERR_ARGUMENT, "num_labels differs from the uploaded volume's");
    return XRT_OK;
}

// The launch of k_volume_paths (validated arguments, a strip of at least one row): the instantiation of the
// smallest label bound that holds the volume's.
static int launch_volume_paths(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                               float* d_paths, hipStream_t stream)
{
    const RenderParams p = volume_params(*camera, row_begin, row_end);
    const uint32_t shift = ctx->vol_tile_shift, tw = 1u << shift, th = 64u >> shift;
    const uint64_t tiles_x = ((uint64_t)p.width + tw - 1u) / tw;
    const uint64_t tiles_y = ((uint64_t)(row_end - row_begin) + th - 1u) / th;
    // (8 x 8 tiles: at most 2^32 / 64 tiles and a ragged edge's; only the row-shaped debug leg can exceed a launch)
    if (tiles_x * tiles_y > 0x7FFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "the strip needs more than 2^31 - 1 workgroups");
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(64);
    const uint32_t M = ctx->vol.num_labels;
    if (M <= 1u)
        hipLaunchKernelGGL((k_volume_paths<1u>), grid, block, 0, stream, p, ctx->vol, (uint32_t)tiles_x, shift, d_paths);
    else if (M <= kVolumeFewLabels)
        hipLaunchKernelGGL((k_volume_paths<kVolumeFewLabels>), grid, block, 0, stream, p, ctx->vol, (uint32_t)tiles_x,
                           shift, d_paths);
    else
        hipLaunchKernelGGL((k_volume_paths<kMaxMeshes>), grid, block, 0, stream, p, ctx->vol, (uint32_t)tiles_x, shift,
                           d_paths);
    XRT_HIP(ctx, hipGetLastError());
    XRT_HIP(ctx, ctx->vol_traced.record(stream));
    return XRT_OK;
}

int xrt_debug_volume_wave_shape(xrt_context* ctx, int rows)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    ctx->vol_tile_shift = rows ? 6u : kVolumeTileShift;
    return XRT_OK;
}

int xrt_volume_paths_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                            uint32_t num_labels, float* d_paths, void* stream)
{
    int rc = volume_paths_arguments(ctx, camera, row_begin, row_end, num_labels, d_paths);
    if (rc || row_begin == row_end) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_volume_paths(ctx, camera, row_begin, row_end, d_paths, (hipStream_t)stream);
}

int xrt_volume_paths(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                     uint32_t num_labels, float* paths)
{
    int rc = volume_paths_arguments(ctx, camera, row_begin, row_end, num_labels, paths);
    if (rc || row_begin == row_end) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)(row_end - row_begin) * camera->width * num_labels;
    DeviceScratch s(ctx, ctx->host_stream, "volume paths");
    float* dp = s.alloc<float>(n);
    if (s.rc()) return s.rc();
    if ((rc = launch_volume_paths(ctx, camera, row_begin, row_end, dp, ctx->host_stream))) return rc;
    s.download(paths, dp, n);
    return s.finish();
}

// --- FDK reconstruction ----------------------------------------

#include "xrt_fdk_host.inc"

// The launch of k_fdk_filter (validated arguments, device pointers).
static int launch_fdk_filter(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                             const float* d_weight, const float* d_taps, uint32_t num_taps, float* d_out,
                             hipStream_t stream)
{
    if (num_taps >= 2u * width - 1u) {   // a table as long as a ramp's: every lane at the same pixel, W steps an output
        const uint32_t segments = (width + kWideSegment - 1u) / kWideSegment;
        const uint64_t rows = (uint64_t)height * num_planes;
        const size_t lds = fdk_wide_lds_bytes(width);
        if (lds > 64u * 1024u)          // past the default limit of a launch's dynamic LDS
            XRT_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fdk_filter_wide),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_fdk_filter_wide, dim3((unsigned)((rows + 1u) / 2u * segments)), dim3(kWideThreads), lds, stream,
                           d_image, d_weight, d_taps, d_out, width, height, rows, num_taps, segments);
        XRT_HIP(ctx, hipGetLastError());
        return XRT_OK;
    }
    const uint32_t segments = (width + kFilterSegment - 1u) / kFilterSegment;
    const uint64_t blocks = (uint64_t)height * num_planes * segments;
    hipLaunchKernelGGL(k_fdk_filter, dim3((unsigned)blocks), dim3(kFilterThreads), 0, stream, d_image, d_weight, d_taps,
                       d_out, width, height, num_taps, segments);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_fdk_filter_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                          const float* d_weight, const float* d_taps, uint32_t num_taps, float* d_out, void* stream)
{
    if (const char* why = fdk_filter_arguments(width, height, num_planes, d_image, d_weight, d_taps, num_taps, d_out, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_fdk_filter(ctx, width, height, num_planes, d_image, d_weight, d_taps, num_taps, d_out,
                             (hipStream_t)stream);
}

int xrt_fdk_filter(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                   const float* weight, const float* taps, uint32_t num_taps, float* out)
{
    if (const char* why = fdk_filter_arguments(width, height, num_planes, image, weight, taps, num_taps, out, true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t plane = (size_t)width * height, all = plane * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "FDK filter");
    const float* din = s.upload(image, all);
    const float* dweight = s.upload(weight, plane);
    const float* dtaps = s.upload(taps, (size_t)num_taps);
    float* dout = s.alloc<float>(all);
    if (s.rc()) return s.rc();
    if (int rc = launch_fdk_filter(ctx, width, height, num_planes, din, dweight, dtaps, num_taps, dout, ctx->host_stream))
        return rc;
    s.download(out, dout, all);
    return s.finish();
}

// The launch of k_backproject (validated arguments, device pointers, a slab range that is not empty).
static int launch_backproject(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                              const double* d_matrices, const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end,
                              double scale, int accumulate, float* d_volume, hipStream_t stream)
{
    const uint32_t spans = (dims[0] + kBackprojectSpan - 1u) / kBackprojectSpan;
    const uint64_t rows = (uint64_t)(slab_end - slab_begin) * dims[1];
    const uint64_t waves = rows * spans, per_block = kBackprojectThreads / 64u;
    hipLaunchKernelGGL(k_backproject, dim3((unsigned)((waves + per_block - 1u) / per_block)), dim3(kBackprojectThreads), 0,
                       stream, d_proj, d_matrices, width, height, num_planes, dims[0], dims[1], slab_begin, rows, spans,
                       scale, (uint32_t)(accumulate != 0), d_volume);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_backproject_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                           const double* d_matrices, const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end,
                           double scale, int accumulate, float* d_volume, void* stream)
{
    if (const char* why = backproject_arguments(width, height, num_planes, d_proj, d_matrices, dims, slab_begin, slab_end,
                                                scale, d_volume, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (slab_begin == slab_end) return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_backproject(ctx, width, height, num_planes, d_proj, d_matrices, dims, slab_begin, slab_end, scale,
                              accumulate, d_volume, (hipStream_t)stream);
}

int xrt_backproject(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                    const double* matrices, const uint32_t dims[3], uint32_t slab_begin, uint32_t slab_end, double scale,
                    int accumulate, float* volume)
{
    if (const char* why = backproject_arguments(width, height, num_planes, proj, matrices, dims, slab_begin, slab_end,
                                                scale, volume, true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (slab_begin == slab_end) return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t all = (size_t)width * height * num_planes;
    const size_t voxels = (size_t)(slab_end - slab_begin) * dims[1] * dims[0];
    DeviceScratch s(ctx, ctx->host_stream, "backprojection");
    const float* dproj = s.upload(proj, all);
    const double* dmat = s.upload(matrices, (size_t)num_planes * 12u);
    float* dvol = accumulate ? s.upload(volume, voxels) : s.alloc<float>(voxels);
    if (s.rc()) return s.rc();
    if (int rc = launch_backproject(ctx, width, height, num_planes, dproj, dmat, dims, slab_begin, slab_end, scale,
                                    accumulate, dvol, ctx->host_stream))
        return rc;
    s.download(volume, dvol, voxels);
    return s.finish();
}

// --- SIRT / OS-SART ---------------------------------------------

#include "xrt_sirt_host.inc"

// The launch of k_forward_project (validated arguments, device pointers); plane p's measurement lies at
// d_meas + p * meas_stride.
static int launch_forward_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                  const float* d_volume, const uint32_t dims[3], const float spacing[3],
                                  const double* d_rays, int mode, const float* d_meas, uint64_t meas_stride, float* d_out,
                                  hipStream_t stream)
{
    const uint32_t tiles_x = (width + kForwardTile - 1u) / kForwardTile, tiles_y = (height + kForwardTile - 1u) / kForwardTile;
    hipLaunchKernelGGL(k_forward_project, dim3(tiles_x * tiles_y, num_planes), dim3(64), 0, stream, d_volume, d_rays, d_meas,
                       meas_stride, d_out, dims[0], dims[1], dims[2], (double)spacing[0], (double)spacing[1],
                       (double)spacing[2], width, height, tiles_x, mode);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_forward_project_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                               const float* d_volume, const uint32_t dims[3], const float spacing[3], const double* d_rays,
                               int mode, const float* d_meas, float* d_out, void* stream)
{
    if (const char* why = forward_project_arguments(width, height, num_planes, d_volume, dims, spacing, d_rays, mode, d_meas,
                                                    d_out, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_forward_project(ctx, width, height, num_planes, d_volume, dims, spacing, d_rays, mode, d_meas,
                                  (uint64_t)width * height, d_out, (hipStream_t)stream);
}

int xrt_forward_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                        const uint32_t dims[3], const float spacing[3], const double* rays, int mode, const float* meas,
                        float* out)
{
    if (const char* why = forward_project_arguments(width, height, num_planes, volume, dims, spacing, rays, mode, meas, out,
                                                    true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t all = (size_t)width * height * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "forward projection");
    const float* dvol = s.upload(volume, (size_t)dims[0] * dims[1] * dims[2]);
    const double* drays = s.upload(rays, (size_t)num_planes * 12u);
    const float* dmeas = mode == XRT_FP_RESIDUAL ? s.upload(meas, all) : nullptr;
    float* dout = s.alloc<float>(all);
    if (s.rc()) return s.rc();
    if (int rc = launch_forward_project(ctx, width, height, num_planes, dvol, dims, spacing, drays, mode, dmeas,
                                        (uint64_t)width * height, dout, ctx->host_stream))
        return rc;
    s.download(out, dout, all);
    return s.finish();
}

static int launch_volume_update(xrt_context* ctx, uint64_t n, float* d_x, const float* d_corr, const float* d_norm,
                                double relax, float lo, float hi, hipStream_t stream)
{
    const uint64_t blocks = std::min<uint64_t>((n + kUpdateThreads - 1u) / kUpdateThreads, kUpdateBlocks);
    hipLaunchKernelGGL(k_volume_update, dim3((unsigned)blocks), dim3(kUpdateThreads), 0, stream, n, d_x, d_corr, d_norm,
                       relax, lo, hi);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_volume_update_device(xrt_context* ctx, uint64_t n, float* d_x, const float* d_corr, const float* d_norm,
                             double relax, float lo, float hi, void* stream)
{
    if (const char* why = volume_update_arguments(n, d_x, d_corr, d_norm, relax, lo, hi)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_volume_update(ctx, n, d_x, d_corr, d_norm, relax, lo, hi, (hipStream_t)stream);
}

int xrt_volume_update(xrt_context* ctx, uint64_t n, float* x, const float* corr, const float* norm, double relax, float lo,
                      float hi)
{
    if (const char* why = volume_update_arguments(n, x, corr, norm, relax, lo, hi)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, ctx->host_stream, "volume update");
    float* dx = s.upload(x, (size_t)n);
    const float* dcorr = s.upload(corr, (size_t)n);
    const float* dnorm = s.upload(norm, (size_t)n);
    if (s.rc()) return s.rc();
    if (int rc = launch_volume_update(ctx, n, dx, dcorr, dnorm, relax, lo, hi, ctx->host_stream)) return rc;
    s.download(x, (const float*)dx, (size_t)n);
    return s.finish();
}

// --- TV-regularised SIRT ------------------------------------------

#include "xrt_tv_host.inc"

// The context's working set (d_sirt) for a call that needs `bytes` of it: the previous call's kernels and upload
// are done with it and it is large enough.  The caller marks sirt_done before it enqueues work on the set and
// records it behind its last.
static int sirt_working_set(xrt_context* ctx, size_t bytes)
{
    XRT_HIP(ctx, ctx->sirt_done.wait());
    ctx->vox_counters = false;                        // (the caller lays its own data over them)
    if (ctx->d_sirt.reserve(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, XRT_ERR_MEMORY, "the working set of " + std::to_string(bytes) + " bytes cannot be allocated");
    }
    return XRT_OK;
}

// The doubles that the sum of n entries needs for its partials: the first level's and the second's.
static size_t sumsq_partials(uint64_t n)
{
    const uint64_t m1 = sumsq_chunks(n);
    return (size_t)(m1 + sumsq_chunks(m1));
}

static int launch_tv_gradient(xrt_context* ctx, const float* d_x, const uint32_t dims[3], double eps, float* d_g,
                              hipStream_t stream)
{
    // at most 67 x 293 tiles and 64 chunks of 256 lanes: 2^28.3 work-items
    const uint32_t tiles_x = (dims[0] + kTvOwnX - 1u) / kTvOwnX, tiles_y = (dims[1] + kTvOwnY - 1u) / kTvOwnY;
    const uint32_t chunks = (dims[2] + kTvChunkZ - 1u) / kTvChunkZ;
    hipLaunchKernelGGL(k_tv_gradient, dim3(tiles_x * tiles_y, chunks), dim3(kTvThreads), 0, stream, d_x, d_g, dims[0], dims[1],
                       dims[2], tiles_x, eps);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

// *d_out = the sum of squares of the n entries of d_a (less d_b's), its levels' partials in d_partials
// (sumsq_partials(n) doubles).
static int launch_sumsq(xrt_context* ctx, uint64_t n, const float* d_a, const float* d_b, double* d_partials, double* d_out,
                        hipStream_t stream)
{
    uint64_t m = sumsq_chunks(n);
    double* level = d_partials;
    hipLaunchKernelGGL(k_sumsq_first, dim3((unsigned)m), dim3(kSumsqLanes), 0, stream, n, d_a, d_b, m == 1u ? d_out : level);
    XRT_HIP(ctx, hipGetLastError());
    while (m > 1u) {
        const uint64_t next = sumsq_chunks(m);
        hipLaunchKernelGGL(k_sumsq_next, dim3((unsigned)next), dim3(kSumsqLanes), 0, stream, m, (const double*)level,
                           next == 1u ? d_out : level + m);
        XRT_HIP(ctx, hipGetLastError());
        level += m;
        m = next;
    }
    return XRT_OK;
}

// xrt_tv_descend's steps on `stream`: d_g a volume's worth of floats, d_sums sumsq_partials(voxels) + 1 doubles
// (the partials, then G).  The step's length is `scale`, or scale * sqrt(*d_moved).
static int launch_tv_descend(xrt_context* ctx, float* d_x, const uint32_t dims[3], double eps, uint32_t steps, double scale,
                             const double* d_moved, float lo, float hi, float* d_g, double* d_sums, hipStream_t stream)
{
    const uint64_t voxels = (uint64_t)dims[0] * dims[1] * dims[2];
    double* d_G = d_sums + sumsq_partials(voxels);
    const uint64_t blocks = std::min<uint64_t>((voxels + kUpdateThreads - 1u) / kUpdateThreads, kUpdateBlocks);
    for (uint32_t s = 0; s < steps; ++s) {
        if (int rc = launch_tv_gradient(ctx, d_x, dims, eps, d_g, stream)) return rc;
        if (int rc = launch_sumsq(ctx, voxels, d_g, nullptr, d_sums, d_G, stream)) return rc;
        hipLaunchKernelGGL(k_tv_step, dim3((unsigned)blocks), dim3(kUpdateThreads), 0, stream, voxels, d_x, (const float*)d_g,
                           (const double*)d_G, scale, d_moved, lo, hi);
        XRT_HIP(ctx, hipGetLastError());
    }
    return XRT_OK;
}

int xrt_tv_gradient_device(xrt_context* ctx, const float* d_volume, const uint32_t dims[3], double eps, float* d_out,
                           void* stream)
{
    if (const char* why = tv_gradient_arguments(d_volume, dims, eps, d_out)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_tv_gradient(ctx, d_volume, dims, eps, d_out, (hipStream_t)stream);
}

int xrt_tv_gradient(xrt_context* ctx, const float* volume, const uint32_t dims[3], double eps, float* out)
{
    if (const char* why = tv_gradient_arguments(volume, dims, eps, out)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "TV gradient");
    const float* dvol = s.upload(volume, voxels);
    float* dout = s.alloc<float>(voxels);
    if (s.rc()) return s.rc();
    if (int rc = launch_tv_gradient(ctx, dvol, dims, eps, dout, ctx->host_stream)) return rc;
    s.download(out, (const float*)dout, voxels);
    return s.finish();
}

// xrt_volume_sumsq over device buffers on `stream`, its partials in the context's working set.
static int run_sumsq(xrt_context* ctx, uint64_t n, const float* d_a, const float* d_b, double* d_out, hipStream_t stream)
{
    if (int rc = sirt_working_set(ctx, std::max<size_t>(sumsq_partials(n), 1u) * sizeof(double))) return rc;
    XRT_HIP(ctx, ctx->sirt_done.mark());
    const int rc = launch_sumsq(ctx, n, d_a, d_b, reinterpret_cast<double*>(ctx->d_sirt.get()), d_out, stream);
    (void)ctx->sirt_done.record(stream);
    return rc;
}

int xrt_volume_sumsq_device(xrt_context* ctx, uint64_t n, const float* d_a, const float* d_b, double* d_out, void* stream)
{
    if (const char* why = sumsq_arguments(n, d_a, d_b, d_out)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return run_sumsq(ctx, n, d_a, d_b, d_out, (hipStream_t)stream);
}

int xrt_volume_sumsq(xrt_context* ctx, uint64_t n, const float* a, const float* b, double* out)
{
    if (const char* why = sumsq_arguments(n, a, b, out)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, ctx->host_stream, "sum of squares");
    const float* da = s.upload(a, (size_t)n);
    const float* db = s.upload(b, (size_t)n);
    double* dout = s.alloc<double>(1);
    if (s.rc()) return s.rc();
    if (int rc = run_sumsq(ctx, n, da, db, dout, ctx->host_stream)) return rc;
    s.download(out, (const double*)dout, 1);
    return s.finish();
}

// xrt_tv_descend over a device volume on `stream`: the sums, then the gradient volume, in the context's working set.
static int run_tv_descend(xrt_context* ctx, float* d_volume, const uint32_t dims[3], double eps, uint32_t steps, double length,
                          float lo, float hi, hipStream_t stream)
{
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    const size_t sums = sumsq_partials(voxels) + 1u;
    if (int rc = sirt_working_set(ctx, sums * sizeof(double) + voxels * sizeof(float))) return rc;
    XRT_HIP(ctx, ctx->sirt_done.mark());
    double* d_sums = reinterpret_cast<double*>(ctx->d_sirt.get());
    const int rc = launch_tv_descend(ctx, d_volume, dims, eps, steps, length, nullptr, lo, hi,
                                     reinterpret_cast<float*>(d_sums + sums), d_sums, stream);
    (void)ctx->sirt_done.record(stream);
    return rc;
}

int xrt_tv_descend_device(xrt_context* ctx, float* d_volume, const uint32_t dims[3], double eps, uint32_t steps,
                          double length, float lo, float hi, void* stream)
{
    if (const char* why = tv_descend_arguments(d_volume, dims, eps, length, lo, hi)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return run_tv_descend(ctx, d_volume, dims, eps, steps, length, lo, hi, (hipStream_t)stream);
}

int xrt_tv_descend(xrt_context* ctx, float* volume, const uint32_t dims[3], double eps, uint32_t steps, double length,
                   float lo, float hi)
{
    if (const char* why = tv_descend_arguments(volume, dims, eps, length, lo, hi)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "TV descent");
    float* dvol = s.upload(volume, voxels);
    if (s.rc()) return s.rc();
    if (int rc = run_tv_descend(ctx, dvol, dims, eps, steps, length, lo, hi, ctx->host_stream)) return rc;
    s.download(volume, (const float*)dvol, voxels);
    return s.finish();
}

// xrt_sirt_tv's loop over device buffers on `stream` (validated arguments, a plan whose every matrix has its ray
// matrix; tv NULL or without steps: xrt_sirt's).  The working set lies in the context's d_sirt: the matrices, with
// TV the sums (the partials, G, D), the residual planes, the correction volume -- the gradient's too --, the norm
// volumes and with TV x0.
static int run_sirt(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                    SirtPlan& plan, const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets,
                    double relax, float lo, float hi, const xrt_tv_params* tv, float* d_volume, hipStream_t stream)
{
    const bool with_tv = tv && tv->steps > 0u;
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    const size_t mat_bytes = (size_t)num_planes * 24u * sizeof(double);
    const size_t sums = with_tv ? sumsq_partials(voxels) + 2u : 0u;
    const size_t bytes = mat_bytes + sums * sizeof(double) +
                         (plane * plan.widest + voxels * ((size_t)subsets + 1u + (with_tv ? 1u : 0u))) * sizeof(float);
    if (int rc = sirt_working_set(ctx, bytes)) return rc;
    double* dA = reinterpret_cast<double*>(ctx->d_sirt.get());
    double* dR = dA + (size_t)num_planes * 12u;
    double* d_sums = dR + (size_t)num_planes * 12u;
    double* d_moved = d_sums + (sums ? sums - 1u : 0u);      // D, behind the partials and G
    float* d_res = reinterpret_cast<float*>(d_sums + sums);
    float* d_corr = d_res + plane * plan.widest;
    float* d_norms = d_corr + voxels;
    float* d_x0 = d_norms + voxels * subsets;
    ctx->sirt_mats.assign(plan.A.begin(), plan.A.end());
    ctx->sirt_mats.insert(ctx->sirt_mats.end(), plan.R.begin(), plan.R.end());
    XRT_HIP(ctx, ctx->sirt_done.mark());              // from here on the set is in use until sirt_done is recorded
    XRT_HIP(ctx, hipMemcpyAsync(dA, ctx->sirt_mats.data(), mat_bytes, hipMemcpyHostToDevice, stream));
    int rc = XRT_OK;
    // N_s: the backprojection of all-ones planes (1.0f's bits, word by word)
    if (hipMemsetD32Async((hipDeviceptr_t)d_res, 0x3F800000, plane * plan.widest, stream) != hipSuccess)
        rc = fail(ctx, XRT_ERR_DEVICE, "SIRT: filling the planes of ones failed");
    for (uint32_t s = 0; s < subsets && !rc; ++s)
        rc = launch_backproject(ctx, width, height, plan.count[s], d_res, dA + (size_t)plan.first[s] * 12u, dims, 0, dims[2],
                                1.0, 0, d_norms + voxels * s, stream);
    double a_k = with_tv ? tv->alpha : 0.0;
    for (uint32_t k = 0; k < iterations && !rc; ++k) {
        if (with_tv && hipMemcpyAsync(d_x0, d_volume, voxels * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            rc = fail(ctx, XRT_ERR_DEVICE, "SIRT: keeping the iteration's start failed");
        for (uint32_t s = 0; s < subsets && !rc; ++s) {
            // subset s's planes lie `subsets` planes apart in the scan, from plane s
            rc = launch_forward_project(ctx, width, height, plan.count[s], d_volume, dims, spacing,
                                        dR + (size_t)plan.first[s] * 12u, XRT_FP_RESIDUAL, d_proj + plane * s,
                                        (uint64_t)plane * subsets, d_res, stream);
            if (!rc)
                rc = launch_backproject(ctx, width, height, plan.count[s], d_res, dA + (size_t)plan.first[s] * 12u, dims, 0,
                                        dims[2], 1.0, 0, d_corr, stream);
            if (!rc) rc = launch_volume_update(ctx, voxels, d_volume, d_corr, d_norms + voxels * s, relax, lo, hi, stream);
        }
        if (with_tv && !rc) {
            // the data step's D stays on the device: every lane of the steps forms a_k * sqrt(D) from it
            rc = launch_sumsq(ctx, voxels, d_volume, d_x0, d_sums, d_moved, stream);
            if (!rc) rc = launch_tv_descend(ctx, d_volume, dims, tv->eps, tv->steps, a_k, d_moved, lo, hi, d_corr, d_sums, stream);
            a_k = a_k * tv->reduction;
        }
    }
    (void)ctx->sirt_done.record(stream);
    return rc;
}

int xrt_sirt_tv_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                       const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                       uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* d_volume,
                       void* stream)
{
    if (const char* why = sirt_arguments(width, height, num_planes, d_proj, matrices, dims, spacing, iterations, subsets, relax,
                                         lo, hi, d_volume, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (const char* why = tv_params_arguments(tv)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return fail(ctx, XRT_ERR_ARGUMENT, "a matrix has no ray matrix (xrt_ray_matrix)");
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return run_sirt(ctx, width, height, num_planes, d_proj, plan, dims, spacing, iterations, subsets, relax, lo, hi, tv,
                    d_volume, (hipStream_t)stream);
}

int xrt_sirt_tv(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
                const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* volume)
{
    if (const char* why = sirt_arguments(width, height, num_planes, proj, matrices, dims, spacing, iterations, subsets, relax,
                                         lo, hi, volume, true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (const char* why = tv_params_arguments(tv)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return fail(ctx, XRT_ERR_ARGUMENT, "a matrix has no ray matrix (xrt_ray_matrix)");
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "SIRT");
    const float* dproj = s.upload(proj, (size_t)width * height * num_planes);
    float* dvol = s.upload(volume, voxels);
    if (s.rc()) return s.rc();
    if (int rc = run_sirt(ctx, width, height, num_planes, dproj, plan, dims, spacing, iterations, subsets, relax, lo, hi, tv,
                          dvol, ctx->host_stream))
        return rc;
    s.download(volume, (const float*)dvol, voxels);
    return s.finish();
}

int xrt_sirt_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_proj,
                    const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations,
                    uint32_t subsets, double relax, float lo, float hi, float* d_volume, void* stream)
{
    return xrt_sirt_tv_device(ctx, width, height, num_planes, d_proj, matrices, dims, spacing, iterations, subsets, relax, lo,
                              hi, nullptr, d_volume, stream);
}

int xrt_sirt(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* proj,
             const double* matrices, const uint32_t dims[3], const float spacing[3], uint32_t iterations, uint32_t subsets,
             double relax, float lo, float hi, float* volume)
{
    return xrt_sirt_tv(ctx, width, height, num_planes, proj, matrices, dims, spacing, iterations, subsets, relax, lo, hi,
                       nullptr, volume);
}

// --- OS-MLTR ------------------------------------------------------

#include "xrt_mltr_host.inc"

// The launch of k_poisson_project (validated arguments, device pointers); plane p's counts lie at
// d_counts + p * stride and its background, when there is one, at d_background + p * stride.
static int launch_poisson_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                  const float* d_volume, const uint32_t dims[3], const float spacing[3],
                                  const double* d_rays, const float* d_counts, const float* d_flat,
                                  const float* d_background, uint64_t stride, float* d_pairs, hipStream_t stream)
{
    const uint32_t tiles_x = (width + kForwardTile - 1u) / kForwardTile, tiles_y = (height + kForwardTile - 1u) / kForwardTile;
    hipLaunchKernelGGL(k_poisson_project, dim3(tiles_x * tiles_y, num_planes), dim3(64), 0, stream, d_volume, d_rays, d_counts,
                       d_flat, d_background, stride, reinterpret_cast<FloatPair*>(d_pairs), dims[0], dims[1], dims[2],
                       (double)spacing[0], (double)spacing[1], (double)spacing[2], width, height, tiles_x);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_poisson_project_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                               const float* d_volume, const uint32_t dims[3], const float spacing[3], const double* d_rays,
                               const float* d_counts, const float* d_flat, const float* d_background, float* d_pairs,
                               void* stream)
{
    if (const char* why = poisson_project_arguments(width, height, num_planes, d_volume, dims, spacing, d_rays, d_counts,
                                                    d_flat, d_background, d_pairs, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_poisson_project(ctx, width, height, num_planes, d_volume, dims, spacing, d_rays, d_counts, d_flat,
                                  d_background, (uint64_t)width * height, d_pairs, (hipStream_t)stream);
}

int xrt_poisson_project(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* volume,
                        const uint32_t dims[3], const float spacing[3], const double* rays, const float* counts,
                        const float* flat, const float* background, float* pairs)
{
    if (const char* why = poisson_project_arguments(width, height, num_planes, volume, dims, spacing, rays, counts, flat,
                                                    background, pairs, true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t plane = (size_t)width * height, all = plane * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "Poisson projection");
    const float* dvol = s.upload(volume, (size_t)dims[0] * dims[1] * dims[2]);
    const double* drays = s.upload(rays, (size_t)num_planes * 12u);
    const float* dcounts = s.upload(counts, all);
    const float* dflat = s.upload(flat, plane);
    const float* dbg = s.upload(background, all);
    float* dpairs = s.alloc<float>(2u * all);
    if (s.rc()) return s.rc();
    if (int rc = launch_poisson_project(ctx, width, height, num_planes, dvol, dims, spacing, drays, dcounts, dflat, dbg,
                                        (uint64_t)plane, dpairs, ctx->host_stream))
        return rc;
    s.download(pairs, (const float*)dpairs, 2u * all);
    return s.finish();
}

// The launch of k_backproject_update (validated arguments, device pointers).
static int launch_backproject_update(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                     const float* d_pairs, const double* d_matrices, const uint32_t dims[3], double relax,
                                     float lo, float hi, float* d_volume, hipStream_t stream)
{
    const uint32_t spans = (dims[0] + kPairSpan - 1u) / kPairSpan;
    const uint64_t rows = (uint64_t)dims[2] * dims[1];
    const uint64_t waves = rows * spans, per_block = kBackprojectThreads / 64u;
    hipLaunchKernelGGL(k_backproject_update, dim3((unsigned)((waves + per_block - 1u) / per_block)), dim3(kBackprojectThreads),
                       0, stream, reinterpret_cast<const FloatPair*>(d_pairs), d_matrices, width, height, num_planes, dims[0],
                       dims[1], rows, spans, relax, lo, hi, d_volume);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_backproject_update_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                  const float* d_pairs, const double* d_matrices, const uint32_t dims[3], double relax,
                                  float lo, float hi, float* d_volume, void* stream)
{
    if (const char* why = backproject_update_arguments(width, height, num_planes, d_pairs, d_matrices, dims, relax, lo, hi,
                                                       d_volume, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_backproject_update(ctx, width, height, num_planes, d_pairs, d_matrices, dims, relax, lo, hi, d_volume,
                                     (hipStream_t)stream);
}

int xrt_backproject_update(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* pairs,
                           const double* matrices, const uint32_t dims[3], double relax, float lo, float hi, float* volume)
{
    if (const char* why = backproject_update_arguments(width, height, num_planes, pairs, matrices, dims, relax, lo, hi, volume,
                                                       true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "backprojection update");
    const float* dpairs = s.upload(pairs, (size_t)width * height * num_planes * 2u);
    const double* dmat = s.upload(matrices, (size_t)num_planes * 12u);
    float* dvol = s.upload(volume, voxels);
    if (s.rc()) return s.rc();
    if (int rc = launch_backproject_update(ctx, width, height, num_planes, dpairs, dmat, dims, relax, lo, hi, dvol,
                                           ctx->host_stream))
        return rc;
    s.download(volume, (const float*)dvol, voxels);
    return s.finish();
}

// xrt_mltr's loop over device buffers on `stream` (validated arguments, a plan whose every matrix has its ray
// matrix).  The working set lies in the context's d_sirt: the matrices, with TV the sums (the partials, G, D), the
// largest subset's pairs, and with TV the gradient volume and x0.
static int run_mltr(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_counts,
                    const float* d_flat, const float* d_background, SirtPlan& plan, const uint32_t dims[3],
                    const float spacing[3], uint32_t iterations, uint32_t subsets, double relax, float lo, float hi,
                    const xrt_tv_params* tv, float* d_volume, hipStream_t stream)
{
    const bool with_tv = tv && tv->steps > 0u;
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    const size_t mat_bytes = (size_t)num_planes * 24u * sizeof(double);
    const size_t sums = with_tv ? sumsq_partials(voxels) + 2u : 0u;
    const size_t bytes = mat_bytes + sums * sizeof(double) +
                         (2u * plane * plan.widest + (with_tv ? 2u * voxels : 0u)) * sizeof(float);
    if (int rc = sirt_working_set(ctx, bytes)) return rc;
    double* dA = reinterpret_cast<double*>(ctx->d_sirt.get());
    double* dR = dA + (size_t)num_planes * 12u;
    double* d_sums = dR + (size_t)num_planes * 12u;
    double* d_moved = d_sums + (sums ? sums - 1u : 0u);      // D, behind the partials and G
    float* d_pairs = reinterpret_cast<float*>(d_sums + sums);  // (behind doubles: aligned to 8 bytes)
    float* d_grad = d_pairs + 2u * plane * plan.widest;
    float* d_x0 = d_grad + voxels;
    ctx->sirt_mats.assign(plan.A.begin(), plan.A.end());
    ctx->sirt_mats.insert(ctx->sirt_mats.end(), plan.R.begin(), plan.R.end());
    XRT_HIP(ctx, ctx->sirt_done.mark());              // from here on the set is in use until sirt_done is recorded
    XRT_HIP(ctx, hipMemcpyAsync(dA, ctx->sirt_mats.data(), mat_bytes, hipMemcpyHostToDevice, stream));
    int rc = XRT_OK;
    double a_k = with_tv ? tv->alpha : 0.0;
    for (uint32_t k = 0; k < iterations && !rc; ++k) {
        if (with_tv && hipMemcpyAsync(d_x0, d_volume, voxels * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            rc = fail(ctx, XRT_ERR_DEVICE, "MLTR: keeping the iteration's start failed");
        for (uint32_t s = 0; s < subsets && !rc; ++s) {
            // subset s's planes lie `subsets` planes apart in the scan, from plane s
            rc = launch_poisson_project(ctx, width, height, plan.count[s], d_volume, dims, spacing,
                                        dR + (size_t)plan.first[s] * 12u, d_counts + plane * s, d_flat,
                                        d_background ? d_background + plane * s : nullptr, (uint64_t)plane * subsets, d_pairs,
                                        stream);
            if (!rc)
                rc = launch_backproject_update(ctx, width, height, plan.count[s], d_pairs, dA + (size_t)plan.first[s] * 12u,
                                               dims, relax, lo, hi, d_volume, stream);
        }
        if (with_tv && !rc) {
            rc = launch_sumsq(ctx, voxels, d_volume, d_x0, d_sums, d_moved, stream);
            if (!rc) rc = launch_tv_descend(ctx, d_volume, dims, tv->eps, tv->steps, a_k, d_moved, lo, hi, d_grad, d_sums, stream);
            a_k = a_k * tv->reduction;
        }
    }
    (void)ctx->sirt_done.record(stream);
    return rc;
}

int xrt_mltr_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_counts,
                    const float* d_flat, const float* d_background, const double* matrices, const uint32_t dims[3],
                    const float spacing[3], uint32_t iterations, uint32_t subsets, double relax, float lo, float hi,
                    const xrt_tv_params* tv, float* d_volume, void* stream)
{
    if (const char* why = mltr_arguments(width, height, num_planes, d_counts, d_flat, d_background, matrices, dims, spacing,
                                         iterations, subsets, relax, lo, hi, d_volume, false))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (const char* why = tv_params_arguments(tv)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return fail(ctx, XRT_ERR_ARGUMENT, "a matrix has no ray matrix (xrt_ray_matrix)");
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return run_mltr(ctx, width, height, num_planes, d_counts, d_flat, d_background, plan, dims, spacing, iterations, subsets,
                    relax, lo, hi, tv, d_volume, (hipStream_t)stream);
}

int xrt_mltr(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* counts, const float* flat,
             const float* background, const double* matrices, const uint32_t dims[3], const float spacing[3],
             uint32_t iterations, uint32_t subsets, double relax, float lo, float hi, const xrt_tv_params* tv, float* volume)
{
    if (const char* why = mltr_arguments(width, height, num_planes, counts, flat, background, matrices, dims, spacing,
                                         iterations, subsets, relax, lo, hi, volume, true))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (const char* why = tv_params_arguments(tv)) return fail(ctx, XRT_ERR_ARGUMENT, why);
    SirtPlan plan;
    if (!sirt_plan(num_planes, subsets, matrices, plan)) return fail(ctx, XRT_ERR_ARGUMENT, "a matrix has no ray matrix (xrt_ray_matrix)");
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t plane = (size_t)width * height, voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "MLTR");
    const float* dcounts = s.upload(counts, plane * num_planes);
    const float* dflat = s.upload(flat, plane);
    const float* dbg = s.upload(background, plane * num_planes);
    float* dvol = s.upload(volume, voxels);
    if (s.rc()) return s.rc();
    if (int rc = run_mltr(ctx, width, height, num_planes, dcounts, dflat, dbg, plan, dims, spacing, iterations, subsets, relax,
                          lo, hi, tv, dvol, ctx->host_stream))
        return rc;
    s.download(volume, (const float*)dvol, voxels);
    return s.finish();
}

// --- voxelisation ---------------------------------------------

#include "xrt_voxel_host.inc"

// The bytes of the voxeliser's working set ahead of the flip volume: the control words, then the queue.
constexpr size_t kVoxelQueueAt = 64, kVoxelFlipAt = kVoxelQueueAt + (size_t)kVoxelQueueCap * sizeof(uint2);
static_assert(sizeof(VoxelControl) <= kVoxelQueueAt, "the control words lie ahead of the queue");

// The checks both forms share, the arguments' first (no context needed).
static int voxelize_checks(xrt_context* ctx, const uint32_t* dims, const float* origin, const float* spacing,
                           const float* value, const void* mask, const void* labels, const void* volume, const void* odd)
{
    const std::string why = voxelize_arguments(dims, origin, spacing, value, mask, labels, volume, odd);
    if (!why.empty()) return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (ctx->mesh_tris.empty()) return fail(ctx, XRT_ERR_NO_MESH, "no scene uploaded (xrt_upload_mesh, xrt_upload_scene)");
    return XRT_OK;
}

// The voxeliser over device buffers on `stream` (validated arguments): a k_pose that is due goes to the preparation
// stream as before a render and `stream` waits for it by an event; then the working set is cleared, the scatter and
// the tile waves flip it and the scan writes the outputs.
static int run_voxelize(xrt_context* ctx, const uint32_t* dims, const float* origin, const float* spacing, const float* value,
                        uint16_t* d_mask, uint8_t* d_labels, float* d_volume, uint64_t* d_odd, hipStream_t stream)
{
    const VoxelGrid g = voxel_grid(dims, origin, spacing);
    const uint64_t plane = (uint64_t)g.nx * g.ny;
    const size_t flip_bytes = ((size_t)(plane * (g.nz + 1u)) * sizeof(uint16_t) + 3u) & ~(size_t)3u;
    VoxelMeshes meshes = {};
    const size_t M = ctx->mesh_tris.size();
    uint64_t end = 0;
    for (size_t m = 0; m < kMaxMeshes; ++m) {
        if (m < M) end += ctx->mesh_tris[m];
        meshes.end[m] = m < M ? (uint32_t)end : 0xFFFFFFFFu;
        meshes.value[m] = m < M && value ? value[m] : 0.0f;
    }
    meshes.num = (uint32_t)M;
    if (ctx->num_tris > 0xFFFFFF00ull) return fail(ctx, XRT_ERR_ARGUMENT, "too many triangles to voxelise");
    const float* soup = nullptr;
    if (int rc = render_soup(ctx, soup)) return rc;
    if (soup != ctx->d_tris.get()) {                        // the posed soup: behind its k_pose on the preparation stream
        XRT_HIP(ctx, ctx->vox_pose_ev.create());
        XRT_HIP(ctx, hipEventRecord(ctx->vox_pose_ev.get(), ctx->prep_stream));
        XRT_HIP(ctx, hipStreamWaitEvent(stream, ctx->vox_pose_ev.get(), 0));
    }
    // (the set's last user ran on `stream` and the set is large enough: the stream orders this call behind it)
    if (ctx->vox_counters && ctx->vox_stream == stream && kVoxelFlipAt + flip_bytes <= ctx->d_sirt.cap())
        ctx->sirt_done.forget();
    if (int rc = sirt_working_set(ctx, kVoxelFlipAt + flip_bytes)) return rc;
    XRT_HIP(ctx, ctx->sirt_done.mark());
    ctx->vox_stream = stream;
    VoxelControl* ctl = reinterpret_cast<VoxelControl*>(ctx->d_sirt.get());
    uint2* queue = reinterpret_cast<uint2*>(ctx->d_sirt.get() + kVoxelQueueAt);
    uint32_t* flip = reinterpret_cast<uint32_t*>(ctx->d_sirt.get() + kVoxelFlipAt);
    const bool clear = ctx->vox_stages & 4u, scatter = ctx->vox_stages & 1u, scan = ctx->vox_stages & 2u;
    hipError_t e = hipMemsetAsync(ctl, 0, kVoxelQueueAt, stream);
    if (e == hipSuccess) e = hipMemsetAsync(queue, 0xFF, kVoxelFlipAt - kVoxelQueueAt, stream);
    if (e == hipSuccess && clear) e = hipMemsetAsync(flip, 0, flip_bytes, stream);
    if (e == hipSuccess && d_odd) e = hipMemsetAsync(d_odd, 0, XRT_MAX_MESHES * sizeof(uint64_t), stream);
    if (e == hipSuccess && ctx->num_tris && scatter) {
        const uint32_t T = (uint32_t)ctx->num_tris;
        hipLaunchKernelGGL(k_voxel_scatter, dim3((T + kVoxelThreads - 1u) / kVoxelThreads), dim3(kVoxelThreads), 0, stream,
                           soup, T, meshes, g, ctx->vox_threshold, flip, ctl, queue);
        hipLaunchKernelGGL(k_voxel_tiles, dim3(kVoxelTileBlocks), dim3(kVoxelThreads), 0, stream, soup, meshes, g, flip,
                           (const VoxelControl*)ctl, (const uint2*)queue);
        e = hipGetLastError();
        if (e == hipSuccess) e = ctx->vox_scattered.record(stream);
    }
    if (e == hipSuccess && scan) {
        // runs of slices, so that a grid of few columns still fills the device (vox_stages & 8: one run, for the A/B)
        const uint64_t waves = (plane + 63u) / 64u;
        uint32_t runs = (uint32_t)std::min<uint64_t>(kVoxelScanRuns, std::max<uint64_t>(1u, kVoxelScanWaves / waves));
        if (ctx->vox_stages & 8u) runs = 1u;
        const uint32_t chunk = std::max(kVoxelScanRun, (g.nz + runs - 1u) / runs);
        hipLaunchKernelGGL(k_voxel_scan, dim3((unsigned)((plane + kVoxelThreads - 1u) / kVoxelThreads), (g.nz + chunk - 1u) / chunk),
                           dim3(kVoxelThreads), 0, stream, g, meshes, reinterpret_cast<const uint16_t*>(flip), d_mask, d_labels,
                           d_volume, reinterpret_cast<unsigned long long*>(d_odd), chunk);
        e = hipGetLastError();
    }
    (void)ctx->sirt_done.record(stream);
    ctx->vox_counters = e == hipSuccess;
    if (e != hipSuccess) return fail(ctx, XRT_ERR_DEVICE, std::string("xrt_voxelize: ") + hipGetErrorString(e));
    return XRT_OK;
}

int xrt_voxelize_device(xrt_context* ctx, const uint32_t dims[3], const float origin[3], const float spacing[3],
                        const float* value, uint16_t* d_mask, uint8_t* d_labels, float* d_volume, uint64_t* d_odd_columns,
                        void* stream)
{
    if (int rc = voxelize_checks(ctx, dims, origin, spacing, value, d_mask, d_labels, d_volume, d_odd_columns)) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return run_voxelize(ctx, dims, origin, spacing, value, d_mask, d_labels, d_volume, d_odd_columns, (hipStream_t)stream);
}

int xrt_voxelize(xrt_context* ctx, const uint32_t dims[3], const float origin[3], const float spacing[3], const float* value,
                 uint16_t* mask, uint8_t* labels, float* volume, uint64_t* odd_columns)
{
    if (int rc = voxelize_checks(ctx, dims, origin, spacing, value, mask, labels, volume, odd_columns)) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t voxels = (size_t)dims[0] * dims[1] * dims[2];
    DeviceScratch s(ctx, ctx->host_stream, "voxelisation");
    uint16_t* dmask = s.alloc<uint16_t>(voxels, mask != nullptr);
    uint8_t* dlabels = s.alloc<uint8_t>(voxels, labels != nullptr);
    float* dvolume = s.alloc<float>(voxels, volume != nullptr);
    uint64_t* dodd = s.alloc<uint64_t>(XRT_MAX_MESHES, odd_columns != nullptr);
    if (s.rc()) return s.rc();
    if (int rc = run_voxelize(ctx, dims, origin, spacing, value, dmask, dlabels, dvolume, dodd, ctx->host_stream)) return rc;
    s.download(mask, (const uint16_t*)dmask, voxels);
    s.download(labels, (const uint8_t*)dlabels, voxels);
    s.download(volume, (const float*)dvolume, voxels);
    s.download(odd_columns, (const uint64_t*)dodd, XRT_MAX_MESHES);
    return s.finish();
}

int xrt_debug_voxelize_threshold(xrt_context* ctx, uint32_t columns)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    ctx->vox_threshold = columns ? columns : kVoxelQueueColumns;
    return XRT_OK;
}

int xrt_debug_voxelize_stages(xrt_context* ctx, uint32_t stages)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    ctx->vox_stages = stages & 15u;
    return XRT_OK;
}

int xrt_debug_voxelize_counters(xrt_context* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    if (!ctx->vox_counters) return fail(ctx, XRT_ERR_ARGUMENT, "the working set no longer holds a voxelisation's counters");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    XRT_HIP(ctx, ctx->sirt_done.wait());
    VoxelControl c = {};
    XRT_HIP(ctx, hipMemcpy(&c, ctx->d_sirt.get(), sizeof c, hipMemcpyDeviceToHost));
    counters[0] = c.direct;
    counters[1] = c.queued;
    counters[2] = c.entries;
    counters[3] = c.overflowed;
    return XRT_OK;
}

// --- material decomposition ----------------------------------

#include "xrt_decompose_host.inc"

int xrt_decompose_guess(const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                        uint32_t num_channels, double* guess)
{
    if (!guess) return fail(nullptr, XRT_ERR_ARGUMENT, "guess is NULL");
    const char* why = decompose_table_arguments(weight, mu, num_basis, num_bins, response, num_channels, 1.0f);
    if (!why) why = decompose_guess_matrix(weight, mu, num_basis, num_bins, response, num_channels, guess);
    return why ? fail(nullptr, XRT_ERR_ARGUMENT, why) : XRT_OK;
}

// The launch of k_decompose (validated arguments, device pointers): the instantiation of num_basis and of
// the smallest channel bound that holds num_channels.
static int launch_decompose(xrt_context* ctx, uint64_t n, const float* d_channels, const uint16_t* d_open, const float* weight,
                            const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                            uint32_t num_channels, float gain, int in_mode, const double* guess, uint32_t max_iter, double tol,
                            double damping, float* d_out, uint8_t* d_iters, hipStream_t stream)
{
    DecomposeTable tab;                 // by value: the launch owns its copy (no context state, no wait)
    decompose_table(weight, mu, num_basis, num_bins, response, num_channels, gain, in_mode, guess, max_iter, tol, damping,
                    &tab);
    tab.channels = d_channels;
    tab.open = d_open;
    tab.out = d_out;
    tab.iters = d_iters;
    tab.plane = n;
    const dim3 grid((unsigned)((n + kDecomposeThreads - 1u) / kDecomposeThreads)), block(kDecomposeThreads);
#define XRT_DECOMPOSE_LAUNCH(B)                                                                                  \
    do {                                                                                                         \
        if (num_channels <= 2u)                                                                                  \
            hipLaunchKernelGGL((k_decompose<B, 2>), grid, block, 0, stream, (size_t)n, tab);                     \
        else if (num_channels <= 4u)                                                                             \
            hipLaunchKernelGGL((k_decompose<B, 4>), grid, block, 0, stream, (size_t)n, tab);                     \
        else                                                                                                     \
            hipLaunchKernelGGL((k_decompose<B, 8>), grid, block, 0, stream, (size_t)n, tab);                     \
    } while (0)
    if (num_basis == 1u) XRT_DECOMPOSE_LAUNCH(1);
    else if (num_basis == 2u) XRT_DECOMPOSE_LAUNCH(2);
    else XRT_DECOMPOSE_LAUNCH(3);
#undef XRT_DECOMPOSE_LAUNCH
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_decompose_device(xrt_context* ctx, uint64_t num_pixels, const float* d_channels, const uint16_t* d_open,
                         const float* weight, const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response,
                         uint32_t num_channels, float gain, int in_mode, const double* guess, uint32_t max_iter, double tol,
                         double damping, float* d_out, uint8_t* d_iters, void* stream)
{
    if (const char* why = decompose_arguments(num_pixels, d_channels, d_open, weight, mu, num_basis, num_bins, response,
                                              num_channels, gain, in_mode, guess, max_iter, tol, damping, d_out, d_iters))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_decompose(ctx, num_pixels, d_channels, d_open, weight, mu, num_basis, num_bins, response, num_channels, gain,
                            in_mode, guess, max_iter, tol, damping, d_out, d_iters, (hipStream_t)stream);
}

int xrt_decompose(xrt_context* ctx, uint64_t num_pixels, const float* channels, const uint16_t* open, const float* weight,
                  const float* mu, uint32_t num_basis, uint32_t num_bins, const float* response, uint32_t num_channels,
                  float gain, int in_mode, const double* guess, uint32_t max_iter, double tol, double damping, float* out,
                  uint8_t* iters)
{
    if (const char* why = decompose_arguments(num_pixels, channels, open, weight, mu, num_basis, num_bins, response,
                                              num_channels, gain, in_mode, guess, max_iter, tol, damping, out, iters))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)num_pixels;
    DeviceScratch s(ctx, ctx->host_stream, "decomposition");
    const float* dc = s.upload(channels, n * num_channels);
    const uint16_t* dopen = s.upload(open, n);
    float* dout = s.alloc<float>(n * num_basis);
    uint8_t* diters = s.alloc<uint8_t>(n, iters != nullptr);
    if (s.rc()) return s.rc();
    if (int rc = launch_decompose(ctx, n, dc, dopen, weight, mu, num_basis, num_bins, response, num_channels, gain, in_mode,
                                  guess, max_iter, tol, damping, dout, diters, ctx->host_stream))
        return rc;
    s.download(out, dout, n * num_basis);
    s.download(iters, static_cast<const uint8_t*>(diters), n);
    return s.finish();
}

int xrt_hole_fill_device(xrt_context* ctx, uint32_t width, uint32_t height, const float* d_lbuffer,
                         float* d_image, uint8_t* d_u8, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    const uint64_t n = (uint64_t)width * height;
    if (n > 0xFFFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "image larger than 2^32-1 pixels");
    if (!n) return XRT_OK;
    if (!d_lbuffer) return fail(ctx, XRT_ERR_ARGUMENT, "L-buffer is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_hole_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_lbuffer, d_image, d_u8, width, height);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_hole_fill(xrt_context* ctx, uint32_t width, uint32_t height, const float* lbuffer, float* image,
                  uint8_t* image_u8)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    const size_t n = (size_t)width * height;
    if (!n) return XRT_OK;
    if (!lbuffer) return fail(ctx, XRT_ERR_ARGUMENT, "L-buffer is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = stage_planes(ctx, n))) return rc;
    XRT_HIP(ctx, hipMemcpyAsync(ctx->d_lbuffer.get(), lbuffer, n * sizeof(float), hipMemcpyHostToDevice, ctx->host_stream));
    if ((rc = xrt_hole_fill_device(ctx, width, height, ctx->d_lbuffer.get(), image ? ctx->d_image.get() : nullptr,
                                   image_u8 ? ctx->d_u8.get() : nullptr, ctx->host_stream)))
        return rc;
    return d2h_copy(ctx, ctx->host_stream, plane_copies(n, image, ctx->d_image.get(), nullptr, nullptr, image_u8, ctx->d_u8.get()));
}

// --- the detector response -------------------------------------

#include "xrt_lsf_host.inc"

// The launch of k_lsf (validated arguments, device pointers).
static int launch_lsf(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                      const float* lsf_x, uint32_t taps_x, const float* lsf_y, uint32_t taps_y, float* d_out,
                      uint8_t* d_out_u8, hipStream_t stream)
{
    LsfTable tab;                       // by value: the launch owns its copy (no context state, no wait)
    lsf_table_set(tab, lsf_x, taps_x, lsf_y, taps_y);
    const size_t lds = lsf_lds_bytes(taps_x, taps_y);
    if (lds > 64u * 1024u)              // past the default limit of a launch's dynamic LDS
        XRT_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsf),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((width + kLsfTile - 1u) / kLsfTile, (height + kLsfTile - 1u) / kLsfTile, num_planes);
    hipLaunchKernelGGL(k_lsf, grid, dim3(kLsfThreads), lds, stream, d_image, d_out, d_out_u8, width, height, tab);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_detector_response_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                 const float* d_image, const float* lsf_x, uint32_t taps_x, const float* lsf_y,
                                 uint32_t taps_y, float* d_out, uint8_t* d_out_u8, void* stream)
{
    if (const char* why = lsf_arguments(width, height, num_planes, d_image, lsf_x, taps_x, lsf_y, taps_y, d_out, d_out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_lsf(ctx, width, height, num_planes, d_image, lsf_x, taps_x, lsf_y, taps_y, d_out, d_out_u8,
                      (hipStream_t)stream);
}

int xrt_detector_response(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                          const float* image, const float* lsf_x, uint32_t taps_x, const float* lsf_y,
                          uint32_t taps_y, float* out, uint8_t* out_u8)
{
    if (const char* why = lsf_arguments(width, height, num_planes, image, lsf_x, taps_x, lsf_y, taps_y, out, out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)width * height * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "detector response");
    const float* din = s.upload(image, n);
    float* dout = s.alloc<float>(n, out != nullptr);
    uint8_t* du8 = s.alloc<uint8_t>(n, out_u8 != nullptr);
    if (s.rc()) return s.rc();
    if (int rc = launch_lsf(ctx, width, height, num_planes, din, lsf_x, taps_x, lsf_y, taps_y, dout, du8, ctx->host_stream))
        return rc;
    s.download(out, dout, n);
    s.download(out_u8, du8, n);
    return s.finish();
}

// --- line-integral projections ---------------------------------

#include "xrt_projection_host.inc"

// The launch of k_log_projection (validated arguments, device pointers).
static int launch_log_projection(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                                 const float* d_image, const float* d_flat, const float* d_dark, float flat_value,
                                 float t_min, int order, float* d_out, hipStream_t stream)
{
    const LogProjectionPlan plan = log_projection_plan(width, (uint64_t)num_planes * height);
    // (a workgroup within one row -- planes from 510 pixels' width -- does the row's arithmetic as scalars)
    const auto kernel = plan.lanes_log2 == kProjThreadsLog2 ? k_log_projection<true> : k_log_projection<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.blocks), dim3(kProjThreads), 0, stream, d_image, d_flat, d_dark, d_out,
                       width, height, num_planes, flat_value, t_min, (uint32_t)(order == XRT_ORDER_SINOGRAMS),
                       plan.lanes_log2, plan.chunks);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_log_projection_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes,
                              const float* d_image, const float* d_flat, const float* d_dark, float flat_value,
                              float t_min, int order, float* d_out, void* stream)
{
    if (const char* why = projection_arguments(width, height, num_planes, d_image, d_flat, d_dark, flat_value, t_min,
                                               order, d_out))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_log_projection(ctx, width, height, num_planes, d_image, d_flat, d_dark, flat_value, t_min, order,
                                 d_out, (hipStream_t)stream);
}

int xrt_log_projection(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                       const float* flat, const float* dark, float flat_value, float t_min, int order, float* out)
{
    if (const char* why = projection_arguments(width, height, num_planes, image, flat, dark, flat_value, t_min, order, out))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t plane = (size_t)width * height, all = plane * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "log projection");
    const float* din = s.upload(image, all);
    const float* dflat = s.upload(flat, plane);
    const float* ddark = s.upload(dark, plane);
    float* dout = s.alloc<float>(all);
    if (s.rc()) return s.rc();
    if (int rc = launch_log_projection(ctx, width, height, num_planes, din, dflat, ddark, flat_value, t_min, order, dout,
                                       ctx->host_stream))
        return rc;
    s.download(out, dout, all);
    return s.finish();
}

// --- photon noise ----------------------------------------------

#include "xrt_noise_host.inc"

// The launch of k_photon_noise (validated arguments, device pointers).
static int launch_photon_noise(xrt_context* ctx, uint64_t n, const float* d_image, float gain, uint64_t seed,
                               uint64_t first_index, int mode, float* d_out, hipStream_t stream)
{
    const uint64_t blocks = (photon_noise_lanes(first_index, n) + kNoiseThreads - 1u) / kNoiseThreads;
    hipLaunchKernelGGL(k_photon_noise, dim3((unsigned)blocks), dim3(kNoiseThreads), 0, stream, d_image, d_out, n, gain, seed,
                       first_index, (uint32_t)(mode == XRT_NOISE_COUNTS));
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_photon_noise_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* d_image,
                            float gain, uint64_t seed, uint64_t first_index, int mode, float* d_out, void* stream)
{
    uint64_t n = 0;
    if (const char* why = noise_arguments(width, height, num_planes, d_image, gain, first_index, mode, d_out, &n))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_photon_noise(ctx, n, d_image, gain, seed, first_index, mode, d_out, (hipStream_t)stream);
}

int xrt_photon_noise(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, const float* image,
                     float gain, uint64_t seed, uint64_t first_index, int mode, float* out)
{
    uint64_t n = 0;
    if (const char* why = noise_arguments(width, height, num_planes, image, gain, first_index, mode, out, &n))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, ctx->host_stream, "photon noise");
    float* d = s.upload(image, (size_t)n);              // in place on the device: the pass is pointwise
    if (s.rc()) return s.rc();
    if (int rc = launch_photon_noise(ctx, n, d, gain, seed, first_index, mode, d, ctx->host_stream)) return rc;
    s.download(out, d, (size_t)n);
    return s.finish();
}

// The sampler on the device over caller-chosen means and words (a test hook).
int xrt_debug_poisson_batch(xrt_context* ctx, const double* lam, const uint32_t* words, uint64_t n, double* outp)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (n == 0) return XRT_OK;
    if (!lam || !words || !outp) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    if (n > 0x7FFFFFFFull * 256u) return fail(ctx, XRT_ERR_ARGUMENT, "too many values");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, nullptr, "probe");
    const double* dl = s.upload(lam, n);
    const uint32_t* dw = s.upload(words, n);
    double* dout = s.alloc<double>(n);
    if (s.rc()) return s.rc();
    hipLaunchKernelGGL(k_probe_poisson, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dl, dw, n, dout);
    s.launched();
    s.download(outp, dout, n);
    return s.finish();
}

// --- area sampling ---------------------------------------------

#include "xrt_area_host.inc"

// The launch of k_area_integrate (validated arguments, device pointers).
static int launch_area_integrate(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y,
                                 uint32_t num_sources, uint32_t num_planes, const float* weight, const float* d_image,
                                 float* d_out, uint8_t* d_out_u8, hipStream_t stream)
{
    AreaWeights tab;                    // by value: the launch owns its copy (no context state, no wait)
    area_weights_set(tab, weight, num_sources, bin_x, bin_y);
    const AreaPlan plan = area_plan(width, (uint64_t)num_planes * height, bin_x, bin_y, num_sources, height);
    const bool wide = plan.lanes_log2 == kAreaThreadsLog2;
    auto kernel = wide ? k_area_integrate<0, true> : k_area_integrate<0, false>;
    switch (plan.vector) {
    case 1: kernel = wide ? k_area_integrate<1, true> : k_area_integrate<1, false>; break;
    case 2: kernel = wide ? k_area_integrate<2, true> : k_area_integrate<2, false>; break;
    case 4: kernel = wide ? k_area_integrate<4, true> : k_area_integrate<4, false>; break;
    case 8: kernel = wide ? k_area_integrate<8, true> : k_area_integrate<8, false>; break;
    default: break;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.blocks), dim3(kAreaThreads), 0, stream, d_image, d_out, d_out_u8, width,
                       height, num_planes, bin_x, bin_y, num_sources, plan.lanes_log2, plan.chunks, tab);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_area_integrate_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y,
                              uint32_t num_sources, uint32_t num_planes, const float* weight, const float* d_image,
                              float* d_out, uint8_t* d_out_u8, void* stream)
{
    if (const char* why = area_arguments(width, height, bin_x, bin_y, num_sources, num_planes, weight, d_image, d_out,
                                         d_out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_area_integrate(ctx, width, height, bin_x, bin_y, num_sources, num_planes, weight, d_image, d_out,
                                 d_out_u8, (hipStream_t)stream);
}

int xrt_area_integrate(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t bin_x, uint32_t bin_y,
                       uint32_t num_sources, uint32_t num_planes, const float* weight, const float* image, float* out,
                       uint8_t* out_u8)
{
    if (const char* why = area_arguments(width, height, bin_x, bin_y, num_sources, num_planes, weight, image, out, out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)width * height * num_planes, n_in = n * bin_x * bin_y * num_sources;
    DeviceScratch s(ctx, ctx->host_stream, "area integration");
    const float* din = s.upload(image, n_in);
    float* dout = s.alloc<float>(n, out != nullptr);
    uint8_t* du8 = s.alloc<uint8_t>(n, out_u8 != nullptr);
    if (s.rc()) return s.rc();
    if (int rc = launch_area_integrate(ctx, width, height, bin_x, bin_y, num_sources, num_planes, weight, din, dout, du8,
                                       ctx->host_stream))
        return rc;
    s.download(out, dout, n);
    s.download(out_u8, du8, n);
    return s.finish();
}

// --- the scatter model ------------------------------------------

#include "xrt_scatter_host.inc"

// The launch of k_scatter_source (validated arguments, device pointers): the instantiation of the smallest mesh
// bound that holds num_meshes.
static int launch_scatter_source(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                                 const float* d_paths, const uint16_t* d_open, const float* weight, const float* mu,
                                 const float* sigma, uint32_t num_bins, uint32_t bin, float* d_lbuffer, float* d_source,
                                 hipStream_t stream)
{
    ScatterTable tab = {};              // by value: the launch owns its copy (no context state, no wait)
    std::copy(weight, weight + num_bins, tab.weight);
    for (uint32_t m = 0; m < num_meshes; ++m)
        for (uint32_t e = 0; e < num_bins; ++e) {
            tab.mu[e * kMaxMeshes + m] = mu[m * num_bins + e];
            tab.sigma[e * kMaxMeshes + m] = sigma[m * num_bins + e];
        }
    tab.num_bins = num_bins;
    tab.miss = spectrum_miss(tab.weight, num_bins);
    const uint32_t lg = (uint32_t)scatter_bin_log2(bin), th = scatter_tile_rows(lg);
    auto kernel = k_scatter_source<kMaxMeshes>;
    if (num_meshes <= 2u) kernel = k_scatter_source<2>;
    else if (num_meshes <= 4u) kernel = k_scatter_source<4>;
    else if (num_meshes <= 8u) kernel = k_scatter_source<8>;
    const dim3 grid((width + kScatterTile - 1u) / kScatterTile, (height + th - 1u) / th, num_planes);
    hipLaunchKernelGGL(kernel, grid, dim3(kScatterThreads), 0, stream, d_paths, d_open, width, height, num_meshes, lg, tab,
                       d_lbuffer, d_source);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_scatter_source_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                              const float* d_paths, const uint16_t* d_open, const float* weight, const float* mu,
                              const float* sigma, uint32_t num_bins, uint32_t bin, float* d_lbuffer, float* d_source,
                              void* stream)
{
    if (const char* why = scatter_source_arguments(width, height, num_planes, num_meshes, d_paths, d_open, weight, mu, sigma,
                                                   num_bins, bin, d_lbuffer, d_source))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_scatter_source(ctx, width, height, num_planes, num_meshes, d_paths, d_open, weight, mu, sigma, num_bins,
                                 bin, d_lbuffer, d_source, (hipStream_t)stream);
}

int xrt_scatter_source(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t num_meshes,
                       const float* paths, const uint16_t* open, const float* weight, const float* mu, const float* sigma,
                       uint32_t num_bins, uint32_t bin, float* lbuffer, float* source)
{
    if (const char* why = scatter_source_arguments(width, height, num_planes, num_meshes, paths, open, weight, mu, sigma,
                                                   num_bins, bin, lbuffer, source))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)width * height * num_planes;
    const size_t nc = (size_t)((width + bin - 1u) / bin) * ((height + bin - 1u) / bin) * num_planes;
    DeviceScratch s(ctx, ctx->host_stream, "scatter source");
    const float* dp = s.upload(paths, n * num_meshes);
    const uint16_t* dopen = s.upload(open, n);
    float* dl = s.alloc<float>(n, lbuffer != nullptr);
    float* ds = s.alloc<float>(nc);
    if (s.rc()) return s.rc();
    if (int rc = launch_scatter_source(ctx, width, height, num_planes, num_meshes, dp, dopen, weight, mu, sigma, num_bins, bin,
                                       dl, ds, ctx->host_stream))
        return rc;
    s.download(lbuffer, (const float*)dl, n);
    s.download(source, (const float*)ds, nc);
    return s.finish();
}

// The launch of k_scatter_add (validated arguments, device pointers).
static int launch_scatter_add(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                              const float* d_blurred, uint32_t num_kernels, const float* amp, const float* d_primary,
                              float* d_out, float* d_out_scatter, uint8_t* d_out_u8, hipStream_t stream)
{
    ScatterAmps amps = {};              // by value, as the tables
    std::copy(amp, amp + num_kernels, amps.amp);
    amps.num = num_kernels;
    const dim3 grid((width + kScatterTile - 1u) / kScatterTile, (height + kScatterTile - 1u) / kScatterTile, num_planes);
    hipLaunchKernelGGL(k_scatter_add, grid, dim3(kScatterThreads), 0, stream, d_blurred, d_primary, width, height,
                       (uint32_t)scatter_bin_log2(bin), amps, d_out, d_out_scatter, d_out_u8);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_scatter_add_device(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                           const float* d_blurred, uint32_t num_kernels, const float* amp, const float* d_primary,
                           float* d_out, float* d_out_scatter, uint8_t* d_out_u8, void* stream)
{
    if (const char* why = scatter_add_arguments(width, height, num_planes, bin, d_blurred, num_kernels, amp, d_primary, d_out,
                                                d_out_scatter, d_out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    return launch_scatter_add(ctx, width, height, num_planes, bin, d_blurred, num_kernels, amp, d_primary, d_out,
                              d_out_scatter, d_out_u8, (hipStream_t)stream);
}

int xrt_scatter_add(xrt_context* ctx, uint32_t width, uint32_t height, uint32_t num_planes, uint32_t bin,
                    const float* blurred, uint32_t num_kernels, const float* amp, const float* primary, float* out,
                    float* out_scatter, uint8_t* out_u8)
{
    if (const char* why = scatter_add_arguments(width, height, num_planes, bin, blurred, num_kernels, amp, primary, out,
                                                out_scatter, out_u8))
        return fail(ctx, XRT_ERR_ARGUMENT, why);
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)width * height * num_planes;
    const size_t nc = (size_t)((width + bin - 1u) / bin) * ((height + bin - 1u) / bin) * num_planes * num_kernels;
    DeviceScratch s(ctx, ctx->host_stream, "scatter add");
    const float* db = s.upload(blurred, nc);
    const float* dprim = s.upload(primary, n);
    float* dout = s.alloc<float>(n, out != nullptr);
    float* dsc = s.alloc<float>(n, out_scatter != nullptr);
    uint8_t* du8 = s.alloc<uint8_t>(n, out_u8 != nullptr);
    if (s.rc()) return s.rc();
    if (int rc = launch_scatter_add(ctx, width, height, num_planes, bin, db, num_kernels, amp, dprim, dout, dsc, du8,
                                    ctx->host_stream))
        return rc;
    s.download(out, (const float*)dout, n);
    s.download(out_scatter, (const float*)dsc, n);
    s.download(out_u8, (const uint8_t*)du8, n);
    return s.finish();
}

// Render of the L-buffer plane and the fork's hole fill over it, into host buffers.
static int render_and_fill(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                           uint8_t* image_u8, xrt_stats* stats)
{
    int rc = check_camera(ctx, camera, 0, camera ? camera->height : 0);
    if (rc) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)camera->width * camera->height;
    if ((rc = stage_planes(ctx, n))) return rc;
    if ((rc = enqueue_render(ctx, camera, 0, camera->height, nullptr, ctx->d_lbuffer.get(), nullptr, ctx->host_stream)))
        return rc;
    if ((rc = xrt_hole_fill_device(ctx, camera->width, camera->height, ctx->d_lbuffer.get(),
                                   image ? ctx->d_image.get() : nullptr, image_u8 ? ctx->d_u8.get() : nullptr,
                                   ctx->host_stream)))
        return rc;
    const std::vector<D2HCopy> copies =
        plane_copies(n, image, ctx->d_image.get(), lbuffer, ctx->d_lbuffer.get(), image_u8, ctx->d_u8.get());
    if ((rc = d2h_copy(ctx, ctx->host_stream, copies))) return rc;
    xrt_stats local;
    return xrt_read_stats(ctx, stats ? stats : &local);
}

int xrt_render_signed(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                      uint8_t* image_u8, xrt_stats* stats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (ctx->model != kModelSigned) return fail(ctx, XRT_ERR_ARGUMENT, "xrt_render_signed needs XRT_MODEL_SIGNED");
    return render_and_fill(ctx, camera, image, lbuffer, image_u8, stats);
}

int xrt_render_materials(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                         uint8_t* image_u8, xrt_stats* stats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (ctx->model != kModelMaterials)
        return fail(ctx, XRT_ERR_ARGUMENT, "xrt_render_materials needs xrt_set_materials");
    return render_and_fill(ctx, camera, image, lbuffer, image_u8, stats);
}

int xrt_render_spectrum(xrt_context* ctx, const xrt_camera* camera, float* image, float* lbuffer,
                        uint8_t* image_u8, xrt_stats* stats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (ctx->model != kModelSpectrum)
        return fail(ctx, XRT_ERR_ARGUMENT, "xrt_render_spectrum needs xrt_set_spectrum");
    return render_and_fill(ctx, camera, image, lbuffer, image_u8, stats);
}

int xrt_set_miss_code(xrt_context* ctx, uint32_t bits)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (bits && bits != kMissTransit) return fail(ctx, XRT_ERR_ARGUMENT, "miss code must be 0 or XRT_MISS_TRANSIT");
    ctx->miss_code = bits;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_expand_rows_device(xrt_context* ctx, uint64_t num_pixels, float* d_lbuffer, float* d_image,
                           uint8_t* d_u8, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_pixels && !d_lbuffer) return fail(ctx, XRT_ERR_ARGUMENT, "lbuffer is NULL");
    if (!num_pixels) return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t threads = (num_pixels + 3) / 4;
    hipLaunchKernelGGL(k_expand, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_lbuffer, d_image, d_u8, num_pixels);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_set_hit_capacity(xrt_context* ctx, uint32_t capacity)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (capacity > (uint32_t)kMaxHits)
        return fail(ctx, XRT_ERR_ARGUMENT, "capacity > " + std::to_string(kMaxHits));
    ctx->hit_capacity = capacity ? capacity : (uint32_t)kMaxHits;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_set_bin_capacity(xrt_context* ctx, uint64_t entries)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    ctx->bin_force_cap = (size_t)entries;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_plan_region_map(xrt_context* ctx, uint32_t width, uint32_t rows, uint32_t* map, uint64_t n_regions,
                        uint32_t* n_packed)
{
    if (!ctx || !map || !n_packed) return fail(ctx, XRT_ERR_ARGUMENT, "NULL argument");
    const uint32_t rx = (width + kRegion - 1) / kRegion, ry = (rows + kRegion - 1) / kRegion;
    if (n_regions != (uint64_t)rx * ry)
        return fail(ctx, XRT_ERR_ARGUMENT, "map must hold ceil(width/32) x ceil(rows/32) regions");
    const SlotLayout& L = ctx->compact_layout;
    const bool layout = L.rx == rx && L.ry == ry && L.slot_region.size() == n_regions;
    const bool planned = ctx->last_fill_regions > 0 && ctx->plan_valid && layout;
    // no region of the geometry is empty: every region travels, in slot order
    // (the order of the hit layout's tiles)
    const bool whole = !ctx->plan_valid && ctx->last_fill_regions == 0 && layout && ctx->geo.compact &&
                       ctx->geo.bin_key_valid && ctx->geo.last_key.same(ctx->geo.bin_key);
    if (!planned && !whole) {                       // every region travels
        for (uint64_t r = 0; r < n_regions; ++r) map[r] = (uint32_t)r;
        *n_packed = (uint32_t)n_regions;
        return XRT_OK;
    }
    for (uint64_t s = 0; s < n_regions; ++s)
        map[L.slot_region[s]] = s < ctx->plan_tile_slots ? (uint32_t)s : kEmpty;
    *n_packed = ctx->plan_tile_slots;
    return XRT_OK;
}

int xrt_pack_regions_device(xrt_context* ctx, uint32_t width, uint32_t rows, const uint32_t* d_map,
                            const float* d_lbuffer, float* d_packed, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    const uint32_t rx = (width + kRegion - 1) / kRegion, ry = (rows + kRegion - 1) / kRegion;
    if (!rx || !ry) return XRT_OK;
    if (!d_map || !d_lbuffer || !d_packed) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(d_packed) & 15u) return fail(ctx, XRT_ERR_ARGUMENT, "packed buffer not 16-B aligned");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_pack_regions, dim3(rx * ry), dim3(256), 0, (hipStream_t)stream, d_lbuffer, d_packed, d_map,
                       width, rows, rx);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_unpack_regions_device(xrt_context* ctx, uint32_t width, uint32_t rows, const uint32_t* d_map,
                              const float* d_packed, float* d_lbuffer, float* d_image, uint8_t* d_u8, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    const uint32_t rx = (width + kRegion - 1) / kRegion, ry = (rows + kRegion - 1) / kRegion;
    if (!rx || !ry) return XRT_OK;
    if (!d_map || !d_packed) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(d_packed) & 15u) return fail(ctx, XRT_ERR_ARGUMENT, "packed buffer not 16-B aligned");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_unpack_regions, dim3(rx * ry), dim3(256), 0, (hipStream_t)stream, d_packed, d_map,
                       d_lbuffer, d_image, d_u8, width, rows, rx);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_unpack_blocks_device(xrt_context* ctx, uint32_t width, uint64_t n_blocks, const uint32_t* d_desc,
                             const float* d_packed, float* d_lbuffer, float* d_image, uint8_t* d_u8, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (!n_blocks) return XRT_OK;
    if (!d_desc || !d_packed) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    if (n_blocks > 0x7FFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many blocks");
    if ((reinterpret_cast<uintptr_t>(d_packed) | reinterpret_cast<uintptr_t>(d_desc)) & 15u)
        return fail(ctx, XRT_ERR_ARGUMENT, "packed buffer or descriptors not 16-B aligned");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_unpack_blocks, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, d_packed,
                       reinterpret_cast<const uint4*>(d_desc), d_lbuffer, d_image, d_u8, width);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_set_transit_layout(xrt_context* ctx, uint64_t packed_floats)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    ctx->packed_cap = packed_floats;
    if (packed_floats) ctx->hits_cap = 0;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_set_transit_hits(xrt_context* ctx, uint64_t capacity_words)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    ctx->hits_cap = capacity_words;
    if (capacity_words) ctx->packed_cap = 0;
    ++ctx->state_gen;
    return XRT_OK;
}

int xrt_plan_hit_layout(xrt_context* ctx, uint32_t* tile_hits, uint64_t capacity, uint64_t* n_tiles,
                        uint64_t* words)
{
    if (!ctx || !n_tiles || !words) return fail(ctx, XRT_ERR_ARGUMENT, "NULL argument");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);
    if (rc) return rc;
    const FrameSet* fs = ctx->last_set;
    // the last frame rendered the lists' geometry over its fill plan (or, with
    // no empty region, every region in slot order): its records s * 16 + t
    // (s < the plan's tile slots) are the plan's tiles
    const bool fill_frame = ctx->plan_valid && ctx->last_fill_regions > 0;
    const bool whole_frame = !ctx->plan_valid && ctx->last_fill_regions == 0;
    if (!fs || !fs->binned || !ctx->geo.bin_key_valid || !ctx->geo.compact || !(fill_frame || whole_frame) ||
        !ctx->geo.last_key.same(ctx->geo.bin_key) || (uint64_t)ctx->plan_tile_slots * kWavesPerRegion > fs->rendered_blocks)
        return fail(ctx, XRT_ERR_ARGUMENT, "the hit plan needs a BINNED frame rendered over its geometry's fill "
                                           "plan just before");
    const uint32_t tiles = ctx->plan_tile_slots * kWavesPerRegion;
    std::vector<BlockStats> rec(tiles);
    if (tiles) XRT_HIP(ctx, hipMemcpy(rec.data(), fs->block_stats.get(), tiles * sizeof(BlockStats), hipMemcpyDeviceToHost));
    std::vector<uint32_t> off(tiles + 1u);
    uint64_t run = 0;
    for (uint32_t i = 0; i < tiles; ++i) {
        off[i] = (uint32_t)run;
        run += rec[i].hit_rays;
        if (tile_hits && i < capacity) tile_hits[i] = rec[i].hit_rays;
    }
    if (run + 2ull * tiles > 0xFFFFFFFFull) return fail(ctx, XRT_ERR_OVERFLOW, "hit message exceeds 2^32 words");
    off[tiles] = (uint32_t)run;
    if ((rc = ensure(ctx, ctx->d_hit_off, (size_t)tiles + 1u))) return rc;
    XRT_HIP(ctx, hipMemcpy(ctx->d_hit_off.get(), off.data(), off.size() * 4u, hipMemcpyHostToDevice));
    ctx->hit_key = ctx->geo.bin_key;
    ctx->hit_tiles = tiles;
    ctx->hit_words = 2ull * tiles + run;
    ctx->hit_valid = true;
    ++ctx->state_gen;                   // frames prepared ahead carry the old plan
    *n_tiles = tiles;
    *words = ctx->hit_words;
    return XRT_OK;
}

int xrt_unpack_hits_device(xrt_context* ctx, uint32_t width, uint64_t n_blocks, const uint32_t* d_desc,
                           const uint32_t* d_tdesc, const uint32_t* d_msg, float* d_lbuffer, float* d_image,
                           uint8_t* d_u8, uint32_t* d_bad, void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (!n_blocks) return XRT_OK;
    if (!d_desc || !d_tdesc || !d_msg) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    if (n_blocks > 0x7FFFFFFFull) return fail(ctx, XRT_ERR_ARGUMENT, "too many blocks");
    if (((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_tdesc)) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_msg) & 7u))
        return fail(ctx, XRT_ERR_ARGUMENT, "descriptors not 16-B aligned or message not 8-B aligned");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_unpack_hits, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, d_msg,
                       reinterpret_cast<const uint4*>(d_desc), reinterpret_cast<const uint4*>(d_tdesc), d_lbuffer,
                       d_image, d_u8, width, d_bad);
    XRT_HIP(ctx, hipGetLastError());
    return XRT_OK;
}

int xrt_debug_fill_regions(xrt_context* ctx, uint32_t* regions)
{
    if (!ctx || !regions) return XRT_ERR_ARGUMENT;
    *regions = ctx->last_fill_regions;
    return XRT_OK;
}

int xrt_debug_geometry_counters(xrt_context* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_sizings;
    counters[1] = ctx->hp_reused;
    counters[2] = ctx->hp_plan_miss;
    counters[3] = ctx->hp_overflow;
    return XRT_OK;
}

int xrt_debug_first_frames(xrt_context* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_dev_first;
    counters[1] = ctx->hp_dev_first_recounts;
    counters[2] = ctx->dev_first_pairs;
    counters[3] = ctx->dev_first_pool;
    return XRT_OK;
}

int xrt_debug_host_call_ms(xrt_context* ctx, double ms[16])
{
    if (!ctx || !ms) return XRT_ERR_ARGUMENT;
    std::copy(ctx->host_call_ms, ctx->host_call_ms + kHostCallFields, ms);
    return XRT_OK;
}

int xrt_debug_prep_times(xrt_context* ctx, int enable, uint32_t* dst, uint64_t capacity, uint64_t* n_waves)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (enable >= 0) ctx->prep_times_on = enable != 0;
    if (n_waves) *n_waves = ctx->prep_times_n;
    if (!dst || !ctx->d_prep_times.get() || !ctx->prep_times_n) return XRT_OK;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);
    if (rc) return rc;
    const size_t n = std::min<size_t>(capacity, ctx->prep_times_n);
    XRT_HIP(ctx, hipMemcpy(dst, ctx->d_prep_times.get(), n * 2 * sizeof(uint4), hipMemcpyDeviceToHost));
    return XRT_OK;
}

int xrt_debug_direction_grid(const xrt_camera* camera, int grids[2])
{
    if (!camera || !grids) return XRT_ERR_ARGUMENT;
    const CullParams cp = make_cull_params(*camera);
    grids[0] = cp.dir_grid;
    grids[1] = direction_grid(*camera, cp.dmax, true);
    return XRT_OK;
}

// Host evaluation of the tile cull's footprints (compute_footprint, same
// source, host-compiled): the CPU suite checks them against every hit of the
// oracle without a GPU.
int xrt_host_footprints(const xrt_camera* camera, const float* tris, uint64_t n, float* footprint16)
{
    if (!camera || (n && (!tris || !footprint16))) return XRT_ERR_ARGUMENT;
    host_footprints(*camera, tris, n, footprint16);
    return XRT_OK;
}

int xrt_debug_set_tile_plan(xrt_context* ctx, int on)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (ctx->tile_plan_enabled != (on != 0)) ++ctx->state_gen;   // frames prepared ahead are dropped
    ctx->tile_plan_enabled = on != 0;
    return XRT_OK;
}

int xrt_debug_tile_plan(xrt_context* ctx, uint64_t counters[2])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_tile_plan_frames;
    counters[1] = ctx->hp_tile_plans;
    return XRT_OK;
}

int xrt_debug_set_ray_table(xrt_context* ctx, int on)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    ctx->ray_enabled = on != 0;        // read at every launch; a table kept while off stays valid for its key
    return XRT_OK;
}

int xrt_debug_ray_table_counters(xrt_context* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_ray_fills;
    counters[1] = ctx->hp_ray_frames;
    counters[2] = ctx->hp_ray_computed;
    counters[3] = ctx->d_rays.cap() * sizeof(float);
    return XRT_OK;
}

int xrt_debug_ray_table_read(xrt_context* ctx, float* dst, uint64_t floats, uint32_t dims[4])
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (!ctx->ray_valid) return fail(ctx, XRT_ERR_NO_MESH, "no ray table is valid");
    const xrt_context::RayKey& k = ctx->ray_key;
    const uint64_t n = ray_table_floats(k.width, k.row_begin, k.row_end);
    if (!dst || floats < n) return fail(ctx, XRT_ERR_ARGUMENT, "dst is NULL or smaller than the table");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    XRT_HIP(ctx, ctx->ray_filled.wait());
    XRT_HIP(ctx, hipMemcpy(dst, ctx->d_rays.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    if (dims) {
        dims[0] = k.width;
        dims[1] = k.height;
        dims[2] = k.row_begin;
        dims[3] = k.row_end;
    }
    return XRT_OK;
}

int xrt_debug_ray_table_index(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t row,
                              uint32_t col, uint64_t* index, uint64_t* floats)
{
    if (!width || !height || row_begin >= row_end || row_end > height || row < row_begin || row >= row_end ||
        col >= width || !index)
        return XRT_ERR_ARGUMENT;
    *index = ray_table_index(width, row_begin, row, col);
    if (floats) *floats = ray_table_floats(width, row_begin, row_end);
    return XRT_OK;
}

int xrt_debug_pipeline_counters(xrt_context* ctx, uint64_t counters[4])
{
    if (!ctx || !counters) return XRT_ERR_ARGUMENT;
    counters[0] = ctx->hp_ahead_used;
    counters[1] = ctx->hp_ahead_dropped;
    counters[2] = ctx->hp_launch_nowait;
    counters[3] = ctx->hp_host_waits;
    return XRT_OK;
}

int xrt_set_fill_plan(xrt_context* ctx, int mode)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (mode < 0 || mode > 2) return fail(ctx, XRT_ERR_ARGUMENT, "fill plan mode must be 0, 1 or 2");
    ctx->fill_plan = mode;
    ctx->geo.resize_next_frame();       // the next frame re-sizes and re-plans
    ctx->plan_valid = false;
    ++ctx->state_gen;                   // frames prepared ahead are stale
    return XRT_OK;
}

int xrt_debug_block_records(xrt_context* ctx, void* dst, uint64_t capacity, uint64_t* n_records)
{
    if (!ctx || !n_records) return XRT_ERR_ARGUMENT;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->pending) {
        XRT_HIP(ctx, hipStreamSynchronize(ctx->last_stream));
        ctx->pending = false;
    }
    const FrameSet* fs = ctx->last_set;
    *n_records = fs ? fs->rendered_blocks : 0u;
    const size_t bytes = std::min<size_t>((size_t)capacity, (size_t)*n_records * sizeof(BlockStats));
    if (bytes && dst) XRT_HIP(ctx, hipMemcpy(dst, fs->block_stats.get(), bytes, hipMemcpyDeviceToHost));
    return XRT_OK;
}

int xrt_debug_wave_times(xrt_context* ctx, uint32_t frames_back, uint32_t* dst, uint64_t capacity,
                         uint64_t* n_records)
{
    if (!ctx || !n_records) return XRT_ERR_ARGUMENT;
    if (frames_back >= (uint32_t)kFrameSets)
        return fail(ctx, XRT_ERR_ARGUMENT, "frames_back must be < " + std::to_string(kFrameSets));
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sync_context(ctx);
    if (rc) return rc;
    const FrameSet* fs = ctx->last_set
                             ? &ctx->sets[((ctx->last_set - ctx->sets) + kFrameSets - (int)frames_back) % kFrameSets]
                             : nullptr;
    // the set's last RENDER's count (a frame prepared ahead into the set since has its own)
    *n_records = fs && fs->last_times ? fs->rendered_blocks : 0u;
    const size_t n = std::min<size_t>((size_t)capacity, (size_t)*n_records);
    if (n && dst) XRT_HIP(ctx, hipMemcpy(dst, fs->last_times, n * sizeof(uint2), hipMemcpyDeviceToHost));
    return XRT_OK;
}

int xrt_render_rows_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin,
                           uint32_t row_end, float* d_image, float* d_lbuffer, uint8_t* d_u8,
                           void* stream)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    return enqueue_render(ctx, camera, row_begin, row_end, d_image, d_lbuffer, d_u8,
                          (hipStream_t)stream, true);
}

int xrt_render_frames_device(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                             uint32_t n_frames, uint32_t n_sets, float* const* d_image, float* const* d_lbuffer,
                             uint8_t* const* d_u8, void* const* streams)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (n_frames && !n_sets) return fail(ctx, XRT_ERR_ARGUMENT, "n_sets must be >= 1");
    for (uint32_t k = 0; k < n_frames; ++k) {
        const uint32_t s = k % n_sets;
        int rc = enqueue_render(ctx, camera, row_begin, row_end, d_image ? d_image[s] : nullptr,
                                d_lbuffer ? d_lbuffer[s] : nullptr, d_u8 ? d_u8[s] : nullptr,
                                streams ? (hipStream_t)streams[s] : nullptr, true);
        if (rc) return rc;
    }
    return XRT_OK;
}

int xrt_render_frames(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin, uint32_t row_end,
                      uint32_t n_frames, float* image, float* lbuffer, uint8_t* image_u8, xrt_stats* stats,
                      double* ms_per_frame)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    int rc = check_camera(ctx, camera, row_begin, row_end);
    if (rc) return rc;
    if (!n_frames) return fail(ctx, XRT_ERR_ARGUMENT, "n_frames must be >= 1");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)(row_end - row_begin) * camera->width;
    if ((rc = stage_planes(ctx, n))) return rc;
    float* di = image ? ctx->d_image.get() : nullptr;
    float* dl = lbuffer ? ctx->d_lbuffer.get() : nullptr;
    uint8_t* du = image_u8 ? ctx->d_u8.get() : nullptr;
    void* st = ctx->host_stream;
    const auto t0 = HostClock::now();
    if ((rc = xrt_render_frames_device(ctx, camera, row_begin, row_end, n_frames, 1, &di, &dl, &du, &st))) return rc;
    XRT_HIP(ctx, hipStreamSynchronize(ctx->host_stream));
    if (ms_per_frame)
        *ms_per_frame = std::chrono::duration<double, std::milli>(HostClock::now() - t0).count() / n_frames;
    const std::vector<D2HCopy> copies =
        plane_copies(n, image, ctx->d_image.get(), lbuffer, ctx->d_lbuffer.get(), image_u8, ctx->d_u8.get());
    if ((rc = d2h_copy(ctx, ctx->host_stream, copies))) return rc;
    xrt_stats local;
    return xrt_read_stats(ctx, stats ? stats : &local);
}

int xrt_read_stats(xrt_context* ctx, xrt_stats* stats)
{
    if (!ctx || !stats) return XRT_ERR_ARGUMENT;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    std::memset(stats, 0, sizeof *stats);
    stats->kernel = (uint32_t)ctx->last_kernel;
    const FrameSet* fs = ctx->last_set;
    if (!fs || !fs->rendered_blocks) {
        if (ctx->pending) XRT_HIP(ctx, hipStreamSynchronize(ctx->last_stream));
        ctx->pending = false;
        return XRT_OK;
    }
    // The last render's records (and where its timing records went, and its
    // BinState) summed on the device behind the render, on its stream: one
    // record comes back instead of every wave's.
    const uint32_t n = fs->rendered_blocks;
    const hipStream_t s = ctx->last_stream;
    const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>(kReduceMaxBlocks, (n + 4 * kReduceThreads - 1) /
                                                                                          (4 * kReduceThreads)));
    hipLaunchKernelGGL(k_reduce_stats, dim3(blocks), dim3(kReduceThreads), 0, s, fs->block_stats.get(), fs->last_times, n,
                       fs->binned ? (const BinState*)fs->last_state : nullptr, ctx->d_stats_partial.get(), ctx->d_stats_done.get(),
                       ctx->d_stats_out.get());
    XRT_HIP(ctx, hipGetLastError());
    XRT_HIP(ctx, hipMemcpyAsync(ctx->h_stats.get(), ctx->d_stats_out.get(), sizeof(StatsSum), hipMemcpyDeviceToHost, s));
    XRT_HIP(ctx, hipStreamSynchronize(s));
    ctx->pending = false;
    const StatsSum& t = *ctx->h_stats.get();
    stats->rays = t.rays;
    stats->hit_rays = t.hit_rays;
    stats->odd_rays = t.odd_rays;
    stats->overflow_rays = t.overflow_rays;
    stats->hits = t.hits;
    stats->tile_tests = t.tile_tests;
    stats->candidates = t.candidates;
    stats->max_hits = t.max_hits;
    stats->kernel_ms = fs->last_times && t.span_hi > t.span_lo ? (double)(t.span_hi - t.span_lo) / kTicksPerMs : 0.0;
    stats->global_triangles = fs->binned ? t.global_count : 0u;
    if (fs->binned && t.overflow && !ctx->bin_force_cap) {   // the next frame re-sizes its lists
        ctx->geo.resize_next_frame();
        ++ctx->state_gen;
    }
    return XRT_OK;
}

int xrt_timing_begin(xrt_context* ctx)
{
    if (!ctx) return XRT_ERR_ARGUMENT;
    if (ctx->timing) {                 // a region still open: end it (its results are dropped)
        double ms = 0.0;
        uint64_t n = 0;
        if (int rc = xrt_timing_end(ctx, &ms, &n)) return rc;
    }
    // Frames in flight may mark their completion with events of the previous
    // timed region, which this one re-records: wait for them first.
    for (FrameSet& fs : ctx->sets) {
        if (fs.done_valid) XRT_HIP(ctx, hipEventSynchronize(fs.done_ev));
        fs.done_valid = false;
    }
    // the region's record space and events, before the region
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t last_blocks = ctx->last_set ? ctx->last_set->n_blocks : 0u;
    const size_t space = std::min(kTimingRecords, std::max<size_t>((size_t)1 << 20, kTimingFrames * last_blocks));
    bool have = false;
    for (auto& c : ctx->tchunks) have = have || c.p.cap() >= space;
    if (!have)
        if (int rc = region_chunk(ctx, space)) return rc;
    ctx->timing_space = space;
    if (int rc = region_events(ctx, kTimingEvents)) return rc;
    ctx->timing = true;
    ctx->tev_used = 0;
    ctx->timed_frames = 0;
    ctx->timed_records = 0;
    for (auto& c : ctx->tchunks) c.used = 0;
    ctx->tsamples.clear();
    return XRT_OK;
}

int xrt_timing_end(xrt_context* ctx, double* total_ms, uint64_t* launches)
{
    if (!ctx || !total_ms || !launches) return XRT_ERR_ARGUMENT;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    double ev = 0.0;
    for (size_t i = 0; i + 1 < ctx->tev_used; i += 2) {
        XRT_HIP(ctx, hipEventSynchronize(ctx->tev[i + 1].get()));
        float ms = 0.0f;
        XRT_HIP(ctx, hipEventElapsedTime(&ms, ctx->tev[i].get(), ctx->tev[i + 1].get()));
        ev += ms;
    }
    ctx->event_ms = ev;
    ctx->event_launches = ctx->tev_used / 2;
    if (int rc = sync_context(ctx)) return rc;     // the sampled frames' records are written
    double sum = 0.0;
    std::vector<uint2> t;
    for (const auto& smp : ctx->tsamples) {
        t.resize(smp.n);
        XRT_HIP(ctx, hipMemcpy(t.data(), smp.p, smp.n * sizeof(uint2), hipMemcpyDeviceToHost));
        sum += records_span_ms(t);
    }
    *total_ms = sum;
    *launches = ctx->tsamples.size();
    ctx->tsamples.clear();
    ctx->timing = false;
    ctx->tev_used = 0;
    // Each set's last records back into its own buffer (xrt_read_stats and
    // xrt_debug_wave_times read them there), then the chunks go: a context
    // keeps at most one small chunk (kKeptTimingBytes) for its next region.
    for (FrameSet& fs : ctx->sets) {
        if (fs.last_times && fs.last_times != fs.times.get() && fs.times.get() && fs.rendered_blocks <= fs.times.cap())
            XRT_HIP(ctx, hipMemcpy(fs.times.get(), fs.last_times, fs.rendered_blocks * sizeof(uint2),
                                   hipMemcpyDeviceToDevice));
        if (fs.last_times) fs.last_times = fs.times.get();
    }
    size_t keep = ctx->tchunks.size();
    for (size_t k = 0; k < ctx->tchunks.size(); ++k)
        if (ctx->tchunks[k].p.cap() * sizeof(uint2) <= kKeptTimingBytes &&
            (keep == ctx->tchunks.size() || ctx->tchunks[k].p.cap() > ctx->tchunks[keep].p.cap()))
            keep = k;
    std::vector<xrt_context::TimesChunk> kept;
    if (keep < ctx->tchunks.size()) {
        kept.push_back(std::move(ctx->tchunks[keep]));
        kept.back().used = 0;
    }
    ctx->tchunks = std::move(kept);                // the others are freed
    return XRT_OK;
}

int xrt_timing_events(xrt_context* ctx, double* total_ms, uint64_t* launches)
{
    if (!ctx || !total_ms || !launches) return XRT_ERR_ARGUMENT;
    *total_ms = ctx->event_ms;
    *launches = ctx->event_launches;
    return XRT_OK;
}

int xrt_render_rows(xrt_context* ctx, const xrt_camera* camera, uint32_t row_begin,
                    uint32_t row_end, float* image, float* lbuffer, uint8_t* image_u8,
                    xrt_stats* stats)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    int rc = check_camera(ctx, camera, row_begin, row_end);
    if (rc) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    double* hc = ctx->host_call_ms;
    const auto t0 = HostClock::now();
    auto lap = [&](int k, HostClock::time_point& t) {
        const auto now = HostClock::now();
        hc[k] = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    };
    auto t = t0;
    std::fill(hc, hc + kHostCallFields, 0.0);
    double acc0[kAccFields];
    std::copy(ctx->acc_ms, ctx->acc_ms + kAccFields, acc0);
    const size_t n = (size_t)(row_end - row_begin) * camera->width;
    if ((rc = stage_planes(ctx, n))) return rc;
    lap(0, t);
    // the context's own non-blocking stream (not the null stream)
    rc = enqueue_render(ctx, camera, row_begin, row_end, image ? ctx->d_image.get() : nullptr,
                        lbuffer ? ctx->d_lbuffer.get() : nullptr, image_u8 ? ctx->d_u8.get() : nullptr, ctx->host_stream);
    if (rc) return rc;
    XRT_HIP(ctx, hipEventRecord(ctx->host_render_done.get(), ctx->host_stream));
    lap(1, t);
    XRT_HIP(ctx, hipEventSynchronize(ctx->host_render_done.get()));
    lap(2, t);
    const std::vector<D2HCopy> copies =
        plane_copies(n, image, ctx->d_image.get(), lbuffer, ctx->d_lbuffer.get(), image_u8, ctx->d_u8.get());
    if ((rc = d2h_copy(ctx, ctx->host_stream, copies))) return rc;
    lap(3, t);
    double bytes = 0.0;
    for (const D2HCopy& c : copies) bytes += (double)c.bytes;
    hc[4] = ctx->pool ? (double)ctx->pool->size() : 0.0;
    hc[5] = bytes / 1e6;
    xrt_stats local;
    rc = xrt_read_stats(ctx, stats ? stats : &local);
    lap(6, t);
    hc[7] = std::chrono::duration<double, std::milli>(t - t0).count();
    for (int k = 0; k < kAccFields; ++k) hc[8 + k] = ctx->acc_ms[k] - acc0[k];
    return rc;
}

int xrt_probe_intersect(xrt_context* ctx, const float* rays, const float* tris, uint64_t n,
                        uint8_t* hit, float* t)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (n == 0) return XRT_OK;
    if (!rays || !tris || !hit || !t) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, nullptr, "probe");
    const float* dr = s.upload(rays, n * 6);
    const float* dt = s.upload(tris, n * 9);
    float* dout = s.alloc<float>(n);
    uint8_t* dh = s.alloc<uint8_t>(n);
    if (s.rc()) return s.rc();
    hipLaunchKernelGGL(k_probe_intersect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dr, dt, n, dh, dout);
    s.launched();
    s.download(hit, dh, n);
    s.download(t, dout, n);
    return s.finish();
}

int xrt_probe_math(xrt_context* ctx, int op, const float* in, float* outp, uint64_t n)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (op < XRT_PROBE_EXPF || op > XRT_PROBE_LOGF) return fail(ctx, XRT_ERR_ARGUMENT, "bad op");
    if (n == 0) return XRT_OK;
    if (!in || !outp) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceScratch s(ctx, nullptr, "probe");
    const float* di = s.upload(in, n);
    float* dout = s.alloc<float>(n);
    if (s.rc()) return s.rc();
    hipLaunchKernelGGL(k_probe_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, di, dout, n);
    s.launched();
    s.download(outp, dout, n);
    return s.finish();
}

int xrt_probe_materials(xrt_context* ctx, const float* distance, const int32_t* sign_sum, const float* mu,
                        uint32_t num_meshes, float* outp, uint64_t n)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_meshes < 1 || num_meshes > XRT_MAX_MESHES) return fail(ctx, XRT_ERR_ARGUMENT, "bad mesh count");
    if (n == 0) return XRT_OK;
    if (!distance || !mu || !outp) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t terms = (size_t)n * num_meshes;
    DeviceScratch s(ctx, nullptr, "probe");
    const float* dd = s.upload(distance, terms);
    const float* dmu = s.upload(mu, num_meshes);
    const int* ds = s.upload(sign_sum, terms);
    float* dout = s.alloc<float>(n);
    if (s.rc()) return s.rc();
    hipLaunchKernelGGL(k_probe_materials, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dd, ds, dmu, num_meshes,
                       dout, (size_t)n);
    s.launched();
    s.download(outp, dout, n);
    return s.finish();
}

int xrt_probe_spectrum(xrt_context* ctx, const float* distance, const int32_t* sign_sum, const float* weight,
                       const float* mu, uint32_t num_meshes, uint32_t num_bins, float* outp, uint64_t n)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    if (num_meshes < 1 || num_meshes > XRT_MAX_MESHES) return fail(ctx, XRT_ERR_ARGUMENT, "bad mesh count");
    if (num_bins < 1 || num_bins > XRT_MAX_BINS) return fail(ctx, XRT_ERR_ARGUMENT, "bad bin count");
    if (n == 0) return XRT_OK;
    if (!distance || !weight || !mu || !outp) return fail(ctx, XRT_ERR_ARGUMENT, "NULL buffer");
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t terms = (size_t)n * num_meshes, coeffs = (size_t)num_meshes * num_bins;
    DeviceScratch s(ctx, nullptr, "probe");
    const float* dd = s.upload(distance, terms);
    const float* dw = s.upload(weight, num_bins);
    const float* dmu = s.upload(mu, coeffs);
    const int* ds = s.upload(sign_sum, terms);
    float* dout = s.alloc<float>(n);
    if (s.rc()) return s.rc();
    hipLaunchKernelGGL(k_probe_spectrum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dd, ds, dw, dmu, num_meshes,
                       num_bins, dout, (size_t)n);
    s.launched();
    s.download(outp, dout, n);
    return s.finish();
}

int xrt_probe_prep(xrt_context* ctx, const xrt_camera* camera, float* records, float* footprint)
{
    if (!ctx) return fail(nullptr, XRT_ERR_ARGUMENT, "context is NULL");
    int rc = check_camera(ctx, camera, 0, camera ? camera->height : 0);
    if (rc) return rc;
    XRT_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t T = render_tris(ctx);
    if (!T) return XRT_OK;
    if ((rc = sync_context(ctx))) return rc;      // no frame in flight uses the set
    FrameSet& fs = ctx->sets[ctx->next_set];
    if ((rc = ensure(ctx, fs.recs, T))) return rc;
    if ((rc = ensure(ctx, fs.cull, (size_t)T * kCullPlanes))) return rc;
    RenderParams p = make_params(*camera, 0, camera->height, T, ctx->hit_capacity);
    p.model = ctx->model;
    CullParams cp = make_cull_params(*camera);
    BinBuffers nobins = {};
    // (k_pose, when one is due, runs on the prep stream; this k_prep on the null stream)
    const float* soup = nullptr;
    if ((rc = render_soup(ctx, soup))) return rc;
    XRT_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    hipLaunchKernelGGL(k_prep, dim3((unsigned)((T + kPrepWaves * p.prep_tris - 1) / (kPrepWaves * p.prep_tris))),
                       dim3(kPrepThreads), 0, 0, soup,
                       (uint32_t)T, p, cp, fs.recs.get(), fs.cull.get(), nobins, nullptr, nullptr, nullptr, nullptr);
    XRT_HIP(ctx, hipGetLastError());
    if (records)
        XRT_HIP(ctx, hipMemcpy(records, fs.recs.get(), T * sizeof(TriRec), hipMemcpyDeviceToHost));
    if (footprint) {
        // planes [bbox | e0 | e1 | e2] of T float4 -> per triangle 16 floats
        std::vector<float4> planes((size_t)T * kCullPlanes);
        XRT_HIP(ctx, hipMemcpy(planes.data(), fs.cull.get(), planes.size() * sizeof(float4),
                               hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < T; ++i)
            for (int k = 0; k < kCullPlanes; ++k)
                std::memcpy(footprint + 16 * i + 4 * k, &planes[(size_t)k * T + i], sizeof(float4));
    }
    return XRT_OK;
}

// Host evaluation of the device expf restatement (same source, host-compiled);
// lets the CPU test suite check it exhaustively against libm without a GPU.
// Host evaluation of the culled tests' division-free reject (mt_may_hit) and
// of the exact remainder (mt_finish), same source: the CPU suite checks that
// the reject never drops a hit.
void xrt_host_mt_check(const float* det, const float* a, const float* b, const float* tnum, uint64_t n,
                       uint8_t* may_hit, uint8_t* hit, float* t)
{
    for (uint64_t i = 0; i < n; ++i) {
        bool h = false;
        t[i] = mt_finish(det[i], a[i], b[i], tnum[i], h);
        hit[i] = h ? 1 : 0;
        may_hit[i] = mt_may_hit(det[i], a[i], b[i], tnum[i]) ? 1 : 0;
    }
}

void xrt_host_expf_batch(const float* in, float* outp, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) outp[i] = xrt_expf(in[i]);
}

void xrt_host_exp_batch(const double* in, double* outp, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) outp[i] = xrt_exp(in[i]);
}

void xrt_host_signed_lbuffer_batch(const float* distance, const int32_t* sign_sum, float mu, float* outp,
                                   uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) outp[i] = signed_lbuffer(distance[i], sign_sum ? sign_sum[i] : 0, mu);
}

void xrt_host_materials_lbuffer_batch(const float* distance, const int32_t* sign_sum, const float* mu,
                                      uint32_t num_meshes, float* outp, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        float L = 80.0f;
        for (uint32_t m = 0; m < num_meshes; ++m)
            L = materials_update(L, distance[i * num_meshes + m], sign_sum ? sign_sum[i * num_meshes + m] : 0, mu[m]);
        outp[i] = L;
    }
}

void xrt_host_spectrum_lbuffer_batch(const float* distance, const int32_t* sign_sum, const float* weight,
                                     const float* mu, uint32_t num_meshes, uint32_t num_bins, float* outp,
                                     uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const float* d = distance + i * num_meshes;
        const int32_t* s = sign_sum ? sign_sum + i * num_meshes : nullptr;
        outp[i] = spectrum_lbuffer(
            num_meshes, num_bins, [=](uint32_t m) { return d[m]; }, [=](uint32_t m) { return s ? s[m] : 0; },
            [=](uint32_t m, uint32_t e) { return mu[m * num_bins + e]; }, [=](uint32_t e) { return weight[e]; });
    }
}

float xrt_host_spectrum_miss(const float* weight, uint32_t num_bins) { return spectrum_miss(weight, num_bins); }

}  // extern "C"

#include "xrt_multi.inc"
