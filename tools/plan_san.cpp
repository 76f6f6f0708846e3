// plan_san.cpp -- the host arithmetic of a frame's list sizing
// (simpleraytracing_amd/csrc/xrt_plan_host.inc: choose_list_mode over a
// GeometryState, centre_first_order and plan_lists) over its sequences and
// edge cases, as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Isimpleraytracing_amd/csrc tools/plan_san.cpp \
//         -o plan_san
//
// The expected values are literals worked out by hand for the small grids and,
// for the larger ones, a naive restatement (an O(n^2) selection in integer
// arithmetic, no sort) -- never the functions under test.  Exact-size heap
// buffers, so that a read one counter past the counts is seen.  Prints
// "plan_san: OK" and returns 0 when every call returned what it should
// (tests/test_plan_cpu.py runs it).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "xrt.h"

#include "xrt_plan_host.inc"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("plan_san: line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using U32s = std::vector<uint32_t>;

static uint32_t lcg(uint32_t& s) { return (s = s * 1664525u + 1013904223u) >> 8; }

// ---------------------------------------------------------------- the decision

// Camera `id` (its origin's x) over a width x height frame, all rows, mesh of 100 triangles.
static BinKey key_of(float id, uint32_t width = 400, uint32_t height = 300)
{
    BinKey k;
    std::memset(&k, 0, sizeof k);
    k.cam.origin[0] = id;
    k.cam.width = width;
    k.cam.height = height;
    k.row_end = height;
    k.T = 100;
    k.gen = 1;
    return k;
}

// A BINNED attenuation frame of a host-buffer call on an ordinary context.
static FrameFacts facts(const BinKey& k)
{
    return FrameFacts{k, true, true, false, false, true, true, true};
}

// What the host sizing does to the state once its layout is uploaded.
static void sized(GeometryState& g)
{
    g.compact = true;
    g.bin_key = g.last_key;
    g.bin_key_valid = true;
}

#define STEP(g, f, want) EXPECT(choose_list_mode(g, f) == ListMode::want)
#define STATE(g, valid, cmp, dev, mov, still)                                                         \
    EXPECT(g.bin_key_valid == valid && g.compact == cmp && g.dev_geometry == dev && g.moving == mov && \
           g.still_frames == still)

static void test_decision()
{
    const BinKey A = key_of(1.0f), B = key_of(2.0f), C = key_of(3.0f), wide = key_of(1.0f, 432, 300);
    {   // an ordinary context's host-buffer frames
        GeometryState g;
        STEP(g, facts(A), DeviceFirst);                 // a geometry's first frame
        STATE(g, true, false, true, false, 0u);
        EXPECT(g.bin_key.same(A) && g.last_key.same(A));
        STEP(g, facts(A), HostSized);                   // the same key: no compact lists yet
        STATE(g, true, false, false, false, 1u);
        sized(g);
        STEP(g, facts(A), Compact);
        STATE(g, true, true, false, false, 2u);
        STEP(g, facts(A), Compact);
        STATE(g, true, true, false, false, 3u);
        STEP(g, facts(B), DeviceMoving);                // a new camera over the same grid
        STATE(g, true, true, false, true, 0u);
        EXPECT(g.bin_key.same(A) && g.last_key.same(B));
        STEP(g, facts(B), DeviceMoving);                // held for two frames
        STATE(g, true, true, false, true, 1u);
        STEP(g, facts(B), HostSized);                   // the third: sized for itself, as a still camera
        STATE(g, false, false, false, false, 2u);
        sized(g);
        EXPECT(g.bin_key.same(B));
        STEP(g, facts(B), Compact);
        STEP(g, facts(C), DeviceMoving);
        STEP(g, facts(A), DeviceMoving);                // every new camera keeps moving
        STATE(g, true, true, false, true, 0u);
        EXPECT(g.bin_key.same(B));
        STEP(g, facts(wide), DeviceFirst);              // another frame size: a new geometry, not moving
        STATE(g, true, false, true, false, 0u);
        EXPECT(g.bin_key.same(wide));
        STEP(g, facts(B), DeviceFirst);                 // (and back: the layout differs again)
        EXPECT(g.bin_key.same(B) && !g.moving);
    }
    {   // a device-sized first frame's grid serves the next cameras at once
        GeometryState g;
        STEP(g, facts(A), DeviceFirst);
        STEP(g, facts(B), DeviceMoving);
        STATE(g, true, false, true, true, 0u);
        EXPECT(g.bin_key.same(A));
        g.resize_next_frame();                          // an overflow seen: the next camera is a new geometry
        STEP(g, facts(C), DeviceFirst);
        STATE(g, true, false, true, true, 0u);
        EXPECT(g.bin_key.same(C));
        STEP(g, facts(A), DeviceMoving);
    }
    {   // back on the keyed camera after a moving frame: its lists serve, until it has stayed
        GeometryState g;
        FrameFacts f = facts(A);
        f.device_first = false;
        STEP(g, f, HostSized);
        sized(g);
        STEP(g, facts(B), DeviceMoving);
        STEP(g, facts(A), Compact);
        STATE(g, true, true, false, true, 0u);
        STEP(g, facts(A), Compact);
        STEP(g, facts(A), HostSized);                   // kStillFrames on one camera since it moved
        STATE(g, false, false, false, false, 2u);
    }
    {   // another frame size while moving, from a device-pointer caller
        GeometryState g;
        FrameFacts f = facts(A);
        f.host_stream = false;
        STEP(g, f, HostSized);                          // never device-sized first
        STATE(g, false, false, false, false, 0u);
        sized(g);
        f.key = B;
        STEP(g, f, DeviceMoving);
        EXPECT(g.moving);
        f.key = wide;
        STEP(g, f, HostSized);
        STATE(g, true, false, false, false, 0u);        // (still keyed to A until it is sized)
        EXPECT(g.bin_key.same(A));
    }
    {   // a multi-device render's context sizes every camera on the host
        GeometryState g;
        FrameFacts f = facts(A);
        f.reuse_cameras = false;
        for (const BinKey& k : {A, B, C, A}) {
            f.key = k;
            STEP(g, f, HostSized);
            EXPECT(!g.moving && !g.dev_geometry);
            sized(g);
            STEP(g, f, Compact);
        }
    }
    {   // XRT_DEVICE_FIRST=0
        GeometryState g;
        FrameFacts f = facts(A);
        f.device_first = false;
        STEP(g, f, HostSized);
        sized(g);
        f.key = B;
        STEP(g, f, DeviceMoving);                       // (the moving path is not its switch)
    }
    {   // a forced capacity: fixed lists, and the key untouched
        GeometryState g;
        FrameFacts f = facts(A);
        f.forced_cap = true;
        STEP(g, f, Fixed);                              // with nothing known
        STATE(g, false, false, false, false, 0u);
        f.forced_cap = false;
        STEP(g, f, HostSized);
        sized(g);
        STEP(g, f, Compact);
        f.forced_cap = true;
        STEP(g, f, Fixed);                              // after compact lists: they stay the geometry's
        STATE(g, true, true, false, false, 3u);
        EXPECT(g.bin_key.same(A));
        f.forced_cap = false;
        STEP(g, f, Compact);
        f.forced_cap = true;
        f.key = B;
        STEP(g, f, Fixed);                              // a new camera: no device sizing, A's lists dropped
        STATE(g, true, false, false, false, 0u);
        EXPECT(g.bin_key.same(A));
        f.forced_cap = false;
        f.key = A;
        STEP(g, f, Fixed);                              // A again: keyed, but no better lists known
        f.key = B;
        STEP(g, f, DeviceFirst);                        // (a first frame of B's on the host stream)
    }
    {   // a transit layout: no device sizing, first frame or new camera
        GeometryState g;
        FrameFacts f = facts(A);
        f.transit = true;
        STEP(g, f, HostSized);
        sized(g);
        STEP(g, f, Compact);
        f.key = B;
        STEP(g, f, HostSized);
        STATE(g, true, false, false, false, 0u);
        sized(g);
        f.transit = false;
        f.key = C;
        STEP(g, f, DeviceMoving);
        f.transit = true;
        f.key = A;
        STEP(g, f, HostSized);                          // (moving stays set: the lists will have room)
        EXPECT(g.moving);
    }
    {   // the other models: host-sized or compact only
        GeometryState g;
        FrameFacts f = facts(A);
        f.attenuation = false;
        STEP(g, f, HostSized);
        sized(g);
        STEP(g, f, Compact);
        f.key = B;
        STEP(g, f, HostSized);
        STATE(g, true, false, false, false, 0u);
    }
    {   // not binned (or no rows): no lists, yet the frame counts
        GeometryState g;
        FrameFacts f = facts(A);
        f.binned = false;
        STEP(g, f, None);
        STATE(g, false, false, false, false, 0u);
        EXPECT(g.last_key.same(A));
        STEP(g, f, None);
        STATE(g, false, false, false, false, 1u);
        f.binned = true;
        STEP(g, f, HostSized);                          // a third frame of the key: not a first one
        STATE(g, false, false, false, false, 2u);
        sized(g);
        f.key = B;
        STEP(g, f, DeviceMoving);
        f.binned = false;
        f.key = C;
        STEP(g, f, None);
        STATE(g, true, true, false, true, 0u);          // (the same grid: still moving)
        EXPECT(g.bin_key.same(A) && g.last_key.same(C));
        f.key = wide;
        STEP(g, f, None);
        EXPECT(!g.moving && g.compact && g.bin_key.same(A));
    }
}

// ------------------------------------------------------- centre_first_order

static uint64_t centre_key(uint32_t r, uint32_t rx, uint32_t ry)
{
    const int64_t dx = 2 * (int64_t)(r % rx) + 1 - (int64_t)rx, dy = 2 * (int64_t)(r / rx) + 1 - (int64_t)ry;
    return (uint64_t)(dx * dx + dy * dy);
}

static void test_centre_first()
{
    EXPECT(centre_first_order(1, 1) == U32s({0}));
    EXPECT(centre_first_order(1, 5) == U32s({2, 1, 3, 0, 4}));
    EXPECT(centre_first_order(5, 1) == U32s({2, 1, 3, 0, 4}));
    EXPECT(centre_first_order(2, 2) == U32s({0, 1, 2, 3}));          // all ties: region order
    EXPECT(centre_first_order(3, 2) == U32s({1, 4, 0, 2, 3, 5}));
    EXPECT(centre_first_order(5, 5) == U32s({12, 7, 11, 13, 17, 6, 8, 16, 18, 2, 10, 14, 22,
                                             1, 3, 5, 9, 15, 19, 21, 23, 0, 4, 20, 24}));
    EXPECT(centre_first_order(0, 3).empty());
    const U32s o = centre_first_order(64, 64);
    EXPECT(o.size() == 4096u);
    std::vector<char> seen(4096, 0);
    for (size_t k = 0; k < o.size(); ++k) {
        EXPECT(o[k] < 4096u && !seen[o[k]]);
        if (o[k] < 4096u) seen[o[k]] = 1;
        if (k) {
            const uint64_t a = centre_key(o[k - 1], 64, 64), b = centre_key(o[k], 64, 64);
            EXPECT(a < b || (a == b && o[k - 1] < o[k]));
        }
    }
}

// ----------------------------------------------------------------- the plan

constexpr uint32_t kWaves = 16;           // tile waves of a region in the product
constexpr uint32_t kBigGpu = 8192;        // wave slots that make every test frame a small one

struct Want {
    U32s slot_region, cap;
    uint32_t tile_slots, split_slots;
};

// The plan restated naively: counts by region, the tile regions picked one by
// one (the largest count left, the earliest in the fixed order among equals),
// the rule of the split in integers.
static Want naive(const U32s& by_slot, const U32s& fixed, uint32_t global, int mode, bool moving, uint32_t split_min,
                  uint32_t wave_slots, uint32_t wpr)
{
    const size_t n = fixed.size();
    std::vector<uint64_t> count(n);
    for (size_t s = 0; s < n; ++s) count[fixed[s]] = by_slot[s];
    Want w;
    w.split_slots = 0;
    if (mode == 0 || global != 0 || moving) {
        w.slot_region = fixed;
        w.tile_slots = (uint32_t)n;
    } else {
        std::vector<char> placed(n, 0);
        for (;;) {
            size_t best = n;
            for (size_t s = 0; s < n; ++s) {
                const uint32_t r = fixed[s];
                if (placed[r] || count[r] == 0 || mode == 2) continue;
                if (best == n || count[r] > count[fixed[best]]) best = s;
            }
            if (best == n) break;
            placed[fixed[best]] = 1;
            w.slot_region.push_back(fixed[best]);
        }
        w.tile_slots = (uint32_t)w.slot_region.size();
        for (size_t s = 0; s < n; ++s)
            if (!placed[fixed[s]]) w.slot_region.push_back(fixed[s]);
        uint64_t least = split_min;
        if (split_min == kSplitAuto) {
            const uint64_t heaviest = w.tile_slots ? count[w.slot_region[0]] : 0;
            const bool small = (uint64_t)w.tile_slots * wpr <= 2ull * wave_slots;
            least = small ? std::max<uint64_t>(64, (3 * heaviest + 4) / 5) : 0;
        }
        for (uint32_t s = 0; least && s < w.tile_slots && count[w.slot_region[s]] >= least; ++s) ++w.split_slots;
    }
    for (size_t s = 0; s < n; ++s) {
        const uint64_t c = count[w.slot_region[s]];
        w.cap.push_back((uint32_t)(moving ? 2 * c + 64 : c + c / 8 + 4));
    }
    return w;
}

// plan_lists over counts laid out with `stride` words per slot (a heap block of
// exactly the words it may read), against `want`.
static void expect_plan(int line, const U32s& by_slot, const U32s& fixed, uint32_t global, int mode, bool moving,
                        uint32_t split_min, uint32_t wave_slots, uint32_t wpr, const Want& want, size_t stride = 3)
{
    const size_t n = fixed.size();
    std::vector<uint32_t> lines(n ? (n - 1) * stride + 1 : 0, 0xDEADBEEFu);
    for (size_t s = 0; s < n; ++s) lines[s * stride] = by_slot[s];
    ListPlan p;
    const bool ok = plan_lists(lines.data(), stride, fixed, global, mode, moving, split_min, wave_slots, wpr, p);
    bool good = ok && p.slot_region == want.slot_region && p.cap == want.cap && p.tile_slots == want.tile_slots &&
                p.split_slots == want.split_slots && p.base.size() == n;
    uint64_t run = 0;
    for (size_t s = 0; good && s < n; ++s) {           // base: the prefix sum of the room
        good = p.base[s] == run;
        run += want.cap[s];
    }
    good = good && p.pool == run;
    if (!good) {
        std::printf("plan_san: line %d: plan differs (mode %d, moving %d, split_min %u)\n", line, mode, (int)moving,
                    split_min);
        ++failures;
    }
}

// Both still and moving, each against the naive restatement; `still`, when
// given, is the still plan worked out by hand (the moving one has no plan).
static void both(int line, const U32s& by_slot, const U32s& fixed, uint32_t global, int mode, uint32_t split_min,
                 uint32_t wave_slots, uint32_t wpr, const Want* still = nullptr)
{
    for (const bool moving : {false, true}) {
        const Want w = naive(by_slot, fixed, global, mode, moving, split_min, wave_slots, wpr);
        expect_plan(line, by_slot, fixed, global, mode, moving, split_min, wave_slots, wpr, w);
        if (moving) {
            bool room = w.tile_slots == fixed.size() && w.split_slots == 0u && w.slot_region == fixed;
            for (size_t s = 0; s < fixed.size(); ++s) room = room && w.cap[s] == 2u * by_slot[s] + 64u;
            if (!room) {
                std::printf("plan_san: line %d: the moving restatement is off\n", line);
                ++failures;
            }
        } else if (still) {
            expect_plan(line, by_slot, fixed, global, mode, false, split_min, wave_slots, wpr, *still, 1);
        }
    }
}
#define BOTH(...) both(__LINE__, __VA_ARGS__)

static void test_plan()
{
    const U32s g1 = centre_first_order(1, 1), g32 = centre_first_order(3, 2), g55 = centre_first_order(5, 5);
    {   // 1 x 1
        const Want empty = {{0}, {4}, 0, 0}, one = {{0}, {11}, 1, 0}, all_empty = {{0}, {11}, 0, 0};
        BOTH({0}, g1, 0, 1, kSplitAuto, kBigGpu, kWaves, &empty);
        BOTH({7}, g1, 0, 1, kSplitAuto, kBigGpu, kWaves, &one);         // no zeros: no plan
        BOTH({7}, g1, 0, 2, kSplitAuto, kBigGpu, kWaves, &all_empty);   // mode 2: planned empty all the same
        BOTH({7}, g1, 1, 1, kSplitAuto, kBigGpu, kWaves, &one);
        BOTH({0}, g1, 0, 0, kSplitAuto, kBigGpu, kWaves);
    }
    {   // 3 x 2: slots are regions 1 4 0 2 3 5
        const Want zeros = {g32, {4, 4, 4, 4, 4, 4}, 0, 0};
        BOTH({0, 0, 0, 0, 0, 0}, g32, 0, 1, kSplitAuto, kBigGpu, kWaves, &zeros);
        // no zeros: every region a tile region, heaviest first, equals in the fixed order
        const Want full = {{4, 3, 1, 2, 5, 0}, {24, 24, 20, 20, 20, 5}, 6, 0};
        BOTH({15, 18, 1, 15, 18, 15}, g32, 0, 1, kSplitAuto, kBigGpu, kWaves, &full);
        // zeros among ties: regions 4 and 2 hold 9, 0 and 3 hold 5, 1 and 5 nothing
        const Want mixed = {{4, 2, 0, 3, 1, 5}, {14, 14, 9, 9, 4, 4}, 4, 0};
        BOTH({0, 9, 5, 9, 5, 0}, g32, 0, 1, kSplitAuto, kBigGpu, kWaves, &mixed);
        const Want fixed_order = {g32, {4, 14, 9, 14, 9, 4}, 6, 0};
        BOTH({0, 9, 5, 9, 5, 0}, g32, 3, 1, 1, kBigGpu, kWaves, &fixed_order);     // a global list: no plan, no split
        BOTH({0, 9, 5, 9, 5, 0}, g32, 0, 0, 1, kBigGpu, kWaves, &fixed_order);     // the plan off
        const Want every_empty = {g32, {4, 14, 9, 14, 9, 4}, 0, 0};
        BOTH({0, 9, 5, 9, 5, 0}, g32, 0, 2, 1, kBigGpu, kWaves, &every_empty);     // mode 2: nothing to split
    }
    {   // 5 x 5: regions 0 (8), 12, 7 and 24 (3 each), 6 (1); by slot of the centre-first order
        U32s by_slot(25, 0u);
        by_slot[0] = 3; by_slot[1] = 3; by_slot[5] = 1; by_slot[21] = 8; by_slot[24] = 3;
        Want w = {{0, 12, 7, 24, 6, 11, 13, 17, 8, 16, 18, 2, 10, 14, 22, 1, 3, 5, 9, 15, 19, 21, 23, 4, 20},
                  {13, 7, 7, 7, 5}, 5, 0};
        w.cap.resize(25, 4u);
        BOTH(by_slot, g55, 0, 1, kSplitAuto, kBigGpu, kWaves, &w);
        BOTH(U32s(25, 0u), g55, 0, 1, kSplitAuto, kBigGpu, kWaves);
        BOTH(U32s(25, 6u), g55, 0, 1, kSplitAuto, kBigGpu, kWaves);
        BOTH(by_slot, g55, 7, 1, kSplitAuto, kBigGpu, kWaves);
        BOTH(by_slot, g55, 0, 0, kSplitAuto, kBigGpu, kWaves);
        BOTH(by_slot, g55, 0, 2, kSplitAuto, kBigGpu, kWaves);
    }
    {   // the split rule's count: kSplitFloor against ceil(0.6 x heaviest); 2 x 2, slots are regions
        const U32s g22 = centre_first_order(2, 2);
        const Want h63 = {{1, 0, 3, 2}, {74, 67, 67, 4}, 3, 0};        // floor 64: none
        BOTH({56, 63, 0, 56}, g22, 0, 1, kSplitAuto, kBigGpu, kWaves, &h63);
        const Want h64 = {{1, 0, 3, 2}, {76, 74, 74, 4}, 3, 1};        // ceil(38.4) = 39 < 64: the 64 alone
        BOTH({63, 64, 0, 63}, g22, 0, 1, kSplitAuto, kBigGpu, kWaves, &h64);
        const Want h107 = {{2, 0, 1, 3}, {124, 77, 76, 4}, 3, 2};      // ceil(64.2) = 65: 107 and 65, not 64
        BOTH({65, 64, 107, 0}, g22, 0, 1, kSplitAuto, kBigGpu, kWaves, &h107);
        // split_min 0 never, 1 every tile region, an explicit value
        const Want never = {{2, 0, 1, 3}, {124, 77, 76, 4}, 3, 0}, every = {{2, 0, 1, 3}, {124, 77, 76, 4}, 3, 3};
        BOTH({65, 64, 107, 0}, g22, 0, 1, 0u, kBigGpu, kWaves, &never);
        BOTH({65, 64, 107, 0}, g22, 0, 1, 1u, kBigGpu, kWaves, &every);
        BOTH({65, 64, 107, 0}, g22, 0, 1, 65u, kBigGpu, kWaves, &h107);
        BOTH({65, 64, 107, 0}, g22, 0, 1, 1u, 0u, kWaves, &every);     // (explicit: whatever the GPU's size)
    }
    {   // the split rule's frame size: tile waves one below, at and one above 2 x 3 wave slots
        const U32s g42 = centre_first_order(4, 2);
        for (uint32_t tiles = 5; tiles <= 7; ++tiles) {
            U32s by_slot(8, 0u);
            for (uint32_t s = 0; s < tiles; ++s) by_slot[s] = 100u;
            Want w = {g42, U32s(8, 4u), tiles, tiles <= 6 ? tiles : 0u};   // 100 >= max(64, 60): every tile region
            for (uint32_t s = 0; s < tiles; ++s) w.cap[s] = 116u;
            BOTH(by_slot, g42, 0, 1, kSplitAuto, 3u, 1u, &w);
        }
        // and in the product's units: 3 tile regions of 16 waves against 2 x 23, 24 and 25 slots
        const Want split = {{1, 2, 5, 6, 0, 3, 4, 7}, {116, 116, 116, 4, 4, 4, 4, 4}, 3, 3};
        Want whole = split;
        whole.split_slots = 0;
        BOTH({100, 100, 100, 0, 0, 0, 0, 0}, g42, 0, 1, kSplitAuto, 23u, kWaves, &whole);
        BOTH({100, 100, 100, 0, 0, 0, 0, 0}, g42, 0, 1, kSplitAuto, 24u, kWaves, &split);
        BOTH({100, 100, 100, 0, 0, 0, 0, 0}, g42, 0, 1, kSplitAuto, 25u, kWaves, &split);
    }
    {   // 64 x 64: many equals and empties, against the restatement
        const U32s g = centre_first_order(64, 64);
        uint32_t seed = 7u;
        U32s by_slot(g.size());
        for (uint32_t& c : by_slot) {
            const uint32_t v = lcg(seed) % 40u;
            c = v < 12u ? 0u : v < 30u ? v : v * v;
        }
        BOTH(by_slot, g, 0, 1, kSplitAuto, 8192u, kWaves);          // 256 CUs
        BOTH(by_slot, g, 0, 1, kSplitAuto, 65536u, kWaves);         // (a GPU that holds the frame: it splits)
        BOTH(by_slot, g, 0, 1, 700u, 8192u, kWaves);
        BOTH(by_slot, g, 2, 1, kSplitAuto, 8192u, kWaves);
        BOTH(by_slot, g, 0, 2, kSplitAuto, 8192u, kWaves);
    }
    {   // past 2^32 entries: the failure, and nothing written
        const U32s g21 = centre_first_order(2, 1);
        for (const bool moving : {false, true}) {
            const uint32_t half[2] = {0x80000000u, 0x80000000u};
            ListPlan p;
            p.slot_region = {9u};
            p.tile_slots = 77u;
            p.pool = 5u;
            EXPECT(!plan_lists(half, 1, g21, 0, 1, moving, kSplitAuto, kBigGpu, kWaves, p));
            EXPECT(p.slot_region == U32s({9u}) && p.base.empty() && p.cap.empty() && p.tile_slots == 77u &&
                   p.split_slots == 0u && p.pool == 5u);
        }
        // one region: c + c/8 + 4 = 2^32 - 2 fits, the next count gives 2^32
        const uint32_t fits = 3817748703u, over = 3817748704u;
        ListPlan p;
        EXPECT(plan_lists(&fits, 1, g1, 0, 1, false, kSplitAuto, kBigGpu, kWaves, p));
        EXPECT(p.pool == 0xFFFFFFFEull && p.cap == U32s({0xFFFFFFFEu}) && p.base == U32s({0u}));
        EXPECT(!plan_lists(&over, 1, g1, 0, 1, false, kSplitAuto, kBigGpu, kWaves, p));
        EXPECT(p.pool == 0xFFFFFFFEull);
        EXPECT(!plan_lists(&fits, 1, g1, 0, 1, true, kSplitAuto, kBigGpu, kWaves, p));   // 2c + 64
    }
}

int main()
{
    test_decision();
    test_centre_first();
    test_plan();
    if (failures) {
        std::printf("plan_san: %d FAILED\n", failures);
        return 1;
    }
    std::printf("plan_san: OK\n");
    return 0;
}
