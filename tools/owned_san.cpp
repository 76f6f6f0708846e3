// owned_san.cpp -- the owning types of the contexts' buffers and events
// (simpleraytracing_amd/csrc/xrt_owned_host.inc) over a counting allocator and
// a fake event, as a stand-alone program for a host sanitizer build:
//
//   hipcc --cuda-host-only -x hip -O1 -g -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Isimpleraytracing_amd/csrc tools/owned_san.cpp -o owned_san
//
// The allocator hands out malloc blocks of the exact size, so that a write one
// element past a buffer, a double free and a leak are seen; no HIP call is
// made.  Prints "owned_san: OK" and returns 0 when every check held
// (tests/test_owned_cpu.py runs it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "xrt_owned_host.inc"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("owned_san: line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// malloc / free of the exact size; counts the live blocks, logs the calls and
// fails the next allocation on request.
struct CountingMem {
    static int live, allocs, frees;
    static bool fail_next;
    static size_t last_bytes;
    static std::string log;
    static hipError_t alloc(void** p, size_t bytes)
    {
        log += 'a';
        if (fail_next) {
            fail_next = false;
            return hipErrorOutOfMemory;
        }
        *p = std::malloc(bytes);
        std::memset(*p, 0xA5, bytes);
        last_bytes = bytes;
        ++live;
        ++allocs;
        return hipSuccess;
    }
    static void free(void* p)
    {
        log += 'f';
        std::free(p);
        --live;
        ++frees;
    }
};
int CountingMem::live = 0, CountingMem::allocs = 0, CountingMem::frees = 0;
bool CountingMem::fail_next = false;
size_t CountingMem::last_bytes = 0;
std::string CountingMem::log;

using Buf = Owned<double, CountingMem>;

// Events as small integers behind a pointer; `done` says which have passed.
struct FakeEvents {
    struct Rec {
        bool recorded = false, done = false;
        int stream = 0;
    };
    using Event = Rec*;
    using Stream = int;
    static int live, syncs, queries, stream_waits;
    static hipError_t fail_create;
    static hipError_t create(Event* e, unsigned flags)
    {
        if (fail_create != hipSuccess) return fail_create;
        EXPECT(flags == hipEventDisableTiming);
        *e = new Rec();
        ++live;
        return hipSuccess;
    }
    static void destroy(Event e)
    {
        delete e;
        --live;
    }
    static hipError_t record(Event e, Stream s)
    {
        e->recorded = true;
        e->done = false;
        e->stream = s;
        return hipSuccess;
    }
    static hipError_t synchronize(Event e)
    {
        ++syncs;
        e->done = true;
        return hipSuccess;
    }
    static hipError_t query(Event e)
    {
        ++queries;
        return !e->recorded || e->done ? hipSuccess : hipErrorNotReady;
    }
    static hipError_t stream_wait(Stream, Event e)
    {
        ++stream_waits;
        return e ? hipSuccess : hipErrorInvalidHandle;
    }
};
int FakeEvents::live = 0, FakeEvents::syncs = 0, FakeEvents::queries = 0, FakeEvents::stream_waits = 0;
hipError_t FakeEvents::fail_create = hipSuccess;

using TestFence = BasicFence<FakeEvents>;

static void fill(Buf& b)                           // every element: one past the end is the sanitizer's to see
{
    for (size_t i = 0; i < b.cap(); ++i) b.get()[i] = (double)i;
}

static void owned_checks()
{
    using M = CountingMem;
    {
        Buf b;
        EXPECT(!b && b.get() == nullptr && b.cap() == 0);
        b.reset();                                 // empty: nothing to free
        EXPECT(M::frees == 0);
        EXPECT(b.reserve(10) == hipSuccess && b && b.cap() == 10 && M::last_bytes == 10 * sizeof(double) && M::live == 1);
        fill(b);
        double* const first = b.get();
        EXPECT(b.reserve(4) == hipSuccess && b.get() == first && b.cap() == 10);     // smaller: stays
        EXPECT(b.reserve(10) == hipSuccess && b.get() == first && M::allocs == 1);   // equal: stays
        EXPECT(b.reserve(0) == hipSuccess && b.get() == first);
        M::log.clear();
        EXPECT(b.reserve(11) == hipSuccess && b.cap() == 11 && M::live == 1);        // larger: replaced
        EXPECT(M::log == "fa");                                                        // freed first, then allocated
        fill(b);
        M::fail_next = true;                       // a failed growth leaves the owner empty
        M::log.clear();
        EXPECT(b.reserve(100) == hipErrorOutOfMemory && !b && b.cap() == 0 && M::live == 0 && M::log == "fa");
        EXPECT(b.reserve(3) == hipSuccess && b.cap() == 3 && M::live == 1);
        fill(b);
        b.reset();
        b.reset();                                 // twice: one free
        EXPECT(!b && b.cap() == 0 && M::live == 0);
        EXPECT(b.reserve(0) == hipSuccess && b.cap() == 1 && M::last_bytes == sizeof(double));   // an empty owner: one element
        fill(b);
    }
    EXPECT(M::live == 0);                          // the destructor
    {
        Buf a, c;
        EXPECT(a.reserve(5) == hipSuccess && c.reserve(7) == hipSuccess && M::live == 2);
        double* const pa = a.get();
        double* const pc = c.get();
        Buf moved(std::move(a));                   // move construction: the source is empty
        EXPECT(moved.get() == pa && moved.cap() == 5 && !a && a.cap() == 0 && M::live == 2);
        c = std::move(moved);                      // move assignment onto a non-empty owner: its block is freed
        EXPECT(c.get() == pa && c.cap() == 5 && !moved && M::live == 1);
        (void)pc;
        Buf& self = c;
        c = std::move(self);                       // self-assignment keeps the block
        EXPECT(c.get() == pa && c.cap() == 5 && M::live == 1);
        Buf d;
        EXPECT(d.reserve(2) == hipSuccess);
        double* const pd = d.get();
        std::swap(c, d);
        EXPECT(c.get() == pd && c.cap() == 2 && d.get() == pa && d.cap() == 5 && M::live == 2);
        fill(c);
        fill(d);
        Buf empty;
        d = std::move(empty);                      // an empty source releases the target
        EXPECT(!d && M::live == 1);
    }
    EXPECT(M::live == 0);
    {
        struct Chunk {
            Buf p;
            size_t used = 0;
        };
        std::vector<Chunk> v;                      // grows by reallocation: every element is moved
        std::vector<double*> where;
        for (size_t k = 0; k < 40; ++k) {
            Chunk c;
            EXPECT(c.p.reserve(k + 1) == hipSuccess);
            where.push_back(c.p.get());
            v.push_back(std::move(c));
        }
        EXPECT(M::live == 40);
        for (size_t k = 0; k < 40; ++k) {
            EXPECT(v[k].p.get() == where[k] && v[k].p.cap() == k + 1);
            fill(v[k].p);
        }
        std::swap(v[3], v.back());
        EXPECT(v[3].p.cap() == 40 && v.back().p.cap() == 4);
        v.erase(v.begin() + 10, v.end());
        EXPECT(M::live == 10);
        std::vector<std::array<Buf, 2>> pairs(3);
        EXPECT(pairs[1][0].reserve(6) == hipSuccess);
        pairs.resize(50);
        EXPECT(pairs[1][0].cap() == 6 && M::live == 11);
        pairs[1] = {};
        EXPECT(M::live == 10);
        Buf x, y;
        EXPECT(x.reserve(1) == hipSuccess && y.reserve(1) == hipSuccess);
        release(x, y);
        EXPECT(!x && !y && M::live == 10);
    }
    EXPECT(M::live == 0 && M::allocs == M::frees);
}

static void fence_checks()
{
    using E = FakeEvents;
    {
        TestFence f;
        EXPECT(!f.pending() && E::live == 0);      // no event until it is needed
        EXPECT(f.wait() == hipSuccess && f.passed() == hipSuccess && E::syncs == 0 && E::queries == 0);
        EXPECT(f.record(3) == hipSuccess && f.pending() && E::live == 1);
        EXPECT(f.passed() == hipErrorNotReady && f.pending() && E::queries == 1);
        EXPECT(f.order(5) == hipSuccess && E::stream_waits == 1 && f.pending());
        EXPECT(f.wait() == hipSuccess && !f.pending() && E::syncs == 1);
        EXPECT(f.wait() == hipSuccess && E::syncs == 1);                  // nothing pending: no second synchronise
        EXPECT(f.passed() == hipSuccess && E::queries == 1);
        EXPECT(f.record(3) == hipSuccess && E::live == 1);                // the same event again
        f.forget();
        EXPECT(!f.pending() && f.wait() == hipSuccess && E::syncs == 1);
        EXPECT(f.mark() == hipSuccess && f.pending());                    // in use before anything is recorded
        EXPECT(f.record(4) == hipSuccess && f.pending());
        TestFence g(std::move(f));                 // a moved-from fence is empty and not pending
        EXPECT(g.pending() && !f.pending() && E::live == 1);
        EXPECT(f.wait() == hipSuccess && E::syncs == 1);
        TestFence h;
        EXPECT(h.record(1) == hipSuccess && E::live == 2);
        h = std::move(g);                          // onto a fence with an event: that event is destroyed
        EXPECT(h.pending() && !g.pending() && E::live == 1);
        EXPECT(h.passed() == hipErrorNotReady);
        EXPECT(h.wait() == hipSuccess && h.passed() == hipSuccess && !h.pending());
        std::vector<std::array<TestFence, 2>> v(2);
        EXPECT(v[1][1].record(2) == hipSuccess);
        v.resize(40);
        EXPECT(v[1][1].pending() && !v[1][0].pending() && E::live == 2);
        h.reset();
        h.reset();
        EXPECT(E::live == 1);
    }
    EXPECT(E::live == 0);
    {
        TestFence f;                               // a failed creation: the error comes back, nothing is pending
        E::fail_create = hipErrorOutOfMemory;
        EXPECT(f.mark() == hipErrorOutOfMemory && !f.pending());
        EXPECT(f.record(1) == hipErrorOutOfMemory && !f.pending() && f.wait() == hipSuccess);
        E::fail_create = hipSuccess;
        EXPECT(f.mark() == hipSuccess && f.pending() && f.wait() == hipSuccess && !f.pending());   // marked, never recorded
    }
    EXPECT(E::live == 0);
    {
        TestFence f;                               // the working set's fence through the voxeliser's shortcut (run_voxelize)
        const int syncs = E::syncs;
        EXPECT(f.mark() == hipSuccess && f.record(7) == hipSuccess && f.pending());   // a voxelisation on stream 7
        f.forget();                                // the next one on stream 7: the stream orders it
        EXPECT(!f.pending() && f.wait() == hipSuccess && E::syncs == syncs);           // the set's wait finds nothing
        EXPECT(f.mark() == hipSuccess && f.pending());                                 // in use again ahead of its kernels
        EXPECT(f.record(7) == hipSuccess && f.pending() && E::live == 1);              // the same event
        EXPECT(f.wait() == hipSuccess && E::syncs == syncs + 1 && !f.pending());       // a user on another stream waits, once
        f.forget();                                // nothing pending: nothing changes
        EXPECT(!f.pending() && f.wait() == hipSuccess && E::syncs == syncs + 1);
        EXPECT(f.mark() == hipSuccess && f.pending());
        f.forget();                                // marked, never recorded, forgotten: no wait on an event never recorded
        EXPECT(!f.pending() && f.wait() == hipSuccess && E::syncs == syncs + 1);
    }
    EXPECT(E::live == 0);
}

int main()
{
    owned_checks();
    fence_checks();
    if (!failures) std::printf("owned_san: OK\n");
    return failures ? 1 : 0;
}
