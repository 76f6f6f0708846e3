// xrt_owned_host.inc -- the owning types of the contexts' device buffers,
// pinned host buffers and events, included by xrt_abi.hip ahead of the
// context structs.  Self-contained over the HIP runtime header, <algorithm>
// and <utility>, so that a stand-alone program can compile it under a host
// sanitizer with a counting allocator and a fake event (tools/owned_san.cpp).
// Owners live only inside heap-allocated contexts: no static object of libxrt
// has a destructor.

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
template <unsigned Flags = hipHostMallocDefault>
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static void free(void* p) { (void)hipHostFree(p); }
};

// cap() elements of T from Mem.  Move-only; a moved-from owner is empty.
template <typename T, typename Mem = DeviceMem>
class Owned {
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Owned() { reset(); }

    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    // At least n elements.  A buffer that is large enough stays; otherwise the
    // old one is freed first (its contents are never kept) and max(n, 1)
    // elements are allocated.  On failure the owner is left empty.
    hipError_t reserve(size_t n)
    {
        if (n <= cap_ && p_) return hipSuccess;
        reset();
        n = std::max<size_t>(n, 1);
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
    void reset()
    {
        if (p_) Mem::free((void*)p_);
        p_ = nullptr;
        cap_ = 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T>
using Pinned = Owned<T, PinnedMem<>>;

struct HipEvents {
    using Event = hipEvent_t;
    using Stream = hipStream_t;
    static hipError_t create(Event* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
    static void destroy(Event e) { (void)hipEventDestroy(e); }
    static hipError_t record(Event e, Stream s) { return hipEventRecord(e, s); }
    static hipError_t synchronize(Event e) { return hipEventSynchronize(e); }
    static hipError_t query(Event e) { return hipEventQuery(e); }
    static hipError_t stream_wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0); }
};

// One event, created on first use.  Move-only (the move constructor deletes the copies).
template <unsigned Flags, typename Ev = HipEvents>
class OwnedEvent {
public:
    OwnedEvent() = default;
    OwnedEvent(OwnedEvent&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    OwnedEvent& operator=(OwnedEvent&& o) noexcept
    {
        if (this != &o) {
            reset();
            ev_ = std::exchange(o.ev_, nullptr);
        }
        return *this;
    }
    ~OwnedEvent() { reset(); }

    typename Ev::Event get() const { return ev_; }
    hipError_t create() { return ev_ ? hipSuccess : Ev::create(&ev_, Flags); }
    void reset()
    {
        if (ev_) Ev::destroy(ev_);
        ev_ = nullptr;
    }

private:
    typename Ev::Event ev_ = nullptr;
};

using TimedEvent = OwnedEvent<hipEventDefault>;      // render and region timing: elapsed times are read from these
using PlainEvent = OwnedEvent<hipEventDisableTiming>;

// An event without timing that marks the last work on something, and whether
// that work may still be running (pending).
template <typename Ev = HipEvents>
class BasicFence {
public:
    BasicFence() = default;
    BasicFence(BasicFence&& o) noexcept : ev_(std::move(o.ev_)), pending_(std::exchange(o.pending_, false)) {}
    BasicFence& operator=(BasicFence&& o) noexcept
    {
        ev_ = std::move(o.ev_);
        pending_ = std::exchange(o.pending_, false);
        return *this;
    }

    bool pending() const { return pending_; }
    // Behind everything enqueued on `stream` so far.
    hipError_t record(typename Ev::Stream stream)
    {
        hipError_t e = ev_.create();
        if (e == hipSuccess) e = Ev::record(ev_.get(), stream);
        if (e == hipSuccess) pending_ = true;
        return e;
    }
    // The host waits for the recorded work, if any is pending.
    hipError_t wait()
    {
        if (!pending_) return hipSuccess;
        const hipError_t e = Ev::synchronize(ev_.get());
        if (e == hipSuccess) pending_ = false;
        return e;
    }
    // hipSuccess: nothing pending (any more); hipErrorNotReady: still running.
    hipError_t passed()
    {
        if (!pending_) return hipSuccess;
        const hipError_t e = Ev::query(ev_.get());
        if (e == hipSuccess) pending_ = false;
        return e;
    }
    // `stream` waits for the recorded work on the device.
    hipError_t order(typename Ev::Stream stream) { return Ev::stream_wait(stream, ev_.get()); }
    // Pending from now on, ahead of the record() that follows the work about
    // to be enqueued: a failure in between leaves the owner marked in use.
    hipError_t mark()
    {
        const hipError_t e = ev_.create();
        if (e == hipSuccess) pending_ = true;
        return e;
    }
    // Not pending, without a wait: the caller knows the work is ordered otherwise.
    void forget() { pending_ = false; }
    void reset()
    {
        ev_.reset();
        pending_ = false;
    }

private:
    OwnedEvent<hipEventDisableTiming, Ev> ev_;
    bool pending_ = false;
};

using Fence = BasicFence<>;

// reset() of each, in the order given.
template <typename... Owner>
void release(Owner&... owner)
{
    (owner.reset(), ...);
}
