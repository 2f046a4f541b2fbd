// Who owns what in the host code of liblorahip.so: move-only handles for device memory, pinned host memory, events and streams, and
// the context that is made of them. HOST code only (the .cpp units and the host half of lorahip_chan.hip): no header the kernels' units
// include may include this one. A handle is null by default and releases in its destructor; it records nothing about devices -- the
// owner's DeviceGuard makes the right one current around every allocation and release.
#pragma once
#include "lorahip_internal.h"
#include "lorahip_worker.h"
#include <memory>
#include <new>

namespace lorahip {

//! device memory: a typed pointer and its capacity in bytes
template <class T> class DevBuf
{
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { reset(); }
    T *get() const { return p; }
    size_t bytes() const { return cap; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    //! nothing when `want` bytes fit; otherwise the old block goes FIRST (the peak is one block, not two) and want + slack bytes are
    //! allocated. A failure leaves the handle empty.
    hipError_t grow(const size_t want, const size_t slack = 0)
    {
        if (want <= cap) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc((void **)&p, want + slack);
        if (e != hipSuccess) p = nullptr; else cap = want + slack;
        return e;
    }
private:
    T *p = nullptr;
    size_t cap = 0;
};

//! pinned host memory (hipHostMalloc with the caller's flags)
template <class T> class HostBuf
{
public:
    HostBuf() = default;
    HostBuf(HostBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HostBuf &operator=(HostBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~HostBuf() { reset(); }
    T *get() const { return p; }
    T *operator->() const { return p; }
    size_t bytes() const { return cap; }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t grow(const size_t want, const unsigned flags, const size_t slack = 0)
    {
        if (want <= cap) return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc((void **)&p, want + slack, flags);
        if (e != hipSuccess) p = nullptr; else cap = want + slack;
        return e;
    }
private:
    T *p = nullptr;
    size_t cap = 0;
};

//! a device block and a pinned one that are replaced together: both old blocks go, then both are allocated, or both are left empty
template <class D, class H> hipError_t regrowPair(DevBuf<D> &d, const size_t dBytes, HostBuf<H> &h, const size_t hBytes, const unsigned hostFlags)
{
    d.reset(); h.reset();
    hipError_t e = d.grow(dBytes);
    if (e == hipSuccess && (e = h.grow(hBytes, hostFlags)) != hipSuccess) d.reset();
    return e;
}

class Event
{
public:
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { reset(); }
    hipEvent_t get() const { return e; }
    void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    //! creates the event unless there is one: what is made on first use is asked for on EVERY use, so a failure is retried by the next call
    hipError_t ensure(const unsigned flags = hipEventDefault)
    {
        if (e) return hipSuccess;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) e = nullptr;
        return r;
    }
private:
    hipEvent_t e = nullptr;
};

class Stream
{
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return s; }
    void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    //! like Event::ensure; with `priority` the stream is created at that priority
    hipError_t ensure(const unsigned flags, const int *priority = nullptr)
    {
        if (s) return hipSuccess;
        const hipError_t r = priority ? hipStreamCreateWithPriority(&s, flags, *priority) : hipStreamCreateWithFlags(&s, flags);
        if (r != hipSuccess) s = nullptr;
        return r;
    }
private:
    hipStream_t s = nullptr;
};

struct CopyPool;                                     // the parked helpers of the staging fills: lorahip_upload.cpp
struct CopyPoolDelete { void operator()(CopyPool *p) const; };

//! two pinned staging buffers of the host -> device gather (lorahip_upload.cpp)
struct Uploader
{
    HostBuf<char> buf[2];
    Event ev[2];
    bool busy[2] = {false, false};
    bool ready = false;
    std::unique_ptr<CopyPool, CopyPoolDelete> pool;
    void release();                 // back to "not initialised": buffers, events and the pool's threads
    ~Uploader() { release(); }
};

//! fn(i) on threadOf(i) for every i < n at once (runOnAll), as the containers of several devices or parts need it: the first failure's
//! code, and its text -- lorahip_last_error is per thread, so it is read on the worker -- as the calling thread's last error
template <class ThreadOf, class Fn> int runOnThreads(const size_t n, const ThreadOf &threadOf, const Fn &fn)
{
    try
    {
        std::vector<std::string> err(n);
        size_t failed = 0;
        const int rc = runOnAll(n, threadOf, [&](const size_t i) {
            const int r = fn(i);
            try { if (r != LORAHIP_OK) err[i] = lorahip_last_error(); } catch (const std::bad_alloc &) {}   // (the code without its text)
            return r; }, &failed);
        if (rc != LORAHIP_OK) setLastError(err[failed]);
        return rc;
    }
    catch (const std::bad_alloc &) { setLastError("out of host memory"); return LORAHIP_E_NOMEM; }        // nothing may cross the C ABI
}

} // namespace lorahip

// Members are destroyed in reverse order: the tables, the staging and the events go before the stream they were used on.
struct lorahip_ctx
{
    int device = 0;
    int sf = 0;
    size_t N = 0;
    int variant = 0;
    lorahip::Stream ownStream;
    hipStream_t stream = nullptr;
    lorahip::DevBuf<float2> dUp, dDown, dFine, dTw, dTwStage;
    lorahip::DevBuf<double2> dFineA, dFineB;    // empty when the split did not verify on this host (kernels gather then)
    int fineGather = 0;             // A/B switch (lorahip_set_fine_gather): read the fine-tune table itself even though the split verified
    int cuCount = 0;
    lorahip::Event ev0, ev1;
    float powerScale = 0.0f;
    // staging for the host-pointer entry points (grown on demand, both or neither)
    lorahip::DevBuf<char> dStage;
    lorahip::HostBuf<char> hStage;
    lorahip::Uploader up;
};
