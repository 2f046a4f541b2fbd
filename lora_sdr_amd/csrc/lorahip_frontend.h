// What the four front ends (lorahip_chan.hip, lorahip_synth.hip, lorahip_pfb.hip, lorahip_psb.hip) have in common, stated once: the
// state that carries one stream across calls, the output count of the decimators, the sample lookup and the history kernel of the two
// channelisers with the sample formats they read, the integer formats the two synthesisers store with their clip counter, and the way an
// object's tables reach the device when it is created. The rational-rate resampler (lorahip_resamp.hip) carries its rows with the same
// StreamCarry, reads them through iqLoad / carriedSample and uploads its taps with uploadTables.
#pragma once
#include "lorahip_own.h"
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

namespace lorahip {

//! What a front end keeps between calls: the last `len` float2 elements the next call reaches back to (zeros before the start of the
//! stream) and the stream position. A call reads current() and writes next(); advance() makes next() the current one. The rule, for all
//! four: nothing is carried when len == 0 (a synthesiser with n_taps <= interp) -- no buffer, no memset, no flip.
struct StreamCarry
{
    DevBuf<float2> hist[2];
    int cur = 0;
    unsigned long long n0 = 0;      // samples (per row) consumed since the last reset
    size_t len = 0;

    //! at create: both buffers ...
    hipError_t allocate(const size_t elements)
    {
        len = elements; cur = 0; n0 = 0;
        const hipError_t e = hist[0].grow(len * sizeof(float2));
        return e != hipSuccess ? e : hist[1].grow(len * sizeof(float2));
    }
    //! ... and zeros in the current one (synchronous)
    hipError_t zero() { return len ? hipMemset(hist[cur].get(), 0, len * sizeof(float2)) : hipSuccess; }
    const float2 *current() const { return hist[cur].get(); }
    float2 *next() const { return hist[cur ^ 1].get(); }
    //! after the history kernel of a call of nIn samples was launched into next()
    void advance(const size_t nIn)
    {
        if (len) cur ^= 1;
        n0 += nIn;
    }
    //! a new stream: zeros on `stream`, position 0
    hipError_t reset(hipStream_t stream)
    {
        const hipError_t e = len ? hipMemsetAsync(hist[cur].get(), 0, len * sizeof(float2), stream) : hipSuccess;
        if (e == hipSuccess) n0 = 0;
        return e;
    }
};

//! outputs a decimator by D makes of the nIn samples that follow the first n0: one for every multiple of D reached
inline size_t decimatedCount(const unsigned long long n0, const size_t nIn, const int D)
{
    return size_t((n0 + nIn) / (unsigned long long)D - n0 / (unsigned long long)D);
}

// The sample formats of the receive front ends (include/lorahip.h: LORAHIP_IQ_*). A chunk of format S holds one S per sample: float2
// (cf32), short2 (sc16: int16 I, int16 Q) or char2 (sc8). The definition, stated once: x[n] = (scale * (float)I[n], scale * (float)Q[n])
// -- the integer converted exactly, then ONE fp32 multiply per component, an operation of its own (-ffp-contract=off) -- and everything
// after that is the cf32 definition, operation for operation. Only reads from the chunk convert: the history holds converted samples.
// A format needs no alignment beyond its own size (4 / 2 / 8 bytes).

//! the chunk's sample at p as cf32; the one place a format is read
__device__ __forceinline__ float2 iqLoad(const float2 *p, const float) { return *p; }
__device__ __forceinline__ float2 iqLoad(const short2 *p, const float scale)
{
    const short2 v = *p;
    return make_float2(scale * float(v.x), scale * float(v.y));
}
__device__ __forceinline__ float2 iqLoad(const char2 *p, const float scale)
{
    const char2 v = *p;
    return make_float2(scale * float(v.x), scale * float(v.y));
}

// The same formats on the transmit side (include/lorahip.h, "Integer IQ output", has the definition; nothing here restates it
// differently): a synthesiser's cf32 output sample y is stored as float2 as it is, or per component as t = scale * c (ONE fp32 multiply,
// an operation of its own), r = rint(t) (v_rndne_f32: ties to even), then 0 for NaN, lo for r < lo, hi for r > hi, (int)r otherwise;
// a component is clipped when r is NaN or outside [lo, hi].

//! one component by that definition; clipped counts it when it clips
template <int LO, int HI> __device__ __forceinline__ int iqQuantize(const float c, const float scale, unsigned &clipped)
{
    const float r = rintf(scale * c);
    const bool nan = r != r, low = r < float(LO), high = r > float(HI);
    clipped += unsigned(nan | low | high);
    return nan ? 0 : low ? LO : high ? HI : int(r);
}
//! sample y in the format of *p, quantised: the one place a format is written
__device__ __forceinline__ float2 iqPack(const float2 *, const float2 y, const float, unsigned &) { return y; }
__device__ __forceinline__ short2 iqPack(const short2 *, const float2 y, const float scale, unsigned &clipped)
{
    const int i = iqQuantize<-32768, 32767>(y.x, scale, clipped), q = iqQuantize<-32768, 32767>(y.y, scale, clipped);
    return make_short2(short(i), short(q));
}
__device__ __forceinline__ char2 iqPack(const char2 *, const float2 y, const float scale, unsigned &clipped)
{
    const int i = iqQuantize<-128, 127>(y.x, scale, clipped), q = iqQuantize<-128, 127>(y.y, scale, clipped);
    return make_char2((signed char)i, (signed char)q);
}
//! *p = y in p's format; clipped grows by the lane's clipped components (never for float2)
template <class S> __device__ __forceinline__ void iqStore(S *p, const float2 y, const float scale, unsigned &clipped)
{
    *p = iqPack(p, y, scale, clipped);
}

//! The clipped components of a wavefront (per lane < 2^BITS) go to *counter: bit b of every lane's count is one ballot, so lanes that
//! have left the kernel count nothing; then ONE lane adds, and no lane where the wavefront clipped nothing. Call it where the lanes
//! that stored have come together again.
template <int BITS> __device__ __forceinline__ void iqCountClipped(unsigned long long *counter, const unsigned clipped)
{
    unsigned total = 0;
#pragma unroll
    for (int b = 0; b < BITS; b++) total += unsigned(__popcll(__ballot(int((clipped >> b) & 1u)))) << b;
    const int lane = int(__lane_id());
    if (total && lane == __builtin_amdgcn_readfirstlane(lane)) atomicAdd(counter, (unsigned long long)total);
}

//! the clip counter of a synthesiser: 8 bytes on the device, allocated and zeroed by the first integer run (an object that only ever
//! writes cf32 allocates what it always did), zeroed again by reset
struct ClipCount
{
    DevBuf<unsigned long long> dev;
    //! before an integer run is launched on `stream`
    hipError_t ensure(hipStream_t stream)
    {
        if (dev.get()) return hipSuccess;
        const hipError_t e = dev.grow(sizeof(unsigned long long));
        return e != hipSuccess ? e : hipMemsetAsync(dev.get(), 0, sizeof(unsigned long long), stream);
    }
    hipError_t reset(hipStream_t stream) { return dev.get() ? hipMemsetAsync(dev.get(), 0, sizeof(unsigned long long), stream) : hipSuccess; }
    //! the count of everything launched on `stream` so far (synchronises it)
    hipError_t read(hipStream_t stream, unsigned long long *count) const
    {
        *count = 0;
        const hipError_t e = dev.get() ? hipMemcpyAsync(count, dev.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, stream) : hipSuccess;
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    }
};

//! bytes of one sample of a LORAHIP_IQ_* format, 0 for anything else
inline size_t iqSampleBytes(const int format)
{
    return format == LORAHIP_IQ_CF32 ? sizeof(float2) : format == LORAHIP_IQ_SC16 ? sizeof(short2) : format == LORAHIP_IQ_SC8 ? sizeof(char2) : 0;
}

//! what every *_run_iq refuses before it looks at anything else: LORAHIP_OK, or LORAHIP_E_INVALID and "<who>: ..." in lorahip_last_error.
//! wide is the chunk a channeliser reads or the buffer a synthesiser writes: the same four rules hold for both directions.
inline int iqCheck(const std::string &who, const void *wide, const int format, const float scale)
{
    const size_t bytes = iqSampleBytes(format);
    std::string why;
    if (bytes == 0) why = "unknown sample format (LORAHIP_IQ_CF32, LORAHIP_IQ_SC16 or LORAHIP_IQ_SC8)";
    else if (!std::isfinite(scale)) why = "scale must be finite";
    else if (format == LORAHIP_IQ_CF32 && scale != 1.0f) why = "LORAHIP_IQ_CF32 takes scale 1";
    else if (uintptr_t(wide) % bytes) why = "wide_dev must be aligned to the sample size (" + std::to_string(bytes) + " bytes)";
    if (why.empty()) return LORAHIP_OK;
    setLastError(who + ": " + why);
    return LORAHIP_E_INVALID;
}

//! f(chunk) with wide as the sample type of `format` (one iqCheck has passed)
template <class F> int iqDispatch(const void *wide, const int format, F &&f)
{
    if (format == LORAHIP_IQ_SC16) return f(static_cast<const short2 *>(wide));
    if (format == LORAHIP_IQ_SC8) return f(static_cast<const char2 *>(wide));
    return f(static_cast<const float2 *>(wide));
}
//! the same for the buffer a synthesiser writes
template <class F> int iqDispatch(void *wide, const int format, F &&f)
{
    if (format == LORAHIP_IQ_SC16) return f(static_cast<short2 *>(wide));
    if (format == LORAHIP_IQ_SC8) return f(static_cast<char2 *>(wide));
    return f(static_cast<float2 *>(wide));
}

//! sample n of the stream (absolute index): from this call's chunk (format S, converted), from the history kept from earlier calls
//! (cf32), or 0
template <class S>
__device__ __forceinline__ float2 carriedSample(const S *chunk, const long long nChunk, const float2 *hist, const int histLen,
                                                const long long n0, const long long n, [[maybe_unused]] const float scale)
{
    const long long c = n - n0, h = c + histLen;
    float2 v = make_float2(0.0f, 0.0f);
    if constexpr (std::is_same<S, float2>::value)
    {
        const float2 *src = c >= 0 ? chunk + c : hist + h;
        const bool ok = c >= 0 ? c < nChunk : h >= 0;
        if (ok) v = *src;
    }
    else if (c >= 0)
    {
        if (c < nChunk) v = iqLoad(chunk + c, scale);
    }
    else if (h >= 0) v = hist[h];
    return v;
}

//! the histLen samples that precede the next call (the two channelisers launch it; internal linkage: every unit has its own)
template <class S>
static __global__ void carryHistory(const S *chunk, const long long nChunk, const float2 *hist, const int histLen, const long long n0,
                                    float2 *newHist, const float scale)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < histLen) newHist[i] = carriedSample(chunk, nChunk, hist, histLen, n0, n0 + nChunk - histLen + i, scale);
}

inline hipError_t growTables() { return hipSuccess; }
template <class T, class... Rest> hipError_t growTables(DevBuf<T> &d, const T *, const size_t count, Rest &&...rest)
{
    const hipError_t e = d.grow(count * sizeof(T));
    return e != hipSuccess ? e : growTables(rest...);
}
inline hipError_t copyTables() { return hipSuccess; }
template <class T, class... Rest> hipError_t copyTables(DevBuf<T> &d, const T *src, const size_t count, Rest &&...rest)
{
    const hipError_t e = hipMemcpy(d.get(), src, count * sizeof(T), hipMemcpyHostToDevice);
    return e != hipSuccess ? e : copyTables(rest...);
}

//! The last step of every *_create. tables = (device buffer, host source, element count) triples; carryLen = what obj->carry holds.
//! Every buffer is allocated, every table copied, the history zeroed, the device synchronised. *out = obj and LORAHIP_OK; or obj is
//! deleted, *out stays null and the result is LORAHIP_E_NOMEM where memory ran out (HIP's sticky error cleared: the next launch's
//! hipGetLastError is its own) and hipFail(e, "<who> table upload") where a copy failed.
template <class Obj, class... Tables>
int uploadTables(Obj **out, Obj *obj, const std::string &who, const size_t carryLen, Tables &&...tables)
{
    const DeviceGuard guard(obj->ctx->device);
    hipError_t e = growTables(tables...);
    if (e == hipSuccess) e = obj->carry.allocate(carryLen);
    if (e != hipSuccess) { (void)hipGetLastError(); delete obj; return LORAHIP_E_NOMEM; }
    e = copyTables(tables...);
    if (e == hipSuccess) e = obj->carry.zero();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { delete obj; return hipFail(e, (who + " table upload").c_str()); }
    *out = obj;
    return LORAHIP_OK;
}

} // namespace lorahip
