// What the four front ends (lorahip_chan.hip, lorahip_synth.hip, lorahip_pfb.hip, lorahip_psb.hip) have in common, stated once: the
// state that carries one stream across calls, the output count of the decimators, the sample lookup and the history kernel of the two
// channelisers, and the way an object's tables reach the device when it is created.
#pragma once
#include "lorahip_own.h"
#include <string>

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

//! sample n of the stream (absolute index): from this call's chunk, from the history kept from earlier calls, or 0
__device__ __forceinline__ float2 carriedSample(const float2 *chunk, const long long nChunk, const float2 *hist, const int histLen,
                                                const long long n0, const long long n)
{
    const long long c = n - n0, h = c + histLen;
    const float2 *src = c >= 0 ? chunk + c : hist + h;
    const bool ok = c >= 0 ? c < nChunk : h >= 0;
    float2 v = make_float2(0.0f, 0.0f);
    if (ok) v = *src;
    return v;
}

//! the histLen samples that precede the next call (the two channelisers launch it; internal linkage: every unit has its own)
[[maybe_unused]] static __global__ void carryHistory(const float2 *chunk, const long long nChunk, const float2 *hist, const int histLen, const long long n0,
                                    float2 *newHist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < histLen) newHist[i] = carriedSample(chunk, nChunk, hist, histLen, n0, n0 + nChunk - histLen + i);
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
