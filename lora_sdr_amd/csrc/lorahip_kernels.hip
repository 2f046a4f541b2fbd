// CDNA4 (gfx950) kernels of the LoRa demod hot path: dechirp -> 2^SF-point FFT -> detect.
// This TU: the generic LDS kernel (variant 1, every SF), the launch dispatch and the memory-bandwidth
// probe. The tuned register/LDS-phase kernels live in lorahip_fast.hip; the modulators, the
// synthetic-IQ generator and the AWGN channel in lorahip_tx.hip.
// Numerics contract and shared helpers: lorahip_device.h.
#include "lorahip_device.h"

namespace lorahip {

/***********************************************************************
 * Variant 1: generic LDS kernel. N/4 threads per window, every stage through LDS.
 * Correct for every SF; the tuned per-SF kernels below are validated against it.
 **********************************************************************/
template <int LOG2N>
__global__ void __launch_bounds__((1 << LOG2N) / 4 < 256 ? 256 : (1 << LOG2N) / 4)
detectGeneric(const DetectArgs a)
{
    typedef Plan<LOG2N> P;
    constexpr int N = P::N;
    constexpr int TW = N / 4;                        // threads per window
    constexpr int BLOCK = TW < 256 ? 256 : TW;
    constexpr int WPB = BLOCK / TW;                  // windows per block
    constexpr int WAVES_PER_WIN = TW >= 64 ? TW / 64 : 1;
    constexpr int M = N * LORAHIP_FINE_STEPS;

    __shared__ float2 sA[WPB][N];
    __shared__ int sIdx[WPB][N];
    __shared__ float sRedV[WPB][WAVES_PER_WIN];
    __shared__ int sRedI[WPB][WAVES_PER_WIN];
    __shared__ double sRedT[WPB][WAVES_PER_WIN];

    const int lw = threadIdx.x / TW;                 // local window
    const int t = threadIdx.x % TW;
    const unsigned w = blockIdx.x * WPB + lw;
    const bool active = w < a.nWindows;
    float2 *A = sA[lw];

    int sel = LORAHIP_CHIRP_NONE;
    int idx0 = 0;
    float err = 0.0f;
    const float2 *in = nullptr;
    if (active)
    {
        sel = a.chirpSel ? a.chirpSel[w] : a.chirpSelAll;
        idx0 = a.fineIdx0 ? a.fineIdx0[w] : 0;
        err = a.fineErr ? a.fineErr[w] : 0.0f;
        in = a.iq + (a.offsets ? a.offsets[w] : (long long)w * a.stride);
    }
    const bool dechirp = sel != LORAHIP_CHIRP_NONE;
    const float d = err * (float)LORAHIP_FINE_STEPS;
    const bool moving = dechirp && d != 0.0f;        // index changes from sample to sample

    // fine-tune index chain (sequential by definition; one lane walks it)
    if (moving && t == 0)
    {
        int idx = idx0;
        for (int i = 0; i < N; i++) { sIdx[lw][i] = idx; idx = fineStep(idx, d, M); }
        if (a.fineIdxOut) a.fineIdxOut[w] = idx;
    }
    if (active && !moving && t == 0 && a.fineIdxOut) a.fineIdxOut[w] = idx0;
    __syncthreads();

    // load + dechirp (LoRaDemod.cpp:158-159), scatter to the DIT work-array order
    if (active)
    {
        const float2 *chirp = sel == LORAHIP_CHIRP_DOWN ? a.down : a.up;
        const float2 fconst = a.fine[idx0];
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int n = t + j * TW;
            float2 x = in[n];
            if (dechirp)
            {
                x = cmul(x, chirp[n]);
                x = cmul(x, moving ? a.fine[sIdx[lw][n]] : fconst);
            }
            if (a.decOut) a.decOut[(size_t)w * N + n] = x;
            A[P::pos(n)] = x;
        }
    }
    __syncthreads();

    // innermost radix-2 stage: m = 1, fstride = N/2, twiddle(0)
    if (P::HAS_R2)
    {
        if (active)
        {
            const float2 t0 = a.tw[0];
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
                const int b = t + j * TW;
                float2 f0 = A[2 * b], f1 = A[2 * b + 1];
                bfly2(f0, f1, t0);
                A[2 * b] = f0; A[2 * b + 1] = f1;
            }
        }
        __syncthreads();
    }

    // radix-4 stages, innermost (smallest m) first
#pragma unroll
    for (int s = P::R4 - 1; s >= 0; s--)
    {
        const int m = N >> (2 * (s + 1));            // remainder of stage s
        const int fstride = 1 << (2 * s);            // 4^s
        if (active)
        {
            const int k = t & (m - 1);
            const int base = ((t / m) * 4 * m) + k;
            float2 f0 = A[base], f1 = A[base + m], f2 = A[base + 2 * m], f3 = A[base + 3 * m];
            bfly4(f0, f1, f2, f3, a.tw[k * fstride], a.tw[k * fstride * 2], a.tw[k * fstride * 3]);
            A[base] = f0; A[base + m] = f1; A[base + 2 * m] = f2; A[base + 3 * m] = f3;
        }
        __syncthreads();
    }

    // scan (LoRaDetector.hpp:36-48): per-lane partials over 4 bins, then tree
    float bestV = 0.0f;
    int bestI = 0;
    double tot = 0.0;
    if (active)
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int i = t + j * TW;
            const float2 b = A[i];
            if (a.fftOut) a.fftOut[(size_t)w * N + i] = b;
            const float mag2 = b.x * b.x + b.y * b.y;
            tot += (double)mag2;
            if (mag2 > bestV) { bestV = mag2; bestI = i; }
        }
        if (!(bestV > 0.0f)) bestI = 0;
    }
    constexpr int SEG = TW < 64 ? TW : 64;
#pragma unroll
    for (int off = SEG / 2; off > 0; off >>= 1)
    {
        const float ov = __shfl_xor(bestV, off, 64);
        const int oi = __shfl_xor(bestI, off, 64);
        const double ot = __shfl_xor(tot, off, 64);
        argmaxCombine(bestV, bestI, ov, oi);
        tot += ot;
    }
    if (WAVES_PER_WIN > 1)
    {
        const int wv = t / 64;
        if ((t & 63) == 0) { sRedV[lw][wv] = bestV; sRedI[lw][wv] = bestI; sRedT[lw][wv] = tot; }
        __syncthreads();
        if (t == 0)
        {
            bestV = sRedV[lw][0]; bestI = sRedI[lw][0]; tot = sRedT[lw][0];
            for (int k = 1; k < WAVES_PER_WIN; k++)
            {
                argmaxCombine(bestV, bestI, sRedV[lw][k], sRedI[lw][k]);
                tot += sRedT[lw][k];
            }
        }
    }
    if (active && t == 0)
    {
        const float2 l = A[bestI > 0 ? bestI - 1 : N - 1];
        const float2 r = A[bestI < N - 1 ? bestI + 1 : 0];
        detectTail(a, w, bestI, bestV, tot, l, r);
    }
}

template <int LOG2N>
static hipError_t launchGeneric(const DetectArgs &a, hipStream_t stream)
{
    constexpr int N = 1 << LOG2N;
    constexpr int TW = N / 4;
    constexpr int BLOCK = TW < 256 ? 256 : TW;
    constexpr int WPB = BLOCK / TW;
    const unsigned grid = (a.nWindows + WPB - 1) / WPB;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(detectGeneric<LOG2N>, dim3(grid), dim3(BLOCK), 0, stream, a);
    return hipGetLastError();
}

} // namespace lorahip
// the contracted build's entry points (lorahip_fma_fast.hip / lorahip_fma_wide.hip: their own namespace, plain C hand-over)
extern "C" int lorahip_fma_fast_launch(int sf, const void *args, const void *tables, void *stream);
extern "C" int lorahip_fma_wide_launch(int sf, const void *args, const void *tables, void *stream);
namespace lorahip {

hipError_t launchDetect(const int sf, const int variant, const DetectArgs &a, const FastTables &ft, hipStream_t stream)
{
    if (variant == LORAHIP_VARIANT_FMA)
    {
        if (sf >= 6 && sf <= 10) return hipError_t(lorahip_fma_fast_launch(sf, &a, &ft, stream));
        if (sf == 11 || sf == 12) return hipError_t(lorahip_fma_wide_launch(sf, &a, &ft, stream));
        return hipErrorInvalidValue;
    }
    if (variant != 1 && fastAvailable(sf)) return launchFast(sf, variant, a, ft, stream);
    if (variant != 1 && wideAvailable(sf)) return launchWide(sf, variant, a, ft, stream);
    switch (sf)
    {
    case 6: return launchGeneric<6>(a, stream);
    case 7: return launchGeneric<7>(a, stream);
    case 8: return launchGeneric<8>(a, stream);
    case 9: return launchGeneric<9>(a, stream);
    case 10: return launchGeneric<10>(a, stream);
    case 11: return launchGeneric<11>(a, stream);
    case 12: return launchGeneric<12>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

/***********************************************************************
 * HBM read probe (measurement aid, not part of the demod path): streams `n16` 16-byte words
 * and folds them into one checksum per lane. pattern 0: lane-linear float4 (the classic copy
 * shape); pattern 1: the tuned SF7 kernel's shape -- a wave owns 8 KB, reads it as 8 row loads in
 * which each group of 8 lanes covers 128 contiguous bytes of a different 1 KB window.
 **********************************************************************/
__global__ void __launch_bounds__(256) membwProbe(const float4 *__restrict__ in, const size_t n16, const int pattern, float *out)
{
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pattern == 0)
    {
        for (size_t i = gid; i < n16; i += nthreads)
        {
            const float4 v = in[i];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    else
    {
        const int lane = threadIdx.x & 63;
        const size_t wave = gid >> 6, nwaves = nthreads >> 6;
        const size_t nsets = n16 / 512;                   // 8 KB per wave iteration
        for (size_t s = wave; s < nsets; s += nwaves)
        {
            const float4 *base = in + s * 512 + (size_t)(lane >> 3) * 64 + (lane & 7);
            float4 v[8];
#pragma unroll
            for (int r = 0; r < 8; r++) v[r] = base[r * 8];
#pragma unroll
            for (int r = 0; r < 8; r++) { acc.x += v[r].x; acc.y += v[r].y; acc.z += v[r].z; acc.w += v[r].w; }
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 1.2345e-30f) out[0] = acc.x;   // keep the loads alive
}

hipError_t launchMembw(const float2 *iq, const size_t nBytes, const int pattern, const int blocks, float *scratch, hipStream_t stream)
{
    hipLaunchKernelGGL(membwProbe, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const float4 *>(iq), nBytes / 16, pattern, scratch);
    return hipGetLastError();
}

} // namespace lorahip
