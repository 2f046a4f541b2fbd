// Transmit side and test signals: the batched modulator, one lane per frame (lorahip_mod_frames, lorahip_mod_frames_var), the
// synthetic up-chirp symbols and the AWGN channel of the benchmarks and the loopback tests. The scheduled modulator: lorahip_txsched.hip.
#include "lorahip_internal.h"
#include "lorahip_framewalk.h"

namespace lorahip {

/***********************************************************************
 * Batched modulator: the frame of the LoRaMod block (LoRaMod.cpp:109-238) for many packets at once, one lane per frame.
 * genChirp<float> is a sequential float recurrence with one running accumulator through the whole frame (lorahip_framewalk.h), so a
 * frame is walked by one lane exactly as the reference walks it, 64 frames per wavefront; 16 samples at a time go through LDS so
 * that the stores are 128-byte rows.
 *
 * Frame f has nsymsOf[f] symbols, or maxNsyms where nsymsOf is null (the uniform entry point), and EVERY frame is walked to the
 * length of maxNsyms symbols: the chirps behind a frame's own symbols are zero chirps. A zero chirp does not touch the phase
 * accumulator, so row f is the uniform frame for the same symbols with padding + maxNsyms - nsymsOf[f].
 **********************************************************************/
__global__ void __launch_bounds__(256) modFrames(float2 *__restrict__ iq, const long long frameStride,
                                                 const unsigned short *__restrict__ syms, const long long symStride,
                                                 const int *__restrict__ nsymsOf, const unsigned nFrames, const int maxNsyms,
                                                 const int sync, const float ampl, const int padding, const int N)
{
    __shared__ float2 stage[4][64][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned frame0 = (blockIdx.x * 4 + wave) * 64;
    const unsigned frame = frame0 + lane;
    const bool mine = frame < nFrames;
    const unsigned short *mySyms = syms + (size_t)(mine ? frame : 0) * symStride;
    int nsyms = nsymsOf == nullptr ? maxNsyms : mine ? nsymsOf[frame] : -1;
    if (nsyms > maxNsyms) nsyms = -1;                                      // more than the row holds: silent, as a refused packet (< 0) is
    FrameWalk w(N);
    long long pos = 0;
    const int pad = padding < 1 ? 1 : padding;                             // one zero symbol is emitted before the test (LoRaMod.cpp:218-224)
    const int nChirps = 10 + 2 + 3 + maxNsyms + pad;                       // the same for every frame of the launch
    for (int c = 0; c < nChirps; c++)
    {
        w.chirp(c, sync, mySyms, nsyms);
        for (int i0 = 0; i0 < w.NN; i0 += 16)
        {
#pragma unroll 4
            for (int i = 0; i < 16; i++) stage[wave][lane][i] = w.zero ? make_float2(0.0f, 0.0f) : polar(ampl, w.next());
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll 4
            for (int r = 0; r < 16; r++)
            {
                const int fr = r * 4 + (lane >> 4), sidx = lane & 15;
                if (frame0 + fr < nFrames) iq[(size_t)(frame0 + fr) * frameStride + pos + i0 + sidx] = stage[wave][fr][sidx];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (!w.zero) w.endChirp();
        pos += w.NN;
    }
}

static hipError_t launchMod(float2 *iq, const long long frameStride, const unsigned short *syms, const long long symStride, const int *nsyms,
                            const size_t nFrames, const int maxNsyms, const int sync, const float ampl, const int padding, const int sf,
                            hipStream_t stream)
{
    if (nFrames == 0) return hipSuccess;
    const unsigned grid = unsigned((nFrames + 255) / 256);
    hipLaunchKernelGGL(modFrames, dim3(grid), dim3(256), 0, stream, iq, frameStride, syms, symStride, nsyms, unsigned(nFrames), maxNsyms,
                       sync, ampl, padding, 1 << sf);
    return hipGetLastError();
}

hipError_t launchModFrames(float2 *iq, const long long frameStride, const unsigned short *syms, const size_t nFrames,
                           const int nsyms, const int sync, const float ampl, const int padding, const int sf, hipStream_t stream)
{
    return launchMod(iq, frameStride, syms, nsyms, nullptr, nFrames, nsyms, sync, ampl, padding, sf, stream);
}

hipError_t launchModFramesVar(float2 *iq, const long long frameStride, const unsigned short *syms, const long long symStride,
                              const int *nsyms, const size_t nFrames, const int maxNsyms, const int sync, const float ampl,
                              const int padding, const int sf, hipStream_t stream)
{
    return launchMod(iq, frameStride, syms, symStride, nsyms, nFrames, maxNsyms, sync, ampl, padding, sf, stream);
}

/***********************************************************************
 * Synthetic up-chirp symbols + AWGN, generated in HBM (bench / test input).
 * Window w = ampl * exp(j*phi_i), phi following ChirpGenerator.hpp:22-47 for an up-chirp
 * with f0 = 2*pi*sym/N and ovs = 1 in closed form (per-window phase origin 0):
 *   f_i = -pi + f0 + (i+1)*2pi/N, wrapped by -2pi once it exceeds +pi
 *   phi_i = sum_{j<=i} f_j
 * evaluated in fp64 then rounded; noise: counter-based splitmix64 -> Box-Muller.
 **********************************************************************/
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

//! sample e of the noise stream `seed`: a unit complex Gaussian (re, im) in double, Box-Muller of the two 32-bit halves of one draw
__device__ __forceinline__ double2 noiseSample(const unsigned long long seed, const size_t e)
{
    const unsigned long long r = splitmix64(seed ^ (e * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull));
    const double u1 = ((double)(r >> 32) + 1.0) * (1.0 / 4294967296.0);
    const double u2 = (double)(r & 0xffffffffu) * (1.0 / 4294967296.0);
    const double rad = sqrt(-2.0 * log(u1));
    double s2, c2;
    sincos(6.283185307179586476925 * u2, &s2, &c2);
    return make_double2(rad * c2, rad * s2);
}

template <int LOG2N>
__global__ void synthSymbols(float2 *iq, const unsigned short *sym, const size_t nWindows,
                             const float ampl, const float sigma, const unsigned long long seed)
{
    constexpr int N = 1 << LOG2N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = nWindows * (size_t)N;
    for (size_t e = gid; e < total; e += (size_t)gridDim.x * blockDim.x)
    {
        const size_t w = e >> LOG2N;
        const int i = (int)(e & (N - 1));
        const int s = sym[w] & (N - 1);
        // number of samples j<=i whose instantaneous frequency has already wrapped: j+1+s > N  <=>  j >= N-s
        const double twoPiN = 6.283185307179586476925 / N;
        const double n1 = (double)(i + 1);
        double phi = n1 * (-3.14159265358979323846 + twoPiN * s) + twoPiN * 0.5 * n1 * (n1 + 1.0);
        const int wrapped = i - (N - s) + 1;     // count of wrapped samples among 0..i
        if (wrapped > 0) phi -= 6.283185307179586476925 * (double)wrapped;
        phi -= 6.283185307179586476925 * floor(phi / 6.283185307179586476925);
        double sn, cs;
        sincos(phi, &sn, &cs);
        float re = ampl * (float)cs, im = ampl * (float)sn;
        if (sigma > 0.0f)
        {
            const double2 g = noiseSample(seed, e);
            re += sigma * (float)g.x;
            im += sigma * (float)g.y;
        }
        iq[e] = make_float2(re, im);
    }
}

hipError_t launchSynth(const int sf, float2 *iq, const unsigned short *sym, const size_t nWindows,
                       const float ampl, const float sigma, const unsigned long long seed, hipStream_t stream)
{
    if (nWindows == 0) return hipSuccess;
    const dim3 block(256), grid(2048);
    switch (sf)
    {
#define LORAHIP_SYNTH_CASE(SF) case SF: hipLaunchKernelGGL(synthSymbols<SF>, grid, block, 0, stream, iq, sym, nWindows, ampl, sigma, seed); break;
    LORAHIP_SYNTH_CASE(6) LORAHIP_SYNTH_CASE(7) LORAHIP_SYNTH_CASE(8) LORAHIP_SYNTH_CASE(9)
    LORAHIP_SYNTH_CASE(10) LORAHIP_SYNTH_CASE(11) LORAHIP_SYNTH_CASE(12)
#undef LORAHIP_SYNTH_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

//! complex AWGN added in place: the channel of the loopback test (TestLoopback.cpp:98-99 adds a noise source to the
//! modulator output). Same counter-based generator as synthSymbols.
__global__ void addAwgn(float2 *iq, const size_t n, const float sigma, const unsigned long long seed)
{
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t e = gid; e < n; e += (size_t)gridDim.x * blockDim.x)
    {
        const double2 g = noiseSample(seed, e);
        float2 v = iq[e];
        v.x += sigma * (float)g.x;
        v.y += sigma * (float)g.y;
        iq[e] = v;
    }
}

hipError_t launchAwgn(float2 *iq, const size_t n, const float sigma, const unsigned long long seed, hipStream_t stream)
{
    if (n == 0 || sigma == 0.0f) return hipSuccess;
    hipLaunchKernelGGL(addAwgn, dim3(2048), dim3(256), 0, stream, iq, n, sigma, seed);
    return hipGetLastError();
}

} // namespace lorahip
