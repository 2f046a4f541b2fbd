// Transmit side, per-frame symbol counts: the batched modulator for packets of different lengths (the encoder's output rows).
//
// modFramesVar walks a frame exactly as modFrames (lorahip_kernels.hip) does -- one lane per frame, the reference's float frequency /
// phase recurrence statement by statement (LoRaMod.cpp:135-229 on ChirpGenerator.hpp:22-47), 16 samples at a time through LDS so
// that the stores are 128-byte rows -- but reads the frame's symbol count from nsyms[frame] and walks EVERY frame to the length of
// maxNsyms symbols: the chirps behind a frame's own symbols are zero chirps. A zero chirp does not touch the phase accumulator, so
// row f is the uniform kernel's frame for the same symbols with padding + maxNsyms - nsyms[f].
//
// The ~60 lines of the frame walk are a SECOND COPY of modFrames' on purpose: lorahip_kernels.hip is one of the files the committed
// counter measurements are stamped with (build.py: kernel_digest), and sharing the walk would mean editing it. The two are kept in step
// by tests/test_gpu_encoder.py, which requires bit-identical frames from both kernels when all counts are equal.
#include "lorahip_internal.h"

namespace lorahip {

__global__ void __launch_bounds__(256) modFramesVar(float2 *__restrict__ iq, const long long frameStride,
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
    int nsyms = mine ? nsymsOf[frame] : -1;
    // a refused packet (negative count) or a count the rows of this launch cannot hold: the whole frame is zero chirps
    const bool silent = nsyms < 0 || nsyms > maxNsyms;
    if (silent) nsyms = 0;
    const float fMin = (float)(-M_PI), fMax = (float)M_PI;                 // ovs = 1   ChirpGenerator.hpp:25-26
    const float fStep = (float)((2 * M_PI) / N);                           //           :27
    float phaseAccum = 0.0f;                                               // LoRaMod.cpp:135
    long long pos = 0;
    const int pad = padding < 1 ? 1 : padding;                             // one zero symbol is emitted before the test (LoRaMod.cpp:218-224)
    const int nChirps = 10 + 2 + 3 + maxNsyms + pad;                       // the same for every frame of the launch
    for (int c = 0; c < nChirps; c++)
    {
        // what this chirp is (LoRaMod.cpp:141-229); length and direction are the same for every frame, f0 and where the zeros begin differ
        int NN = N;
        bool down = false, zero = silent;
        float f0 = 0.0f;
        if (c < 10) {}
        else if (c == 10) f0 = (float)((2 * M_PI * ((sync >> 4) * 8)) / N);
        else if (c == 11) f0 = (float)((2 * M_PI * ((sync & 0xf) * 8)) / N);
        else if (c < 14) down = true;
        else if (c == 14) { down = true; NN = N / 4; }
        else if (c < 15 + nsyms) f0 = (float)((2 * M_PI * (int)mySyms[c - 15]) / N);
        else zero = true;
        float f = fMin + f0;                                               // ChirpGenerator.hpp:28
        for (int i0 = 0; i0 < NN; i0 += 16)
        {
#pragma unroll 4
            for (int i = 0; i < 16; i++)
            {
                float2 v = make_float2(0.0f, 0.0f);
                if (!zero)
                {
                    f += fStep;                                            // :31 / :39
                    if (f > fMax) f -= (fMax - fMin);
                    phaseAccum = down ? phaseAccum - f : phaseAccum + f;
                    double sn, cs;
                    sincos((double)phaseAccum, &sn, &cs);
                    v = make_float2(ampl * (float)cs, ampl * (float)sn);   // std::polar(ampl, phaseAccum)
                }
                stage[wave][lane][i] = v;
            }
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
        if (!zero) phaseAccum = (float)((double)phaseAccum - floor((double)phaseAccum / (2 * M_PI)) * 2 * M_PI);   // :45
        pos += NN;
    }
}

hipError_t launchModFramesVar(float2 *iq, const long long frameStride, const unsigned short *syms, const long long symStride,
                              const int *nsyms, const size_t nFrames, const int maxNsyms, const int sync, const float ampl,
                              const int padding, const int sf, hipStream_t stream)
{
    if (nFrames == 0) return hipSuccess;
    const unsigned grid = unsigned((nFrames + 255) / 256);
    hipLaunchKernelGGL(modFramesVar, dim3(grid), dim3(256), 0, stream, iq, frameStride, syms, symStride, nsyms, unsigned(nFrames), maxNsyms,
                       sync, ampl, padding, 1 << sf);
    return hipGetLastError();
}

} // namespace lorahip
