// The LoRa transmit frame, walked: the ONE copy of the reference's float frequency / phase recurrence (LoRaMod.cpp:135-229 on
// genChirp<float>, ChirpGenerator.hpp:22-47) that every modulator kernel follows statement by statement -- modFrames (lorahip_tx.hip),
// one lane per frame, and modFramesSched<L> (lorahip_txsched.hip), lane 0 of a group of L. A frame is 10 up-chirps, the two sync chirps,
// 2 1/4 down-chirps, one up-chirp per symbol and zero chirps behind them; ONE float phase accumulator runs from 0 through all of it and
// is reduced mod 2 pi in double at the end of every chirp. tests/modulator_def.py states the same in numpy.
//
// The walker is plain C++ over <cmath> and compiles for the host as well: tests/framewalk_check.cpp walks frames on the CPU and
// tests/test_framewalk_cpu.py requires its phases bit-equal to the definition's. polar() exists for device code only -- the sample is
// "sincos in double, rounded once", and the host's sincos is not the device's.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define LORAHIP_WALK_FN __host__ __device__ __forceinline__
#else
#define LORAHIP_WALK_FN inline
#endif

namespace lorahip {

struct FrameWalk
{
    const float fMin = (float)(-M_PI), fMax = (float)M_PI;                 // ovs = 1   ChirpGenerator.hpp:25-26
    const float fStep;                                                     //           :27
    float phaseAccum = 0.0f;                                               // LoRaMod.cpp:135
    float f = 0.0f;
    const int N;
    int NN = 0;                                                            // samples of the current chirp
    bool down = false, zero = false;                                       // a zero chirp touches neither f nor the accumulator

    LORAHIP_WALK_FN explicit FrameWalk(const int N_) : fStep((float)((2 * M_PI) / N_)), N(N_) {}

    //! what chirp c is (LoRaMod.cpp:141-229) in a frame of nsyms of the symbols at syms: length and direction depend on c alone, f0 and
    //! where the zeros begin on the frame. A negative nsyms is a silent frame, zero chirps from the first. A zero chirp reads no symbol
    LORAHIP_WALK_FN void chirp(const int c, const int sync, const unsigned short *syms, const int nsyms)
    {
        NN = N;
        down = false;
        zero = nsyms < 0;
        float f0 = 0.0f;
        if (c < 10) {}
        else if (c == 10) f0 = (float)((2 * M_PI * ((sync >> 4) * 8)) / N);
        else if (c == 11) f0 = (float)((2 * M_PI * ((sync & 0xf) * 8)) / N);
        else if (c < 14) down = true;
        else if (c == 14) { down = true; NN = N / 4; }
        else if (c < 15 + nsyms) f0 = (float)((2 * M_PI * (int)syms[c - 15]) / N);
        else zero = true;
        f = fMin + f0;                                                     // ChirpGenerator.hpp:28
    }

    //! one sample of a chirp that is not a zero chirp: its phase
    LORAHIP_WALK_FN float next()
    {
        f += fStep;                                                        // :31 / :39
        if (f > fMax) f -= (fMax - fMin);
        phaseAccum = down ? phaseAccum - f : phaseAccum + f;
        return phaseAccum;
    }

    //! the end of a chirp that is not a zero chirp: the accumulator mod 2 pi, in double. Whoever walks zero chirps skips it for them
    LORAHIP_WALK_FN void endChirp()
    {
        phaseAccum = (float)((double)phaseAccum - floor((double)phaseAccum / (2 * M_PI)) * 2 * M_PI);   // :45
    }
};

#ifdef __HIPCC__
//! std::polar(ampl, phase): cos / sin in double, rounded once -- the correctly rounded float but for rare last-ulp cases (tests/)
__device__ __forceinline__ float2 polar(const float ampl, const float phase)
{
    double sn, cs;
    sincos((double)phase, &sn, &cs);
    return make_float2(ampl * (float)cs, ampl * (float)sn);
}
#endif

} // namespace lorahip

#undef LORAHIP_WALK_FN
