// Transmit side, scheduled frames: the modulator that takes SF, channel row and start sample PER FRAME and writes each frame's body into
// (nRows, rowLen) channel rows (lorahip_mod_frames_sched) -- the load generator in front of a synthesiser, a downlink scheduler.
//
// The frame is the one modFrames (lorahip_tx.hip) walks, by the same walker (lorahip_framewalk.h): the reference's float frequency / phase
// recurrence, one accumulator from 0 through 10 up-chirps, the two sync chirps, 2 1/4 down-chirps and the data chirps, reduced mod 2 pi in
// double at the end of every chirp. Only that recurrence is serial -- three float operations a sample. The sincos of the phase in double,
// which is nearly all of the work, is independent per sample. So a GROUP of L = 4 / 16 / 64 lanes of a wavefront owns a frame: lane 0
// walks a tile of LORAHIP_SCHED_TILE samples and leaves their float32 phases in the group's LDS slice, then the L lanes take the samples of
// the tile L apart -- consecutive lanes consecutive samples, so the stores coalesce at any start -- evaluate, scale and store. Groups never span a wavefront: wave-level fences order the LDS traffic, as in modFrames.
// L = 64 is one frame per wavefront and no divergence between frames of different SF; with L = 4 / 16 the groups of a wavefront are frames
// taken in the order given, and the wavefront runs as long as its longest frame. tests/test_gpu_mod_sched.py requires every body
// bit-identical to lorahip_mod_frames' frame for the same symbols.
#include "lorahip_internal.h"
#include "lorahip_framewalk.h"

namespace lorahip {

#define LORAHIP_SCHED_TILE 64                  // samples a group's walker runs ahead of its sincos lanes

/* Frame f: status -1 (no usable symbol count: the encoder's refusals arrive here), -3 (no such SF or row), -2 (the body does not lie inside
 * the row), in that order; any of them writes nothing. The slices are TILE + L floats apart (L < 64): the walkers of a wavefront then write,
 * and its lanes then read, 64 different banks. */
template <int L>
__global__ void __launch_bounds__(256) modFramesSched(const ModSchedArgs a)
{
    constexpr int T = LORAHIP_SCHED_TILE, PER = 256 / L, SLICE = T + (L < 64 ? L : 0);
    static_assert(T % 16 == 0 && (1 << LORAHIP_SF_MIN) / 4 % 16 == 0, "the walk below is unrolled over 16 samples");
    __shared__ float sPhase[PER * SLICE];
    const int g = threadIdx.x / L, t = threadIdx.x % L;
    float *sP = sPhase + g * SLICE;
    const unsigned frame = blockIdx.x * PER + g;
    const bool have = frame < a.nFrames;
    const unsigned fc = have ? frame : 0;
    const int nsyms = a.nsyms[fc], sf = a.sf[fc], row = a.row[fc];
    const long long start = a.start[fc];
    int status = 0;
    long long body = 0;
    if (nsyms < 1 || nsyms > a.symStride) status = -1;
    else if (sf < LORAHIP_SF_MIN || sf > LORAHIP_SF_MAX || row < 0 || row >= a.nRows) status = -3;
    else
    {
        body = ((long long)(14 + nsyms) << sf) + (1ll << (sf - 2));
        if (start < 0 || body > a.rowLen || start > a.rowLen - body) status = -2;
    }
    if (have && t == 0 && a.status != nullptr) a.status[frame] = status;
    if (!have || status != 0) body = 0;                                    // (group-uniform: the whole group leaves the loop below alone)

    const int N = 1 << (body ? sf : LORAHIP_SF_MIN);
    const unsigned short *mySyms = a.syms + (size_t)fc * a.symStride;
    const float ampl = a.amplOf != nullptr ? a.amplOf[fc] : a.ampl;
    float2 *out = a.iq + (body ? (size_t)row * a.rowStride + start : 0);
    FrameWalk w(N);
    // the walker's place in the frame: chirp c, sample i of its w.NN. The body ends with the last symbol: no zero chirp is walked
    int c = 0, i = 0;
    w.chirp(0, a.sync, mySyms, nsyms);
    for (long long base = 0; base < body; base += T)
    {
        const int n = body - base < T ? int(body - base) : T;
        if (t == 0)
        {
            int j = 0;
            while (j < n)
            {
                // the rest of the tile or of the chirp. A multiple of 16: chirps are N or N / 4 >= 16 samples, so the body, the tiles
                // (of 64) and every chirp boundary inside a tile are -- the walk is unrolled over 16 samples without a remainder
                const int m = n - j < w.NN - i ? n - j : w.NN - i;
                for (int k = 0; k < m; k += 16)
                {
#pragma unroll
                    for (int u = 0; u < 16; u++) sP[j + k + u] = w.next();
                }
                j += m; i += m;
                if (i == w.NN)
                {
                    w.endChirp();
                    w.chirp(++c, a.sync, mySyms, nsyms);                   // (behind the last chirp: nothing is read)
                    i = 0;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j = t; j < n; j += L) out[base + j] = polar(ampl, sP[j]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

/* lanes = 0: by the frame count alone, from the measurements in DESIGN.md section 8j (SF7 and SF12; 16, 256, 4096 and 65536 frames: 64 lanes
 * are the fastest at 16 and 256, 16 at 4096, 4 at 65536, at both SFs). One frame per wavefront while every wavefront can have a SIMD of its own
 * (1024 of them), narrower groups -- fewer lanes idle during the walk -- once they share. Where exactly the instances cross between the
 * measured counts is not measured: the limits are 1024 = the SIMDs, and 16384 = four 16-lane wavefronts a SIMD. */
int modSchedLanes(const size_t nFrames)
{
    return nFrames <= 1024 ? 64 : nFrames <= 16384 ? 16 : 4;
}

template <int L>
static hipError_t launchSched(const ModSchedArgs &a, hipStream_t stream)
{
    const unsigned per = 256 / L;
    hipLaunchKernelGGL((modFramesSched<L>), dim3((a.nFrames + per - 1) / per), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchModFramesSched(const ModSchedArgs &a, int lanes, hipStream_t stream)
{
    if (a.nFrames == 0) return hipSuccess;
    if (lanes == 0) lanes = modSchedLanes(a.nFrames);
    if (lanes == 4) return launchSched<4>(a, stream);
    if (lanes == 16) return launchSched<16>(a, stream);
    if (lanes == 64) return launchSched<64>(a, stream);
    return hipErrorInvalidValue;
}

} // namespace lorahip
