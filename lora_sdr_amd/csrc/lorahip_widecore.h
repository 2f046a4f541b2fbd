// What the batch kernel (lorahip_wide.hip) and the streaming demod kernel (lorahip_stream_wide.hip) of the long windows (SF11, SF12)
// share: configuration, LDS layouts, the fine-tune index chain of a window that spans several wavefronts, and WideCore<C> -- the
// window load, the chain's read-back and the peak's neighbours for both, and for the streaming kernel phase 0 -> exchange -> last
// phase and the |X|^2 scan finished across the window's wavefronts (the batch kernel has those in its body, see WideCore). One window is spread over the wavefronts of a workgroup, 16 points per lane.
//
// Same algebra as lorahip_fastcore.h (three register phases of kissfft's DIT graph, two transpositions through LDS), but
// T = N/16 lanes per window is 128 (SF11) or 256 (SF12), so the exchanges are fenced with workgroup barriers and the |X|^2
// arg-max / fp64 total is finished across wavefronts through LDS.
//
//   phase 0  bits [0,B1)      lane t holds samples n = VEC*t+u + (N/R)*r, r < R = 16/VEC     (registers)
//   exch 0   row per n_low = VEC*t+u (R elements, padded/rotated so writes and reads tile the banks)
//   phase 1  bits [B1,B1+4)   lane t: klow = t mod R, high = t / R, element e = position bits [B1,B1+4)
//   exch 1   natural position order, 8 elements of padding per 2^(B1+4) block (plain layout; INPLACE: phase 1 writes back in place)
//   phase 2  bits [B1+4,LOG2N) lane t holds bins t + T*e                                       (registers)
#pragma once
#include "lorahip_fft.h"

namespace lorahip {

constexpr int SCAN_CHAINS_WIDE = 1;     // independent compare-and-select chains of a lane's 16-bin scan (laneScan)

// The chirp values of a lane's sample positions and the last-phase twiddles live in registers; the twiddles of the first two phases in LDS.
template <int LOG2N_, int VEC_, int MINW_, int X0ROT_, int X0PAD_, int X0S_, int X0D_, bool PREFETCH_ = true, bool NT_ = false, int WPB_ = 0,
          bool INPLACE_ = false, int X0S2_ = 0, int X0D2_ = 0>
struct WideCfg
{
    static constexpr int LOG2N = LOG2N_, N = 1 << LOG2N_;
    static constexpr int P = 16;                               // points per lane
    static constexpr int LOG2T = LOG2N_ - 4, T = 1 << LOG2T;    // lanes per window
    static constexpr int VEC = VEC_, R = P / VEC_;
    static constexpr int B1 = (VEC_ == 1 ? 4 : 3), B2 = B1 + 4;
    static constexpr int WPB = WPB_ ? WPB_ : 256 / T;           // windows per workgroup iteration
    static constexpr int BLOCK = WPB * T;                       // threads per workgroup (128 or 256)
    static constexpr int BPC = MINW_ * 256 / BLOCK;             // workgroups per CU at MINW waves per SIMD
    static constexpr int WPWIN = T / 64;                        // wavefronts per window
    static constexpr int MINW = MINW_;
    static constexpr bool NT = NT_;                             // non-temporal hint on the IQ loads
    static constexpr bool INPLACE = INPLACE_;                   // the middle phase writes its results back where it read its inputs:
                                                                // no barrier between the two, the last phase reads the exchange-0 layout
    static constexpr bool PREFETCH = PREFETCH_;                 // next set's samples in registers during this set (else: loaded at the top, hidden by co-resident workgroups)
    static constexpr int HB = LOG2N_ - B2;                      // = 4: position bits of the last phase
    static constexpr int NL = VEC_ * T, LOG2NL = LOG2N_ - B1;   // rows of exchange 0
    static_assert(B2 + 4 == LOG2N_, "VEC 1 <-> SF12, VEC 2 <-> SF11");
    static_assert(T >= 64 && T <= 256, "a window is 1..4 wavefronts");
    static constexpr int RS0 = R + X0PAD_;
    __host__ __device__ static constexpr int x0off(const int nlow)
    {
        const int rot = ((nlow >> X0ROT_) | (nlow << (LOG2NL - X0ROT_))) & (NL - 1);
        return rot * RS0 + ((nlow >> X0S_) & 1) * X0D_ + ((nlow >> X0S2_) & 1) * X0D2_;
    }
    static constexpr int X0ELEMS = NL * RS0 + X0D_ + X0D2_;
    static constexpr int X1 = 16 * R + 8;                       // one block of `high` in exchange 1
    static constexpr int X1ELEMS = INPLACE_ ? 0 : 16 * X1;
    static constexpr int XE = X0ELEMS > X1ELEMS ? X0ELEMS : X1ELEMS;
    static constexpr int XW = ((XE * 2 > N ? XE : (N + 1) / 2) + 1) & ~1;   // v2f per window; also holds N ints
    static constexpr int TW_LDS = twStageOffset(LOG2N_, B2);          // twiddle entries staged in LDS: the stages below the last phase
    static constexpr int TWN = (TW_LDS + 1) & ~1;
};

struct RedRec { float v; int i; double tot; };

//! where fineChainGroup<64,16> (1024-sample chunks) leaves the index of sample n
__device__ __forceinline__ int chainSlot(const int n) { return (n & ~1023) + (n & 15) * 64 + ((n >> 4) & 63); }

/*! The fine-tune index recurrence of a window that spans WPWIN wavefronts (fineChainGroup's scheme with the hand-over
 * between wavefronts through LDS): every lane walks its 16 consecutive samples from a guessed start, the ends are
 * compared with the successors' starts, the guesses repaired by the prefix sum of the mismatches, until all agree.
 * Called by every thread of the workgroup (workgroup barriers inside); t = lane inside the window, wwin = wavefront
 * inside the window, sC = 12 ints of LDS scratch per window. Leaves the index of sample n at sIdx[chainSlot(n)] and
 * returns the index after the N steps (to every thread of the window). */
template <int T, int M>
__device__ __forceinline__ int fineChainBlock(const int idx0, const float d, const int t, const int wwin, int *sIdx, int *sC)
{
    constexpr int WPWIN = T / 64;
    const int lane = t & 63;
    const int first = fineStep(idx0, d, M);
    int c = first - idx0;
    if (c > M / 2) c -= M;
    else if (c < -M / 2) c += M;
    int g = (idx0 + c * (16 * t)) & (M - 1);
    int loc[16];
    int e = 0;
    for (int round = 0; round <= T; round++)
    {
        int idx = g;
#pragma unroll
        for (int i = 0; i < 16; i++) { loc[i] = idx; idx = fineStep(idx, d, M); }
        e = idx;
        if (lane == 63) sC[wwin] = e;                       // hand-over to the next wavefront
        __syncthreads();
        const int up = __shfl_up(e, 1, 64);
        const int prevE = lane > 0 ? up : (wwin == 0 ? idx0 : sC[wwin - 1]);
        int delta = (prevE - g) & (M - 1);
        if (!__syncthreads_or(delta != 0)) break;
        // inclusive prefix sum of the mismatches over the window's lanes (mod M)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
        {
            const int o = __shfl_up(delta, off, 64);
            if (lane >= off) delta += o;
        }
        if (lane == 63) sC[4 + wwin] = delta;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WPWIN - 1; k++) if (k < wwin) delta += sC[4 + k];
        g = (g + delta) & (M - 1);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) sIdx[wwin * 1024 + i * 64 + lane] = loc[i];
    if (t == T - 1) sC[8] = e;
    __syncthreads();
    return sC[8];
}

//! the dynamic LDS of a workgroup, batch and streaming: what the kernels carve and the launchers ask for
template <class C>
struct WideSmem
{
    //! detectWide: everything but the split fine-tune tables (16-byte multiple: the tables follow)
    static constexpr size_t base()
    {
        return (size_t(C::TWN + C::WPB * C::XW) * sizeof(float2) + 4 * sizeof(RedRec) + size_t(C::WPB) * 2 * sizeof(float2) + sizeof(TailRec) + size_t(C::WPB) * 12 * sizeof(int) + 15) & ~size_t(15);
    }
    static constexpr size_t bytes(const bool withFine) { return base() + (withFine ? FineDims<C::LOG2N>::BYTES : 0); }

    //! demodStreamWide (one window per workgroup): this record, the split fine-tune tables (lorahip_fine.h) behind it, and behind
    //! those the resident receiver's ResLds (resLds = its size; 0 in the other instances)
    struct Stream
    {
        v2f tw[C::TWN];                  // stage twiddles below the last phase
        v2f x[C::XW];                    // the exchange region
        RedRec red[4];                   // one per wavefront
        v2f nb[2];                       // bins left/right of the peak
        int chain[12];                   // fineChainBlock scratch
    };
    static_assert(sizeof(Stream) % 16 == 0, "the split tables are read with ds_read_b128");
    static constexpr size_t streamBytes(const size_t resLds = 0) { return sizeof(Stream) + FineDims<C::LOG2N>::BYTES + resLds; }
};

/***********************************************************************
 * configurations: geometry per SF x layout (the plain padded exchange-0 layout, or the swizzled one the in-place middle
 * phase needs -- both found with tools/lds_conflicts.py), plus an option mask.
 **********************************************************************/
template <int SF, bool INPLACE> struct WGeo;
//                                                  VEC  X0: ROT PAD S  D   S2 D2
template <> struct WGeo<11, false> { enum { VEC = 2, ROT = 0, PAD = 1, S = 4, D = 1,  S2 = 0, D2 = 0 }; };    // 128 lanes x 16 pts: [R2,4] X [4,4] X [4,4]
template <> struct WGeo<11, true>  { enum { VEC = 2, ROT = 3, PAD = 1, S = 1, D = 4,  S2 = 2, D2 = 8 }; };
template <> struct WGeo<12, false> { enum { VEC = 1, ROT = 0, PAD = 1, S = 0, D = 0,  S2 = 0, D2 = 0 }; };    // 256 lanes x 16 pts: [4,4] X [4,4] X [4,4]
template <> struct WGeo<12, true>  { enum { VEC = 1, ROT = 0, PAD = 1, S = 6, D = 16, S2 = 7, D2 = 16 }; };

enum : unsigned
{
    WW2 = 1u << 0,                       // register budget set for two waves per SIMD (default: three)
    WPF_NONE = 1u << 1,                  // no register prefetch of the next window
    WNT = 1u << 2,                       // non-temporal IQ loads
    WONE = 1u << 3,                      // one window per workgroup (SF11: 128 threads)
    WINPLACE = 1u << 4                   // in-place middle phase (3 barriers per window instead of 4)
};
template <int SF, unsigned O>
using Wide = WideCfg<SF, WGeo<SF, (O & WINPLACE) != 0>::VEC, (O & WW2) ? 2 : 3,
                     WGeo<SF, (O & WINPLACE) != 0>::ROT, WGeo<SF, (O & WINPLACE) != 0>::PAD, WGeo<SF, (O & WINPLACE) != 0>::S,
                     WGeo<SF, (O & WINPLACE) != 0>::D, !(O & WPF_NONE), (O & WNT) != 0,
                     (O & WONE) ? 1 : 0, (O & WINPLACE) != 0, WGeo<SF, (O & WINPLACE) != 0>::S2, WGeo<SF, (O & WINPLACE) != 0>::D2>;

// streaming demodulator configurations (demodStreamWide, lorahip_stream_wide.hip): one channel per workgroup, in-place middle phase
typedef Wide<11, WW2 | WPF_NONE | WONE | WINPLACE> StreamWide11;
typedef Wide<12, WW2 | WPF_NONE | WINPLACE> StreamWide12;

//! host-side check of a configuration's exchange-0 layout: every (row, element) has its own word inside the region
template <class C>
static bool layoutOk()
{
    std::vector<char> used(size_t(C::XW), 0);
    for (int n = 0; n < C::NL; n++)
        for (int e = 0; e < C::R; e++)
        {
            const int a = C::x0off(n) + e;
            if (a < 0 || a >= C::XW || used[size_t(a)]) return false;
            used[size_t(a)] = 1;
        }
    return true;
}

/***********************************************************************
 * the window code. t = lane inside the window, X = the window's exchange region, sTw = the LDS copy of the stage twiddles
 * below the last phase. Every thread of the workgroup calls fft / scanReduce (workgroup barriers inside).
 * Both kernels call load, chainIndices and postNeighbours. loadChirp, fft and scanReduce are demodStreamWide's: detectWide
 * keeps those three blocks, its register twiddles and variant 10's plain-layout arm in its own body, because through a member
 * its launch-uniform instances (the steady state) compile to other code and measured 0.2-0.3 % slower (profiles/r14/README.md).
 **********************************************************************/
template <class C>
struct WideCore
{
    static constexpr int N = C::N, T = C::T, VEC = C::VEC, R = C::R, WPWIN = C::WPWIN;
    static constexpr int LOG2N = C::LOG2N, LOG2T = C::LOG2T, B1 = C::B1, B2 = C::B2, HB = C::HB;
    static constexpr int SLOTS = lastPhaseSlots<LOG2N, B2, LOG2N>();
    static constexpr int M = N * LORAHIP_FINE_STEPS;
    typedef v2f TwR[SLOTS];

    //! chirp table values of this lane's sample positions; s0 = -1: _upChirpTable = conj(_downChirpTable) (LoRaDemod.cpp:103-104)
    static __device__ __forceinline__ void loadChirp(v2f (&ch)[R][VEC], const v2f *down, const int t, const float s0)
    {
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++)
            {
                const v2f c = down[VEC * t + u + VEC * T * r];
                ch[r][u] = MAKE2(c.x, s0 * c.y);
            }
    }

    //! coalesced window load: VEC*8 bytes per lane, a wavefront covers 512 or 1024 contiguous bytes, R rows
    static __device__ __forceinline__ void load(v2f (&xn)[R][VEC], const v2f *in_, const int t)
    {
#pragma unroll
        for (int r = 0; r < R; r++)
        {
            const v2f *p = in_ + VEC * t + VEC * T * r;
            if (VEC == 2)
            {
                const v4f q = C::NT ? __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p)) : *reinterpret_cast<const v4f *>(p);
                xn[r][0] = MAKE2(q.x, q.y);
                xn[r][VEC - 1] = MAKE2(q.z, q.w);
            }
            else xn[r][0] = C::NT ? __builtin_nontemporal_load(p) : *p;
        }
    }

    //! fine-tune indices of this lane's samples from where fineChainBlock left them
    static __device__ __forceinline__ void chainIndices(unsigned (&yv)[R][VEC], const int *sIdx, const int t)
    {
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) yv[r][u] = (unsigned)sIdx[chainSlot(VEC * t + u + VEC * T * r)];
    }

    //! dechirped samples x -> FFT bins vl (lane t holds bins t + T*e), in-place middle phase (C::INPLACE): three barriers' worth of
    //! detectWide's window body without its prefetch and deferred tail work
    //! unit: phase 0 multiplies by twiddle(0) as kissfft does (runPhase's UNITMUL), workgroup-uniform: the streaming kernels' second pass
    //! over a window whose bins came out non-finite
    static __device__ __forceinline__ void fft(const v2f (&x)[R][VEC], v2f *X, const int t, const v2f *sTw, const TwR &twR, v2f (&vl)[16],
                                               const bool unit = false)
    {
        static_assert(C::INPLACE, "the swizzled exchange-0 layout");
        // ---- phase 0: bits [0, B1) in registers, one group per u -----------------------------
        v2f v0[VEC][R];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) v0[u][Plan<LOG2N>::pos(VEC * T * r) & (R - 1)] = x[r][u];
#pragma unroll
        for (int u = 0; u < VEC; u++)
        {
            if (unit) runPhase<LOG2N, 0, B1, false, true>(v0[u], 0, sTw, nullptr);
            else runPhase<LOG2N, 0, B1, false>(v0[u], 0, sTw, nullptr);
        }

        // ---- exchange 0 ----------------------------------------------------------------------
#pragma unroll
        for (int u = 0; u < VEC; u++)
        {
            v2f *row = X + C::x0off(VEC * t + u);
#pragma unroll
            for (int e = 0; e < R; e++) row[e] = v0[u][e];
        }
        __syncthreads();                                                                      // B1
        // phase 1 (middle) in place: bits [B1, B2); klow = t mod R, high = t / R
        v2f v1[16];
        const int klow = t & (R - 1), rhigh = rev4(t >> B1, HB);
#pragma unroll
        for (int e = 0; e < 16; e++) v1[e] = X[C::x0off((rev4(e, 4) << HB) | rhigh) + klow];
        runPhase<LOG2N, B1, B2, false>(v1, klow, sTw, nullptr);
        // write-back in place: only this lane touches these 16 words between B1 and B3
#pragma unroll
        for (int e = 0; e < 16; e++) X[C::x0off((rev4(e, 4) << HB) | rhigh) + klow] = v1[e];
        __syncthreads();                                                                      // B3
        // last phase: lane t holds positions t + T*e2; t = klow + R*e_mid, e2 = high
        const int rmid = rev4(t >> B1, 4) << HB;
#pragma unroll
        for (int e = 0; e < 16; e++) vl[e] = X[C::x0off(rmid | rev4(e, HB)) + klow];
        runPhase<LOG2N, B2, LOG2N, true>(vl, 0, nullptr, twR);
    }

    //! LoRaDetector.hpp:36-48 over the window's bins (bin = t + T*e, ascending in e): the lane scan, the wavefront's reduction, its
    //! record to sRed[wave], a barrier (B4), and the window's WPWIN records combined by every lane in the same order: identical
    //! results on all of them. !exact: the total in fp32 (laneScanQuick: the squelch estimate), the same winner
    static __device__ __forceinline__ void scanReduce(const v2f (&vl)[16], RedRec *sRed, const int t, const int lane, const int wave,
                                                      float &bestV, int &bestI, double &tot, const bool exact)
    {
        int bestE;
        if (exact) bestE = laneScan<16, SCAN_CHAINS_WIDE>([&](const int e) { return vl[e]; }, bestV, tot);
        else
        {
            float totF;
            bestE = laneScanQuick<16>([&](const int e) { return vl[e]; }, bestV, totF);
            tot = (double)groupSumF32<64>(totF);
        }
        bestI = t + (bestE << LOG2T);
        if (!(bestV > 0.0f)) bestI = 0;
        groupArgmax<64>(bestV, bestI);
        if (exact) tot = groupSumF64<64>(tot);
        if (lane == 0) { sRed[wave].v = bestV; sRed[wave].i = bestI; sRed[wave].tot = tot; }
        __syncthreads();                                                                      // B4
        const RedRec r0 = sRed[0];
        bestV = r0.v; bestI = r0.i; tot = r0.tot;
#pragma unroll
        for (int k = 1; k < WPWIN; k++)
        {
            const RedRec rk = sRed[k];
            argmaxCombine(bestV, bestI, rk.v, rk.i);
            tot += rk.tot;
        }
    }

    //! neighbours of the peak for fIndex (LoRaDetector.hpp:56-57): the owners post them to sNb[0] / sNb[1]. Only the wavefront(s) that
    //! hold bin k-1 / k+1 walk the register-select tree.
    // (a tree of scalar branches on the wave-uniform bin number instead of the per-lane select tree measured 1 % SLOWER:
    // profiles/r03/s6_ab_scalar_pick_negative.txt)
    static __device__ __forceinline__ void postNeighbours(const v2f (&vl)[16], v2f *sNb, const int bestI, const int t)
    {
        const int bl = (bestI + N - 1) & (N - 1), br = (bestI + 1) & (N - 1);
        const bool ownL = (bl & (T - 1)) == t, ownR = (br & (T - 1)) == t;
        if (__any(ownL | ownR))
        {
            const v2f mine = selectFlat<16>(vl, ownL ? (bl >> LOG2T) : (br >> LOG2T));
            if (ownL) sNb[0] = mine;
            if (ownR) sNb[1] = mine;
        }
    }
};

} // namespace lorahip
