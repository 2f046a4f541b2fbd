// Tuned CDNA4 batch kernels for the long windows (SF11, SF12): one window spread over the wavefronts of a 256-thread workgroup
// (SF11: two windows per workgroup, or one in 128 threads; SF12: one), 16 points per lane. The configuration, the LDS layout, the
// index chain, the window load and the neighbour post are lorahip_widecore.h's, shared with the streaming kernel
// (lorahip_stream_wide.hip); the three FFT phases and the scan stand in the kernel's body (see WideCore there for why). Barrier budget per window set: 4, or 3 with the in-place middle phase (after each
// exchange write, and before the region is overwritten by the next exchange); the cross-wave reduction shares the last one and
// the read-back of the peak's neighbours is deferred behind the first barrier of the NEXT set, as is the sqrt/log tail (queued in
// LDS, executed 64 windows at a time by wave 0 with all lanes busy).
#include "lorahip_widecore.h"

namespace lorahip {

template <class C, bool DBG, bool UNI>
__global__ void __launch_bounds__(C::BLOCK, C::MINW)
detectWide(const DetectArgs a, const FastTables ft, const unsigned nSets)
{
    typedef WideCore<C> Core;
    constexpr int N = C::N, T = C::T, VEC = C::VEC, R = C::R, WPB = C::WPB, LOG2N = C::LOG2N, LOG2T = C::LOG2T, M = Core::M;
    constexpr int WPWIN = C::WPWIN, B1 = C::B1, B2 = C::B2, HB = C::HB, SLOTS = lastPhaseSlots<LOG2N, B2, LOG2N>();

    extern __shared__ __attribute__((aligned(16))) char smemRaw[];
    v2f *sTw = reinterpret_cast<v2f *>(smemRaw);                         // [TWN]
    v2f *sX = sTw + C::TWN;                                              // [WPB][XW]
    RedRec *sRed = reinterpret_cast<RedRec *>(sX + WPB * C::XW);         // [4]: one per wavefront
    v2f *sNb = reinterpret_cast<v2f *>(sRed + 4);                        // [WPB][2]: bins left/right of the peak
    TailRec &tr = *reinterpret_cast<TailRec *>(sNb + WPB * 2);
    int *sChain = reinterpret_cast<int *>(&tr + 1) + (threadIdx.x >> LOG2T) * 12;    // fineChainBlock scratch of this window
    double2 *sFine = reinterpret_cast<double2 *>(smemRaw + WideSmem<C>::base());     // split fine-tune tables (non-UNI kernels)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wsub = tid >> LOG2T;                        // window inside the workgroup iteration
    const int t = tid & (T - 1);
    v2f *X = sX + wsub * C::XW;

    const v2f *gIq = reinterpret_cast<const v2f *>(a.iq), *gDown = reinterpret_cast<const v2f *>(a.down);
    const v2f *gFine = reinterpret_cast<const v2f *>(a.fine);
    v2f *gDec = reinterpret_cast<v2f *>(a.decOut), *gFft = reinterpret_cast<v2f *>(a.fftOut);

    // ---- one-time set-up -------------------------------------------------------------
    if (tid < 64) tr.w[tid] = 0xffffffffu;                // empty tail slots
    for (int i = tid; i < C::TW_LDS; i += C::BLOCK) sTw[i] = reinterpret_cast<const v2f *>(ft.twStage)[i];

    // register twiddles of the last phase (klow = t there)
    v2f twR[SLOTS];
    {
        int slot = 0;
#pragma unroll
        for (int b = B2; b < LOG2N; b += 2)
#pragma unroll
            for (int kl = 0; kl < (1 << (b - B2)); kl++)
            {
                const int k = t + (kl << B2);
                const int base = twStageOffset(LOG2N, b) + k;
                twR[slot] = reinterpret_cast<const v2f *>(ft.twStage)[base];
                twR[slot + 1] = reinterpret_cast<const v2f *>(ft.twStage)[base + (1 << b)];
                twR[slot + 2] = reinterpret_cast<const v2f *>(ft.twStage)[base + (2 << b)];
                slot += 3;
            }
    }

    FineLds fl;
    fl.A = nullptr; fl.B = nullptr; fl.split = false;
    if (!UNI) fl = fineLoadLds<LOG2N>(sFine, a.fineA, a.fineB, tid, C::BLOCK);

    // chirp table values of this lane's sample positions: _upChirpTable = conj(_downChirpTable) (LoRaDemod.cpp:103-104)
    const bool perWindowSel = !UNI && a.chirpSel != nullptr;
    const float s0 = (!perWindowSel && a.chirpSelAll == LORAHIP_CHIRP_UP) ? -1.0f : 1.0f;
    v2f ch[R][VEC];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int u = 0; u < VEC; u++)
        {
            const v2f c = gDown[VEC * t + u + VEC * T * r];
            ch[r][u] = MAKE2(c.x, s0 * c.y);
        }
    __syncthreads();

    v2f xn[R][VEC];
    auto issueLoads = [&](const unsigned set_)
    {
        const unsigned w_ = set_ * WPB + wsub;
        const unsigned wc_ = w_ < a.nWindows ? w_ : a.nWindows - 1;
        Core::load(xn, gIq + (a.offsets ? a.offsets[wc_] : (long long)wc_ * a.stride), t);
    };
    if (C::PREFETCH) issueLoads(blockIdx.x);
    const v2f fconst0 = gFine[0];

    // result of the previous set, waiting for its neighbours / tail record
    bool havePrev = false, pActive = false;
    unsigned pW = 0, cnt = 0;
    int pI = 0;
    float pV = 0.0f;
    double pTot = 0.0;

    auto recordPrev = [&]()
    {
        if (havePrev && pActive && t == 0)
        {
            const int s = (cnt + wsub) & 63;
            tr.w[s] = pW; tr.idx[s] = pI; tr.val[s] = pV; tr.tot[s] = pTot;
            tr.l[s] = sNb[wsub * 2]; tr.r[s] = sNb[wsub * 2 + 1];
        }
    };
    auto flushIfFull = [&]()
    {
        if (havePrev)
        {
            cnt += WPB;
            if ((cnt & 63) == 0 && wave == 0)
            {
                const unsigned ww = tr.w[lane];
                if (ww < a.nWindows) detectTail(a, ww, tr.idx[lane], tr.val[lane], tr.tot[lane], tr.l[lane], tr.r[lane]);
                tr.w[lane] = 0xffffffffu;
            }
        }
    };

    const int prioSlot = wavefrontSlot();
    for (unsigned set = blockIdx.x; set < nSets; set += gridDim.x)
    {
        rotatePriority<C::MINW, LORAHIP_PRIO_BATCH>(prioSlot);
        const unsigned w = set * WPB + wsub;
        const bool active = w < a.nWindows;
        const unsigned wc = active ? w : a.nWindows - 1;  // an inactive half redoes the last window, results dropped
        const int sel = perWindowSel ? a.chirpSel[wc] : a.chirpSelAll;
        const int idx0 = a.fineIdx0 ? a.fineIdx0[wc] : 0;
        const float err = (!UNI && a.fineErr) ? a.fineErr[wc] : 0.0f;
        const bool dechirp = sel != LORAHIP_CHIRP_NONE;
        const float d = err * (float)LORAHIP_FINE_STEPS;
        const bool moving = dechirp && d != 0.0f;

        v2f x[R][VEC];
        if (!C::PREFETCH) issueLoads(set);
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) x[r][u] = xn[r][u];

        // ---- fine-tune indices of this lane's samples for windows whose index moves (LoRaDemod.cpp:160-162): closed form
        // (lorahip_fine.h); a workgroup that holds a window where the form does not apply walks the exact chain instead
        int *sIdx = reinterpret_cast<int *>(X);             // aliases the exchange region (free until phase 0 ends)
        bool anyMoving = false, usedChain = false;
        unsigned yv[R][VEC];
        if constexpr (!UNI)
        {
            // one window per workgroup (the default shapes): `moving` is the same in every thread, no vote needed
            if constexpr (WPB == 1) anyMoving = moving;
            else anyMoving = __syncthreads_or(moving);
            if (anyMoving)
            {
                const FinePlan pl = finePlan(moving ? d : 0.0f, M);
                const unsigned ymax = fineLaneIndices<LOG2N, VEC, T, R>(idx0, pl, t, yv);
                int idxEnd = fineEndIndex(idx0, pl, LOG2N, LOG2N + 7);
                // the closed form can only reach the value M under the modulus M + 1 (a positive non-integer step that is not the
                // walk-down-and-stay case, lorahip_fine.h): every other window of a one-window workgroup skips the vote and its barrier
                if (WPB == 1 && (pl.mod == (unsigned)M || pl.sat)) usedChain = !pl.regular;
                else usedChain = __syncthreads_or(!pl.regular || ymax == (unsigned)M);
                if (usedChain)
                {
                    idxEnd = fineChainBlock<T, M>(idx0, moving ? d : 0.0f, t, t >> 6, sIdx, sChain);
                    Core::chainIndices(yv, sIdx, t);
                }
                if (moving && t == 0 && a.fineIdxOut && active) a.fineIdxOut[w] = idxEnd;
            }
        }
        if (!moving && t == 0 && active && a.fineIdxOut) a.fineIdxOut[w] = idx0;

        // ---- dechirp: (samp * chirp) * fine   (LoRaDemod.cpp:159) ---------------------------
        const v2f fconst = a.fineIdx0 ? gFine[idx0] : fconst0;
        v2f cw[R][VEC];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) cw[r][u] = ch[r][u];
        if (UNI || (!perWindowSel && !anyMoving))
        {
            if (a.chirpSelAll != LORAHIP_CHIRP_NONE)
            {
                dechirpMany<R * VEC>(&x[0][0], &cw[0][0], fconst);
            }
        }
        else
        {
            const float sgn = (perWindowSel && sel == LORAHIP_CHIRP_UP) ? -1.0f : 1.0f;
            const v2f *cwf = &cw[0][0];
            const v2f sgn2 = MAKE2(1.0f, sgn);                       // one packed multiply: (re, +-im), both exact
            const auto chirpOf = [&](const int i) { return cwf[i] * sgn2; };
            if (anyMoving)
            {
                // yv = idx0 in the windows that do not move; a launch-uniform selection is already in the values (s0): no sign multiply
                const auto chirpRaw = [&](const int i) { return cwf[i]; };
                if (perWindowSel) dechirpFine<fineSplitLog2H(LOG2N), R * VEC>(&x[0][0], chirpOf, &yv[0][0], fl, gFine, dechirp);
                else dechirpFine<fineSplitLog2H(LOG2N), R * VEC>(&x[0][0], chirpRaw, &yv[0][0], fl, gFine, dechirp);
            }
            else
            {
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                    {
                        const v2f y = cmulv(cmulv(x[r][u], chirpOf(r * VEC + u)), fconst);
                        x[r][u] = dechirp ? y : x[r][u];
                    }
            }
            if (usedChain) __syncthreads();               // sIdx is about to be overwritten by exchange 0
        }
        if (DBG && a.decOut && active)
        {
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int u = 0; u < VEC; u++) gDec[(size_t)w * N + VEC * t + u + VEC * T * r] = x[r][u];
        }

        // ---- phase 0: bits [0, B1) in registers, one group per u -----------------------------
        v2f v0[VEC][R];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) v0[u][Plan<LOG2N>::pos(VEC * T * r) & (R - 1)] = x[r][u];
        // next set's samples go in flight now (past the end: re-read the last set, harmless and branch-free)
        if (C::PREFETCH) issueLoads(set + gridDim.x < nSets ? set + gridDim.x : nSets - 1);
#pragma unroll
        for (int u = 0; u < VEC; u++) runPhase<LOG2N, 0, B1, false, DBG>(v0[u], 0, sTw, nullptr);

        // ---- exchange 0 ----------------------------------------------------------------------
#pragma unroll
        for (int u = 0; u < VEC; u++)
        {
            v2f *row = X + C::x0off(VEC * t + u);
#pragma unroll
            for (int e = 0; e < R; e++) row[e] = v0[u][e];
        }
        __syncthreads();                                                                      // B1
        recordPrev();                                   // previous set: its neighbours are visible now

        // phase 1 (middle): bits [B1, B2); klow = t mod R, high = t / R
        v2f v1[16];
        {
            const int klow = t & (R - 1), high = t >> B1;
            const int rhigh = rev4(high, HB);
#pragma unroll
            for (int e = 0; e < 16; e++) v1[e] = X[C::x0off((rev4(e, 4) << HB) | rhigh) + klow];
        }
        if (!C::INPLACE)
        {
            __syncthreads();                                                                  // B2
            flushIfFull();                              // wave 0, once per 64 windows
        }
        runPhase<LOG2N, B1, B2, false>(v1, t & (R - 1), sTw, nullptr);
        v2f vl[16];
        if (C::INPLACE)
        {
            // write-back in place: only this lane touches these 16 words between B1 and B3
            const int klow = t & (R - 1), rhigh = rev4(t >> B1, HB);
#pragma unroll
            for (int e = 0; e < 16; e++) X[C::x0off((rev4(e, 4) << HB) | rhigh) + klow] = v1[e];
            __syncthreads();                                                                  // B3
            flushIfFull();
            // last phase: lane t holds positions t + T*e2; t = klow + R*e_mid, e2 = high
            const int rmid = rev4(t >> B1, 4) << HB;
#pragma unroll
            for (int e = 0; e < 16; e++) vl[e] = X[C::x0off(rmid | rev4(e, HB)) + klow];
        }
        else
        {
            // exchange 1: position klow + R*e + 16R*high, 8 elements of padding per `high`
            v2f *base = X + (t >> B1) * C::X1 + (t & (R - 1));
#pragma unroll
            for (int e = 0; e < 16; e++) base[e * R] = v1[e];
            __syncthreads();                                                                  // B3
            // phase 2 = last: lane t holds positions t + T*e
#pragma unroll
            for (int e = 0; e < 16; e++) vl[e] = X[e * C::X1 + t];
        }
        runPhase<LOG2N, B2, LOG2N, true>(vl, 0, nullptr, twR);

        // ---- scan (LoRaDetector.hpp:36-48): bin = t + T*e, ascending in e ----------------------
        if (DBG && a.fftOut && active)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) gFft[(size_t)w * N + t + (e << LOG2T)] = vl[e];
        }
        float bestV;
        double tot;
        const int bestE = laneScan<16, SCAN_CHAINS_WIDE>([&](const int e) { return vl[e]; }, bestV, tot);
        int bestI = t + (bestE << LOG2T);
        if (!(bestV > 0.0f)) bestI = 0;
        groupArgmax<64>(bestV, bestI);
        tot = groupSumF64<64>(tot);
        if (lane == 0) { sRed[wave].v = bestV; sRed[wave].i = bestI; sRed[wave].tot = tot; }
        __syncthreads();                                                                      // B4
        // every lane combines the window's wavefronts in the same order: identical results on all of them
        {
            const RedRec r0 = sRed[wsub * WPWIN];
            bestV = r0.v; bestI = r0.i; tot = r0.tot;
#pragma unroll
            for (int k = 1; k < WPWIN; k++)
            {
                const RedRec rk = sRed[wsub * WPWIN + k];
                argmaxCombine(bestV, bestI, rk.v, rk.i);
                tot += rk.tot;
            }
        }
        Core::postNeighbours(vl, sNb + wsub * 2, bestI, t);      // read by recordPrev() behind the NEXT set's first barrier
        havePrev = true; pActive = active; pW = w; pI = bestI; pV = bestV; pTot = tot;
    }

    // ---- drain: last set's record, then whatever is queued --------------------------------------
    __syncthreads();
    recordPrev();
    __syncthreads();
    if (wave == 0)
    {
        const unsigned ww = tr.w[lane];
        if (ww < a.nWindows) detectTail(a, ww, tr.idx[lane], tr.val[lane], tr.tot[lane], tr.l[lane], tr.r[lane]);
    }
}

/***********************************************************************
 * launch
 **********************************************************************/
template <class C, bool DBG, bool UNI>
static hipError_t launchOneWide(const DetectArgs &a, const FastTables &ft, hipStream_t stream)
{
    const size_t smem = WideSmem<C>::bytes(!UNI);
    static unsigned long long attrDone = 0;
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(detectWide<C, DBG, UNI>), smem, attrDone);
        if (e != hipSuccess) return e;
    }
    const unsigned nSets = (a.nWindows + C::WPB - 1) / C::WPB;
    // persistent: as many workgroups as stay resident, never more than there are sets of work
    unsigned perCu = unsigned((160u * 1024u) / smem);
    if (perCu > unsigned(C::BPC)) perCu = unsigned(C::BPC);
    if (perCu < 1) perCu = 1;
    unsigned grid = unsigned(ft.nBlocksHint > 0 ? ft.nBlocksHint : 256) * perCu;
    if (grid > nSets) grid = nSets;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL((detectWide<C, DBG, UNI>), dim3(grid), dim3(C::BLOCK), smem, stream, a, ft, nSets);
    return hipGetLastError();
}

bool wideAvailable(const int sf) { return sf == 11 || sf == 12; }

bool wideLayoutsOk();

/***********************************************************************
 * selectable variants (lorahip_set_variant): 0 = the measured best per SF (profiles/r01/s8_variants.txt)
 **********************************************************************/
typedef hipError_t (*WideLaunch)(const DetectArgs &, const FastTables &, hipStream_t);
struct WideVariant { int sf, variant; WideLaunch launch; bool (*layoutOk)(); };
// ships: the default (0) and one alternative per SF (10: the plain exchange-0 layout, four barriers per window, register
// prefetch); every other number runs the default (launchWide below).
// Retired option sets (the parent of the commit that removed them has the code and their old numbers): the rest of the round-1 A/B
// set, with four waves per SIMD and the chirp values / last-phase twiddles read from LDS among its losers
// (profiles/r01/s8_variants.txt); the round-2 sets at two waves per SIMD (profiles/r02/s3_explore_moving_variants.txt); and round 4's
// two-waves-per-SIMD kernels with the chirp values from an LDS copy (profiles/r04).

//! defaults by call shape, like lorahip_fast.hip's: per-window settings (moving fine-tune index) at two waves per SIMD
template <class UNI_CFG, class MOVING_CFG>
static hipError_t launchWideByShape(const DetectArgs &a, const FastTables &ft, hipStream_t stream)
{
    // the debug ports (dec / fft outputs, 3x the traffic: not occupancy-bound) at the two-waves-per-SIMD register budget too: at three
    // they kept 408-508 B of scratch (tools/kernel_resources.py, profiles/r04)
    if (a.decOut || a.fftOut) return launchOneWide<MOVING_CFG, true, false>(a, ft, stream);
    const bool uni = a.chirpSel == nullptr && a.fineErr == nullptr;
    return uni ? launchOneWide<UNI_CFG, false, true>(a, ft, stream) : launchOneWide<MOVING_CFG, false, false>(a, ft, stream);
}
static bool defaultLayoutsOk()
{
    return layoutOk<Wide<11, WPF_NONE | WNT | WONE | WINPLACE>>() && layoutOk<Wide<11, WW2 | WNT | WONE | WINPLACE>>() &&
           layoutOk<Wide<12, WNT | WINPLACE>>() && layoutOk<Wide<12, WW2 | WNT | WINPLACE>>();
}
static const WideVariant kWideVariants[] = {
    { 11, 0, &launchWideByShape<Wide<11, WPF_NONE | WNT | WONE | WINPLACE>, Wide<11, WW2 | WNT | WONE | WINPLACE>>, &defaultLayoutsOk },   // default
#ifndef LORAHIP_FMA      // (the contracted build carries the defaults only)
    { 11, 10, &launchWideByShape<Wide<11, 0>, Wide<11, WW2>>, &layoutOk<Wide<11, 0>> },
#endif
    { 12, 0, &launchWideByShape<Wide<12, WNT | WINPLACE>, Wide<12, WW2 | WNT | WINPLACE>>, &defaultLayoutsOk },                            // default
#ifndef LORAHIP_FMA
    { 12, 10, &launchWideByShape<Wide<12, 0>, Wide<12, WW2>>, &layoutOk<Wide<12, 0>> },
#endif
};

bool wideLayoutsOk()
{
    for (const WideVariant &v : kWideVariants) if (!v.layoutOk()) return false;
    return layoutOk<StreamWide11>() && layoutOk<StreamWide12>();
}

hipError_t launchWide(const int sf, const int variant, const DetectArgs &a, const FastTables &ft, hipStream_t stream)
{
    const WideVariant *def = nullptr;
    for (const WideVariant &v : kWideVariants)
    {
        if (v.sf != sf) continue;
        if (v.variant == variant) return v.launch(a, ft, stream);
        if (v.variant == 0) def = &v;
    }
    return def ? def->launch(a, ft, stream) : hipErrorInvalidValue;     // unknown numbers run the default
}

} // namespace lorahip
