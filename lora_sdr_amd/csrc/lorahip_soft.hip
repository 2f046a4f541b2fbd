// Soft symbols (lorahip_soft_symbols, include/lorahip.h): per symbol window of a packet, one max-log LLR for each bit the decoder reads
// from the symbol -- a second pass over packets the demodulator has already found.
//
// A RUN is a packet's consecutive data-symbol windows. The fine-tune index (LoRaDemod.cpp:160-162) is carried from window to window, so
// a run is walked in order by the lanes that own it: a window's lane group inside a wavefront at SF6-SF10 (64 / T runs per wavefront,
// softFast on FastCore), a workgroup at SF11 / SF12 (softWide on WideCore). Load, dechirp, index chain and FFT are the window cores';
// the bins are the batch kernels' debug-port bins bit for bit (phase 0 multiplies by twiddle(0) as kissfft does). Only the bin scan is
// new: beside the arg-max, 2 * ppm maxima of |X|^2 over the bins whose Gray-coded, rounded symbol value has bit m set / clear.
// |X|^2 is never negative, so the maxima start from 0, order like their bit patterns, and cross the lanes as unsigned maxima.
#include "lorahip_fastcore.h"
#include "lorahip_widecore.h"

namespace lorahip {

namespace {

//! the lane's part of the soft scan over CNT bins, bin(j) the complex bin and binIndex(j) its number, ascending in j: the first
//! strict maximum (LoRaDetector.hpp:36-48) and, for each of the SF bits of g(k), the largest |X|^2 with the bit set (hi) / clear (lo)
template <int SF, int CNT, class BIN, class INDEX>
__device__ __forceinline__ void softLaneScan(BIN bin, INDEX binIndex, const int shift, const int half, float &bestV, int &bestI,
                                             float (&hi)[SF], float (&lo)[SF])
{
#pragma unroll
    for (int m = 0; m < SF; m++) { hi[m] = 0.0f; lo[m] = 0.0f; }
    bestV = 0.0f;
    bestI = 0;
#pragma unroll
    for (int j = 0; j < CNT; j++)
    {
        const auto b = bin(j);
        const float mag2 = b.x * b.x + b.y * b.y;
        const int k = binIndex(j);
        if (mag2 > bestV) { bestV = mag2; bestI = k; }
        const unsigned v = (unsigned)((k + half) >> shift) & 0xffffu;           // LoRaDecoder.cpp:218-222
        const unsigned g = v ^ (v >> 1);
#pragma unroll
        for (int m = 0; m < SF; m++)
        {
            const bool one = (g >> m) & 1u;
            const float h = mag2 > hi[m] ? mag2 : hi[m], l = mag2 > lo[m] ? mag2 : lo[m];
            hi[m] = one ? h : hi[m];
            lo[m] = one ? lo[m] : l;
        }
    }
    if (!(bestV > 0.0f)) bestI = 0;
}

//! maximum of a non-negative float over the aligned group of T lanes, in every lane
template <int T>
__device__ __forceinline__ float groupMaxPos(const float v) { return __uint_as_float(groupReduceU<T, true>(__float_as_uint(v))); }

} // namespace

/***********************************************************************
 * SF6-SF10: a run per lane group of a wavefront
 **********************************************************************/
// lorahip_fast.hip's geometry per SF (lanes per window, vector width, phases, exchange-0 layout), every table read from LDS, the
// register budget of two waves per SIMD: the option set of that file's debug-port instances of variant 10 (the prefetch option is
// the batch kernel's own; softFast loads a window ahead by itself)
//                                            LOG2T VEC NPH PB1 PB2 PB3 WPS  X0: ROT PAD S  D  X1PAD  chirp  twiddles prefetch
typedef FastCfg<6, 2, 4, 2, 2, 6, 0, 2, 2, 1, 0, 0, 8, true, true, false> SoftFast6;
typedef FastCfg<7, 3, 2, 2, 3, 7, 0, 2, 1, 1, 0, 0, 8, true, true, false> SoftFast7;
typedef FastCfg<8, 4, 1, 2, 4, 8, 0, 2, 0, 1, 0, 0, 8, true, true, false> SoftFast8;
typedef FastCfg<9, 5, 2, 3, 3, 7, 0, 2, 2, 1, 1, 8, 8, true, true, false> SoftFast9;
typedef FastCfg<10, 6, 1, 3, 4, 8, 0, 2, 0, 1, 0, 0, 8, true, true, false> SoftFast10;

template <class C>
__global__ void __launch_bounds__(256, 2)
softFast(const SoftArgs a, const FastTables ft)
{
    typedef FastCore<C> K;
    constexpr int N = C::N, T = C::T, VEC = C::VEC, R = C::R, WPW = C::WPW, LOG2T = C::LOG2T, LOG2N = C::LOG2N;
    constexpr int NGL = C::NGL, GL = C::GL, BL = C::BL, XW = C::XW;
    const int waves = blockDim.x >> 6;                     // 1 or 4 wavefronts (launchSoftFast)

    extern __shared__ __attribute__((aligned(16))) char smemRaw[];
    v2f *sTw = reinterpret_cast<v2f *>(smemRaw);                                   // [TWN]
    v2f *sCh = sTw + C::TWN;                                                       // [N]
    v2f *sX = sCh + C::CH_ELEMS;                                                   // [waves][XW]
    double2 *sFine = reinterpret_cast<double2 *>(sX + ((waves * XW + 1) & ~1));    // split fine-tune tables (read with ds_read_b128)
    static_assert(((C::TWN + C::CH_ELEMS) & 1) == 0, "the split tables are read with ds_read_b128");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wsub = lane >> LOG2T;
    const int t = lane & (T - 1);
    v2f *X = sX + wave * XW;

    const v2f *gIq = reinterpret_cast<const v2f *>(a.iq), *gDown = reinterpret_cast<const v2f *>(a.down);
    const v2f *gFine = reinterpret_cast<const v2f *>(a.fine);

    for (int i = threadIdx.x; i < C::TW_LDS; i += blockDim.x) sTw[i] = reinterpret_cast<const v2f *>(ft.twStage)[i];
    for (int i = threadIdx.x; i < N; i += blockDim.x)
    {
        const v2f c = gDown[i];
        sCh[i] = MAKE2(c.x, -c.y);                        // _upChirpTable = conj(_downChirpTable) (LoRaDemod.cpp:103-104)
    }
    typename K::TwR twR;
    K::loadTwR(twR, reinterpret_cast<const v2f *>(ft.twStage), t);
    typename K::TwM twM;
    K::loadTwM(twM, reinterpret_cast<const v2f *>(ft.twStage), t);
    const FineLds fl = fineLoadLds<LOG2N>(sFine, a.fineA, a.fineB, threadIdx.x, blockDim.x);
    __syncthreads();

    // this lane group's run
    const unsigned p = (blockIdx.x * waves + wave) * WPW + wsub;
    const bool have = p < a.nRuns;
    int n = have ? a.nsyms[p] : 0;
    n = n < a.symStride ? n : a.symStride;
    n = n > 0 ? n : 0;
    const long long first = have && n > 0 ? a.first[p] : 0;
    int idx = (have && a.fineIdx0 ? a.fineIdx0[p] : 0) & (K::M - 1);       // (an index outside the table: masked, the row is unspecified)
    const float err = have && a.fineErr ? a.fineErr[p] : 0.0f;
    const float d = err * (float)LORAHIP_FINE_STEPS;
    const int nMax = (int)__builtin_amdgcn_readfirstlane(groupReduceU<64, true>((unsigned)n));
    const int shift = LOG2N - a.ppm, half = (1 << shift) / 2;
    float *llrRow = a.llr + (size_t)(have ? p : 0) * a.symStride * a.ppm;
    unsigned short *symRow = a.sym ? a.sym + (size_t)(have ? p : 0) * a.symStride : nullptr;

    // a window's samples are loaded while the window before it is transformed (a finished group walks on with zero samples)
    v2f xn[R][VEC];
    auto issueLoads = [&](const int s_)
    {
        if (s_ < n) K::load(xn, gIq + first + (long long)s_ * N, t);
        else
        {
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int u = 0; u < VEC; u++) xn[r][u] = MAKE2(0.0f, 0.0f);
        }
    };
    issueLoads(0);

    for (int s = 0; s < nMax; s++)
    {
        const bool active = s < n;                        // (a finished group's results are dropped)
        const bool moving = active && d != 0.0f;
        const bool anyMoving = __any(moving);

        v2f x[R][VEC];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int u = 0; u < VEC; u++) x[r][u] = xn[r][u];

        // ---- dechirp (LoRaDemod.cpp:159): (samp * chirp) * fine, the index moving inside the window where the run has an error ----
        v2f cw[R][VEC];
        K::chirpFromLds(cw, sCh, t);
        if (anyMoving)
        {
            // as lorahip_fast.hip: the closed form (lorahip_fine.h), or the exact chain for the whole wavefront where it does not apply
            int *sIdx = reinterpret_cast<int *>(X) + wsub * N;   // aliases the exchange region (free until phase 0 ends)
            unsigned yv[R][VEC];
            const FinePlan pl = finePlan(moving ? d : 0.0f, K::M);
            const unsigned ymax = fineLaneIndices<LOG2N, VEC, T, R>(idx, pl, t, yv);
            int idxEnd = fineEndIndex(idx, pl, LOG2N, LOG2N + 7);
            if (__any(!pl.regular || ymax == (unsigned)K::M))
            {
                idxEnd = K::fineChain(idx, moving ? d : 0.0f, t, sIdx);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int u = 0; u < VEC; u++) yv[r][u] = (unsigned)sIdx[K::idxSlot(VEC * t + u + VEC * T * r)];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            const v2f *cwf = &cw[0][0];
            dechirpFine<fineSplitLog2H(LOG2N), R * VEC>(&x[0][0], [&](const int i) { return cwf[i]; }, &yv[0][0], fl, gFine, true);
            if (moving) idx = idxEnd;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        else dechirpMany<R * VEC>(&x[0][0], &cw[0][0], gFine[idx]);

        // ---- FFT: the debug-port bins (UNITMUL) ----
        v2f vl[NGL][GL];
        K::template fft<true>(x, X, wsub, t, sTw, twR, vl, [&]() { issueLoads(s + 1); }, &twM);

        // ---- soft scan: element j = e*NGL + g of the lane is bin (t + T g) + (e << BL), ascending in j ----
        float bestV, hi[LOG2N], lo[LOG2N];
        int bestI;
        softLaneScan<LOG2N, GL * NGL>([&](const int j) { return vl[j % NGL][j / NGL]; },
                                      [&](const int j) { return (t + T * (j % NGL)) + ((j / NGL) << BL); }, shift, half, bestV, bestI, hi, lo);
        groupArgmax<T>(bestV, bestI);
#pragma unroll
        for (int m = 0; m < LOG2N; m++) { hi[m] = groupMaxPos<T>(hi[m]); lo[m] = groupMaxPos<T>(lo[m]); }
        if (active && t == 0)
        {
            float *o = llrRow + (size_t)s * a.ppm;
#pragma unroll
            for (int m = 0; m < LOG2N; m++) if (m < a.ppm) o[m] = hi[m] - lo[m];
            if (symRow) symRow[s] = (unsigned short)bestI;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <class C>
static SoftTiling planSoftFast(const unsigned nRuns, const int cuCount)
{
    // four wavefronts share a workgroup's tables; fewer runs than keep two such workgroups on every CU go one wavefront per workgroup,
    // so that a short list of long runs still spreads over the device (a run is walked by ONE lane group, window after window)
    const unsigned cus = unsigned(cuCount > 0 ? cuCount : 256);
    const int waves = (nRuns + 4 * C::WPW - 1) / (4 * C::WPW) < 2 * cus ? 1 : 4;
    const unsigned perBlock = unsigned(waves * C::WPW);
    return { C::WPW, waves, (nRuns + perBlock - 1) / perBlock };
}

template <class C>
static hipError_t launchSoftFast(const SoftArgs &a, const FastTables &ft, hipStream_t stream)
{
    const auto smemOf = [](const int waves) { return size_t(C::TWN + C::CH_ELEMS) * sizeof(float2) + size_t((waves * C::XW + 1) & ~1) * sizeof(float2) + FineDims<C::LOG2N>::BYTES; };
    static unsigned long long attrDone = 0;
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(softFast<C>), smemOf(4), attrDone);
        if (e != hipSuccess) return e;
    }
    const SoftTiling tl = planSoftFast<C>(a.nRuns, ft.nBlocksHint);
    hipLaunchKernelGGL((softFast<C>), dim3(tl.blocks), dim3(tl.waves * 64), smemOf(tl.waves), stream, a, ft);
    return hipGetLastError();
}

/***********************************************************************
 * SF11 / SF12: a run per workgroup (the streaming kernel's geometry: one window per workgroup, in-place middle phase)
 **********************************************************************/
template <class C>
__global__ void __launch_bounds__(C::BLOCK, C::MINW)
softWide(const SoftArgs a, const FastTables ft)
{
    typedef WideCore<C> Core;
    typedef typename WideSmem<C>::Stream Lds;
    constexpr int N = C::N, T = C::T, VEC = C::VEC, R = C::R, LOG2N = C::LOG2N, LOG2T = C::LOG2T, M = Core::M, WPWIN = C::WPWIN;
    constexpr int B2 = C::B2;
    static_assert(C::WPB == 1, "one run per workgroup");

    extern __shared__ __attribute__((aligned(16))) char smemRaw[];
    Lds &L = *reinterpret_cast<Lds *>(smemRaw);
    double2 *sFine = reinterpret_cast<double2 *>(smemRaw + sizeof(Lds));
    float *sSoft = reinterpret_cast<float *>(smemRaw + sizeof(Lds) + FineDims<LOG2N>::BYTES);    // [WPWIN][2 * LOG2N]

    const int tid = threadIdx.x, t = tid, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const v2f *gIq = reinterpret_cast<const v2f *>(a.iq), *gDown = reinterpret_cast<const v2f *>(a.down);
    const v2f *gFine = reinterpret_cast<const v2f *>(a.fine);

    for (int i = tid; i < C::TW_LDS; i += C::BLOCK) L.tw[i] = reinterpret_cast<const v2f *>(ft.twStage)[i];
    typename Core::TwR twR;                              // register twiddles of the last phase (klow = t there)
    {
        int slot = 0;
#pragma unroll
        for (int b = B2; b < LOG2N; b += 2)
#pragma unroll
            for (int kl = 0; kl < (1 << (b - B2)); kl++)
            {
                const int base = twStageOffset(LOG2N, b) + t + (kl << B2);
                twR[slot] = reinterpret_cast<const v2f *>(ft.twStage)[base];
                twR[slot + 1] = reinterpret_cast<const v2f *>(ft.twStage)[base + (1 << b)];
                twR[slot + 2] = reinterpret_cast<const v2f *>(ft.twStage)[base + (2 << b)];
                slot += 3;
            }
    }
    const FineLds fl = fineLoadLds<LOG2N>(sFine, a.fineA, a.fineB, tid, C::BLOCK);
    v2f ch[R][VEC];
    Core::loadChirp(ch, gDown, t, -1.0f);
    __syncthreads();

    const unsigned p = blockIdx.x;                        // (the grid is the run count)
    int n = a.nsyms[p];
    n = n < a.symStride ? n : a.symStride;
    const long long first = n > 0 ? a.first[p] : 0;
    int idx = (a.fineIdx0 ? a.fineIdx0[p] : 0) & (M - 1);
    const float err = a.fineErr ? a.fineErr[p] : 0.0f;
    const float d = err * (float)LORAHIP_FINE_STEPS;
    const bool moving = d != 0.0f;                        // workgroup-uniform, like everything that steers a barrier below
    const int shift = LOG2N - a.ppm, half = (1 << shift) / 2;
    float *llrRow = a.llr + (size_t)p * a.symStride * a.ppm;
    unsigned short *symRow = a.sym ? a.sym + (size_t)p * a.symStride : nullptr;

    for (int s = 0; s < n; s++)
    {
        v2f x[R][VEC];
        Core::load(x, gIq + first + (long long)s * N, t);
        if (moving)
        {
            // as lorahip_wide.hip's one-window workgroups: the closed form, or the exact chain where it does not apply
            int *sIdx = reinterpret_cast<int *>(L.x);       // aliases the exchange region (free until phase 0 ends)
            unsigned yv[R][VEC];
            const FinePlan pl = finePlan(d, M);
            const unsigned ymax = fineLaneIndices<LOG2N, VEC, T, R>(idx, pl, t, yv);
            int idxEnd = fineEndIndex(idx, pl, LOG2N, LOG2N + 7);
            bool usedChain;
            if (pl.mod == (unsigned)M || pl.sat) usedChain = !pl.regular;
            else usedChain = __syncthreads_or(!pl.regular || ymax == (unsigned)M);
            if (usedChain)
            {
                idxEnd = fineChainBlock<T, M>(idx, d, t, t >> 6, sIdx, L.chain);
                Core::chainIndices(yv, sIdx, t);
            }
            const v2f *cwf = &ch[0][0];
            dechirpFine<fineSplitLog2H(LOG2N), R * VEC>(&x[0][0], [&](const int i) { return cwf[i]; }, &yv[0][0], fl, gFine, true);
            idx = idxEnd;
            if (usedChain) __syncthreads();               // sIdx is about to be overwritten by exchange 0
        }
        else dechirpMany<R * VEC>(&x[0][0], &ch[0][0], gFine[idx]);

        v2f vl[16];
        Core::fft(x, L.x, t, L.tw, twR, vl, true);        // the debug-port bins (phase 0 as kissfft)

        // ---- soft scan: bin = t + T*e, ascending in e; the wavefronts' maxima and arg-maxima meet in LDS behind one barrier ----
        float bestV, hi[LOG2N], lo[LOG2N];
        int bestI;
        softLaneScan<LOG2N, 16>([&](const int e) { return vl[e]; }, [&](const int e) { return t + (e << LOG2T); }, shift, half, bestV, bestI, hi, lo);
#pragma unroll
        for (int m = 0; m < LOG2N; m++)
        {
            hi[m] = groupMaxPos<64>(hi[m]);
            lo[m] = groupMaxPos<64>(lo[m]);
            if (lane == 0) { sSoft[wave * 2 * LOG2N + 2 * m] = hi[m]; sSoft[wave * 2 * LOG2N + 2 * m + 1] = lo[m]; }
        }
        groupArgmax<64>(bestV, bestI);
        if (lane == 0) { L.red[wave].v = bestV; L.red[wave].i = bestI; }
        __syncthreads();
        if (t == 0 && symRow)
        {
#pragma unroll
            for (int k = 1; k < WPWIN; k++) argmaxCombine(bestV, bestI, L.red[k].v, L.red[k].i);
            symRow[s] = (unsigned short)bestI;
        }
        if (t < a.ppm)
        {
            float h = sSoft[2 * t], l = sSoft[2 * t + 1];
#pragma unroll
            for (int k = 1; k < WPWIN; k++)
            {
                const float hk = sSoft[k * 2 * LOG2N + 2 * t], lk = sSoft[k * 2 * LOG2N + 2 * t + 1];
                h = hk > h ? hk : h;
                l = lk > l ? lk : l;
            }
            llrRow[(size_t)s * a.ppm + t] = h - l;
        }
        // (the next window's first write to sSoft / L.red lies behind the barriers of its FFT)
    }
}

template <class C>
static SoftTiling planSoftWide(const unsigned nRuns)
{
    static_assert(C::BLOCK == C::WPWIN * 64, "the workgroup is the window's wavefronts");
    return { 0, C::WPWIN, nRuns };                        // (the grid is the run count)
}

template <class C>
static hipError_t launchSoftWide(const SoftArgs &a, const FastTables &ft, hipStream_t stream)
{
    const size_t smem = sizeof(typename WideSmem<C>::Stream) + FineDims<C::LOG2N>::BYTES + size_t(C::WPWIN) * 2 * C::LOG2N * sizeof(float);
    static unsigned long long attrDone = 0;
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(softWide<C>), smem, attrDone);
        if (e != hipSuccess) return e;
    }
    const SoftTiling tl = planSoftWide<C>(a.nRuns);
    hipLaunchKernelGGL((softWide<C>), dim3(tl.blocks), dim3(tl.waves * 64), smem, stream, a, ft);
    return hipGetLastError();
}

bool softPlan(const int sf, const unsigned nRuns, const int cuCount, SoftTiling &tl)
{
    switch (sf)
    {
    case 6: tl = planSoftFast<SoftFast6>(nRuns, cuCount); return true;
    case 7: tl = planSoftFast<SoftFast7>(nRuns, cuCount); return true;
    case 8: tl = planSoftFast<SoftFast8>(nRuns, cuCount); return true;
    case 9: tl = planSoftFast<SoftFast9>(nRuns, cuCount); return true;
    case 10: tl = planSoftFast<SoftFast10>(nRuns, cuCount); return true;
    case 11: tl = planSoftWide<StreamWide11>(nRuns); return true;
    case 12: tl = planSoftWide<StreamWide12>(nRuns); return true;
    default: return false;
    }
}

hipError_t launchSoftSymbols(const int sf, const SoftArgs &a, const FastTables &ft, hipStream_t stream)
{
    if (a.nRuns == 0) return hipSuccess;
    switch (sf)
    {
    case 6: return launchSoftFast<SoftFast6>(a, ft, stream);
    case 7: return launchSoftFast<SoftFast7>(a, ft, stream);
    case 8: return launchSoftFast<SoftFast8>(a, ft, stream);
    case 9: return launchSoftFast<SoftFast9>(a, ft, stream);
    case 10: return launchSoftFast<SoftFast10>(a, ft, stream);
    case 11: return launchSoftWide<StreamWide11>(a, ft, stream);
    case 12: return launchSoftWide<StreamWide12>(a, ft, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace lorahip
