// Streaming demodulator for the long windows (SF11, SF12): a workgroup OWNS a channel (T = 128 / 256 lanes) and walks its stream
// window after window -- the level-3 twin of lorahip_stream.hip, same frame machine (lorahip_framemachine.h), the window code of
// lorahip_widecore.h with the in-place middle phase, as in detectWide (lorahip_wide.hip). Five workgroup barriers per window (two
// more while the fine-tune index moves).
#include "lorahip_widecore.h"
#include "lorahip_framemachine.h"
#include "lorahip_residentproto.h"

namespace lorahip {

#ifdef LORAHIP_WG_TIMELINE     // profiling build (tools/wg_timeline.py): when and where every workgroup of the last streaming launch ran
__device__ unsigned long long gWgTimeline[16384][4];
__device__ unsigned gWgWaveHwId[16384][4];
extern "C" int lorahip_debug_wg_timeline(void *out, const size_t bytes)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gWgTimeline), bytes < sizeof(gWgTimeline) ? bytes : sizeof(gWgTimeline)) == hipSuccess ? 0 : -1;
}
extern "C" int lorahip_debug_wg_waves(void *out, const size_t bytes)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gWgWaveHwId), bytes < sizeof(gWgWaveHwId) ? bytes : sizeof(gWgWaveHwId)) == hipSuccess ? 0 : -1;
}
#endif

//! the channel of a demodStreamWide workgroup as residentPackOwn sees it: one channel, packed by the 64 lanes of wavefront 0
struct ResPackWide { static constexpr int WPW = 1, T = 64, LOG2T = 6; };

//! RES: the resident receiver (see demodStream in lorahip_streamkernel.h, lorahip_residentproto.h): the launch stays, the steps arrive as
//! messages; a workgroup moves through a step as ONE (its wavefronts share a window), wavefront 0 waits for the message, packs the
//! channel's packets and signals, and reports
template <class C, bool PERSIST, bool RES = false>
__global__ void __launch_bounds__(C::T, 2)
demodStreamWide(const StreamArgs s)
{
    static_assert(!(RES && PERSIST), "the resident receiver walks its channels itself");
#ifdef LORAHIP_WG_TIMELINE
    const unsigned long long tl0 = wall_clock64();
#endif
    static_assert(C::INPLACE && C::WPB == 1, "stream configs: one channel per workgroup, in-place middle phase");
    typedef WideCore<C> Core;
    constexpr int N = C::N, T = C::T, VEC = C::VEC, R = C::R, WPWIN = C::WPWIN, LOG2N = C::LOG2N, M = Core::M;

    extern __shared__ __attribute__((aligned(16))) char smemRaw[];
    typename WideSmem<C>::Stream &sm = *reinterpret_cast<typename WideSmem<C>::Stream *>(smemRaw);
    v2f *sTw = sm.tw, *X = sm.x, *sNb = sm.nb;
    RedRec *sRed = sm.red;
    int *sChain = sm.chain;
    double2 *sFine = reinterpret_cast<double2 *>(&sm + 1);               // split fine-tune tables (lorahip_fine.h)

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const v2f *gIq = reinterpret_cast<const v2f *>(s.iq), *gFine = reinterpret_cast<const v2f *>(s.fine);
    for (int i = t; i < C::TW_LDS; i += T) sTw[i] = reinterpret_cast<const v2f *>(s.twStage)[i];
    // register twiddles of the last phase (klow = t there). (No WideCore member, as detectWide's are none: through a call the persistent
    // SF11 instance took one more VGPR and 24 B more scratch, profiles/r14/README.md)
    typename Core::TwR twR;
    {
        constexpr int B2 = C::B2;
        int slot = 0;
#pragma unroll
        for (int b = B2; b < LOG2N; b += 2)
#pragma unroll
            for (int kl = 0; kl < (1 << (b - B2)); kl++)
            {
                const int base = twStageOffset(LOG2N, b) + t + (kl << B2);
                twR[slot] = reinterpret_cast<const v2f *>(s.twStage)[base];
                twR[slot + 1] = reinterpret_cast<const v2f *>(s.twStage)[base + (1 << b)];
                twR[slot + 2] = reinterpret_cast<const v2f *>(s.twStage)[base + (2 << b)];
                slot += 3;
            }
    }
    v2f ch[R][VEC];                                        // down-chirp values of this lane's sample positions
    Core::loadChirp(ch, reinterpret_cast<const v2f *>(s.down), t, 1.0f);
    const FineLds fl = fineLoadLds<LOG2N>(sFine, s.fineA, s.fineB, t, T);
    ResLds *sR = reinterpret_cast<ResLds *>(smemRaw + WideSmem<C>::streamBytes());       // RES only (the launcher adds the bytes)
    if constexpr (RES)
    {
        if (t == 0) { sR->carry = s.carry; sR->carryCap = s.carryCap; }
        if (t < RES_RING) { sR->calls[t] = 0; sR->arrive[t] = 0; sR->more[t] = 0; sR->msgSeq[t] = 0u; }
        // the census: the host rings the first step only when every workgroup is on the device
        if (t == 0 && atomicAdd(&s.res->arrived, 1u) + 1u == gridDim.x) sysStore(&s.resHost->arrivedAll, 1u);
    }
    __syncthreads();

    // One channel per workgroup: everything the frame machine touches is WORKGROUP-UNIFORM. Saying so (v_readfirstlane where a value
    // comes out of the vector unit: the peak, the squelch decision, fIndex) lets the whole machine -- state, 64-bit positions, record
    // pointers and counters, the fine-tune plan -- live in scalar registers and run on the scalar unit instead of being replicated
    // in every lane's vector registers.
    const auto uniI = [](const int v) { return __builtin_amdgcn_readfirstlane(v); };
    const auto uniF = [](const float v) { return __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); };
    // persistent grid (s.maxBlocks workgroups at most), a workgroup takes one channel after the other: see demodStream
    // RES: one turn of the outer loop per receiver step (otherwise exactly one turn)
    unsigned step = 0;
    unsigned long long resNValid = 0;
    unsigned resCalls = 0;
    bool resMore = false;
    // (ONE loop over the workgroup's channels, step after step -- the wait for the next step's message sits at the end of the last channel's
    // turn, not in a loop around this one: the loop nest the compiler sees is the persistent instance's)
    const auto nextStep = [&]() -> bool
    {
        if (wave == 0)
        {
            ResMsgR m0;
            const bool ok = residentWait(s, step + 1u, m0, sR, true);
            if (lane == 0) sR->go = ok ? 1 : 0;
        }
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(sR->go)) return false;  // (the quit message, the abort flag or the watchdog: the whole workgroup leaves)
        // (of the message only n_valid stays in registers across the windows; every wavefront from LDS, wavefront 0 too: one path)
        resNValid = uni64(sR->msg[(step + 1u) & 3u].nValid);
        step++;
        resCalls = 0; resMore = false;
        return true;
    };
    if constexpr (RES) { if (!nextStep()) return; }
    unsigned c = blockIdx.x;                                // (the grid never exceeds the channel count)
    do
    {
    StreamState st;
    if constexpr (RES)
    {
        // (what this workgroup stored a step ago: read at agent scope -- past the L1 and the scalar cache, which may hold an older copy --
        // and made scalar again)
        const unsigned long long *q = reinterpret_cast<const unsigned long long *>(&s.state[c]);
        unsigned long long w[5];
#pragma unroll
        for (int i = 0; i < 5; i++) w[i] = uni64(agentLoad(q + i));
        static_assert(sizeof(StreamState) == 40, "five 64-bit words");
        __builtin_memcpy(&st, w, sizeof(st));
    }
    else st = s.state[c];
    if (s.flags & 1) { st.pos = 0; st.callCount = 0; }                        // a new run: every stream from its first sample
    if (s.flags & 2) { st.state = ST_FRAMESYNC; st.downTable = 0; }           // activate() (LoRaDemod.cpp:139-143)
    const long long base = s.uniformLen >= 0 ? (long long)c * s.uniformStride : s.base[c];
    const long long len = RES ? (long long)resNValid : (s.uniformLen >= 0 ? s.uniformLen : s.len[c]);         // (RES: what the step's message says)
    StreamOut o;
    o.init(s, c);
    if constexpr (RES)
    {
        // the record arrays of this step's set (StreamArgs::resRecStride)
        const size_t setOff = size_t(step & 3u) * size_t(s.resRecStride);
        o.symOut = reinterpret_cast<short *>(reinterpret_cast<char *>(o.symOut) + setOff);
        o.pktOut = reinterpret_cast<StreamPacket *>(reinterpret_cast<char *>(o.pktOut) + setOff);
        if (o.sigOut) o.sigOut = reinterpret_cast<StreamSignal *>(reinterpret_cast<char *>(o.sigOut) + setOff);
    }
    o.carryIn(s, st, c, t, T, !RES);

    // one window: LoRaDemod.cpp:157-166 + LoRaDetector::detect; every argument is workgroup-uniform
    // What a work() call consumes of the float outputs depends on its state (see demodStream, lorahip_stream.hip): without a
    // trace the squelch decision comes from a quick estimate (squelchQuick) with the exact chain as the fallback near the
    // threshold, fIndex is evaluated only for an unsquelched FRAMESYNC window, and the neighbour fetch with its barrier is skipped
    // whenever neither is needed
    // Signals without a trace (lorahip_demod_set_signals): the DOWNCHIRP1 call of a packet takes the traced path (`full`), see demodStream
    const bool traced = s.calls != nullptr;
    const bool sig = s.sigOut != nullptr;
    // (Requesting the window at off + N while this one is transformed measured 2-3 % slower, profiles/r04/s10_*: every call loads its own.)
    // unitTw: the pass repeats a window whose total came out non-finite, with phase 0's products by twiddle(0) carried out (see
    // demodStream, lorahip_streamkernel.h). Returns whether the window has to be repeated so (workgroup-uniform; nothing is valid then).
    v2f x[R][VEC];
    auto detect = [&](const bool all, const bool wantSq, const int wantFi, const long long off, const bool downTable, const int idx0, const float err, const bool unitTw,
                      int &value, float &power, float &powerAvg, float &fIndex, int &idxEnd, bool &squelched) -> bool
    {
        Core::load(x, gIq + off, t);                         // scalar base, per-lane offsets
        const float d = err * (float)LORAHIP_FINE_STEPS;
        const bool moving = d != 0.0f;                       // workgroup-uniform
        int *sIdx = reinterpret_cast<int *>(X);
        idxEnd = idx0;
        unsigned yv[R][VEC];
        bool usedChain = false;
        if (moving)
        {
            // closed-form indices of this lane's samples (lorahip_fine.h); the exact chain where the form does not apply
            FinePlan pl = finePlan(d, M);
            pl.q = (unsigned)uniI((int)pl.q); pl.mod = (unsigned)uniI((int)pl.mod); pl.regular = uniI(pl.regular); pl.sat = uniI(pl.sat);
            const unsigned ymax = fineLaneIndices<LOG2N, VEC, T, R>(idx0, pl, t, yv);
            idxEnd = uniI(fineEndIndex(idx0, pl, LOG2N, LOG2N + 7));
            // the closed form can only reach the value M under the modulus M + 1 (lorahip_fine.h): no vote, no barrier otherwise
            usedChain = !pl.regular || ((pl.mod != (unsigned)M && !pl.sat) && __syncthreads_or(ymax == (unsigned)M));
            if (!unitTw && t == 0 && nearStep(d)) atomicAdd(s.near + 1, 1u);         // counted (once), not changed (lorahip_internal.h)
            if (usedChain)
            {
                idxEnd = uniI(fineChainBlock<T, M>(idx0, d, t, t >> 6, sIdx, sChain));
                Core::chainIndices(yv, sIdx, t);
            }
        }
        // _upChirpTable = conj(entry) (LoRaDemod.cpp:103): the table selection is workgroup-uniform here, so the conjugation rides on
        // the multiply's sign modifiers (cmulConjv / the CONJ pipeline) instead of a packed multiply by (1, -1) per sample
        const v2f *chf = &ch[0][0];
        const auto chirpRaw = [&](const int i) { return chf[i]; };
        if (moving)
        {
            if (downTable) dechirpFine<fineSplitLog2H(LOG2N), R * VEC, false>(&x[0][0], chirpRaw, &yv[0][0], fl, gFine, true);
            else dechirpFine<fineSplitLog2H(LOG2N), R * VEC, true>(&x[0][0], chirpRaw, &yv[0][0], fl, gFine, true);
        }
        else
        {
            const v2f fconst = gFine[idx0];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    x[r][u] = cmulv(downTable ? cmulv(x[r][u], chf[r * VEC + u]) : cmulConjv(x[r][u], chf[r * VEC + u]), fconst);
        }
        if (usedChain) __syncthreads();                    // sIdx is about to be overwritten by exchange 0

        // phase 0 -> exchange 0 -> phase 1 in place -> last phase: lane t holds bins t + T*e
        v2f vl[16];
        Core::fft(x, X, t, sTw, twR, vl, unitTw);

        // scan (LoRaDetector.hpp:36-48). Without a trace the total only feeds the quick squelch estimate: fp32 then (laneScanQuick,
        // squelchQuickF); the fp64 total is summed where the exact chain is evaluated (below)
        float bestV;
        double tot;
        int bestI;
        Core::scanReduce(vl, sRed, t, lane, wave, bestV, bestI, tot, all);
        // workgroup-uniform from here on: every thread combined the same records in the same order
        bestI = uniI(bestI);
        bestV = uniF(bestV);
        tot = __hiloint2double(uniI(__double2hiint(tot)), uniI(__double2loint(tot)));
        if (!unitTw && (__double2hiint(tot) & 0x7ff00000) == 0x7ff00000) return true;      // Inf or NaN: some bin is
        value = bestI;
        bool needLogs = all, needFi = all;
        if (!all)
        {
            bool sure;
            squelched = squelchQuickF(bestV, (float)tot, s.thresh, float(16 + 6 + WPWIN + 2) * 0x1p-24f, sure);
            squelched = uniI(squelched) != 0;
            sure = uniI(sure) != 0;
            power = powerAvg = fIndex = 0.0f;                   // not consumed without a trace
            needLogs = wantSq && !sure;
            needFi = wantFi == 2 || (wantFi == 1 && (!sure || !squelched));   // 2: the second window of a FRAMESYNC call (:203, :217-221)
        }
        if (needLogs || needFi)
        {
            // neighbours of the peak (LoRaDetector.hpp:56-57)
            Core::postNeighbours(vl, sNb, bestI, t);
            __syncthreads();                                                                  // B5
            if (needLogs && !all)
            {
                // the exact chain wants LoRaDetector.hpp:36-48's double total, in the traced path's association (bins still in registers)
                float bv_;
                double te;
                (void)laneScan<16, SCAN_CHAINS_WIDE>([&](const int e) { return vl[e]; }, bv_, te);
                te = groupSumF64<64>(te);
                if (lane == 0) sRed[wave].tot = te;
                __syncthreads();
                tot = sRed[0].tot;
#pragma unroll
                for (int k = 1; k < WPWIN; k++) tot += sRed[k].tot;
                tot = __hiloint2double(uniI(__double2hiint(tot)), uniI(__double2loint(tot)));
            }
            if (needLogs)
            {
                tailValuesPaired(s.powerScale, bestV, tot, sNb[0], sNb[1], lane, power, powerAvg, fIndex);
                power = uniF(power); powerAvg = uniF(powerAvg); fIndex = uniF(fIndex);
                squelched = (power - powerAvg) < s.thresh;                                   // :173-174
                squelched = uniI(squelched) != 0;
                if (wantSq && t == 0 && nearSquelch(power - powerAvg, s.thresh)) atomicAdd(s.near, 1u);
                if (!all) power = powerAvg = 0.0f;
            }
            else fIndex = uniF(fIndexPaired(bestV, sNb[0], sNb[1], lane));
        }
        return false;
    };

    // A FRAMESYNC call that is sync'd and matches the first sync word looks at a SECOND window (LoRaDemod.cpp:183-206): it is taken
    // in the next pass of the loop (`pend`), so that the kernel holds ONE instance of the window code, not two -- nothing is written
    // and nothing is consumed in between, and the limits checked for the first pass cover the whole call (same scheme as demodStream).
    bool pend = false;
    bool unitTw = false;                                    // this pass repeats the last one's window (nothing was committed)
    int value0 = 0, fineIdxBefore0 = 0;
    float snr0 = 0.0f, fineErrBefore0 = 0.0f;
    const int slot = wavefrontSlot();
    const bool lastRound = PERSIST || RES || !LORAHIP_PRIO_HOLD || blockIdx.x >= s.lastRoundFrom;
    holdPriority<LORAHIP_PRIO_ALTERNATE>(!lastRound);
    while (pend || ((len - st.pos >= 2 * N) && o.calls < s.cap && o.nPkt < s.capPkt && o.nSig < s.capPkt))          // LoRaDemod.cpp:148
    {
        if (lastRound) rotatePriority<2, LORAHIP_PRIO_ALTERNATE>(slot);
        const bool second = pend;
        int value, idxEnd;
        float power, powerAvg, fIndex;
        const int fineIdxBefore = second ? fineIdxBefore0 : st.fineTuneIndex;
        const float fineErrBefore = second ? fineErrBefore0 : st.finefreqError;
        const bool fs = st.state == ST_FRAMESYNC;
        bool squelched;
        // window 0 of a call (:157-172), or window 1 of a parked one (:189-206: `int ft = _fineTuneIndex` starts from the committed
        // index and is not committed itself)
        unitTw = detect(traced || (sig && !second && st.state == ST_DOWNCHIRP1), !second && (fs || st.state == ST_DATASYMBOLS), second ? 2 : (fs ? 1 : 0), base + st.pos + (second ? N : 0), st.downTable != 0,
                        st.fineTuneIndex, st.finefreqError, unitTw, value, power, powerAvg, fIndex, idxEnd, squelched);
        if (unitTw) continue;
        float snr = power - powerAvg;                                                   // :173 (squelched = snr < thresh, :174, comes from detect)
        if (!second) st.fineTuneIndex = idxEnd;                                         // :160-162
        bool syncd = !squelched && (st.prevValue + 4) / 8 == 0;                        // :183
        bool match0 = (value + 4) / 8 == (s.sync >> 4);                                // :184
        bool match1 = false, step = true;
        if (second)
        {
            match1 = (value + 4) / 8 == (s.sync & 0xf);                                // :205
            // detect() overwrote power / powerAvg / fIndex (:203); value, snr and what follows from them are window 0's
            value = value0; snr = snr0; squelched = false; syncd = true; match0 = true;
            pend = false;
        }
        else if (fs && syncd && match0)
        {
            pend = true; step = false;
            value0 = value; snr0 = snr; fineIdxBefore0 = fineIdxBefore; fineErrBefore0 = fineErrBefore;
        }
        if (step)
        {
            frameStep<N>(st, s, o, t == 0, value, power, powerAvg, snr, fIndex, squelched, syncd, match0, match1, fineIdxBefore, fineErrBefore);
            st.finefreqError = uniF(st.finefreqError);                                  // a float add runs on the vector unit: back to a scalar
        }
    }
    // (RES: the channel's packets and signals of the step into the step's rows first -- wavefront 0 wrote the records, t == 0 is the writer
    // lane; a packet's first symbols may still be in the carry row carryOut is about to overwrite)
    if constexpr (RES) { if (wave == 0) residentPackOwn<ResPackWide>(s, sR, step, c, o, true, lane, st.state == ST_DATASYMBOLS ? st.symCount : 0); }
    o.carryOut(s, st, c, t, T, true, true);             // T > 64: a barrier between the writer's last store and the other wavefronts' loads
#ifdef LORAHIP_WG_TIMELINE
    if ((t & 63) == 0 && c < 16384) gWgWaveHwId[c][(t >> 6) & 3] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
#endif
    if (t == 0)
    {
        s.state[c] = st;
        s.nCalls[c] = o.calls;
        s.nSym[c] = o.nSym;
        s.nPkt[c] = o.nPkt;
        if (s.nSig) s.nSig[c] = o.nSig;
        s.end[c] = make_int2(st.state == ST_DATASYMBOLS ? st.symCount : -1, st.callCount);
#ifdef LORAHIP_WG_TIMELINE
        if (c < 16384)
        {
            gWgTimeline[c][0] = tl0; gWgTimeline[c][1] = wall_clock64();
            gWgTimeline[c][2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);   // HW_ID, XCC_ID
            gWgTimeline[c][3] = (unsigned long long)o.calls;
        }
#endif
    }
    if constexpr (RES)
    {
        resCalls += unsigned(o.calls);
        resMore = resMore || (len - st.pos >= 2 * N);       // stopped with samples left: a record buffer was full
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the state and the rows are in L2 / in memory before the workgroup moves on
    }
    if (PERSIST || RES) __syncthreads();                    // the next channel reuses the exchange region and the reduction records
    if constexpr (RES)
    {
        c += gridDim.x;
        if (c >= s.nChannels)
        {
            // the step's last channel: report, and on to the next step
            residentLookAhead(s, step + 1u);                // (the relay wavefronts: the next step's message into the mirrors)
            if (t == 0) residentWgDone(s, sR, step, resCalls, resMore ? 1u : 0u);
            if (!nextStep()) break;
            c = blockIdx.x;
        }
    }
    } while (RES || (PERSIST && (c += gridDim.x) < s.nChannels));    // without PERSIST / RES there is no loop at all (it would cost registers)
}


// The grid. One workgroup per channel by default: the dispatcher hands every free slot the next channel. SF11 is the exception: its
// workgroup is TWO wavefronts, four workgroups per compute unit, and when workgroups of a second round are placed as slots free up
// one by one the unit can end with its two free wavefront slots on the SAME SIMD -- where the hardware does not place a workgroup
// (tools/wg_timeline.py, profiles/r04/s19_*: a slot stayed empty for 1.1 ms with a workgroup waiting for it; 2048 channels took
// 4.1-5.6 ms from launch to launch). There the grid is PERSISTENT: the resident number of workgroups, placed once on an empty
// device, each taking channel after channel (c += gridDim.x) -- with the alternating priority (lorahip_framemachine.h) they advance
// alike, so the static split leaves no tail: 3.94-3.97 ms every launch. s.maxBlocks: 0 = this default, < 0 = never persistent,
// > 0 = at most that many workgroups (lorahip_demod_set_stream_grid: tests, A/B).
template <class C>
static hipError_t launchStreamWideCfg(const StreamArgs &args, hipStream_t stream)
{
    const size_t smem = WideSmem<C>::streamBytes();
    static unsigned long long attrDone = 0, attrDoneP = 0;
    static PerDeviceCount resident, residentP;
    StreamArgs s = args;
    if (s.nChannels == 0) return hipSuccess;
    int cap = s.maxBlocks;
    if (cap == 0 && C::LOG2N == 11)
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(demodStreamWide<C, true>), smem, attrDoneP);
        if (e != hipSuccess) return e;
        cap = residentWorkgroupsCached(residentP, reinterpret_cast<const void *>(demodStreamWide<C, true>), C::T, smem);
    }
    if (cap > 0 && s.nChannels > unsigned(cap))
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(demodStreamWide<C, true>), smem, attrDoneP);
        if (e != hipSuccess) return e;
        s.lastRoundFrom = 0;                                    // nobody is replaced: every workgroup takes its turn at the priority
        hipLaunchKernelGGL((demodStreamWide<C, true>), dim3(unsigned(cap)), dim3(C::T), smem, stream, s);
        return hipGetLastError();
    }
    const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(demodStreamWide<C, false>), smem, attrDone);
    if (e != hipSuccess) return e;
    s.lastRoundFrom = lastRoundFrom(s.nChannels, residentWorkgroupsCached(resident, reinterpret_cast<const void *>(demodStreamWide<C, false>), C::T, smem));
    hipLaunchKernelGGL((demodStreamWide<C, false>), dim3(s.nChannels), dim3(C::T), smem, stream, s);
    return hipGetLastError();
}

//! the resident receiver's launch at SF11 / SF12 (see launchStreamResidentCfg in lorahip_streamkernel.h): refused unless every workgroup is
//! resident at once; with more channels than that every workgroup walks several per step
template <class C>
static hipError_t launchStreamResidentWideCfg(const StreamArgs &args, hipStream_t stream, unsigned *gridOut)
{
    const size_t smem = WideSmem<C>::streamBytes(sizeof(ResLds));
    static unsigned long long attrDone = 0;
    static PerDeviceCount resident;
    if (gridOut) *gridOut = 0;
    if (args.nChannels == 0) return hipErrorNotSupported;
    const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(demodStreamWide<C, false, true>), smem, attrDone);
    if (e != hipSuccess) return e;
    const int res = residentWorkgroupsCached(resident, reinterpret_cast<const void *>(demodStreamWide<C, false, true>), C::T, smem);
    if (res <= 0) return hipErrorNotSupported;
    const unsigned perWg = (args.nChannels + unsigned(res) - 1) / unsigned(res);
    const unsigned grid = (args.nChannels + perWg - 1) / perWg;
    if (grid > 4095u) return hipErrorNotSupported;
    if (gridOut) *gridOut = grid;
    hipLaunchKernelGGL((demodStreamWide<C, false, true>), dim3(grid), dim3(C::T), smem, stream, args);
    return hipGetLastError();
}

hipError_t launchStreamResidentWide(const int sf, const StreamArgs &s, hipStream_t stream, unsigned *grid)
{
    return sf == 11 ? launchStreamResidentWideCfg<StreamWide11>(s, stream, grid) : launchStreamResidentWideCfg<StreamWide12>(s, stream, grid);
}

hipError_t launchStreamWide(const int sf, const StreamArgs &s, hipStream_t stream)
{
    return sf == 11 ? launchStreamWideCfg<StreamWide11>(s, stream) : launchStreamWideCfg<StreamWide12>(s, stream);
}


} // namespace lorahip
