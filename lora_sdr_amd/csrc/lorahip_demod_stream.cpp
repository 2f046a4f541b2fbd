// Level 3, the streaming path: the device walks every channel (lorahip_stream.hip); the host only drains the per-call records,
// assembles the packets and keeps the Channel mirrors in step. Also what every streaming launch of the object shares, whoever makes
// it -- a run here, a pipelined step (lorahip_demod_pipe.cpp), the resident receiver (lorahip_demod_resident.cpp).
#include "lorahip_demod_state.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lorahip { namespace demod {

//! device + pinned scratch pair for packed records (grown on demand, both or neither)
int growDense(lorahip_demod *dm, const size_t bytes)
{
    if (bytes <= dm->dDense.bytes()) return LORAHIP_OK;
    LORAHIP_TRY(regrowPair(dm->dDense, bytes + bytes / 4, dm->hDense, bytes + bytes / 4, hipHostMallocDefault));
    return LORAHIP_OK;
}

//! a pipelined or resident receiver step is in flight (lorahip_demod_receive with async = 2 / 3): only receive / receive_flush may touch
//! the object
bool pipeBusy(const lorahip_demod *dm) { return dm->pipe.active || dm->res.active; }
int refuseWhilePiped(const lorahip_demod *dm)
{
    if (!pipeBusy(dm)) return LORAHIP_OK;
    setLastError("a pipelined receiver step is in flight: lorahip_demod_receive_flush first");
    return LORAHIP_E_INVALID;
}

//! packets of one run in the order the host-driven path posts them: round by round, channels ascending inside a round
static void orderNewPackets(lorahip_demod *dm, const size_t firstNewPacket, const int64_t rounds)
{
    // The new packets were appended channel by channel with rounds ascending inside a channel: a stable counting sort by round
    // restores the order in O(packets + rounds) instead of a comparison sort of tens of thousands of records (which cost more
    // than the kernel). Several launches per run can interleave channels inside a round; that case is detected and sorted.
    const size_t nNew = dm->packets.size() - firstNewPacket;
    if (nNew <= 1) return;
    Packet *first = dm->packets.data() + firstNewPacket;
    bool sorted = true, channelsAscendPerRound = true;
    for (size_t i = 1; i < nNew && sorted; i++)
        sorted = first[i - 1].round < first[i].round || (first[i - 1].round == first[i].round && first[i - 1].channel <= first[i].channel);
    if (!sorted && rounds >= 0 && size_t(rounds) <= 4 * nNew + 1024)
    {
        std::vector<size_t> start(size_t(rounds) + 2, 0);
        for (size_t i = 0; i < nNew; i++) start[size_t(first[i].round) + 1]++;
        for (size_t r = 1; r < start.size(); r++) start[r] += start[r - 1];
        std::vector<Packet> tmp(nNew);
        for (size_t i = 0; i < nNew; i++) tmp[start[size_t(first[i].round)]++] = first[i];
        for (size_t i = 1; i < nNew && channelsAscendPerRound; i++)
            channelsAscendPerRound = tmp[i - 1].round != tmp[i].round || tmp[i - 1].channel <= tmp[i].channel;
        std::copy(tmp.begin(), tmp.end(), first);
        sorted = channelsAscendPerRound;
    }
    if (!sorted)
        std::stable_sort(first, first + nNew,
                         [](const Packet &x, const Packet &y) { return x.round != y.round ? x.round < y.round : x.channel < y.channel; });
}

//! the head of the streaming buffers inside dm->sHost: offsets that depend on the channel count only (StreamLayout::make)
StreamLayout headLayout(const lorahip_demod *dm)
{
    StreamLayout L;
    L.make(dm->B, 8, 4, false);
    return L;
}

//! The per-channel state and counts of the last streaming launch into their pinned copy (52 B per channel): a run itself reads back
//! only its summary; whoever needs the arrays -- the Channel mirrors, consumed(), a drain of the records -- asks here first.
int ensureHead(lorahip_demod *dm)
{
    if (!dm->home.headLags() || dm->sHost.get() == nullptr || dm->sDev.get() == nullptr) return LORAHIP_OK;
    const StreamLayout L = headLayout(dm);
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(hipMemcpyAsync(dm->sHost.get() + L.oState, dm->sDev.get() + L.oState, L.oPkt - L.oState, hipMemcpyDeviceToHost, dm->ctx->stream));
    LORAHIP_TRY(hipStreamSynchronize(dm->ctx->stream));
    dm->home.headFetched();
    return LORAHIP_OK;
}

//! records of one launch (still in dm->sDev; the counts in dm->sHost) -> the host queue, the per-channel traces and open packets
static int drainLaunch(lorahip_demod *dm, const StreamLayout &L)
{
    lorahip_ctx *ctx = dm->ctx;
    const size_t B = L.B;
    { const int rc = ensureHead(dm); if (rc != LORAHIP_OK) return rc; }
    char *h = dm->sHost.get(), *d = dm->sDev.get();
    const int *hN = reinterpret_cast<int *>(h + L.oN), *hNSym = reinterpret_cast<int *>(h + L.oNSym), *hNPkt = reinterpret_cast<int *>(h + L.oNPkt);
    std::vector<size_t> &carry = dm->carry;
    // only as many columns of the [channel][capacity] record arrays as the fullest channel used cross PCIe: the capacities are
    // worst-case bounds, several times what a run fills
    const int *hNSig = reinterpret_cast<int *>(h + L.oNSig);
    size_t maxSym = 0, maxPkt = 0, maxCalls = 0, maxSig = 0;
    for (size_t c = 0; c < B; c++)
    {
        if (size_t(hNSym[c]) > maxSym) maxSym = size_t(hNSym[c]);
        if (size_t(hNPkt[c]) > maxPkt) maxPkt = size_t(hNPkt[c]);
        if (size_t(hN[c]) > maxCalls) maxCalls = size_t(hN[c]);
        if (L.signals && size_t(hNSig[c]) > maxSig) maxSig = size_t(hNSig[c]);
    }
    const size_t nbPkt = align256(B * maxPkt * sizeof(StreamPacket)), nbSym = align256(B * maxSym * sizeof(short));
    const size_t nbCalls = L.tracing ? align256(B * maxCalls * sizeof(lorahip_work_result)) : 0;
    const size_t nbSig = align256(B * maxSig * sizeof(StreamSignal));
    const size_t nbDense = nbPkt + nbSym + nbCalls + nbSig;
    { const int grc = growDense(dm, nbDense); if (grc != LORAHIP_OK) return grc; }
    LORAHIP_TRY(launchCompactRows(dm->dDense.get(), d + L.oPkt, B, L.capPkt * sizeof(StreamPacket), maxPkt * sizeof(StreamPacket), ctx->stream));
    LORAHIP_TRY(launchCompactRows(dm->dDense.get() + nbPkt, d + L.oSym, B, L.symStride * sizeof(short), maxSym * sizeof(short), ctx->stream));
    if (L.tracing)
        LORAHIP_TRY(launchCompactRows(dm->dDense.get() + nbPkt + nbSym, d + L.oCalls, B, L.cap * sizeof(lorahip_work_result),
                                      maxCalls * sizeof(lorahip_work_result), ctx->stream));
    if (maxSig)
        LORAHIP_TRY(launchCompactRows(dm->dDense.get() + nbPkt + nbSym + nbCalls, d + L.oSig, B, L.capPkt * sizeof(StreamSignal), maxSig * sizeof(StreamSignal), ctx->stream));
    if (nbDense) LORAHIP_TRY(hipMemcpyAsync(dm->hDense.get(), dm->dDense.get(), nbDense, hipMemcpyDeviceToHost, ctx->stream));
    LORAHIP_TRY(hipStreamSynchronize(ctx->stream));
    const StreamPacket *hPkt = reinterpret_cast<const StreamPacket *>(dm->hDense.get());
    const short *hSym = reinterpret_cast<const short *>(dm->hDense.get() + nbPkt);
    const lorahip_work_result *hCalls = reinterpret_cast<const lorahip_work_result *>(dm->hDense.get() + nbPkt + nbSym);
    const StreamSignal *hSig = reinterpret_cast<const StreamSignal *>(dm->hDense.get() + nbPkt + nbSym + nbCalls);
    for (size_t c = 0; c < B; c++)
    {
        Channel &k = dm->ch[c];
        for (int j = 0; L.signals && j < hNSig[c]; j++)
        {
            const StreamSignal &q = hSig[c * maxSig + size_t(j)];
            Signal g;
            g.channel = int32_t(c); g.round = q.callIndex; g.error = q.error; g.power = q.power; g.snr = q.snr; g.pos = q.pos;
            dm->signals.push_back(g);
        }
        // symbols of this launch continue the packet the previous launches left open (k.outSymbols[0..carry[c]))
        const short *sy = hSym + c * maxSym;
        size_t p = 0;
        for (int j = 0; j < hNPkt[c]; j++)
        {
            const StreamPacket &q = hPkt[c * maxPkt + size_t(j)];
            Packet pk;
            pk.channel = int32_t(c);
            pk.round = q.callIndex;
            pk.off = dm->pktSyms.size();
            pk.len = size_t(q.len);
            pk.endPos = q.endPos; pk.freqError = q.freqError;
            dm->pktSyms.insert(dm->pktSyms.end(), k.outSymbols.begin(), k.outSymbols.begin() + long(carry[c]));
            const size_t fresh = size_t(q.len) - carry[c];
            dm->pktSyms.insert(dm->pktSyms.end(), sy + p, sy + p + fresh);
            p += fresh;
            carry[c] = 0;
            dm->packets.push_back(pk);
        }
        // what is left belongs to a packet still being received
        const size_t left = size_t(hNSym[c]) - p;
        if (left)
        {
            if (k.outSymbols.size() < carry[c] + left) k.outSymbols.resize(carry[c] + left, 0);
            for (size_t i = 0; i < left; i++) k.outSymbols[carry[c] + i] = sy[p + i];
            carry[c] += left;
        }
        if (L.tracing) k.trace.insert(k.trace.end(), hCalls + c * maxCalls, hCalls + c * maxCalls + hN[c]);
    }
    return LORAHIP_OK;
}

//! bring a pending launch's records to the host (any accessor of the queue / traces does this first)
int drainPending(lorahip_demod *dm)
{
    PendingLaunch &P = dm->pending;
    if (!P.valid) return LORAHIP_OK;
    const DeviceGuard guard(dm->ctx->device);
    typedef std::chrono::steady_clock Clock;
    const Clock::time_point t0 = Clock::now();
    // the records stay pending until they HAVE been drained: after a failed drain (HIP error, no memory for the staging) the
    // packet counts reported so far remain true and a later accessor retries. drainLaunch appends to the queue only after its
    // last fallible step (the copy back), so a retry cannot duplicate packets.
    const int rc = drainLaunch(dm, P.lay);
    if (rc != LORAHIP_OK) return rc;
    P.valid = false;
    dm->home.pendingDrained();                        // drainLaunch has written the open packets' symbols of this launch into the mirrors
    orderNewPackets(dm, P.firstNewPacket, P.rounds);
    P.drainMs = std::chrono::duration<double>(Clock::now() - t0).count() * 1e3;
    static const bool timing = std::getenv("LORAHIP_DEMOD_TIMING") != nullptr;
    if (timing) std::fprintf(stderr, "lorahip demod: records of the last launch drained to the host in %.3f ms\n", P.drainMs);
    return LORAHIP_OK;
}

StreamState *hostStates(lorahip_demod *dm)
{
    return reinterpret_cast<StreamState *>(dm->sHost.get() + headLayout(dm).oState);
}

//! the open packets' symbols the device holds (dCarry) into the mirrors' outSymbols; the mirrors' state must be current
static int fetchCarry(lorahip_demod *dm)
{
    if (!dm->home.openPacketsLag()) return LORAHIP_OK;
    const size_t B = dm->B, cap = dm->carryCap;
    bool any = false;
    for (size_t c = 0; c < B && !any; c++) any = dm->ch[c].state == ST_DATASYMBOLS && dm->ch[c].symCount != 0;
    if (any && dm->dCarry.get() && dm->home.carryRowsValid())
    {
        const DeviceGuard guard(dm->ctx->device);
        std::vector<short> rows;
        try { rows.resize(B * cap); } catch (...) { setLastError("no memory for the open packets' symbols"); return LORAHIP_E_NOMEM; }   // nothing may cross the C ABI
        LORAHIP_TRY(hipMemcpyAsync(rows.data(), dm->dCarry.get(), B * cap * sizeof(short), hipMemcpyDeviceToHost, dm->ctx->stream));
        LORAHIP_TRY(hipStreamSynchronize(dm->ctx->stream));
        for (size_t c = 0; c < B; c++)
        {
            Channel &k = dm->ch[c];
            if (k.state != ST_DATASYMBOLS || k.symCount == 0) continue;
            const size_t n = k.symCount < cap ? k.symCount : cap;
            if (k.outSymbols.size() < k.symCount) k.outSymbols.resize(k.symCount, 0);
            std::memcpy(k.outSymbols.data(), rows.data() + c * cap, n * sizeof(short));
        }
    }
    dm->home.openPacketsFetched();
    return LORAHIP_OK;
}

//! bring the Channel mirrors up to date with the device's state (its pinned copy): only the paths that read them pay for it
int syncMirrors(lorahip_demod *dm)
{
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->home.mirrorsLag() && dm->sHost.get())
    {
        { const int rc = ensureHead(dm); if (rc != LORAHIP_OK) return rc; }
        const StreamState *hs = hostStates(dm);
        for (size_t c = 0; c < dm->B; c++)
        {
            Channel &k = dm->ch[c];
            const StreamState &st = hs[c];
            fromStreamState(k, st);
            if (dm->home.pinnedPosCurrent()) { k.pos = size_t(st.pos); k.callCount = st.callCount; }
        }
    }
    dm->home.mirrorsSynced();
    // before a deferred activate() hides which channels were inside a packet. A failed copy leaves the mirrors' symbols lagging and the
    // device's copy valid: the caller must not invalidate it (it returns the error instead)
    { const int rc = fetchCarry(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->home.activateWaiting())
    {
        for (auto &k : dm->ch) { k.state = ST_FRAMESYNC; k.downTable = false; }     // activate() (:139-143), deferred
        dm->home.activateAppliedToMirrors();            // the device copy does not have it: the next streaming run uploads
    }
    return LORAHIP_OK;
}

//! StreamArgs::lanes of this object's launches: what was asked for; where nothing was and sibling parts share the device (a mixed
//! object), the automatic choice made HERE with their wavefronts counted -- as an explicit choice for launchStream
static int lanesArg(const lorahip_demod *dm)
{
    if (dm->streamLanes != 0 || dm->coWaves == 0) return dm->streamLanes;
    const int l = streamLanesChosen(dm->ctx->sf, unsigned(dm->B), 0, dm->coWaves);
    return l == dm->ctx->sf - 4 ? -1 : l;
}

bool usesStreamKernel(const lorahip_demod *dm) { return dm->mode == 1 || (dm->mode == 0 && streamAvailable(dm->ctx->sf)); }

//! per-launch record capacity (work() calls per channel) and packet capacity for streams of at most maxLen samples
void streamCapacity(const lorahip_demod *dm, const size_t maxLen, size_t &cap, size_t &capPkt)
{
    // work() calls per channel per launch: enough for a clean stream in one launch, bounded so that the
    // per-launch buffers stay moderate (the launch is resumable)
    const size_t perCall = sizeof(short) + (dm->tracing ? sizeof(lorahip_work_result) : 0) + sizeof(StreamPacket) / 4 + 1 + (dm->wantSignals ? sizeof(StreamSignal) / 4 : 0);
    // A call consumes N samples except around a frame's sync (N - value, N/4 + error/2: LoRaDemod.cpp:219, :278) -- a handful of short
    // calls per frame -- and in an unsquelched FRAMESYNC window that does not sync (N - value every call: a receiver idling on noise
    // above its threshold makes about two calls per N samples). A launch whose record buffers fill is resumed, but the records have
    // to be drained in between (measured: 9.7 ms instead of 7.0 ms per run at SF7, 16384 channels x 16 frames), so the capacity
    // starts with an eighth of headroom and follows what the runs of this receiver actually needed (never shrinks).
    cap = (maxLen / dm->N) * dm->callsPerWindowQ8 / 256 + 64;
    if (cap > 65536) cap = 65536;
    const size_t capMem = (size_t(1) << 30) / (dm->B * perCall);
    if (cap > capMem) cap = capMem;
    if (cap < 8) cap = 8;
    // lorahip_demod_set_record_capacity: a bound on the per-launch record capacity (tests force the resume path with it)
    if (dm->streamCapMax != 0 && cap > dm->streamCapMax) cap = dm->streamCapMax;
    capPkt = cap / 4 + 2;                            // a packet costs at least 5 calls (3 sync, quarter, 1 symbol)
}

//! the kernels' running near-threshold counters, as read now, into the object's counts: the counters only add, so what is new is
//! the difference to the last read
void foldNear(lorahip_demod *dm, const unsigned squelch, const unsigned step)
{
    dm->nNearSquelch += int64_t(unsigned(squelch - dm->nearSeen[0]));
    dm->nNearStep += int64_t(unsigned(step - dm->nearSeen[1]));
    dm->nearSeen[0] = squelch; dm->nearSeen[1] = step;
}

/*! What every streaming launch of this object shares: its tables and settings, the head of dm->sDev (the per-channel state and the
 * near-threshold counters, which every launch continues), the carry rows, the record arrays of layout L at `rec`, and the grid. The
 * caller sets the placement (uniformLen; base / len for per-channel streams) and the flags; what nobody sets stays zero. */
StreamArgs makeStreamArgs(const lorahip_demod *dm, const float *iqDev, const StreamLayout &L, char *rec)
{
    const lorahip_ctx *ctx = dm->ctx;
    const StreamLayout H = headLayout(dm);
    StreamArgs a{};
    a.iq = reinterpret_cast<const float2 *>(iqDev);
    a.uniformStride = (long long)dm->home.stride();
    a.state = reinterpret_cast<StreamState *>(dm->sDev.get() + H.oState);
    a.near = reinterpret_cast<unsigned *>(dm->sDev.get() + H.oNear);
    a.carry = dm->dCarry.get(); a.carryCap = int(dm->carryCap);
    a.nCalls = reinterpret_cast<int *>(rec + L.oN); a.nSym = reinterpret_cast<int *>(rec + L.oNSym); a.nPkt = reinterpret_cast<int *>(rec + L.oNPkt);
    a.nSig = reinterpret_cast<int *>(rec + L.oNSig); a.end = reinterpret_cast<int2 *>(rec + L.oEnd);
    a.pktOut = reinterpret_cast<StreamPacket *>(rec + L.oPkt); a.symOut = reinterpret_cast<short *>(rec + L.oSym);
    a.sigOut = L.signals ? reinterpret_cast<StreamSignal *>(rec + L.oSig) : nullptr;
    a.calls = L.tracing ? reinterpret_cast<lorahip_work_result *>(rec + L.oCalls) : nullptr;
    a.down = ctx->dDown.get(); a.fine = ctx->dFine.get(); a.twStage = ctx->dTwStage.get();
    a.fineA = ctx->fineGather ? nullptr : ctx->dFineA.get(); a.fineB = ctx->fineGather ? nullptr : ctx->dFineB.get();
    a.nChannels = unsigned(L.B); a.cap = int(L.cap); a.symStride = int(L.symStride); a.capPkt = int(L.capPkt);
    a.powerScale = ctx->powerScale; a.thresh = dm->thresh; a.sync = dm->sync;
    a.mtu = dm->mtu > 0xffffffffu ? 0xffffffffu : unsigned(dm->mtu);
    // The grid (lorahip_demod_set_stream_grid; 0 = the kernels' own default). One workgroup per channel set, however many there are,
    // at every SF but 11: the dispatcher hands a free slot the next set. A PERSISTENT grid (the resident number of workgroups, each
    // looping over sets) lost there even with the alternating priority (profiles/r04/s22_*: SF7 32768 channels 0.34 against 0.44,
    // SF9 0.36 against 0.40; SF8 / 10 / 12 equal) -- the loop costs the wave-per-channel-set kernels registers -- and is the default
    // only where one-by-one placement leaves slots unusable: SF11 (lorahip_stream_wide.hip::launchStreamWideCfg).
    a.maxBlocks = dm->streamGrid; a.lanes = lanesArg(dm); a.lastRoundFrom = 0;
    return a;
}

int runStream(lorahip_demod *dm, const float *iqDev, int64_t *roundsOut)
{
    lorahip_ctx *ctx = dm->ctx;
    const size_t N = dm->N, B = dm->B;
    const DeviceGuard guard(ctx->device);
    // the previous run's records live in the buffers this run is about to reuse
    { const int rc = drainPending(dm); if (rc != LORAHIP_OK) return rc; }
    // diagnostic: LORAHIP_DEMOD_TIMING=1 prints where a run's host wall clock goes
    static const bool timing = std::getenv("LORAHIP_DEMOD_TIMING") != nullptr;
    typedef std::chrono::steady_clock Clock;
    const Clock::time_point t0 = Clock::now();
    double tDev = 0, tAsm = 0;
    const bool cont = dm->home.continues();                     // the channels continue where the last append run left them
    // an append run works through what is new since the last one plus what that one left (fewer than 2N samples per channel)
    const Home &pl = dm->home;
    size_t maxLen = pl.isUniform() ? (cont && pl.prevValid() <= pl.spc() ? pl.spc() - pl.prevValid() + 2 * N : pl.spc()) : 0;
    if (!pl.isUniform()) for (size_t c = 0; c < B; c++) if (dm->ch[c].len - dm->ch[c].pos > maxLen) maxLen = dm->ch[c].len - dm->ch[c].pos;
    size_t cap, capPkt;
    streamCapacity(dm, maxLen, cap, capPkt);

    // open packets on the device (dCarry): rows of mtu + 1 symbols; receivers with longer packets than this keep the host path
    // (the carry rows and their share of the symbol rows stay inside the memory bound of the record buffers above)
    const size_t kCarryLimit = 4096;
    bool useDevCarry = dm->mtu <= kCarryLimit && B * (dm->mtu + 1 < 64 ? 64 : dm->mtu + 1) * sizeof(short) <= (size_t(1) << 29);
    if (useDevCarry && dm->mtu + 1 > dm->carryCap)
    {
        { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }      // what the device holds of open packets goes to the mirrors first
        dm->carryCap = 0; dm->home.carryRowsRegrown();
        const size_t rows = dm->mtu + 1 < 64 ? 64 : dm->mtu + 1;
        LORAHIP_TRY(dm->dCarry.grow(B * rows * sizeof(short)));      // (more rows than it has: the old block goes, then the new one is made)
        dm->carryCap = rows;
    }

    StreamLayout L;
    L.make(B, cap, capPkt, dm->tracing, useDevCarry ? dm->carryCap : 0, dm->wantSignals);
    if (L.total > dm->sDev.bytes())
    {
        { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }      // the pinned copy of the state goes away with the buffers
        dm->home.recordBuffersRegrown();             // (syncMirrors has read what there was)
        // a quarter more than this run needs: the chunks of a running receiver differ by the remainders they start with, and every
        // growth costs two allocations and an upload of the state
        LORAHIP_TRY(regrowPair(dm->sDev, L.total + L.total / 4, dm->sHost, L.oPkt, hipHostMallocDefault));   // the host mirrors only the head: placement, state, counts
        // the kernels' near-threshold counters only ever add: they start at zero with the buffers
        LORAHIP_TRY(hipMemsetAsync(dm->sDev.get() + L.oNear, 0, 2 * sizeof(unsigned), ctx->stream));
        dm->nearSeen[0] = dm->nearSeen[1] = 0;
    }
    char *h = dm->sHost.get(), *d = dm->sDev.get();
    long long *hBase = reinterpret_cast<long long *>(h + L.oBase), *hLen = reinterpret_cast<long long *>(h + L.oLen);
    StreamState *hState = reinterpret_cast<StreamState *>(h + L.oState);
    const StreamSummary *hSum = reinterpret_cast<const StreamSummary *>(h + L.oSum);
    std::vector<size_t> &carry = dm->carry;
    carry.assign(B, 0);
    bool anyCarryIn = false;
    size_t maxCarry = 0;
    // A steady receiver -- run after run in this mode, device buffers, nothing touched in between -- uploads nothing and reads back
    // 72 bytes: the state is where the last run left it on the device, the placement of uniform streams is computed by the kernel,
    // an activate() in between travels as a flag, the open packets' symbols are in the device's carry rows, and what the host needs
    // to know of the last run is its summary (streamSummary). The per-channel state and counts are fetched when somebody asks.
    const bool resident = dm->home.deviceCurrent();
    const bool activate = resident && dm->home.activateWaiting();
    if (resident)
    {
        // symbols of packets that are still being received when the run starts: the last summary says whether there are any
        if (!activate && dm->lastSum.anyOpen && dm->lastSum.openSyms > 0) { anyCarryIn = true; maxCarry = size_t(dm->lastSum.maxOpen); }
        // which channels, and how many symbols each, only matters where the HOST hands them on
        const bool perChannel = anyCarryIn && (!useDevCarry || maxCarry >= dm->carryCap || !dm->home.carryRowsValid());
        if (perChannel)
        {
            { const int rc = ensureHead(dm); if (rc != LORAHIP_OK) return rc; }
            for (size_t c = 0; c < B; c++) if (hState[c].state == ST_DATASYMBOLS && hState[c].symCount) carry[c] = size_t(hState[c].symCount);
        }
    }
    else
    {
        { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }
        for (size_t c = 0; c < B; c++)
        {
            Channel &k = dm->ch[c];
            StreamState &st = hState[c];
            toStreamState(k, st);
            st.callCount = cont ? int(k.callCount) : 0;
            st.pos = cont ? (long long)k.pos : 0;
            if (k.outSymbols.size() < k.symCount) k.outSymbols.resize(k.symCount, 0);
            // symbols of a packet that is still being received when the run starts. _symCount itself is only reset at
            // QUARTERCHIRP (:279), so outside DATASYMBOLS it still holds the length of the LAST packet: nothing is carried then
            carry[c] = k.state == ST_DATASYMBOLS ? k.symCount : 0;
            anyCarryIn = anyCarryIn || carry[c] != 0;
            if (carry[c] > maxCarry) maxCarry = carry[c];
        }
        LORAHIP_TRY(hipMemcpyAsync(d + L.oState, h + L.oState, L.oN - L.oState, hipMemcpyHostToDevice, ctx->stream));
        dm->home.stateUploaded();                     // the pinned copy IS what the device is being given
    }
    // Where do the symbols of those packets come from? From the device's own copy (the carry rows: the kernel copies a channel's open
    // packet to the head of its symbol row and appends behind it, so the host sees packets without a past), unless a packet is
    // longer than those rows -- then from the mirrors' outSymbols, as the launches of a resumed run do among themselves.
    if (useDevCarry && maxCarry >= dm->carryCap) useDevCarry = false;
    if (useDevCarry)
    {
        if (anyCarryIn && !dm->home.carryRowsValid())
        {
            // the mirrors hold them (a host-driven run, or a resumed one, came before): up they go
            const size_t cc = dm->carryCap;
            { const int grc = growDense(dm, B * cc * sizeof(short)); if (grc != LORAHIP_OK) return grc; }
            short *stage = reinterpret_cast<short *>(dm->hDense.get());
            for (size_t c = 0; c < B; c++)
                if (carry[c]) std::memcpy(stage + c * cc, dm->ch[c].outSymbols.data(), (carry[c] < dm->ch[c].outSymbols.size() ? carry[c] : dm->ch[c].outSymbols.size()) * sizeof(short));
            LORAHIP_TRY(hipMemcpyAsync(dm->dCarry.get(), stage, B * cc * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
            LORAHIP_TRY(hipStreamSynchronize(ctx->stream));       // the pinned scratch is reused
        }
        carry.assign(B, 0);
        anyCarryIn = false;                           // as far as the host's assembly of packets is concerned
    }
    else
    {
        if (dm->home.openPacketsLag()) { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }      // (a deferred activate() then travels with the state upload: see syncMirrors)
        if (anyCarryIn)
            for (size_t c = 0; c < B; c++) if (carry[c] && dm->ch[c].outSymbols.size() < carry[c]) dm->ch[c].outSymbols.resize(carry[c], 0);
        dm->home.carryRowsBypassed();
    }
    if (!pl.isUniform())
    {
        for (size_t c = 0; c < B; c++) { hBase[c] = (long long)dm->ch[c].base; hLen[c] = (long long)dm->ch[c].len; }
        LORAHIP_TRY(hipMemcpyAsync(d, h, L.oState, hipMemcpyHostToDevice, ctx->stream));       // base, len
    }

    StreamArgs a = makeStreamArgs(dm, iqDev, L, d);
    a.base = reinterpret_cast<const long long *>(d + L.oBase);
    a.len = reinterpret_cast<const long long *>(d + L.oLen);
    a.uniformLen = pl.isUniform() ? (long long)pl.spc() : -1;
    // first launch of the run: every channel starts at sample 0, call 0 (unless the run continues the streams), behind its open packet's
    // symbols, and leaves the packet it is inside at the end in the carry rows
    a.flags = (cont ? 0 : 1) | (activate ? 2 : 0) | (useDevCarry ? 4 | 8 : 0);
    if (activate) dm->home.activateRidesLaunch();     // applied by the kernel when it loads the state
    dm->home.runBegins();                             // (before the first launch: a failed one leaves the device distrusted)

    const size_t firstNewPacket = dm->packets.size();
    const Clock::time_point t1 = Clock::now();
    dm->kernelMs = 0.0;
    LORAHIP_TRY(dm->evK0.ensure());
    LORAHIP_TRY(dm->evK1.ensure());
    bool lastPending = false;
    int launches = 0;
    size_t runCalls = 0;                              // calls of the fullest channel, launch by launch
    StreamSummary sum;
    while (true)
    {
        const Clock::time_point ta = Clock::now();
        LORAHIP_TRY(hipEventRecord(dm->evK0.get(), ctx->stream));
        LORAHIP_TRY(launchStream(ctx->sf, a, ctx->stream));
        LORAHIP_TRY(hipEventRecord(dm->evK1.get(), ctx->stream));
        a.flags = 0;                                  // a resumed launch continues where the state says
        // what the host needs of the launch, reduced on the device: 72 bytes come back, not 52 per channel
        // (written by the kernel straight into the pinned staging block when the device can address it: no copy to enqueue)
        void *sumDev = nullptr;
        const bool direct = hipHostGetDevicePointer(&sumDev, const_cast<StreamSummary *>(hSum), 0) == hipSuccess && sumDev != nullptr;
        if (!direct) (void)hipGetLastError();
        LORAHIP_TRY(launchStreamSummary(a.end, a.nCalls, a.nSym, a.nPkt, dm->wantSignals ? a.nSig : nullptr, B, int(cap), int(capPkt), a.near, dm->dSumScratch.get(),
                                        direct ? static_cast<StreamSummary *>(sumDev) : reinterpret_cast<StreamSummary *>(d + L.oSum), ctx->stream));
        if (!direct) LORAHIP_TRY(hipMemcpyAsync(h + L.oSum, d + L.oSum, sizeof(StreamSummary), hipMemcpyDeviceToHost, ctx->stream));
        LORAHIP_TRY(hipStreamSynchronize(ctx->stream));
        dm->home.launchSummarised();                  // the pinned copy of the per-channel state and counts lags the device now
        { float ms = 0.0f; if (hipEventElapsedTime(&ms, dm->evK0.get(), dm->evK1.get()) == hipSuccess) dm->kernelMs += ms; }
        const Clock::time_point tb = Clock::now();
        tDev += std::chrono::duration<double>(tb - ta).count();
        sum = *hSum;
        foldNear(dm, sum.nearSquelch, sum.nearStep);
        const bool more = sum.more != 0;
        dm->workCalls += sum.calls;
        runCalls += size_t(sum.fullest);
        launches++;
        // a launch that must be resumed hands its records over now (the next one reuses the buffers); so does a traced run (its
        // callers read the trace next). Otherwise the records wait on the device.
        if (more || dm->tracing)
        {
            const int rc = drainLaunch(dm, L);
            if (rc != LORAHIP_OK) return rc;
            tAsm += std::chrono::duration<double>(Clock::now() - tb).count();
            anyCarryIn = false;
            for (size_t c = 0; c < B; c++) anyCarryIn = anyCarryIn || carry[c] != 0;
        }
        else lastPending = true;
        if (!more) break;
    }
    const Clock::time_point t2 = Clock::now();
    const int64_t rounds = sum.maxCallCount;
    const bool anyOpen = sum.anyOpen != 0;
    const size_t openSyms = size_t(sum.openSyms);
    size_t carriedIn = 0;
    if (anyCarryIn || lastPending) for (size_t c = 0; c < B; c++) carriedIn += carry[c];
    dm->lastSum = sum;
    dm->lastLaunches = launches;
    if (launches > 1 && maxLen >= N)
    {
        // the run had to be resumed: size the record buffers of the runs to come for the fullest channel's rate of calls, a quarter on top
        const size_t q8 = (runCalls * 256 / (maxLen / N)) * 5 / 4 + 16;
        if (q8 > dm->callsPerWindowQ8) dm->callsPerWindowQ8 = q8 > size_t(256) * 64 ? size_t(256) * 64 : q8;
    }
    // the device holds the current state; the pinned copy and the mirrors lag. The packets the channels are inside now: the kernel
    // left the last symCount entries of their symbol rows in the carry rows (a drain -- traced runs -- has brought the mirrors'
    // outSymbols up to date already), unless the run was resumed: its launches handed the symbols on through the mirrors
    dm->home.runEnded(!(useDevCarry && launches == 1) ? Home::THROUGH_MIRRORS : lastPending ? Home::CARRY_RECORDS_PENDING : Home::CARRY_RECORDS_DRAINED);
    PendingLaunch &P = dm->pending;
    if (lastPending)
    {
        P.valid = true;
        P.lay = L;
        P.firstNewPacket = firstNewPacket;
        P.rounds = rounds;
        P.packets = size_t(sum.packets);
        P.packetSyms = carriedIn + size_t(sum.syms) - openSyms;     // symbols of the packets completed by this launch
        P.signals = size_t(sum.signals);
        P.anyCarryIn = anyCarryIn;
        P.anyOpen = anyOpen;
        P.drainMs = 0.0;
    }
    else orderNewPackets(dm, firstNewPacket, rounds);
    if (roundsOut) *roundsOut = rounds;
    if (timing)
        std::fprintf(stderr, "lorahip demod run: setup+H2D %.3f ms%s, kernel+summary D2H+sync %.3f ms (kernel %.3f), record drain %.3f ms%s, rest %.3f ms\n",
                     std::chrono::duration<double>(t1 - t0).count() * 1e3, resident ? " (state resident on the device)" : "", tDev * 1e3, dm->kernelMs, tAsm * 1e3,
                     lastPending ? " (last launch left on the device)" : "", std::chrono::duration<double>(Clock::now() - t2).count() * 1e3);
    return LORAHIP_OK;
}

} } // namespace lorahip::demod
