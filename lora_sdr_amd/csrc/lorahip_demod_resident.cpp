// Level 3, the resident receiver (lorahip_demod_receive with async = 3): the host side. A step is a message copied into the ring in
// device memory (the doorbell) and, one call later, two words read from pinned memory. Packets and signals are written by the kernel
// itself into the rows that came WITH the step's message, i.e. with the call that rang it; they are complete when the next call (or
// the flush) returns. The kernel: lorahip_streamkernel.h (RES); the protocol: lorahip_residentproto.h, INTEGRATION.md section 4.
#include "lorahip_demod_state.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lorahip { namespace demod {

static const double kResidentTimeoutS = 5.0;                // host: longest wait for a step's report
static const unsigned long long kResidentWatchdog = 800000000ull;   // device: 8 s of 100 MHz ticks without a message, then the wavefront leaves

static int residentRing(lorahip_demod *dm, const size_t nValid, const lorahip_packet_rows *rows, const unsigned flags)
{
    Resident &R = dm->res;
    const unsigned seq = R.seq + 1;
    ResidentMsg m;
    std::memset(&m, 0, sizeof(m));
    m.nValid = nValid;
    if (rows)
    {
        m.syms = rows->syms_dev; m.nsyms = rows->nsyms_dev; m.chan = rows->channel_dev;
        m.symStride = unsigned(rows->sym_stride); m.capRows = unsigned(rows->cap_packets > 0xffffffu ? 0xffffffu : rows->cap_packets);
    }
    if (R.sigs && dm->sigRowsOn)
    {
        m.sigCh = dm->sigRows.channel; m.sigErr = dm->sigRows.error; m.sigPow = dm->sigRows.power; m.sigSnr = dm->sigRows.snr;
        m.capSig = unsigned(dm->sigRows.cap > 0xffffffu ? 0xffffffu : dm->sigRows.cap);
    }
    m.flags = flags;
    m.seq = seq;
    m.check = residentCheck(m);
    // plain stores into pinned memory, the step number last (the kernel verifies the check word whenever it sees the number)
    ResidentMsg *slot = &R.host->msg[seq & 7];
    __atomic_store_n(&slot->seq, 0u, __ATOMIC_RELEASE);
    std::memcpy(slot, &m, offsetof(ResidentMsg, seq));
    __atomic_store_n(&slot->seq, seq, __ATOMIC_RELEASE);
    R.seq = seq;
    return LORAHIP_OK;
}

//! wait for step `k`'s report (bounded); *packets / *signals = what the step produced (dropped ones included), *flags = RES_F_*
static int residentReport(lorahip_demod *dm, const unsigned k, size_t *packets, size_t *signals, int64_t *calls, unsigned *flags)
{
    Resident &R = dm->res;
    volatile unsigned long long *h = R.host->sum + 2 * (k & 7);
    typedef std::chrono::steady_clock Clock;
    const Clock::time_point t0 = Clock::now();
    unsigned spins = 0;
    for (;;)
    {
        const unsigned long long w0 = __atomic_load_n(const_cast<unsigned long long *>(h), __ATOMIC_ACQUIRE);
        const unsigned long long w1 = __atomic_load_n(const_cast<unsigned long long *>(h + 1), __ATOMIC_ACQUIRE);
        if (unsigned(w0 >> 32) == k && unsigned(w1 >> 56) == (k & 0xffu))
        {
            R.dbgReports++;
            if (spins == 0) R.dbgImmediate++;
            else R.dbgWaitNs += std::chrono::duration<double, std::nano>(Clock::now() - t0).count();
            *calls = int64_t(w0 & 0xffffffffull);
            *packets = size_t(w1 & 0xffffffull);
            *signals = size_t((w1 >> 24) & 0xffffffull);
            *flags = unsigned((w1 >> 48) & 0xffull);
            return LORAHIP_OK;
        }
        if ((++spins & 1023u) == 0 && std::chrono::duration<double>(Clock::now() - t0).count() > kResidentTimeoutS) break;
    }
    setLastError("lorahip_demod_receive (resident): no report for a step within 5 s -- the kernel is told to leave");
    return LORAHIP_E_HIP;
}

//! get the kernel off the device whatever state the steps are in (error paths, destroy)
void residentAbort(lorahip_demod *dm)
{
    Resident &R = dm->res;
    if (!R.active) return;
    __atomic_store_n(&R.host->abort, 1u, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(R.run.get());
    R.active = false; R.unavailable = true;
    dm->home.aborted();                               // the steps' bookkeeping is incomplete: the state on the device is not trusted (the carry flags stay: Home::aborted)
}

int residentFlush(lorahip_demod *dm, size_t *nPackets, int64_t *calls)
{
    Resident &R = dm->res;
    if (nPackets) *nPackets = 0;
    if (calls) *calls = 0;
    dm->lastSignals = 0;
    if (!R.active) return LORAHIP_OK;
    const DeviceGuard guard(dm->ctx->device);
    size_t pk = 0, sg = 0;
    int64_t cl = 0;
    unsigned fl = 0;
    bool lost = false;
    R.nRep = 0;
    while (R.reported < R.seq)
    {
        size_t p1 = 0, s1 = 0; int64_t c1 = 0;
        const int rc = residentReport(dm, R.reported + 1, &p1, &s1, &c1, &fl);
        if (rc != LORAHIP_OK) { residentAbort(dm); return rc; }
        R.reported++;
        if (R.nRep <= RES_DEPTH_MAX) { R.repPk[R.nRep] = p1; R.repSg[R.nRep] = dm->sigRowsOn ? s1 : 0; R.nRep++; }
        pk += p1; sg += s1; cl += c1;
        dm->workCalls += c1;
        lost = lost || (fl & (RES_F_PKT_OVERFLOW | RES_F_SIG_OVERFLOW));
        R.lastMore = (fl & RES_F_MORE) != 0;
    }
    // the quit message, then the kernel's end: the state, the read positions and the open packets are on the device as a streaming run leaves them
    { const int rc = residentRing(dm, R.lastValid, nullptr, 1u); if (rc != LORAHIP_OK) { residentAbort(dm); return rc; } }
    LORAHIP_TRY(hipStreamSynchronize(R.run.get()));
    R.active = false;
    if (nPackets) *nPackets = pk;
    if (calls) *calls = cl;
    dm->lastSignals = dm->sigRowsOn ? sg : 0;
    leaveStateOnDevice(dm);
    std::memset(&dm->lastSum, 0, sizeof(dm->lastSum));
    dm->lastSum.anyOpen = 1;                          // (not tracked per step: the carry rows are valid, which is all `anyOpen` guards)
    dm->lastSum.more = (R.lastMore || R.tail) ? 1 : 0;
    if (std::getenv("LORAHIP_RESIDENT_DEBUG"))
    {
        std::vector<char> cbuf(sizeof(ResidentCtl));
        ResidentCtl &c = *reinterpret_cast<ResidentCtl *>(cbuf.data());
        if (hipMemcpy(&c, R.ctl.get(), sizeof(c), hipMemcpyDeviceToHost) == hipSuccess)
            for (int k = 0; k < 8; k++)                     // (slot k holds the last step with (step - 1) & 7 == k; the wait stamp of slot k is of the step after)
                std::fprintf(stderr, "resident slot %d (workgroup 0, wave 0; us): waited %.1f, setup %.1f, windows + records %.1f, look-ahead + step end %.1f; since the end of the slot before %.1f\n", k + 1,
                             (c.dbg[k][1] - c.dbg[k][0]) / 100.0, (c.dbg[k][2] - c.dbg[k][1]) / 100.0, (c.dbg[k][4] - c.dbg[k][2]) / 100.0,
                             (c.dbg[k][5] - c.dbg[k][4]) / 100.0, (double(c.dbg[k][5]) - double(c.dbg[(k + 7) & 7][5])) / 100.0);
        {
            // every wavefront's stamps of the chosen step: when the step began (the first wavefront that saw the message), and how the
            // wavefronts' finishing times -- windows done, step end -- are spread behind it
            const unsigned nw = R.grid * 4u < 16384u ? R.grid * 4u : 16384u;
            std::vector<double> seen, done, end, busy;
            unsigned long long first = ~0ull;
            for (unsigned w = 0; w < nw; w++) if (c.dbgWave[w][1] && c.dbgWave[w][1] < first) first = c.dbgWave[w][1];
            for (unsigned w = 0; w < nw; w++)
                if (c.dbgWave[w][1])
                {
                    seen.push_back((c.dbgWave[w][1] - first) / 100.0); done.push_back((c.dbgWave[w][2] - first) / 100.0); end.push_back((c.dbgWave[w][3] - first) / 100.0);
                    busy.push_back((c.dbgWave[w][2] - c.dbgWave[w][1]) / 100.0);
                }
            {
                // who the late ones are: the relay wavefronts (wavefront 0 of workgroups 0..7), and the twelve that ended the step last
                std::vector<std::pair<double, unsigned>> byEnd;
                for (unsigned w = 0; w < nw; w++) if (c.dbgWave[w][1]) byEnd.push_back(std::make_pair((c.dbgWave[w][3] - first) / 100.0, w));
                std::sort(byEnd.begin(), byEnd.end());
                const auto show = [&](const unsigned w, const char *tag)
                {
                    size_t rank = 0;
                    for (; rank < byEnd.size() && byEnd[rank].second != w; rank++) {}
                    std::fprintf(stderr, "resident wavefront %5u (workgroup %4u wave %u) %s: waiting since %.1f, message seen %.1f, windows + records done %.1f, step end %.1f (rank %zu of %zu)\n", w, w / 4u, w % 4u, tag,
                                 (double(c.dbgWave[w][0]) - double(first)) / 100.0, (c.dbgWave[w][1] - first) / 100.0, (c.dbgWave[w][2] - first) / 100.0, (c.dbgWave[w][3] - first) / 100.0, rank + 1, byEnd.size());
                };
                for (unsigned g = 0; g < 8u && g * 4u < nw; g++) show(g * 4u, "relay");
                for (size_t i = byEnd.size() > 12 ? byEnd.size() - 12 : 0; i < byEnd.size(); i++) show(byEnd[i].second, "late ");
                for (size_t i = 0; i < 4 && i < byEnd.size(); i++) show(byEnd[i].second, "early");
            }
            const auto pct = [](std::vector<double> &v, const double p) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[size_t(p * double(v.size() - 1))]; };
            const char *what[4] = {"message seen", "windows + records done", "step end", "(windows + records alone)"};
            std::vector<double> *vs[4] = {&seen, &done, &end, &busy};
            for (int q = 0; q < 4; q++)
                std::fprintf(stderr, "resident step of %zu wavefronts, us after the first one saw the message: %-28s min %.1f  10%% %.1f  50%% %.1f  90%% %.1f  99%% %.1f  max %.1f\n", vs[q]->size(),
                             what[q], pct(*vs[q], 0.0), pct(*vs[q], 0.1), pct(*vs[q], 0.5), pct(*vs[q], 0.9), pct(*vs[q], 0.99), pct(*vs[q], 1.0));
        }
        std::fprintf(stderr, "resident host: %llu reports, %llu there at the first look, %.1f us waited per report on average; %.1f us between two receive calls on average\n",
                     (unsigned long long)R.dbgReports, (unsigned long long)R.dbgImmediate, R.dbgReports ? R.dbgWaitNs / 1e3 / double(R.dbgReports) : 0.0,
                     R.dbgCalls > 1 ? R.dbgBetweenNs / 1e3 / double(R.dbgCalls - 1) : 0.0);
    }
    {
        // the kernels' running near-threshold counters
        const StreamLayout H = headLayout(dm);
        unsigned near[2] = {0, 0};
        LORAHIP_TRY(hipMemcpy(near, dm->sDev.get() + H.oNear, sizeof(near), hipMemcpyDeviceToHost));
        foldNear(dm, near[0], near[1]);
    }
    if (lost)
    {
        setLastError("lorahip_demod_receive (resident): rows too small for a step's packets or signals -- the excess was dropped (counted in *n_packets)");
        return LORAHIP_E_INVALID;
    }
    return LORAHIP_OK;
}

/*! One step of the resident receiver. handled = false: the resident mode is not in place (yet) or not to be had for this object -- the
 * caller takes an ordinary step. *nPackets / *calls / lastSignals are those of the PREVIOUS step (0 for the first), whose rows -- the
 * ones that came with the previous call -- are complete now. */
int residentStep(lorahip_demod *dm, const float *iqDev, const size_t rowStride, const size_t nValid, const lorahip_packet_rows *rows, size_t *nPackets,
                        int64_t *calls, bool &handled)
{
    handled = false;
    Resident &R = dm->res;
    lorahip_ctx *ctx = dm->ctx;
    const size_t N = dm->N, B = dm->B;
    const bool compatible = steadyAppend(dm, rowStride, nValid) && ctx->sf >= 7 && ctx->sf <= 12 && !dm->pipe.active && rowsHold(rows, 1) &&
                            // rows of whole 128-byte lines: a step then never reads a line that holds samples which arrive later (no cache to invalidate)
                            (rowStride & 15u) == 0 && (reinterpret_cast<uintptr_t>(iqDev) & 127u) == 0;
    if (R.active && (!compatible || iqDev != dm->stepIq))
    {
        setLastError("lorahip_demod_receive (resident): a setting or the rows changed under the resident kernel (lorahip_demod_receive_flush first)");
        return LORAHIP_E_INVALID;
    }
    if (!R.active)
    {
        const bool ready = compatible && !R.unavailable && stateOnDevice(dm);
        if (!ready) return LORAHIP_OK;
        const DeviceGuard guard(ctx->device);
        // (made on first use; each is asked for at every launch, so that a call that failed half way is completed by the next)
        LORAHIP_TRY(R.ctl.grow(sizeof(ResidentCtl)));
        LORAHIP_TRY(R.host.grow(sizeof(ResidentHost), hipHostMallocMapped));
        LORAHIP_TRY(R.run.ensure(hipStreamNonBlocking));
        LORAHIP_TRY(R.ev.ensure(hipEventDisableTiming));
        // a step's records: sized for a step as long as this one (a longer one fills them, stops the channel and the next step resumes it)
        size_t cap, capPkt;
        streamCapacity(dm, nValid - dm->home.prevValid() + 2 * N, cap, capPkt);
        StreamLayout L;
        L.make(B, cap, capPkt, false, dm->carryCap, dm->wantSignals);
        // (RES_RING sets of record arrays: a step writes set step & 3 -- StreamArgs::resRecStride)
        LORAHIP_TRY(R.rec.grow(RES_RING * L.total, L.total / 4));
        R.lay = L;
        R.sigs = dm->wantSignals;
        void *hostDev = nullptr;
        LORAHIP_TRY(hipHostGetDevicePointer(&hostDev, R.host.get(), 0));
        std::memset(R.host.get(), 0, sizeof(ResidentHost));
        LORAHIP_TRY(hipMemsetAsync(R.ctl.get(), 0, std::getenv("LORAHIP_RESIDENT_DEBUG") ? sizeof(ResidentCtl) : offsetof(ResidentCtl, dbgWave), ctx->stream));
        StreamArgs a = makeStreamArgs(dm, iqDev, L, R.rec.get());
        a.uniformLen = 0;                             // (the length of a step comes with its message)
        a.flags = 4 | 8;
        a.maxBlocks = 0; a.lanes = -1;
        a.res = R.ctl.get(); a.resHost = static_cast<ResidentHost *>(hostDev); a.resWatchdog = kResidentWatchdog; a.resRecStride = L.total;
        if (const char *e = std::getenv("LORAHIP_RESIDENT_DEBUG")) a.resDebug = unsigned(std::atoi(e));     // (the step whose stamps every wavefront leaves)
        // behind everything queued on the launch stream (the state of the run before, the cleared control block)
        LORAHIP_TRY(hipEventRecord(R.ev.get(), ctx->stream));
        LORAHIP_TRY(hipStreamWaitEvent(R.run.get(), R.ev.get(), 0));
        const hipError_t le = launchStreamResident(ctx->sf, a, R.run.get(), &R.grid);
        if (le == hipErrorNotSupported) { (void)hipGetLastError(); R.unavailable = true; return LORAHIP_OK; }     // not for this geometry: ordinary steps
        LORAHIP_TRY(le);
        R.active = true; R.seq = 0; R.reported = 0; R.lastMore = false;
        R.dbgReports = R.dbgImmediate = R.dbgCalls = 0; R.dbgWaitNs = R.dbgBetweenNs = 0.0;
        R.depth = rows->reserved >= 1 ? (rows->reserved > RES_DEPTH_MAX ? unsigned(RES_DEPTH_MAX) : unsigned(rows->reserved)) : 1u;
        {
            // the census: every workgroup must be ON the device before a step is rung (bounded wait; otherwise the kernel is told to
            // leave and the object takes ordinary steps from now on)
            typedef std::chrono::steady_clock Clock;
            const Clock::time_point t0 = Clock::now();
            while (__atomic_load_n(&R.host->arrivedAll, __ATOMIC_ACQUIRE) == 0u && std::chrono::duration<double>(Clock::now() - t0).count() < 2.0) {}
            if (__atomic_load_n(&R.host->arrivedAll, __ATOMIC_ACQUIRE) == 0u)
            {
                residentAbort(dm);
                dm->home.censusFailed();              // (no step was taken: the state on the device is what it was)
                return LORAHIP_OK;
            }
        }
        dm->stepIq = iqDev; dm->stepStride = rowStride;
        dm->home.takenOver();                         // until the kernel has left, only it knows where the state stands
    }
    handled = true;
    {
        const std::chrono::steady_clock::time_point now = std::chrono::steady_clock::now();
        if (R.dbgCalls++) R.dbgBetweenNs += std::chrono::duration<double, std::nano>(now - R.dbgLast).count();
        R.dbgLast = now;
    }
    if (nPackets) *nPackets = 0;
    if (calls) *calls = 0;
    dm->lastSignals = 0;
    R.nRep = 0;
    const DeviceGuard guard(ctx->device);
    // (up to the last whole line of every row: the < 16 samples behind it wait for the next step, or for the flush's ordinary step)
    { const int rc = residentRing(dm, nValid & ~size_t(15), rows, 0u); if (rc != LORAHIP_OK) { residentAbort(dm); return rc; } }
    R.lastValid = nValid & ~size_t(15);
    R.tail = (nValid & 15u) != 0;
    noteSteadyStep(dm, rowStride, nValid);
    if (R.seq <= R.depth) return LORAHIP_OK;
    // ... and while it runs: the step `depth` calls back
    size_t pk = 0, sg = 0;
    int64_t cl = 0;
    unsigned fl = 0;
    const int rc = residentReport(dm, R.seq - R.depth, &pk, &sg, &cl, &fl);
    if (rc != LORAHIP_OK) { residentAbort(dm); return rc; }
    R.reported = R.seq - R.depth;
    R.repPk[0] = pk; R.repSg[0] = dm->sigRowsOn ? sg : 0; R.nRep = 1;
    R.lastMore = (fl & RES_F_MORE) != 0;
    dm->workCalls += cl;
    if (nPackets) *nPackets = pk;
    if (calls) *calls = cl;
    dm->lastSignals = dm->sigRowsOn ? sg : 0;
    if (fl & (RES_F_PKT_OVERFLOW | RES_F_SIG_OVERFLOW))
    {
        setLastError("lorahip_demod_receive (resident): the rows of the call before were too small for its step -- the excess was dropped (counted in *n_packets)");
        return LORAHIP_E_INVALID;
    }
    return LORAHIP_OK;
}

} } // namespace lorahip::demod
