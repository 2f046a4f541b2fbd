// Level 3, the PIPELINED receiver step (lorahip_demod_receive with async = 2). A receiver step is: streaming kernel, 72-byte summary back,
// packets packed for the decoder. Run strictly one after the other, the host's share (launch latencies, the wait for the summary,
// the packing launches: ~60 us) is exposed once per step -- half the step at chunks of 8 windows. Here step k's kernel is launched
// BEFORE step k-1's summary is read: the host waits for summary k-1 and packs step k-1's packets while kernel k runs, and the
// caller gets every packet one step later (lorahip_demod_receive_flush delivers the last step's). Nothing the host learns from
// summary k-1 is needed to launch kernel k: the per-channel state, the read positions and the open packets' symbols are on the
// device, in stream order; a channel that filled its record buffer in step k-1 is simply continued by kernel k (the kernels are
// resumable by design). The per-launch record arrays exist twice (kernel k writes one set while step k-1's are packed from the other).
#include "lorahip_demod_state.h"

namespace lorahip { namespace demod {

/*! What a pipelined or resident step needs in place, beside its own terms: the streaming kernel, no trace / ports / deferred
 * activate(), a continuing append stream over the same rows (no fewer valid samples than the step before), carry rows long enough
 * for a packet. Anything else takes the ordinary step (which establishes exactly that). */
bool steadyAppend(const lorahip_demod *dm, const size_t rowStride, const size_t nValid)
{
    return usesStreamKernel(dm) && !dm->tracing && !dm->portsOn && !dm->home.activateWaiting() && dm->sDev.get() != nullptr && dm->home.continues() &&
           dm->home.stride() == rowStride && nValid >= dm->home.prevValid() && dm->dCarry.get() != nullptr && dm->mtu + 1 <= dm->carryCap;
}

//! ... and to enter either mode: the state and the open packets' symbols on the device, no records of a launch left there
bool stateOnDevice(const lorahip_demod *dm) { return dm->home.mayEnter(dm->lastSum.anyOpen != 0, dm->pending.valid); }

//! a pipelined or resident step has been given the first nValid samples of rows rowStride apart: an append run over those rows, after
//! which the pinned copy of the state and the mirrors lag behind the device
void noteSteadyStep(lorahip_demod *dm, const size_t rowStride, const size_t nValid) { dm->home.steadyStep(rowStride, nValid); }

//! a pipelined or resident receiver has been left: the object is as a streaming run leaves it -- the state (and the open packets'
//! symbols) on the device, the pinned copy and the mirrors behind. (Its steps are not timed one by one: an event pair per step is two
//! more calls.)
void leaveStateOnDevice(lorahip_demod *dm)
{
    dm->kernelMs = 0.0;
    dm->home.givenBack();
    dm->pending.valid = false;
}

//! the n packets of a record set of layout L at `rec` into rows (stream-ordered on `st`, no wait; the rows are numbered on the device,
//! channels ascending). The scratch (growDense) has been sized by the caller.
hipError_t packPackets(const lorahip_demod *dm, const StreamLayout &L, const char *rec, const size_t n, uint16_t *syms, const size_t symStride,
                              int32_t *nsyms, int32_t *chan, lorahip_rx_info *info, hipStream_t st)
{
    const size_t nbRow = align256(L.B * sizeof(int));
    return launchPackPackets(reinterpret_cast<const StreamPacket *>(rec + L.oPkt), reinterpret_cast<const int *>(rec + L.oNPkt),
                             reinterpret_cast<const short *>(rec + L.oSym), reinterpret_cast<int *>(dm->dDense.get()), L.B, int(L.symStride), int(L.capPkt), n,
                             reinterpret_cast<long long *>(dm->dDense.get() + nbRow), syms, int(symStride), nsyms, chan, info, int(dm->N), st);
}

//! the signals of a record set of layout L at `rec` into the registered signal rows from row `first` on (stream-ordered on `st`, no wait)
hipError_t packSignals(const lorahip_demod *dm, const StreamLayout &L, const char *rec, const size_t first, hipStream_t st)
{
    const lorahip_signal_rows &R = dm->sigRows;
    return launchPackSignals(reinterpret_cast<const StreamSignal *>(rec + L.oSig), reinterpret_cast<const int *>(rec + L.oNSig), L.B, int(L.capPkt),
                             R.channel, R.error, R.power, R.snr, reinterpret_cast<long long *>(R.pos), first, R.cap, st);
}

//! summary of record set `set` into the object's books (waits for that step's kernel); its packets stay in the set until packed
static int pipeRead(lorahip_demod *dm, const int set)
{
    Pipe &P = dm->pipe;
    LORAHIP_TRY(hipEventSynchronize(P.ev[set].get()));
    P.pending[set] = false;
    const StreamSummary sum = P.hSum.get()[set];
    foldNear(dm, sum.nearSquelch, sum.nearStep);
    dm->workCalls += sum.calls;
    dm->lastSum = sum;
    P.nPk[set] = size_t(sum.packets);
    P.nCalls[set] = sum.calls;
    P.nSig[set] = P.sigs[set] ? size_t(sum.signals) : 0;
    P.held[set] = true;
    return LORAHIP_OK;
}

bool rowsHold(const lorahip_packet_rows *rows, const size_t n)
{
    return n == 0 || (rows != nullptr && rows->syms_dev != nullptr && rows->nsyms_dev != nullptr && rows->sym_stride != 0 && rows->sym_stride <= 0x7fffffffu &&
                      rows->cap_packets >= n);
}

//! do the registered signal rows hold n signals? (nothing registered: the signals are dropped, as the header says)
static bool sigRowsHold(const lorahip_demod *dm, const size_t n) { return !dm->sigRowsOn || n <= dm->sigRows.cap; }

//! the packets held in record set `set` into `rows` from row `firstRow` on, its signals into the signal rows from `firstSig` on
//! (stream-ordered; no wait); the set is free afterwards. The scratch (growDense) has been sized by the caller.
static int pipePack(lorahip_demod *dm, const int set, const lorahip_packet_rows *rows, const size_t firstRow, const size_t firstSig, const bool beside)
{
    Pipe &P = dm->pipe;
    lorahip_ctx *ctx = dm->ctx;
    const size_t n = P.nPk[set], ns = dm->sigRowsOn ? P.nSig[set] : 0;
    if (n == 0 && ns == 0) { P.held[set] = false; return LORAHIP_OK; }
    const StreamLayout &L = P.lay[set];
    // `beside`: packed on the side stream WHILE the step just launched runs (the host has just waited for this step's summary: its
    // kernel is complete). The side stream first waits for where the launch stream stood when this call began -- whatever the caller
    // queued there to read the rows of the call before (a decoder) and any earlier packing, which shares the scratch -- and the launch
    // stream then waits for the packing before anything later: the next kernel reuses this record set, the caller reads the rows.
    // Worth it for short steps only (profiles/r04/s37_*: 8-window chunks at SF7 +14 %; at 128-window chunks the packing kernels
    // displace workgroups of a streaming grid that exactly fills the device, -5 %).
    hipStream_t packStream = beside ? P.side.get() : ctx->stream;
    if (beside) LORAHIP_TRY(hipStreamWaitEvent(P.side.get(), P.entry.get(), 0));
    if (n)
        LORAHIP_TRY(packPackets(dm, L, P.dev[set].get(), n, rows->syms_dev + firstRow * rows->sym_stride, rows->sym_stride, rows->nsyms_dev + firstRow,
                                rows->channel_dev ? rows->channel_dev + firstRow : nullptr, rows->info_dev ? rows->info_dev + firstRow : nullptr, packStream));
    if (ns) LORAHIP_TRY(packSignals(dm, L, P.dev[set].get(), firstSig, packStream));
    if (beside)
    {
        LORAHIP_TRY(hipEventRecord(P.packDone.get(), P.side.get()));
        LORAHIP_TRY(hipStreamWaitEvent(ctx->stream, P.packDone.get(), 0));
    }
    P.held[set] = false;                              // only now: a launch that failed above leaves the packets where they are
    return LORAHIP_OK;
}

/*! Every step whose summary can be read (oldest first) into `rows`, or -- if they do not all fit -- NONE of them: *nPackets = the
 * rows needed, LORAHIP_E_INVALID, the packets stay in their record sets and the next call (with rows that hold them) delivers
 * them. `sets`: number of record sets to consider, oldest first (1: only the older one). The same holds for the signals and the
 * rows registered for them (lorahip_demod_receive_signal_rows): all or nothing, lorahip_demod_receive_num_signals() = what is due. */
static int pipeDeliverHeld(lorahip_demod *dm, const int older, const int sets, const lorahip_packet_rows *rows, size_t *nPackets, int64_t *calls, const bool beside)
{
    Pipe &P = dm->pipe;
    size_t need = 0, needSig = 0, most = 0;
    for (int i = 0; i < sets; i++)
        if (P.held[older ^ i]) { need += P.nPk[older ^ i]; needSig += P.nSig[older ^ i]; if (P.nPk[older ^ i] > most) most = P.nPk[older ^ i]; }
    if (nPackets) *nPackets = need;
    dm->lastSignals = dm->sigRowsOn ? needSig : 0;
    if (!rowsHold(rows, need))
    {
        setLastError("lorahip_demod_receive (pipelined): the rows cannot hold the packets that are due; they are kept -- call again with rows for *n_packets");
        return LORAHIP_E_INVALID;
    }
    if (!sigRowsHold(dm, needSig))
    {
        setLastError("lorahip_demod_receive (pipelined): the signal rows cannot hold the signals that are due; they are kept -- register rows for lorahip_demod_receive_num_signals()");
        return LORAHIP_E_INVALID;
    }
    // the scratch for the largest set, before any state is touched: a failure here delivers nothing and loses nothing
    if (most) { const int grc = growDense(dm, align256(dm->B * sizeof(int)) + most * sizeof(long long)); if (grc != LORAHIP_OK) return grc; }
    size_t at = 0, atSig = 0;
    int64_t c = 0;
    for (int i = 0; i < sets; i++)
    {
        const int set = older ^ i;
        if (!P.held[set]) continue;
        const size_t n = P.nPk[set], ns = dm->sigRowsOn ? P.nSig[set] : 0;
        const int rc = pipePack(dm, set, rows, at, atSig, beside);
        if (rc != LORAHIP_OK) return rc;
        c += P.nCalls[set];
        at += n; atSig += ns;
    }
    if (calls) *calls = c;
    return LORAHIP_OK;
}

//! leave the pipeline: the packets not delivered yet into `rows` (nullable: they are dropped), the object back in the state a streaming run leaves
int pipeFlush(lorahip_demod *dm, const lorahip_packet_rows *rows, size_t *nPackets, int64_t *calls)
{
    Pipe &P = dm->pipe;
    if (nPackets) *nPackets = 0;
    if (calls) *calls = 0;
    if (!P.active) return LORAHIP_OK;
    const DeviceGuard guard(dm->ctx->device);
    const int last = int((P.k - 1) & 1);
    for (int i = 1; i >= 0; i--)                      // oldest first: the books follow the steps in order
        if (P.k > 0 && P.pending[last ^ i]) { const int rc = pipeRead(dm, last ^ i); if (rc != LORAHIP_OK) return rc; }
    size_t n1 = 0;
    int64_t c1 = 0;
    dm->lastSignals = 0;
    if (rows == nullptr) P.held[0] = P.held[1] = false;                       // dropped on request
    else
    {
        LORAHIP_TRY(hipEventRecord(P.entry.get(), dm->ctx->stream));
        const int rc = pipeDeliverHeld(dm, last ^ 1, 2, rows, &n1, &c1, false);
        if (nPackets) *nPackets = n1;
        if (rc != LORAHIP_OK) return rc;              // (the pipeline stays entered: flush again with rows that hold *n_packets)
    }
    if (calls) *calls = c1;
    LORAHIP_TRY(hipStreamSynchronize(dm->ctx->stream));
    P.active = false;
    leaveStateOnDevice(dm);
    return LORAHIP_OK;
}

int pipeStep(lorahip_demod *dm, const float *iqDev, const size_t rowStride, const size_t nValid, const lorahip_packet_rows *rows, size_t *nPackets,
                    int64_t *calls, bool &handled)
{
    handled = false;
    Pipe &P = dm->pipe;
    lorahip_ctx *ctx = dm->ctx;
    const size_t N = dm->N, B = dm->B;
    const bool compatible = steadyAppend(dm, rowStride, nValid);
    const bool ready = compatible && stateOnDevice(dm);
    if (!P.active && !ready) return LORAHIP_OK;
    if (P.active && !compatible) { setLastError("lorahip_demod_receive (pipelined): a setting or the rows changed under a running pipeline (lorahip_demod_receive_flush first)"); return LORAHIP_E_INVALID; }
    handled = true;
    const DeviceGuard guard(ctx->device);
    if (!P.active)
    {
        // (made on first use; each is asked for every time a pipeline is entered, so that a call that failed half way is completed by the next)
        LORAHIP_TRY(P.hSum.grow(2 * sizeof(StreamSummary), hipHostMallocMapped));
        for (int i = 0; i < 2; i++) LORAHIP_TRY(P.ev[i].ensure(hipEventDisableTiming));
        LORAHIP_TRY(P.packDone.ensure(hipEventDisableTiming));
        LORAHIP_TRY(P.entry.ensure(hipEventDisableTiming));
        LORAHIP_TRY(P.side.ensure(hipStreamNonBlocking));
        P.active = true; P.k = 0; P.pending[0] = P.pending[1] = false; P.held[0] = P.held[1] = false;
        dm->home.takenOver();                         // until the pipeline is flushed, only it knows where the state stands
    }
    const int set = int(P.k & 1);
    if (nPackets) *nPackets = 0;
    if (calls) *calls = 0;
    // where the launch stream stands now: behind whatever the caller queued to read the rows of the call before (pipePack)
    LORAHIP_TRY(hipEventRecord(P.entry.get(), ctx->stream));
    bool delivered = false;
    dm->lastSignals = 0;
    if (P.held[set] || P.held[set ^ 1])
    {
        // A call before could not hand over the packets of a step (rows too small). If they sit in THIS record set the kernel about to
        // be launched would overwrite them; if in the other one (a flush that failed on small rows left the last step's there) they are
        // simply older than anything this call produces. Either way they are due now, oldest first, together with the packets of a step
        // launched since -- or nothing is launched and nothing is lost (the caller comes back with rows for *n_packets; the samples
        // wait in its array).
        const int older = P.held[set] ? set : (set ^ 1);
        if (P.pending[older ^ 1]) { const int rc = pipeRead(dm, older ^ 1); if (rc != LORAHIP_OK) return rc; }
        const int rc = pipeDeliverHeld(dm, older, 2, rows, nPackets, calls, false);
        if (rc != LORAHIP_OK) return rc;
        delivered = true;
    }
    const size_t prevValid = dm->home.prevValid();
    size_t cap, capPkt;
    streamCapacity(dm, nValid - prevValid + 2 * N, cap, capPkt);
    StreamLayout L;
    L.make(B, cap, capPkt, false, dm->carryCap, dm->wantSignals);
    // (this set's last use, step k - 2, was packed during step k - 1's call, stream-ordered before kernel k - 1: freeing waits for it)
    LORAHIP_TRY(P.dev[set].grow(L.total, L.total / 4));
    P.lay[set] = L;
    StreamArgs a = makeStreamArgs(dm, iqDev, L, P.dev[set].get());
    a.uniformLen = (long long)nValid;
    a.flags = 4 | 8;                                  // continue the streams; open packets in from / out to the carry rows
    // the block's signals (:267-269), kept per step like the packets and delivered with them one step late
    P.sigs[set] = dm->wantSignals;
    // four calls per step: the kernel, its summary (written straight into pinned host memory), the event the next call waits on -- and
    // the previous step's packing below. (The summary on a stream of its own, behind the kernel's event and beside the NEXT step's kernel
    // -- it reads only this record set's counts and end words -- was measured: two more API calls and the hand-over between the streams
    // cost more than the 11 us the next kernel would no longer queue behind, 93 -> 108 us per 8-window step at SF7; profiles/r05/s36_*.)
    LORAHIP_TRY(launchStream(ctx->sf, a, ctx->stream));
    LORAHIP_TRY(launchStreamSummary(a.end, a.nCalls, a.nSym, a.nPkt, dm->wantSignals ? a.nSig : nullptr, B, int(cap), int(capPkt), a.near, dm->dSumScratch.get(), P.hSum.get() + set, ctx->stream));
    LORAHIP_TRY(hipEventRecord(P.ev[set].get(), ctx->stream));
    P.pending[set] = true;
    P.k++;
    dm->stepIq = iqDev; dm->stepStride = rowStride;
    noteSteadyStep(dm, rowStride, nValid);
    // ... and while it runs: the step before
    if (delivered || P.k < 2 || !P.pending[set ^ 1]) return LORAHIP_OK;
    { const int rc = pipeRead(dm, set ^ 1); if (rc != LORAHIP_OK) return rc; }
    const bool shortStep = (nValid - prevValid) <= 48 * N;    // (the step launched above)
    return pipeDeliverHeld(dm, set ^ 1, 1, rows, nPackets, calls, shortStep);
}

} } // namespace lorahip::demod
