// Level 3 of the C ABI: B channels of the LoRaDemod block driven in lock-step -- the C entry points.
//
// Mirrors LoRaDemod.cpp: parameters and defaults (:68-74), setters (:124-137), activate() (:139-143) and work() (:145-327), which
// is one of two things: the streaming kernels with the frame machine on the device (lorahip_demod_stream.cpp; a receiver's steps
// also pipelined, lorahip_demod_pipe.cpp, or resident, lorahip_demod_resident.cpp) or host-driven rounds over the batch kernels
// (lorahip_demod_rounds.cpp). The debug ports, the trace and its labels: lorahip_demod_ports.cpp. What the units share:
// lorahip_demod_state.h.
//
// The three members the reference leaves uninitialised (_finefreqError, _freqError, _prevValue) start at zero here.
#include "lorahip_demod_state.h"
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace lorahip;
using namespace lorahip::demod;

namespace lorahip { namespace demod {

//! the next run's streams: channel c's n[c] samples from sample baseOf(c) of the device buffer on, each a new stream
template <class BaseOf> static void placeSegments(lorahip_demod *dm, const size_t *n, const BaseOf &baseOf)
{
    dm->home.placedSegments();
    for (size_t c = 0; c < dm->B; c++)
    {
        Channel &k = dm->ch[c];
        k.base = baseOf(c); k.len = n[c]; k.pos = 0; k.callCount = 0;
    }
}

static int runAny(lorahip_demod *dm, const float *iqDev, int64_t *roundsOut)
{
    const bool stream = usesStreamKernel(dm);
    if (stream && !streamAvailable(dm->ctx->sf)) { setLastError("no streaming kernel for this SF"); return LORAHIP_E_INVALID; }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    { const int rc = drainPending(dm); if (rc != LORAHIP_OK) return rc; }       // the previous run's records, if still on the device
    // the port replay reads the per-call trace; a trace the caller did not ask for lives for this run only (it must neither grow
    // without bound in a long-running receiver nor show up in lorahip_demod_get_trace / _trace_len / _get_labels)
    const bool internalTrace = dm->portsOn && !dm->userTracing;
    const bool cont = dm->home.continues();
    if (internalTrace || (dm->portsOn && cont)) { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }
    if (internalTrace) for (auto &k : dm->ch) { k.trace.clear(); k.traceSymCount0 = k.symCount; }
    if (dm->portsOn) for (auto &k : dm->ch) k.runStart = cont ? k.pos : 0;      // where the port replay starts reading
    dm->tracing = dm->userTracing || dm->portsOn;
    if (dm->tracing || dm->portCountsDirty)
    {
        for (auto &k : dm->ch) { k.traceStart = k.trace.size(); k.portFft = k.portDec = k.portRaw = 0; }
        dm->portCountsDirty = dm->portsOn;                       // a run without ports leaves them at zero: nothing to reset next time
    }
    if (!stream) { dm->kernelMs = 0.0; dm->lastLaunches = 0; }       // what the accessors say of a host-driven run
    int rc = stream ? runStream(dm, iqDev, roundsOut) : runRounds(dm, iqDev, roundsOut);
    if (rc == LORAHIP_OK && dm->portsOn) rc = fillPorts(dm, iqDev);
    if (rc == LORAHIP_OK) dm->home.runCompleted();                      // the next append run continues this one
    if (internalTrace) for (auto &k : dm->ch) { std::vector<lorahip_work_result>().swap(k.trace); k.traceStart = 0; }
    return rc;
}

//! accessors of the host queue first bring over what the last streaming launch left on the device; a failure there is the
//! accessor's failure (the records stay pending, see drainPending)
int drained(const lorahip_demod *dm)
{
    lorahip_demod *m = const_cast<lorahip_demod *>(dm);
    if (m && m->comp) return LORAHIP_OK;                        // the parts drain their own
    if (m) { const int rc = refuseWhilePiped(m); if (rc != LORAHIP_OK) return rc; }
    return m ? drainPending(m) : LORAHIP_E_INVALID;
}

} } // namespace lorahip::demod

namespace lorahip {
void demodSetCoResidentWaves(lorahip_demod *dm, const unsigned waves) { if (dm != nullptr && dm->comp == nullptr) dm->coWaves = waves; }
}

extern "C" {

int lorahip_demod_create(lorahip_demod **out, const int device, const int sf, const size_t n_channels)
{
    if (out == nullptr || n_channels == 0 || n_channels > 0x7fffffffu) return LORAHIP_E_INVALID;
    *out = nullptr;
    lorahip_demod *dm = new (std::nothrow) lorahip_demod();
    if (dm == nullptr) return LORAHIP_E_NOMEM;
    int rc = lorahip_create(&dm->ctx, device, sf);
    if (rc != LORAHIP_OK) { const std::string e = lorahip_last_error(); lorahip_demod_destroy(dm); setLastError(e); return rc; }
    dm->N = size_t(1) << sf;
    dm->B = n_channels;
    try { dm->ch.resize(n_channels); }                              // (value-initialised too: every count and position zero)
    catch (const std::bad_alloc &) { lorahip_demod_destroy(dm); return LORAHIP_E_NOMEM; }
    const size_t stageBytes = roundStagingBytes(n_channels), sumBytes = streamSummaryScratchBytes(n_channels);
    hipError_t e;
    {
        const DeviceGuard guard(device);                    // lorahip_create() restored the caller's device: allocate on OURS
        e = regrowPair(dm->d, stageBytes, dm->h, stageBytes, hipHostMallocDefault);
        // (more than 32768 channels: the summary of a streaming launch is reduced by one workgroup per 4096 of them and a second launch)
        if (e == hipSuccess && n_channels > 32768) e = dm->dSumScratch.grow(sumBytes);
        if (e == hipSuccess && n_channels > 32768) e = hipMemset(dm->dSumScratch.get(), 0, sumBytes);
    }
    if (e != hipSuccess) { lorahip_demod_destroy(dm); return LORAHIP_E_NOMEM; }
    lorahip_demod_activate(dm);
    *out = dm;
    return LORAHIP_OK;
}

int lorahip_demod_create_mixed(lorahip_demod **out, const int *devices, const size_t n_devices, const int32_t *channel_sf, const size_t n_channels)
{
    if (out == nullptr) return LORAHIP_E_INVALID;
    *out = nullptr;
    Composite *k = nullptr;
    const int rc = Composite::create(&k, devices, n_devices, channel_sf, n_channels);
    if (rc != LORAHIP_OK) return rc;
    lorahip_demod *dm = new (std::nothrow) lorahip_demod();         // value-initialised: every pointer null
    if (dm == nullptr) { delete k; return LORAHIP_E_NOMEM; }
    dm->comp = k;
    dm->B = n_channels;
    *out = dm;
    return LORAHIP_OK;
}

size_t lorahip_demod_num_channels(const lorahip_demod *dm) { return dm ? dm->B : 0; }
size_t lorahip_demod_num_parts(const lorahip_demod *dm) { return dm == nullptr ? 0 : (dm->comp ? dm->comp->numParts() : 1); }

int lorahip_demod_part(const lorahip_demod *dm, const size_t i, int32_t *device, int32_t *sf, size_t *n_channels, int32_t *device_slot)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->partInfo(i, device, sf, n_channels, device_slot);
    if (i != 0) return LORAHIP_E_INVALID;
    if (device) *device = dm->ctx->device;
    if (sf) *sf = dm->ctx->sf;
    if (n_channels) *n_channels = dm->B;
    if (device_slot) *device_slot = 0;
    return LORAHIP_OK;
}

int lorahip_demod_part_of(const lorahip_demod *dm, int32_t *part_of_channel, int32_t *local_channel)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->partOf(part_of_channel, local_channel);
    for (size_t c = 0; c < dm->B; c++) { if (part_of_channel) part_of_channel[c] = 0; if (local_channel) local_channel[c] = int32_t(c); }
    return LORAHIP_OK;
}

lorahip_demod *lorahip_demod_part_handle(const lorahip_demod *dm, const size_t i)
{
    if (dm == nullptr) return nullptr;
    if (dm->comp) return dm->comp->part(i);
    return i == 0 ? const_cast<lorahip_demod *>(dm) : nullptr;
}

void lorahip_demod_destroy(lorahip_demod *dm)
{
    if (dm == nullptr) return;
    if (dm->comp) { delete dm->comp; delete dm; return; }
    lorahip_ctx *ctx = dm->ctx;
    {
        const DeviceGuard guard(ctx ? ctx->device : 0);           // the caller's current device is restored on return
        if (ctx) (void)hipStreamSynchronize(ctx->stream);         // a pipelined step may still be writing into what is released below
        residentAbort(dm);                                        // a resident kernel must leave before its memory goes
        if (dm->pipe.side.get()) (void)hipStreamSynchronize(dm->pipe.side.get());
        delete dm;                                                // inside the guard: the members release with the object's device current
    }
    lorahip_destroy(ctx);                                         // last: its stream outlives everything that was ordered on it
}

int lorahip_demod_set_sync(lorahip_demod *dm, const unsigned char sync)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setSync(sync);
    dm->sync = sync;
    return LORAHIP_OK;
}

int lorahip_demod_set_threshold(lorahip_demod *dm, const double thresh_dB)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setThreshold(thresh_dB);
    dm->thresh = float(thresh_dB);
    return LORAHIP_OK;
}

int lorahip_demod_set_mtu(lorahip_demod *dm, const size_t mtu)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setMtu(mtu);
    dm->mtu = mtu;
    return LORAHIP_OK;
}

int lorahip_demod_set_mode(lorahip_demod *dm, const int mode)
{
    if (dm == nullptr || mode < 0 || mode > 2) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setMode(mode);
    dm->mode = mode;
    return LORAHIP_OK;
}

// (A streaming run leaves nothing in flight: the open packets' symbols are saved by the streaming kernel itself and the run ends with
// its stream drained, so moving the object to another stream needs no ordering. A PIPELINED step is in flight by design: refused.)
int lorahip_demod_set_stream(lorahip_demod *dm, void *hip_stream)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setStream(hip_stream);
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }     // the step in flight is ordered on the stream it was launched on
    return lorahip_set_stream(dm->ctx, hip_stream);
}

// What has been queued on the object's launch stream so far -- packing kernels of an async receive, a pipelined step -- before
// anything queued on `hip_stream` from now on. Allowed while a pipelined step is in flight (it is how a consumer on another stream
// reads that mode's rows).
int lorahip_demod_stream_wait(lorahip_demod *dm, void *hip_stream)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->streamWait(hip_stream);
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(dm->evJoin.ensure(hipEventDisableTiming));
    LORAHIP_TRY(hipEventRecord(dm->evJoin.get(), dm->ctx->stream));
    LORAHIP_TRY(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), dm->evJoin.get(), 0));
    return LORAHIP_OK;
}

// ... and the other direction: the launch stream behind what `hip_stream` holds now (the producer of the samples, the consumer of rows
// that the next step will overwrite), without a host wait.
int lorahip_demod_stream_follow(lorahip_demod *dm, void *hip_stream)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->streamFollow(hip_stream);
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(dm->evJoin.ensure(hipEventDisableTiming));
    LORAHIP_TRY(hipEventRecord(dm->evJoin.get(), reinterpret_cast<hipStream_t>(hip_stream)));
    LORAHIP_TRY(hipStreamWaitEvent(dm->ctx->stream, dm->evJoin.get(), 0));
    return LORAHIP_OK;
}

int lorahip_demod_reset_stream(lorahip_demod *dm)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->resetStream();
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    return lorahip_reset_stream(dm->ctx);
}

int lorahip_demod_set_variant(lorahip_demod *dm, const int variant)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    // level 3 promises the reference block's packets, traces and ports: only kernels on the reference's operation graph qualify
    if (variant == LORAHIP_VARIANT_FMA) { setLastError("the contracted kernels (LORAHIP_VARIANT_FMA) are not offered at level 3: their bins are not the reference's"); return LORAHIP_E_INVALID; }
    if (dm->comp)
    {
        for (size_t i = 0; i < dm->comp->numParts(); i++) { const int rc = lorahip_demod_set_variant(dm->comp->part(i), variant); if (rc != LORAHIP_OK) return rc; }
        return LORAHIP_OK;
    }
    return lorahip_set_variant(dm->ctx, variant);
}

int lorahip_demod_set_stream_grid(lorahip_demod *dm, const int max_workgroups)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp)
    {
        for (size_t i = 0; i < dm->comp->numParts(); i++) { const int rc = lorahip_demod_set_stream_grid(dm->comp->part(i), max_workgroups); if (rc != LORAHIP_OK) return rc; }
        return LORAHIP_OK;
    }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    dm->streamGrid = max_workgroups;
    return LORAHIP_OK;
}

int lorahip_demod_set_stream_lanes(lorahip_demod *dm, const int log2_lanes)
{
    if (dm == nullptr || (log2_lanes > 6 && (log2_lanes < (LORAHIP_LANES_AHEAD | 3) || log2_lanes > (LORAHIP_LANES_AHEAD | 5)))) return LORAHIP_E_INVALID;
    if (dm->comp)
    {
        for (size_t i = 0; i < dm->comp->numParts(); i++) { const int rc = lorahip_demod_set_stream_lanes(dm->comp->part(i), log2_lanes); if (rc != LORAHIP_OK) return rc; }
        return LORAHIP_OK;
    }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    dm->streamLanes = log2_lanes;
    return LORAHIP_OK;
}

int lorahip_demod_stream_lanes(const lorahip_demod *dm)
{
    if (dm == nullptr || dm->comp) return LORAHIP_E_INVALID;
    const DeviceGuard guard(dm->ctx->device);
    return streamLanesChosen(dm->ctx->sf, unsigned(dm->B), dm->streamLanes, dm->coWaves);
}

int lorahip_demod_set_record_capacity(lorahip_demod *dm, const size_t max_calls_per_launch)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp)
    {
        for (size_t i = 0; i < dm->comp->numParts(); i++) { const int rc = lorahip_demod_set_record_capacity(dm->comp->part(i), max_calls_per_launch); if (rc != LORAHIP_OK) return rc; }
        return LORAHIP_OK;
    }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    dm->streamCapMax = max_calls_per_launch;
    return LORAHIP_OK;
}

int lorahip_demod_set_fine_gather(lorahip_demod *dm, const int enable)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setFineGather(enable);
    return lorahip_set_fine_gather(dm->ctx, enable);
}

int lorahip_demod_activate(lorahip_demod *dm)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->activate();
    // activate() resets only _state and _chirpTable (:139-143); everything else keeps the
    // constructor / zero state, or whatever the previous activation left. While the state lives on the device (streaming mode)
    // the reset travels with the next launch as a flag; the mirrors get it when they are next brought up to date.
    if (dm->home.deviceCurrent()) dm->home.activateDeferred();
    else
    {
        const int rc = syncMirrors(dm);
        if (rc != LORAHIP_OK) return rc;
        for (auto &k : dm->ch) { k.state = ST_FRAMESYNC; k.downTable = false; }
    }
    dm->nNearSquelch = dm->nNearStep = 0;
    return LORAHIP_OK;
}

int lorahip_demod_run_device(lorahip_demod *dm, const float *iq_dev, const size_t samples_per_channel, int64_t *rounds)
{
    if (dm == nullptr || iq_dev == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) { setLastError("lorahip_demod_run_device: an object made by lorahip_demod_create_mixed takes per-channel segments"); return LORAHIP_E_INVALID; }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }         // before anything of the object changes
    // n_channels streams of equal length back to back: the placement is two numbers, not 3 * n_channels (ch[].base / len / pos are
    // filled only for the paths that read them, applyGeometry)
    dm->home.placedUniform(samples_per_channel, samples_per_channel, false);
    return runAny(dm, iq_dev, rounds);
}

int lorahip_demod_run_device_append(lorahip_demod *dm, const float *iq_dev, const size_t row_stride, const size_t n_valid, int64_t *rounds)
{
    if (dm == nullptr || n_valid > row_stride || (n_valid && iq_dev == nullptr)) return LORAHIP_E_INVALID;
    if (dm->comp) { setLastError("append runs are per part: lorahip_demod_part_handle"); return LORAHIP_E_INVALID; }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->home.appendBegun() && n_valid < dm->home.prevValid()) { setLastError("an append run was given fewer samples than the one before it (lorahip_demod_rewind starts a new stream)"); return LORAHIP_E_INVALID; }
    // every channel's stream is the first n_valid samples of its row; a channel continues at its own read position (the device's
    // copy of the state holds it: nothing is uploaded per run)
    dm->home.placedUniform(n_valid, row_stride, true);
    return runAny(dm, iq_dev, rounds);
}

int lorahip_demod_rewind(lorahip_demod *dm)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) { for (size_t i = 0; i < dm->comp->numParts(); i++) (void)lorahip_demod_rewind(dm->comp->part(i)); return LORAHIP_OK; }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    dm->home.rewound();
    return LORAHIP_OK;
}

int lorahip_demod_run_device_segments(lorahip_demod *dm, const float *iq_dev, const int64_t *first_sample, const size_t *n_samples, int64_t *rounds)
{
    if (dm == nullptr || first_sample == nullptr || n_samples == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->runSegments(&iq_dev, 1, first_sample, n_samples, rounds);
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    bool any = false;
    for (size_t c = 0; c < dm->B; c++)
    {
        if (first_sample[c] < 0 || n_samples[c] > size_t(0x7fffffffffffffffLL) - size_t(first_sample[c])) return LORAHIP_E_INVALID;
        any = any || n_samples[c] != 0;
    }
    if (any && iq_dev == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(dm->ctx->device);
    placeSegments(dm, n_samples, [&](const size_t c) { return size_t(first_sample[c]); });
    return runAny(dm, iq_dev, rounds);
}

int lorahip_demod_run(lorahip_demod *dm, const float *const *streams, const size_t *n_samples, int64_t *rounds)
{
    if (dm == nullptr || streams == nullptr || n_samples == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp)
    {
        for (size_t c = 0; c < dm->B; c++) if (n_samples[c] && streams[c] == nullptr) return LORAHIP_E_INVALID;
        return dm->comp->run(streams, n_samples, rounds);
    }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    const DeviceGuard guard(dm->ctx->device);
    // every argument is checked before anything of the object changes: a refused call leaves consumed() of the last run intact
    for (size_t c = 0; c < dm->B; c++)
        if ((n_samples[c] && streams[c] == nullptr) || n_samples[c] > (size_t(1) << 48)) return LORAHIP_E_INVALID;
    size_t total = 0;
    for (size_t c = 0; c < dm->B; c++) total += n_samples[c];
    LORAHIP_TRY(dm->dIq.grow(total * sizeof(cf32)));
    total = 0;
    placeSegments(dm, n_samples, [&](const size_t c) { const size_t at = total; total += n_samples[c]; return at; });     // back to back
    {
        // the channels' buffers gathered into one device array back to back (base = running total): pinned double-buffered upload
        std::vector<const void *> src(dm->B);
        std::vector<size_t> len(dm->B);
        for (size_t c = 0; c < dm->B; c++) { src[c] = streams[c]; len[c] = n_samples[c] * sizeof(cf32); }
        const int rc = gatherUpload(dm->ctx, dm->dIq.get(), src.data(), len.data(), dm->B);
        if (rc != LORAHIP_OK) return rc;
    }
    LORAHIP_TRY(hipStreamSynchronize(dm->ctx->stream));
    return runAny(dm, dm->dIq.get(), rounds);
}

/* Host buffers that are the ROWS of one block of host memory -- channel c's n_samples[c] samples begin at sample first_sample[c] of
 * row c, row_stride samples per row: what a framework hands a block whose input buffer manager carves every port's slabs out of one
 * pinned allocation (lora_sdr_amd/pothos/LoRaDemodBatch.cpp::getInputBufferManager, the counterpart of LoRaDemod.cpp:346-357). The
 * span of the rows that holds samples crosses PCIe as ONE strided copy straight from the caller's memory (pinned: a plain DMA, no
 * staging, no per-channel call), and the run reads its per-channel segments of the device copy. */
int lorahip_demod_run_host_rows(lorahip_demod *dm, const float *rows, const size_t row_stride, const int64_t *first_sample, const size_t *n_samples, int64_t *rounds)
{
    if (dm == nullptr || first_sample == nullptr || n_samples == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp)
    {
        // one part holds every channel in order: its rows are the caller's; several parts take their channels' buffers one by one
        if (dm->comp->numParts() == 1) return lorahip_demod_run_host_rows(dm->comp->part(0), rows, row_stride, first_sample, n_samples, rounds);
        try
        {
            std::vector<const float *> ptr(dm->B);
            for (size_t c = 0; c < dm->B; c++)
            {
                if (first_sample[c] < 0 || size_t(first_sample[c]) > row_stride || n_samples[c] > row_stride - size_t(first_sample[c])) return LORAHIP_E_INVALID;
                ptr[c] = rows ? rows + 2 * (c * row_stride + size_t(first_sample[c])) : nullptr;
            }
            return lorahip_demod_run(dm, ptr.data(), n_samples, rounds);
        }
        catch (const std::bad_alloc &) { setLastError("out of host memory"); return LORAHIP_E_NOMEM; }
    }
    { const int rc = refuseWhilePiped(dm); if (rc != LORAHIP_OK) return rc; }
    size_t lo = row_stride, hi = 0;
    for (size_t c = 0; c < dm->B; c++)
    {
        if (first_sample[c] < 0 || size_t(first_sample[c]) > row_stride || n_samples[c] > row_stride - size_t(first_sample[c])) return LORAHIP_E_INVALID;
        if (n_samples[c] == 0) continue;
        lo = size_t(first_sample[c]) < lo ? size_t(first_sample[c]) : lo;
        hi = size_t(first_sample[c]) + n_samples[c] > hi ? size_t(first_sample[c]) + n_samples[c] : hi;
    }
    const size_t width = hi > lo ? hi - lo : 0;
    if (width && rows == nullptr) return LORAHIP_E_INVALID;
    if (width > (size_t(1) << 40) / (dm->B ? dm->B : 1)) return LORAHIP_E_INVALID;
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(dm->dIq.grow(dm->B * width * sizeof(cf32)));
    if (width)
        LORAHIP_TRY(hipMemcpy2DAsync(dm->dIq.get(), width * sizeof(cf32), rows + 2 * lo, row_stride * sizeof(cf32), width * sizeof(cf32), dm->B, hipMemcpyHostToDevice,
                                     dm->ctx->stream));
    placeSegments(dm, n_samples, [&](const size_t c) { return n_samples[c] ? c * width + (size_t(first_sample[c]) - lo) : 0; });
    return runAny(dm, dm->dIq.get(), rounds);               // (in stream order behind the copy; returns with the stream drained: the rows are the caller's again)
}

int lorahip_demod_run_device_segments_multi(lorahip_demod *dm, const float *const *iq_dev, const size_t n_devices, const int64_t *first_sample,
                                            const size_t *n_samples, int64_t *rounds)
{
    if (dm == nullptr || iq_dev == nullptr || first_sample == nullptr || n_samples == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->runSegments(iq_dev, n_devices, first_sample, n_samples, rounds);
    if (n_devices != 1) return LORAHIP_E_INVALID;
    return lorahip_demod_run_device_segments(dm, iq_dev[0], first_sample, n_samples, rounds);
}

size_t lorahip_demod_num_packets(const lorahip_demod *dm)
{
    if (dm == nullptr) return 0;
    if (dm->comp) return dm->comp->numPackets();
    const PendingLaunch &P = dm->pending;
    return dm->packets.size() + (P.valid ? P.packets : 0);      // known from the per-channel counts: no drain needed
}

int lorahip_demod_get_packet(const lorahip_demod *dm, const size_t i, int32_t *channel, int64_t *round,
                             size_t *len, int16_t *out, const size_t cap)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->comp) return dm->comp->getPacket(i, channel, round, len, out, cap);
    if (dm == nullptr || i >= dm->packets.size()) return LORAHIP_E_INVALID;
    const Packet &p = dm->packets[i];
    if (channel) *channel = p.channel;
    if (round) *round = p.round;
    if (len) *len = p.len;
    if (out)
    {
        if (cap < p.len) return LORAHIP_E_INVALID;
        std::memcpy(out, dm->pktSyms.data() + p.off, p.len * sizeof(int16_t));
    }
    return LORAHIP_OK;
}

size_t lorahip_demod_num_packet_symbols(const lorahip_demod *dm)
{
    if (dm == nullptr) return 0;
    if (dm->comp) return dm->comp->numPacketSymbols();
    const PendingLaunch &P = dm->pending;
    return dm->pktSyms.size() + (P.valid ? P.packetSyms : 0);
}

int lorahip_demod_get_packets(const lorahip_demod *dm, int32_t *channels, int64_t *rounds, int64_t *lens, const size_t cap_packets,
                              int16_t *syms, const size_t cap_syms)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->comp) return dm->comp->getPackets(channels, rounds, lens, cap_packets, syms, cap_syms);
    if (dm == nullptr || cap_packets < dm->packets.size() || cap_syms < dm->pktSyms.size()) return LORAHIP_E_INVALID;
    size_t o = 0;
    for (size_t i = 0; i < dm->packets.size(); i++)
    {
        const Packet &p = dm->packets[i];
        if (channels) channels[i] = p.channel;
        if (rounds) rounds[i] = p.round;
        if (lens) lens[i] = int64_t(p.len);
        if (syms) std::memcpy(syms + o, dm->pktSyms.data() + p.off, p.len * sizeof(int16_t));
        o += p.len;
    }
    return LORAHIP_OK;
}

int lorahip_demod_get_packets_info(const lorahip_demod *dm, lorahip_rx_info *out, const size_t cap)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->comp) return dm->comp->getPacketsInfo(out, cap);
    if (dm == nullptr || out == nullptr || cap < dm->packets.size()) return LORAHIP_E_INVALID;
    for (size_t i = 0; i < dm->packets.size(); i++)
    {
        const Packet &p = dm->packets[i];
        out[i] = rxInfo(p.endPos, (long long)p.len, p.freqError, (long long)dm->N);
    }
    return LORAHIP_OK;
}

static int packetsToDevice(lorahip_demod *dm, uint16_t *syms_dev, const size_t sym_stride, int32_t *nsyms_dev, int32_t *channel_dev,
                           lorahip_rx_info *info_dev, const size_t cap_packets, size_t *n_packets, const bool sync)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->packetsToDevice(syms_dev, sym_stride, nsyms_dev, channel_dev, info_dev, cap_packets, n_packets);   // (always complete on return)
    {
        // The records of the last streaming launch are still on the device and nothing else is queued: pack them there
        // (rows: channels ascending, time ascending inside a channel). A channel that entered the launch inside a packet found
        // its symbols at the head of its row (carryLoad); only a run that had to take them from the mirrors (anyCarryIn: packets
        // longer than the carry rows, launches of a resumed run) takes the queue path below.
        PendingLaunch &Q = dm->pending;
        if (Q.valid && dm->packets.empty() && !Q.anyCarryIn)
        {
            const size_t n = Q.packets;
            if (n_packets) *n_packets = n;
            if (n == 0) return LORAHIP_OK;
            if (syms_dev == nullptr || nsyms_dev == nullptr || sym_stride == 0 || sym_stride > 0x7fffffffu || cap_packets < n) return LORAHIP_E_INVALID;
            const DeviceGuard guard(dm->ctx->device);
            { const int grc = growDense(dm, align256(Q.lay.B * sizeof(int)) + n * sizeof(long long)); if (grc != LORAHIP_OK) return grc; }
            hipStream_t st = dm->ctx->stream;
            // the rows are numbered on the device (scanDescribe: exclusive prefix sum of the per-channel packet counts): nothing is
            // uploaded, and nothing on the host is reused, so the caller decides whether to wait
            LORAHIP_TRY(packPackets(dm, Q.lay, dm->sDev.get(), n, syms_dev, sym_stride, nsyms_dev, channel_dev, info_dev, st));
            if (sync) LORAHIP_TRY(hipStreamSynchronize(st));
            return LORAHIP_OK;
        }
    }
    { const int rc = drainPending(dm); if (rc != LORAHIP_OK) return rc; }
    const size_t P = dm->packets.size();
    if (n_packets) *n_packets = P;
    if (P == 0) return LORAHIP_OK;
    if (syms_dev == nullptr || nsyms_dev == nullptr || sym_stride == 0 || cap_packets < P) return LORAHIP_E_INVALID;
    const DeviceGuard guard(dm->ctx->device);
    const size_t nbSym = align256(P * sym_stride * sizeof(uint16_t)), nbInt = align256(P * sizeof(int32_t));
    const size_t nbInfo = info_dev ? align256(P * sizeof(lorahip_rx_info)) : 0;
    { const int grc = growDense(dm, nbSym + 2 * nbInt + nbInfo); if (grc != LORAHIP_OK) return grc; }
    lorahip_rx_info *hi = reinterpret_cast<lorahip_rx_info *>(dm->hDense.get() + nbSym + 2 * nbInt);
    uint16_t *hs = reinterpret_cast<uint16_t *>(dm->hDense.get());
    int32_t *hn = reinterpret_cast<int32_t *>(dm->hDense.get() + nbSym), *hc = reinterpret_cast<int32_t *>(dm->hDense.get() + nbSym + nbInt);
    std::memset(hs, 0, P * sym_stride * sizeof(uint16_t));
    for (size_t i = 0; i < P; i++)
    {
        const Packet &p = dm->packets[i];
        std::memcpy(hs + i * sym_stride, dm->pktSyms.data() + p.off, (p.len < sym_stride ? p.len : sym_stride) * sizeof(uint16_t));
        hn[i] = int32_t(p.len > 0x7fffffffu ? 0x7fffffff : p.len);     // the true length: a packet longer than the stride is flagged by the decoder
        hc[i] = p.channel;
        if (info_dev) hi[i] = rxInfo(p.endPos, (long long)p.len, p.freqError, (long long)dm->N);
    }
    hipStream_t st = dm->ctx->stream;
    LORAHIP_TRY(hipMemcpyAsync(syms_dev, hs, P * sym_stride * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    LORAHIP_TRY(hipMemcpyAsync(nsyms_dev, hn, P * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (channel_dev) LORAHIP_TRY(hipMemcpyAsync(channel_dev, hc, P * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (info_dev) LORAHIP_TRY(hipMemcpyAsync(info_dev, hi, P * sizeof(lorahip_rx_info), hipMemcpyHostToDevice, st));
    LORAHIP_TRY(hipStreamSynchronize(st));                              // the pinned scratch is reused by the next run
    return LORAHIP_OK;
}

int lorahip_demod_packets_to_device(lorahip_demod *dm, uint16_t *syms_dev, const size_t sym_stride, int32_t *nsyms_dev, int32_t *channel_dev,
                                    const size_t cap_packets, size_t *n_packets)
{
    return packetsToDevice(dm, syms_dev, sym_stride, nsyms_dev, channel_dev, nullptr, cap_packets, n_packets, true);
}

int lorahip_demod_packets_to_device_info(lorahip_demod *dm, uint16_t *syms_dev, const size_t sym_stride, int32_t *nsyms_dev, int32_t *channel_dev,
                                         lorahip_rx_info *info_dev, const size_t cap_packets, size_t *n_packets)
{
    return packetsToDevice(dm, syms_dev, sym_stride, nsyms_dev, channel_dev, info_dev, cap_packets, n_packets, true);
}

} // extern "C"

namespace lorahip {
int demodPacketsToDeviceQueued(lorahip_demod *dm, uint16_t *symsDev, const size_t symStride, int32_t *nsymsDev, int32_t *channelDev, lorahip_rx_info *infoDev,
                               const size_t capPackets, size_t *nPackets, const int32_t *globalOf, const size_t nLocal)
{
    if (dm == nullptr || dm->comp) return LORAHIP_E_INVALID;
    size_t n = 0;
    const int rc = packetsToDevice(dm, symsDev, symStride, nsymsDev, channelDev, infoDev, capPackets, &n, false);
    if (nPackets) *nPackets = n;
    if (rc != LORAHIP_OK || n == 0 || channelDev == nullptr || globalOf == nullptr) return rc;
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(launchRemapChannels(channelDev, globalOf, n, nLocal, dm->ctx->stream));     // (behind the rows on the same stream, whichever path wrote them)
    return LORAHIP_OK;
}

int demodStreamSync(lorahip_demod *dm)
{
    if (dm == nullptr || dm->comp) return LORAHIP_E_INVALID;
    const DeviceGuard guard(dm->ctx->device);
    LORAHIP_TRY(hipStreamSynchronize(dm->ctx->stream));
    return LORAHIP_OK;
}
} // namespace lorahip

extern "C" {

/*! The signals of the run just made (an ordinary receiver step) into the registered signal rows from row `first` on: packed on the
 * device from the last launch's records while they are the only ones (the packets' device path), else from the host queue. Stream
 * ordered like the packet rows. *n = signals of the run (also when the rows are too small: LORAHIP_E_INVALID, nothing cleared). */
static int signalsToRows(lorahip_demod *dm, const size_t first, size_t *n, const bool sync)
{
    *n = 0;
    if (!dm->wantSignals || !dm->sigRowsOn) return LORAHIP_OK;
    const lorahip_signal_rows &R = dm->sigRows;
    const DeviceGuard guard(dm->ctx->device);
    hipStream_t st = dm->ctx->stream;
    PendingLaunch &Q = dm->pending;
    if (Q.valid && dm->signals.empty())
    {
        *n = Q.signals;
        if (*n == 0) return LORAHIP_OK;
        if (first + *n > R.cap) { setLastError("lorahip_demod_receive: the signal rows cannot hold the signals that are due"); return LORAHIP_E_INVALID; }
        if (!Q.lay.signals) { *n = 0; return LORAHIP_OK; }
        LORAHIP_TRY(packSignals(dm, Q.lay, dm->sDev.get(), first, st));
        if (sync) LORAHIP_TRY(hipStreamSynchronize(st));
        return LORAHIP_OK;
    }
    { const int rc = drainPending(dm); if (rc != LORAHIP_OK) return rc; }
    const size_t S = dm->signals.size();
    *n = S;
    if (S == 0) return LORAHIP_OK;
    if (first + S > R.cap) { setLastError("lorahip_demod_receive: the signal rows cannot hold the signals that are due"); return LORAHIP_E_INVALID; }
    const size_t nb = align256(S * sizeof(int32_t));
    const size_t nbPos = R.pos ? align256(S * sizeof(int64_t)) : 0;
    { const int grc = growDense(dm, 4 * nb + nbPos); if (grc != LORAHIP_OK) return grc; }
    int64_t *hq = reinterpret_cast<int64_t *>(dm->hDense.get() + 4 * nb);
    int32_t *hc = reinterpret_cast<int32_t *>(dm->hDense.get()), *he = reinterpret_cast<int32_t *>(dm->hDense.get() + nb);
    float *hp = reinterpret_cast<float *>(dm->hDense.get() + 2 * nb), *hs = reinterpret_cast<float *>(dm->hDense.get() + 3 * nb);
    for (size_t i = 0; i < S; i++) { const Signal &g = dm->signals[i]; hc[i] = g.channel; he[i] = g.error; hp[i] = g.power; hs[i] = g.snr; if (R.pos) hq[i] = g.pos; }
    if (R.channel) LORAHIP_TRY(hipMemcpyAsync(R.channel + first, hc, S * sizeof(int32_t), hipMemcpyDefault, st));
    if (R.error) LORAHIP_TRY(hipMemcpyAsync(R.error + first, he, S * sizeof(int32_t), hipMemcpyDefault, st));
    if (R.power) LORAHIP_TRY(hipMemcpyAsync(R.power + first, hp, S * sizeof(float), hipMemcpyDefault, st));
    if (R.snr) LORAHIP_TRY(hipMemcpyAsync(R.snr + first, hs, S * sizeof(float), hipMemcpyDefault, st));
    if (R.pos) LORAHIP_TRY(hipMemcpyAsync(R.pos + first, hq, S * sizeof(int64_t), hipMemcpyDefault, st));
    LORAHIP_TRY(hipStreamSynchronize(st));                              // the pinned scratch is reused by the next run
    return LORAHIP_OK;
}

int lorahip_demod_receive_signal_rows(lorahip_demod *dm, const lorahip_signal_rows *rows)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) { setLastError("receiver steps are per part: lorahip_demod_part_handle"); return LORAHIP_E_INVALID; }
    if (rows == nullptr) { std::memset(&dm->sigRows, 0, sizeof(dm->sigRows)); dm->sigRowsOn = false; return LORAHIP_OK; }
    // versioned by struct_size: the size before `pos` existed is still taken, and means "no positions"
    if ((rows->struct_size != sizeof(lorahip_signal_rows) && rows->struct_size != LORAHIP_SIGNAL_ROWS_SIZE_V4) || rows->cap > 0x7fffffffu) return LORAHIP_E_INVALID;
    std::memset(&dm->sigRows, 0, sizeof(dm->sigRows));
    std::memcpy(&dm->sigRows, rows, rows->struct_size);
    dm->sigRows.struct_size = sizeof(lorahip_signal_rows);
    dm->sigRowsOn = rows->cap != 0 && (dm->sigRows.channel || dm->sigRows.error || dm->sigRows.power || dm->sigRows.snr || dm->sigRows.pos);
    return LORAHIP_OK;
}

size_t lorahip_demod_receive_num_signals(const lorahip_demod *dm) { return dm && !dm->comp ? dm->lastSignals : 0; }

size_t lorahip_demod_receive_steps(const lorahip_demod *dm, size_t *packets, size_t *signals, const size_t cap)
{
    if (dm == nullptr || dm->comp) return 0;
    const Resident &R = dm->res;
    for (unsigned i = 0; i < R.nRep && i < cap; i++)
    {
        if (packets) packets[i] = R.repPk[i];
        if (signals) signals[i] = R.repSg[i];
    }
    return R.nRep;
}

int lorahip_demod_resident_active(const lorahip_demod *dm)
{
    return dm && !dm->comp && dm->res.active ? 1 : 0;
}

//! the caller's rows in today's layout: versioned by struct_size, the size before `info_dev` existed is still taken and means "absent"
//! (nothing behind the caller's struct_size is read)
static bool takeRows(const lorahip_packet_rows *rows, lorahip_packet_rows &full)
{
    if (rows->struct_size != sizeof(lorahip_packet_rows) && rows->struct_size != LORAHIP_PACKET_ROWS_SIZE_V4) return false;
    std::memset(&full, 0, sizeof(full));
    std::memcpy(&full, rows, rows->struct_size);
    full.struct_size = sizeof(full);
    return true;
}

int lorahip_demod_receive(lorahip_demod *dm, const float *iq_dev, const size_t row_stride, const size_t n_valid, const lorahip_packet_rows *rows_in,
                          size_t *n_packets, int64_t *work_calls)
{
    lorahip_packet_rows full;
    if (dm == nullptr || rows_in == nullptr || !takeRows(rows_in, full)) return LORAHIP_E_INVALID;
    const lorahip_packet_rows *rows = &full;
    if (n_packets) *n_packets = 0;
    if (work_calls) *work_calls = 0;
    if (dm->comp) { setLastError("append runs are per part: lorahip_demod_part_handle"); return LORAHIP_E_INVALID; }
    if (rows->async == 2 || rows->async == 3)
    {
        if (n_valid > row_stride || (n_valid && iq_dev == nullptr)) return LORAHIP_E_INVALID;
        bool handled = false;
        if (rows->async == 3)
        {
            if (dm->pipe.active) { setLastError("a pipelined step is in flight: lorahip_demod_receive_flush first"); return LORAHIP_E_INVALID; }
            // the step message (and its check word) has no place for them: refused before anything is rung
            if (rows->info_dev != nullptr || (dm->sigRowsOn && dm->sigRows.pos != nullptr))
            {
                setLastError("lorahip_demod_receive (resident, async = 3): info_dev / signal positions are not delivered by resident steps -- use async 0, 1 or 2, or pass rows without them");
                return LORAHIP_E_INVALID;
            }
            const int prc = residentStep(dm, iq_dev, row_stride, n_valid, rows, n_packets, work_calls, handled);
            if (handled || prc != LORAHIP_OK) return prc;
        }
        else
        {
            if (dm->res.active) { setLastError("the resident kernel is on the device: lorahip_demod_receive_flush first"); return LORAHIP_E_INVALID; }
            const int prc = pipeStep(dm, iq_dev, row_stride, n_valid, rows, n_packets, work_calls, handled);
            if (handled || prc != LORAHIP_OK) return prc;
        }
        // not in place yet (first step, or something else touched the object): an ordinary step, its packets delivered at once
    }
    else { const int frc = refuseWhilePiped(dm); if (frc != LORAHIP_OK) return frc; }
    const int64_t calls0 = dm->workCalls;
    int rc = lorahip_demod_run_device_append(dm, iq_dev, row_stride, n_valid, nullptr);
    if (rc != LORAHIP_OK) return rc;
    if (work_calls) *work_calls = dm->workCalls - calls0;
    size_t n = 0;
    dm->lastSignals = 0;
    rc = packetsToDevice(dm, rows->syms_dev, rows->sym_stride, rows->nsyms_dev, rows->channel_dev, rows->info_dev, rows->cap_packets, &n, rows->async == 0);
    if (n_packets) *n_packets = n;
    if (rc != LORAHIP_OK) return rc;                                    // (the packets stay queued: a caller with too few rows can fetch them)
    rc = signalsToRows(dm, 0, &dm->lastSignals, rows->async == 0);      // the block's signals of this step, beside its packets
    if (rc != LORAHIP_OK) return rc;                                    // (... and so do the signals: lorahip_demod_get_signals)
    lorahip_demod_clear_packets(dm);
    return LORAHIP_OK;
}

/*! The LAST step of a pipelined or resident receiver filled a channel's record or packet capacity (lastSum.more): that channel still
 * holds >= 2N samples nobody would look at again. An ordinary step over the same rows resumes it until dry (the receiver has been
 * left: this is lorahip_demod_receive's own path), its packets into `rows` from row `row` on, its signals into the signal rows from
 * row `sig` on. If THEY do not fit they stay queued like any ordinary step's (LORAHIP_E_INVALID, *nPackets = all rows needed; the
 * first rows are filled; lorahip_demod_packets_to_device / the next receive delivers the rest). The counts add to the flush's own:
 * n0 packets, c0 work() calls, lastSignals. */
static int flushResume(lorahip_demod *dm, const lorahip_packet_rows *rows, const size_t row, const size_t sig, const size_t n0, const int64_t c0,
                       size_t *nPackets, int64_t *calls)
{
    const int64_t calls0 = dm->workCalls;
    int rc = lorahip_demod_run_device_append(dm, dm->stepIq, dm->stepStride, dm->home.prevValid(), nullptr);
    if (rc != LORAHIP_OK) return rc;
    if (calls) *calls = c0 + (dm->workCalls - calls0);
    if (rows == nullptr) { lorahip_demod_clear_packets(dm); return LORAHIP_OK; }
    size_t n2 = 0;
    rc = packetsToDevice(dm, rows->syms_dev ? rows->syms_dev + row * rows->sym_stride : nullptr, rows->sym_stride, rows->nsyms_dev ? rows->nsyms_dev + row : nullptr,
                         rows->channel_dev ? rows->channel_dev + row : nullptr, rows->info_dev ? rows->info_dev + row : nullptr, rows->cap_packets - row, &n2, true);
    if (nPackets) *nPackets = n0 + n2;
    if (rc != LORAHIP_OK) return rc;
    const size_t s1 = dm->lastSignals;
    size_t s2 = 0;
    rc = signalsToRows(dm, sig, &s2, true);
    dm->lastSignals = s1 + s2;
    if (rc != LORAHIP_OK) return rc;
    lorahip_demod_clear_packets(dm);
    return LORAHIP_OK;
}

int lorahip_demod_receive_flush(lorahip_demod *dm, const lorahip_packet_rows *rows_in, size_t *n_packets, int64_t *work_calls)
{
    lorahip_packet_rows full;
    if (dm == nullptr || (rows_in != nullptr && !takeRows(rows_in, full))) return LORAHIP_E_INVALID;
    const lorahip_packet_rows *rows = rows_in ? &full : nullptr;
    if (n_packets) *n_packets = 0;
    if (work_calls) *work_calls = 0;
    if (dm->comp) return LORAHIP_OK;
    dm->lastSignals = 0;                                    // (a flush with nothing in flight delivers nothing: not the count of the call before)
    dm->res.nRep = 0;
    if (dm->res.active)
    {
        // the resident receiver: every step's rows came with its own call; what is left to report are the counts of the last step(s)
        size_t n0 = 0; int64_t c0 = 0;
        const int rc0 = residentFlush(dm, &n0, &c0);
        if (n_packets) *n_packets = n0;
        if (work_calls) *work_calls = c0;
        if (rc0 != LORAHIP_OK || dm->lastSum.more == 0) return rc0;
        // packets and signals of the resumed channels into these rows from row 0 on (the steps' are in the rows of their own calls)
        return flushResume(dm, rows, 0, 0, n0, c0, n_packets, work_calls);
    }
    const bool wasPiped = pipeBusy(dm);
    size_t n1 = 0;
    int64_t c1 = 0;
    const int rc = pipeFlush(dm, rows, &n1, &c1);
    if (n_packets) *n_packets = n1;
    if (work_calls) *work_calls = c1;
    if (rc != LORAHIP_OK || !wasPiped || dm->lastSum.more == 0) return rc;
    // packets and signals of the resumed channels behind the ones just delivered
    return flushResume(dm, rows, n1, dm->lastSignals, n1, c1, n_packets, work_calls);
}

int lorahip_demod_set_signals(lorahip_demod *dm, const int enable)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setSignals(enable);
    dm->wantSignals = enable != 0;
    return LORAHIP_OK;
}

size_t lorahip_demod_num_signals(const lorahip_demod *dm)
{
    if (dm == nullptr) return 0;
    if (dm->comp) return dm->comp->numSignals();
    const PendingLaunch &P = dm->pending;
    return dm->signals.size() + (P.valid ? P.signals : 0);
}

int lorahip_demod_get_signals(const lorahip_demod *dm, int32_t *channels, int64_t *rounds, int32_t *errors, float *powers, float *snrs, const size_t cap)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->comp) return dm->comp->getSignals(channels, rounds, errors, powers, snrs, cap);
    if (dm == nullptr || cap < dm->signals.size()) return LORAHIP_E_INVALID;
    for (size_t i = 0; i < dm->signals.size(); i++)
    {
        const Signal &g = dm->signals[i];
        if (channels) channels[i] = g.channel;
        if (rounds) rounds[i] = g.round;
        if (errors) errors[i] = g.error;
        if (powers) powers[i] = g.power;
        if (snrs) snrs[i] = g.snr;
    }
    return LORAHIP_OK;
}

int lorahip_demod_get_signals_pos(const lorahip_demod *dm, int64_t *pos, const size_t cap)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm->comp) return dm->comp->getSignalsPos(pos, cap);
    if (dm == nullptr || pos == nullptr || cap < dm->signals.size()) return LORAHIP_E_INVALID;
    for (size_t i = 0; i < dm->signals.size(); i++) pos[i] = dm->signals[i].pos;
    return LORAHIP_OK;
}

void lorahip_demod_clear_packets(lorahip_demod *dm)
{
    if (dm == nullptr) return;
    if (dm->comp) { dm->comp->clearPackets(); return; }
    PendingLaunch &P = dm->pending;
    if (P.valid)
    {
        // records still on the device: they can simply be dropped unless a channel is inside a packet -- the symbols it has
        // received so far open the first packet of the next run
        if (P.anyOpen && !dm->home.carryRowsValid()) (void)drainPending(dm);
        else P.valid = false;                                   // (with the open packets kept on the device nothing is lost)
    }
    dm->packets.clear();
    dm->pktSyms.clear();
    dm->signals.clear();
}

int64_t lorahip_demod_work_calls(const lorahip_demod *dm) { return dm ? (dm->comp ? dm->comp->workCalls() : dm->workCalls) : 0; }

double lorahip_demod_kernel_ms(const lorahip_demod *dm) { return dm ? (dm->comp ? dm->comp->kernelMs() : dm->kernelMs) : 0.0; }
int lorahip_demod_last_launches(const lorahip_demod *dm) { return dm ? (dm->comp ? dm->comp->lastLaunches() : dm->lastLaunches) : 0; }

int lorahip_demod_near_threshold(const lorahip_demod *dm, int64_t *near_squelch, int64_t *near_step)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->nearThreshold(near_squelch, near_step);
    if (near_squelch) *near_squelch = dm->nNearSquelch;
    if (near_step) *near_step = dm->nNearStep;
    return LORAHIP_OK;
}

//! where the read positions are: the pinned copy's states, fetched first (nullptr if that failed; *rc says how), or -- *rc
//! LORAHIP_OK and nullptr -- the mirrors
static const StreamState *pinnedPositions(const lorahip_demod *dm, int *rc)
{
    *rc = LORAHIP_OK;
    if (!(dm->home.readPinnedPos() && dm->sHost.get())) return nullptr;
    lorahip_demod *m = const_cast<lorahip_demod *>(dm);
    *rc = ensureHead(m);
    return *rc == LORAHIP_OK ? hostStates(m) : nullptr;
}

int64_t lorahip_demod_consumed(const lorahip_demod *dm, const size_t channel)
{
    if (dm == nullptr || channel >= dm->B) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->consumed(channel);
    int rc;
    if (const StreamState *hs = pinnedPositions(dm, &rc)) return int64_t(hs[channel].pos);
    if (rc != LORAHIP_OK) return LORAHIP_E_HIP;
    if (dm->home.placementUntouched()) return 0;
    return int64_t(dm->ch[channel].pos);
}

int lorahip_demod_consumed_all(const lorahip_demod *dm, int64_t *out)
{
    if (dm == nullptr || out == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->consumedAll(out);
    // (while the resident kernel is on the device the positions live in its steps; a copy queued behind it could wait for the flush)
    if (dm->res.active)
    {
        setLastError("the resident kernel is on the device: lorahip_demod_receive_flush first");
        return LORAHIP_E_INVALID;
    }
    // the one read that can fail -- the per-channel state back from the device -- up front: an error is the call's, not a negative
    // entry a caller would take for "nothing consumed"
    { int rc; (void)pinnedPositions(dm, &rc); if (rc != LORAHIP_OK) return rc; }
    for (size_t c = 0; c < dm->B; c++)
    {
        out[c] = lorahip_demod_consumed(dm, c);
        if (out[c] < 0) return int(out[c]);
    }
    return LORAHIP_OK;
}
} // extern "C"
