// Level 3, the debug ports: the block's "raw" / "dec" / "fft" outputs (LoRaDemod.cpp:81-83), and the per-call trace with the labels
// the block posts. The run records, per work() call, the dechirp state it started from (lorahip_work_result.fine_*); the ports are
// then REPLAYED from that trace with the batch kernels -- the same arithmetic on the same inputs, hence the same bits -- and scattered
// into the caller's per-channel port streams. Off unless asked for: they triple the HBM traffic.
#include "lorahip_demod_state.h"
#include <cstdio>
#include <cstring>
#include <string>

using namespace lorahip;
using namespace lorahip::demod;

namespace lorahip { namespace demod {

int fillPorts(lorahip_demod *dm, const float *iqDev)
{
    lorahip_ctx *ctx = dm->ctx;
    const size_t N = dm->N, B = dm->B;
    const lorahip_demod_ports &P = dm->ports;
    const DeviceGuard guard(ctx->device);
    applyGeometry(dm);                                          // the replay reads ch[].base
    struct Seg { long long src, dst; int len; };
    std::vector<int64_t> wOff; std::vector<int32_t> wSel, wIdx; std::vector<float> wErr;
    std::vector<Seg> segFft, segDec, segRaw;                      // src of fft/dec segments: window number * N (chunk-relative later)
    for (size_t c = 0; c < B; c++)
    {
        Channel &k = dm->ch[c];
        size_t decPos = 0, frame = 0;
        for (size_t i = k.traceStart; i < k.trace.size(); i++, frame++)
        {
            const lorahip_work_result &r = k.trace[i];
            const bool down = r.state_before == ST_DOWNCHIRP0 || r.state_before == ST_DOWNCHIRP1;   // _chirpTable == _downChirpTable
            const size_t w = wOff.size();
            wOff.push_back(int64_t(k.base + k.runStart + decPos));  // from where the run began (the head of the stream unless it continues one)
            wSel.push_back(down ? LORAHIP_CHIRP_DOWN : LORAHIP_CHIRP_UP);
            wIdx.push_back(r.fine_idx_before);
            wErr.push_back(r.fine_err_before);
            const size_t total = size_t(r.consumed);
            if (P.fft_dev && frame < P.fft_cap_frames) segFft.push_back({ (long long)(w * N), (long long)((c * P.fft_cap_frames + frame) * N), int(N) });
            if (P.dec_dev)
            {
                const size_t n0 = total < N ? total : N;
                if (decPos < P.dec_cap_samples)
                    segDec.push_back({ (long long)(w * N), (long long)(c * P.dec_cap_samples + decPos), int(decPos + n0 <= P.dec_cap_samples ? n0 : P.dec_cap_samples - decPos) });
            }
            if (total == 2 * N && r.state_before == ST_FRAMESYNC)
            {
                // the sync check dechirped window 1 too (:189-206): it starts from the committed index and is part of what `dec` produces
                const size_t w1 = wOff.size();
                wOff.push_back(int64_t(k.base + k.runStart + decPos + N));
                wSel.push_back(LORAHIP_CHIRP_UP);
                wIdx.push_back(r.fine_idx_after);
                wErr.push_back(r.fine_err_before);
                if (P.dec_dev && decPos + N < P.dec_cap_samples)
                    segDec.push_back({ (long long)(w1 * N), (long long)(c * P.dec_cap_samples + decPos + N),
                                       int(decPos + 2 * N <= P.dec_cap_samples ? N : P.dec_cap_samples - decPos - N) });
            }
            decPos += total;
        }
        k.portFft = frame; k.portDec = decPos; k.portRaw = decPos;
        if (P.raw_dev && decPos) segRaw.push_back({ (long long)(k.base + k.runStart), (long long)(c * P.raw_cap_samples), int(decPos <= P.raw_cap_samples ? decPos : P.raw_cap_samples) });
    }
    hipStream_t st = ctx->stream;
    auto scatter = [&](float *dst, const float *src, const std::vector<Seg> &segs, const size_t first, const size_t last, const long long srcBias, char *scratch) -> int
    {
        // segments [first, last) of `segs`, their src offsets rebased by srcBias
        const size_t n = last - first;
        if (n == 0) return LORAHIP_OK;
        std::vector<long long> so(n), dof(n); std::vector<int> ln(n);
        for (size_t i = 0; i < n; i++) { so[i] = segs[first + i].src - srcBias; dof[i] = segs[first + i].dst; ln[i] = segs[first + i].len; }
        long long *dSo = reinterpret_cast<long long *>(scratch), *dDo = dSo + n;
        int *dLn = reinterpret_cast<int *>(dDo + n);
        LORAHIP_TRY(hipMemcpyAsync(dSo, so.data(), n * sizeof(long long), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(hipMemcpyAsync(dDo, dof.data(), n * sizeof(long long), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(hipMemcpyAsync(dLn, ln.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(launchCopySegments(reinterpret_cast<float2 *>(dst), reinterpret_cast<const float2 *>(src), dSo, dDo, dLn, n, st));
        LORAHIP_TRY(hipStreamSynchronize(st));                  // the host vectors die with this scope
        return LORAHIP_OK;
    };
    const size_t W = wOff.size();
    // replay in chunks: at most ~256 MiB of replayed windows per port at a time
    size_t chunk = (size_t(256) << 20) / (N * sizeof(cf32));
    if (chunk < 64) chunk = 64;
    if (chunk > W) chunk = W;
    const size_t descBytes = align256(chunk * 2 * (2 * sizeof(long long) + sizeof(int)) + segRaw.size() * (2 * sizeof(long long) + sizeof(int)) + 64);
    const size_t winBytes = align256(chunk * N * sizeof(cf32));
    const size_t inBytes = align256(chunk * sizeof(int64_t)) + 3 * align256(chunk * sizeof(int32_t));
    const size_t outBytes = align256(chunk * sizeof(uint16_t)) + 3 * align256(chunk * sizeof(float));
    LORAHIP_TRY(dm->dPort.grow(descBytes + 2 * winBytes + inBytes + outBytes));
    char *cur = dm->dPort.get();
    char *dDesc = cur; cur += descBytes;
    float *tFft = reinterpret_cast<float *>(cur); cur += winBytes;
    float *tDec = reinterpret_cast<float *>(cur); cur += winBytes;
    int64_t *dOff = reinterpret_cast<int64_t *>(cur); cur += align256(chunk * sizeof(int64_t));
    int32_t *dSel = reinterpret_cast<int32_t *>(cur); cur += align256(chunk * sizeof(int32_t));
    int32_t *dIdx = reinterpret_cast<int32_t *>(cur); cur += align256(chunk * sizeof(int32_t));
    float *dErr = reinterpret_cast<float *>(cur); cur += align256(chunk * sizeof(int32_t));
    uint16_t *dSym = reinterpret_cast<uint16_t *>(cur); cur += align256(chunk * sizeof(uint16_t));
    float *dPow = reinterpret_cast<float *>(cur); cur += align256(chunk * sizeof(float));
    float *dAvg = reinterpret_cast<float *>(cur); cur += align256(chunk * sizeof(float));
    float *dFi = reinterpret_cast<float *>(cur);
    if (P.raw_dev) { const int rc = scatter(P.raw_dev, iqDev, segRaw, 0, segRaw.size(), 0, dDesc); if (rc != LORAHIP_OK) return rc; }
    struct HostCopy
    {
        static int run(lorahip_demod *dm, hipStream_t st)
        {
            // host port buffers: what each channel produced, out of the library's device mirrors
            const lorahip_demod_ports &H = dm->hostPorts, &D = dm->ports;
            const size_t N = dm->N;
            for (size_t c = 0; c < dm->B; c++)
            {
                const Channel &k = dm->ch[c];
                const size_t nf = k.portFft < D.fft_cap_frames ? k.portFft : D.fft_cap_frames;
                const size_t nd = k.portDec < D.dec_cap_samples ? k.portDec : D.dec_cap_samples;
                const size_t nr = k.portRaw < D.raw_cap_samples ? k.portRaw : D.raw_cap_samples;
                if (H.fft_dev && nf) LORAHIP_TRY(hipMemcpyAsync(H.fft_dev + 2 * c * D.fft_cap_frames * N, D.fft_dev + 2 * c * D.fft_cap_frames * N, nf * N * sizeof(cf32), hipMemcpyDeviceToHost, st));
                if (H.dec_dev && nd) LORAHIP_TRY(hipMemcpyAsync(H.dec_dev + 2 * c * D.dec_cap_samples, D.dec_dev + 2 * c * D.dec_cap_samples, nd * sizeof(cf32), hipMemcpyDeviceToHost, st));
                if (H.raw_dev && nr) LORAHIP_TRY(hipMemcpyAsync(H.raw_dev + 2 * c * D.raw_cap_samples, D.raw_dev + 2 * c * D.raw_cap_samples, nr * sizeof(cf32), hipMemcpyDeviceToHost, st));
            }
            LORAHIP_TRY(hipStreamSynchronize(st));
            return LORAHIP_OK;
        }
    };
    size_t fi = 0, di = 0;
    for (size_t w0 = 0; w0 < W && (P.fft_dev || P.dec_dev); w0 += chunk)
    {
        const size_t n = W - w0 < chunk ? W - w0 : chunk;
        LORAHIP_TRY(hipMemcpyAsync(dOff, wOff.data() + w0, n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(hipMemcpyAsync(dSel, wSel.data() + w0, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(hipMemcpyAsync(dIdx, wIdx.data() + w0, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        LORAHIP_TRY(hipMemcpyAsync(dErr, wErr.data() + w0, n * sizeof(float), hipMemcpyHostToDevice, st));
        lorahip_batch b;
        std::memset(&b, 0, sizeof(b));
        b.struct_size = sizeof(b);
        b.iq = iqDev; b.n_windows = n; b.offsets = dOff; b.chirp_sel = dSel; b.fine_idx0 = dIdx; b.fine_err = dErr;
        b.sym = dSym; b.power = dPow; b.power_avg = dAvg; b.f_index = dFi;
        b.fft_out = P.fft_dev ? tFft : nullptr;
        b.dec_out = P.dec_dev ? tDec : nullptr;
        const int rc = lorahip_detect_batch(ctx, &b);
        if (rc != LORAHIP_OK) return rc;
        const long long lo = (long long)(w0 * N), hi = (long long)((w0 + n) * N);
        size_t f1 = fi; while (f1 < segFft.size() && segFft[f1].src < hi) f1++;
        size_t d1 = di; while (d1 < segDec.size() && segDec[d1].src < hi) d1++;
        int rc2 = scatter(P.fft_dev, tFft, segFft, fi, f1, lo, dDesc);
        if (rc2 == LORAHIP_OK) rc2 = scatter(P.dec_dev, tDec, segDec, di, d1, lo, dDesc);
        if (rc2 != LORAHIP_OK) return rc2;
        fi = f1; di = d1;
    }
    if (dm->hostPorts.host_buffers) return HostCopy::run(dm, st);
    return LORAHIP_OK;
}

} } // namespace lorahip::demod

extern "C" {

int lorahip_demod_set_trace(lorahip_demod *dm, const int enable)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setTrace(enable);
    const bool was = dm->tracing;
    { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }       // traceSymCount0 is read from the mirrors
    dm->userTracing = enable != 0;
    dm->tracing = dm->userTracing || dm->portsOn;
    if (!dm->userTracing) for (auto &k : dm->ch) { k.trace.clear(); k.traceStart = 0; k.traceSymCount0 = k.symCount; }
    else if (!was) for (auto &k : dm->ch) k.traceSymCount0 = k.symCount;
    return LORAHIP_OK;
}

size_t lorahip_demod_trace_len(const lorahip_demod *dm, const size_t channel)
{
    if (drained(dm) != LORAHIP_OK) return 0;                    // lorahip_last_error() says why
    if (dm == nullptr || channel >= dm->B) return 0;
    if (dm->comp) return dm->comp->traceLen(channel);
    return dm->ch[channel].trace.size();
}

int lorahip_demod_set_ports(lorahip_demod *dm, const lorahip_demod_ports *p)
{
    if (dm == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->setPorts(p);
    const DeviceGuard guard(dm->ctx->device);
    dm->ownFft.reset(); dm->ownDec.reset(); dm->ownRaw.reset();
    std::memset(&dm->ports, 0, sizeof(dm->ports));
    std::memset(&dm->hostPorts, 0, sizeof(dm->hostPorts));
    dm->portsOn = false;
    if (p != nullptr)
    {
        if (p->struct_size != sizeof(lorahip_demod_ports)) return LORAHIP_E_INVALID;
        if ((p->fft_dev && !p->fft_cap_frames) || (p->dec_dev && !p->dec_cap_samples) || (p->raw_dev && !p->raw_cap_samples)) return LORAHIP_E_INVALID;
        dm->ports = *p;
        if (p->host_buffers)
        {
            dm->hostPorts = *p;
            dm->ports.host_buffers = 0;
            dm->ports.fft_dev = dm->ports.dec_dev = dm->ports.raw_dev = nullptr;
            if (p->fft_dev) { LORAHIP_TRY(dm->ownFft.grow(dm->B * p->fft_cap_frames * dm->N * sizeof(cf32))); dm->ports.fft_dev = dm->ownFft.get(); }
            if (p->dec_dev) { LORAHIP_TRY(dm->ownDec.grow(dm->B * p->dec_cap_samples * sizeof(cf32))); dm->ports.dec_dev = dm->ownDec.get(); }
            if (p->raw_dev) { LORAHIP_TRY(dm->ownRaw.grow(dm->B * p->raw_cap_samples * sizeof(cf32))); dm->ports.raw_dev = dm->ownRaw.get(); }
        }
        dm->portsOn = dm->ports.fft_dev || dm->ports.dec_dev || dm->ports.raw_dev;
    }
    if (dm->portsOn && !dm->tracing) { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; for (auto &k : dm->ch) k.traceSymCount0 = k.symCount; }
    dm->tracing = dm->userTracing || dm->portsOn;
    return LORAHIP_OK;
}

int lorahip_demod_port_counts(const lorahip_demod *dm, const size_t channel, size_t *fft_frames, size_t *dec_samples, size_t *raw_samples)
{
    if (dm == nullptr || channel >= dm->B) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->portCounts(channel, fft_frames, dec_samples, raw_samples);
    const Channel &k = dm->ch[channel];
    if (fft_frames) *fft_frames = k.portFft;
    if (dec_samples) *dec_samples = k.portDec;
    if (raw_samples) *raw_samples = k.portRaw;
    return LORAHIP_OK;
}

//! the label LoRaDemod::work() posts for one call (LoRaDemod.cpp:213,220-224,232,245,258,282,302-305): "" = none
static std::string labelOf(const lorahip_work_result &r, const size_t N, const float thresh, size_t &symCount)
{
    char buf[64];
    buf[0] = 0;
    switch (r.state_before)
    {
    case ST_FRAMESYNC:
        if (size_t(r.consumed) == 2 * N) return "SYNC";                                           // :213
        if (!(r.snr < thresh)) { std::snprintf(buf, sizeof(buf), "P %.4f", double(r.f_index)); return buf; }   // :220-224 (fixed, precision 4)
        return "";                                                                                // :232
    case ST_DOWNCHIRP0: return "DC";                                                              // :245
    case ST_DOWNCHIRP1: return "";                                                                // :258
    case ST_QUARTERCHIRP: symCount = 0; return "QC";                                              // :281-282
    default:
        symCount++;                                                                               // :290
        std::snprintf(buf, sizeof(buf), "S%zu %.4f", symCount, double(r.f_index));                // :302-305
        return buf;
    }
}

int lorahip_demod_get_labels(const lorahip_demod *dm, const size_t channel, char *buf, const size_t cap, size_t *n_calls, size_t *bytes)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm == nullptr || channel >= dm->B) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->getLabels(channel, buf, cap, n_calls, bytes);
    const auto &t = dm->ch[channel].trace;
    // _symCount is only reset at QUARTERCHIRP (:279): a trace that starts inside a packet continues the count the channel held then
    size_t symCount = dm->ch[channel].traceSymCount0;
    size_t used = 0;
    for (const auto &r : t)
    {
        const std::string s = labelOf(r, dm->N, dm->thresh, symCount);
        if (buf && used + s.size() + 1 <= cap) std::memcpy(buf + used, s.c_str(), s.size() + 1);
        used += s.size() + 1;
    }
    if (n_calls) *n_calls = t.size();
    if (bytes) *bytes = used;
    return (buf == nullptr || used <= cap) ? LORAHIP_OK : LORAHIP_E_INVALID;
}

int lorahip_demod_get_trace(const lorahip_demod *dm, const size_t channel, lorahip_work_result *out, const size_t cap)
{
    { const int rc = drained(dm); if (rc != LORAHIP_OK) return rc; }
    if (dm == nullptr || channel >= dm->B || out == nullptr) return LORAHIP_E_INVALID;
    if (dm->comp) return dm->comp->getTrace(channel, out, cap);
    const auto &t = dm->ch[channel].trace;
    if (cap < t.size()) return LORAHIP_E_INVALID;
    if (!t.empty()) std::memcpy(out, t.data(), t.size() * sizeof(lorahip_work_result));
    return LORAHIP_OK;
}

} // extern "C"
