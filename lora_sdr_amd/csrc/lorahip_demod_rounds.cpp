// Level 3, the host-driven rounds (mode 2; the A/B partner of the streaming kernels). One work() "round" = every channel that has
// >= 2N samples left performs one work() call (LoRaDemod.cpp:145-327). The dechirp+FFT+detect of all those calls is ONE batch
// launch (lorahip_detect_batch); the frame state machine -- a handful of integer operations per call whose only coupling is the
// per-channel window offset; lorahip_framestep.h::frameStep, the function the streaming kernels run -- runs on the host between launches. Channels that hit "syncd and match0" (:189) get their second
// window in a second, compacted launch, exactly like the reference's nested loop (:189-206).
#include "lorahip_demod_state.h"
#include "lorahip_framestep.h"
#include <cstring>
#include <type_traits>

namespace lorahip { namespace demod {

struct Round
{
    int64_t *off; int32_t *sel; int32_t *idx0; float *err;                  // inputs
    uint16_t *sym; float *power; float *pavg; float *fidx; int32_t *idxOut; // outputs
    size_t inBytes, total;
};

static Round carve(char *p, const size_t B)
{
    // (offsets first, pointers last: the size of the block is asked for with p == nullptr, and arithmetic on a null pointer is
    // undefined -- found by the -fsanitize=undefined pass, profiles/r05)
    Round r;
    size_t cur = 0;
    const size_t oOff = cur; cur += align256(B * sizeof(int64_t));
    const size_t oSel = cur; cur += align256(B * sizeof(int32_t));
    const size_t oIdx0 = cur; cur += align256(B * sizeof(int32_t));
    const size_t oErr = cur; cur += align256(B * sizeof(float));
    r.inBytes = cur;
    const size_t oSym = cur; cur += align256(B * sizeof(uint16_t));
    const size_t oPower = cur; cur += align256(B * sizeof(float));
    const size_t oPavg = cur; cur += align256(B * sizeof(float));
    const size_t oFidx = cur; cur += align256(B * sizeof(float));
    const size_t oIdxOut = cur; cur += align256(B * sizeof(int32_t));
    r.total = cur;
    r.off = nullptr; r.sel = nullptr; r.idx0 = nullptr; r.err = nullptr;
    r.sym = nullptr; r.power = nullptr; r.pavg = nullptr; r.fidx = nullptr; r.idxOut = nullptr;
    if (p == nullptr) return r;
    r.off = reinterpret_cast<int64_t *>(p + oOff); r.sel = reinterpret_cast<int32_t *>(p + oSel);
    r.idx0 = reinterpret_cast<int32_t *>(p + oIdx0); r.err = reinterpret_cast<float *>(p + oErr);
    r.sym = reinterpret_cast<uint16_t *>(p + oSym); r.power = reinterpret_cast<float *>(p + oPower);
    r.pavg = reinterpret_cast<float *>(p + oPavg); r.fidx = reinterpret_cast<float *>(p + oFidx);
    r.idxOut = reinterpret_cast<int32_t *>(p + oIdxOut);
    return r;
}

//! the staging block of one round for B windows, in bytes (host pinned and device alike)
size_t roundStagingBytes(const size_t B) { return carve(nullptr, B).total; }

//! one compacted launch over `n` windows described in the host staging block
static int launchRound(lorahip_demod *dm, const float *iqDev, const size_t n)
{
    lorahip_ctx *ctx = dm->ctx;
    const Round hr = carve(dm->h.get(), dm->B), dr = carve(dm->d.get(), dm->B);
    LORAHIP_TRY(hipMemcpyAsync(dm->d.get(), dm->h.get(), hr.inBytes, hipMemcpyHostToDevice, ctx->stream));
    lorahip_batch b;
    std::memset(&b, 0, sizeof(b));
    b.struct_size = sizeof(b);
    b.iq = iqDev;
    b.n_windows = n;
    b.offsets = dr.off;
    b.chirp_sel = dr.sel;
    b.fine_idx0 = dr.idx0;
    b.fine_err = dr.err;
    b.sym = dr.sym; b.power = dr.power; b.power_avg = dr.pavg; b.f_index = dr.fidx;
    b.fine_idx_out = dr.idxOut;
    const int rc = lorahip_detect_batch(ctx, &b);
    if (rc != LORAHIP_OK) return rc;
    LORAHIP_TRY(hipMemcpyAsync(dm->h.get() + hr.inBytes, dm->d.get() + hr.inBytes, hr.total - hr.inBytes,
                               hipMemcpyDeviceToHost, ctx->stream));
    LORAHIP_TRY(hipStreamSynchronize(ctx->stream));
    return LORAHIP_OK;
}

//! ch[].base / len / pos of a uniform run (filled only for the paths that read them: host-driven rounds, the port replay)
void applyGeometry(lorahip_demod *dm)
{
    if (dm->home.geometryCurrent()) return;
    const bool cont = dm->home.continues();                     // an append run continues at the mirrors' read positions (synced by the caller)
    for (size_t c = 0; c < dm->B; c++)
    {
        dm->ch[c].base = c * dm->home.stride(); dm->ch[c].len = dm->home.spc();
        if (!cont) { dm->ch[c].pos = 0; dm->ch[c].callCount = 0; }
    }
    dm->home.geometryApplied();
}

//! frameStep<2^sf> on the host: the call whose detect results stand in r (the first pass filled it), its record into r -- o.out points
//! at the caller's r, hence the copy here
static void stepFrame(const int sf, StreamState &st, const StreamArgs &s, OneCall &o, const lorahip_work_result r, const bool squelched, const bool syncd,
                      const bool match0, const bool match1)
{
    const auto step = [&](auto n)
    {
        frameStep<decltype(n)::value>(st, s, o, true, r.value, r.power, r.power_avg, r.snr, r.f_index, squelched, syncd, match0, match1, r.fine_idx_before, r.fine_err_before);
    };
    switch (sf)                                                 // LORAHIP_SF_MIN .. LORAHIP_SF_MAX
    {
    case 6: step(std::integral_constant<int, 64>()); break;
    case 7: step(std::integral_constant<int, 128>()); break;
    case 8: step(std::integral_constant<int, 256>()); break;
    case 9: step(std::integral_constant<int, 512>()); break;
    case 10: step(std::integral_constant<int, 1024>()); break;
    case 11: step(std::integral_constant<int, 2048>()); break;
    default: step(std::integral_constant<int, 4096>()); break;      // 12
    }
}

int runRounds(lorahip_demod *dm, const float *iqDev, int64_t *roundsOut)
{
    const size_t N = dm->N, B = dm->B;
    { const int rc = syncMirrors(dm); if (rc != LORAHIP_OK) return rc; }       // (a failed fetch of the open packets' symbols: nothing is invalidated)
    applyGeometry(dm);
    if (!dm->home.continues()) for (auto &k : dm->ch) k.callCount = 0;
    dm->home.roundsBegin();                                     // the mirrors are about to change: the device's copies go stale (syncMirrors fetched the open packets)
    const DeviceGuard guard(dm->ctx->device);
    const Round hr = carve(dm->h.get(), B);
    std::vector<uint32_t> live, second;
    std::vector<lorahip_work_result> res(B);
    StreamArgs args{};                                          // (frameStep reads the mtu)
    args.mtu = dm->mtu > 0xffffffffu ? 0xffffffffu : unsigned(dm->mtu);
    int64_t rounds = 0;
    while (true)
    {
        // ---- who can work this round (LoRaDemod.cpp:148) ----
        live.clear();
        for (size_t c = 0; c < B; c++)
        {
            Channel &k = dm->ch[c];
            if (k.len - k.pos < 2 * N) continue;
            const size_t i = live.size();
            live.push_back(uint32_t(c));
            hr.off[i] = int64_t(k.base + k.pos);
            hr.sel[i] = k.downTable ? LORAHIP_CHIRP_DOWN : LORAHIP_CHIRP_UP;
            hr.idx0[i] = k.fineTuneIndex;
            hr.err[i] = k.finefreqError;
        }
        if (live.empty()) break;
        int rc = launchRound(dm, iqDev, live.size());       // loop A + detect (:157-172)
        if (rc != LORAHIP_OK) return rc;

        // ---- first pass: commit the index, find channels needing window 1 ----
        second.clear();
        for (size_t i = 0; i < live.size(); i++)
        {
            Channel &k = dm->ch[live[i]];
            lorahip_work_result &r = res[live[i]];
            std::memset(&r, 0, sizeof(r));
            r.worked = 1;
            r.state_before = k.state;
            r.value = hr.sym[i];
            r.power = hr.power[i]; r.power_avg = hr.pavg[i]; r.f_index = hr.fidx[i];
            r.snr = r.power - r.power_avg;                                      // :173
            r.fine_idx_before = k.fineTuneIndex; r.fine_err_before = k.finefreqError;
            if ((k.state == ST_FRAMESYNC || k.state == ST_DATASYMBOLS) && nearSquelch(r.snr, dm->thresh)) dm->nNearSquelch++;
            if (nearStep(k.finefreqError * float(LORAHIP_FINE_STEPS))) dm->nNearStep++;
            k.fineTuneIndex = hr.idxOut[i];
            r.fine_idx_after = k.fineTuneIndex;
            if (k.state == ST_FRAMESYNC)
            {
                const bool squelched = r.snr < dm->thresh;                      // :174
                const bool syncd = !squelched && (k.prevValue + 4) / 8 == 0;    // :183
                const bool match0 = (size_t(r.value) + 4) / 8 == unsigned(dm->sync >> 4); // :184
                if (syncd && match0) second.push_back(live[i]);
            }
        }
        std::vector<uint16_t> value1(second.size());
        if (!second.empty())
        {
            for (size_t i = 0; i < second.size(); i++)
            {
                Channel &k = dm->ch[second[i]];
                hr.off[i] = int64_t(k.base + k.pos + N);                         // inBuff[i + N]  :194
                hr.sel[i] = k.downTable ? LORAHIP_CHIRP_DOWN : LORAHIP_CHIRP_UP;
                hr.idx0[i] = k.fineTuneIndex;                                    // int ft = _fineTuneIndex  :191
                hr.err[i] = k.finefreqError;
                if (nearStep(k.finefreqError * float(LORAHIP_FINE_STEPS))) dm->nNearStep++;
            }
            rc = launchRound(dm, iqDev, second.size());
            if (rc != LORAHIP_OK) return rc;
            for (size_t i = 0; i < second.size(); i++)
            {
                lorahip_work_result &r = res[second[i]];
                value1[i] = hr.sym[i];
                // detect(power,powerAvg,fIndex) of window 1 overwrites the locals (:203); snr is not recomputed
                r.power = hr.power[i]; r.power_avg = hr.pavg[i]; r.f_index = hr.fidx[i];
            }
        }

        // ---- second pass: the state machine (:176-312), frameStep with room for this one call's records ----
        size_t si = 0;
        for (size_t i = 0; i < live.size(); i++)
        {
            const uint32_t c = live[i];
            Channel &k = dm->ch[c];
            lorahip_work_result &r = res[c];
            const bool squelched = r.snr < dm->thresh;                                           // :174
            const bool syncd = !squelched && (k.prevValue + 4) / 8 == 0;                         // :183
            const bool match0 = (size_t(r.value) + 4) / 8 == unsigned(dm->sync >> 4);            // :184
            bool match1 = false;
            if (k.state == ST_FRAMESYNC && syncd && match0) match1 = (size_t(value1[si++]) + 4) / 8 == unsigned(dm->sync & 0xf);   // :205
            StreamState st;
            toStreamState(k, st);
            st.pos = 0; st.callCount = 0;                                                        // (the mirror's own, wider ones count on below)
            short sym = 0;
            StreamPacket pkt;
            OneCall o = {&r, &sym, &pkt, nullptr, 0, 0, 0, 0};
            stepFrame(dm->ctx->sf, st, args, o, r, squelched, syncd, match0, match1);            // fills r: consumed, packet_len, signals, sig_*
            fromStreamState(k, st);
            if (r.signals)                                                                       // DOWNCHIRP1  :256-269
            {
                k.outSymbols.assign(dm->mtu ? dm->mtu : 1, 0);
                if (dm->wantSignals)
                {
                    Signal g;
                    g.channel = int32_t(c); g.round = k.callCount; g.error = r.sig_error; g.power = r.sig_power; g.snr = r.sig_snr;
                    g.pos = int64_t(k.pos);                                                      // the call has not consumed yet (below)
                    dm->signals.push_back(g);
                }
            }
            if (o.nSym)                                                                          // out[_symCount++] = value  :290
            {
                if (k.outSymbols.size() < k.symCount) k.outSymbols.resize(k.symCount, 0);        // a packet begun on the streaming path
                k.outSymbols[k.symCount - 1] = sym;
            }
            if (o.nPkt)                                                                          // postMessage  :295-298
            {
                Packet p;
                p.channel = int32_t(c);
                p.round = k.callCount;                                                           // = the lock-step round where every stream began with the run
                p.off = dm->pktSyms.size();
                p.len = k.symCount;
                p.endPos = int64_t(k.pos) + r.consumed; p.freqError = k.freqError;               // as frameStep records them (st.pos is the mirror's here)
                dm->pktSyms.insert(dm->pktSyms.end(), k.outSymbols.begin(), k.outSymbols.begin() + long(k.symCount));
                dm->packets.push_back(p);
            }
            k.pos += size_t(r.consumed);                                                         // consume(total)  :320
            k.callCount++;
            dm->workCalls++;
            if (dm->tracing) k.trace.push_back(r);
        }
        rounds++;
    }
    if (roundsOut) *roundsOut = rounds;
    return LORAHIP_OK;
}

} } // namespace lorahip::demod
