// The LoRaDemod frame state machine (LoRaDemod.cpp:176-312): ONE work() call, written once. The streaming kernels run it in the
// registers of every lane that owns the channel (lorahip_framemachine.h has their record arrays, lorahip_stream.hip and
// lorahip_stream_wide.hip the loops around it); the host-driven rounds run it between two batch launches
// (lorahip_demod_rounds.cpp::runRounds). Nothing here is device-only: the .cpp units include it too. Tests pin it against the
// verbatim LoRaDemod.cpp through both.
#pragma once
#include "lorahip_internal.h"

namespace lorahip {

enum { ST_FRAMESYNC = 0, ST_DOWNCHIRP0, ST_DOWNCHIRP1, ST_QUARTERCHIRP, ST_DATASYMBOLS };

//! Room for the records of ONE work() call, with the members frameStep writes through (the kernels' StreamOut has rows of them): what
//! the host hands in. After the call nSym / nPkt / nSig say which of *symOut, *pktOut, *sigOut it wrote; *out is always written.
struct OneCall
{
    lorahip_work_result *out;
    short *symOut;
    StreamPacket *pktOut;
    StreamSignal *sigOut;       // nullable: signals are not kept as records (out->signals / sig_* carry them anyway)
    int calls, nSym, nPkt, nSig;
};

/*! One work() call after its detect(s): `value` .. `fIndex` are the locals of LoRaDemod::work() as they stand after the
 * optional second detect (:203 overwrites power / powerAvg / fIndex, not snr), `match1` the second sync-word test.
 *
 * Written WITHOUT branches on the state: where a wavefront carries several channels (demodStream, SF6-9) they are in different
 * states at the same time, and a switch over the five states executes every arm present in the wave one after the other under
 * exec masks (~200 instructions per call, profiles/r04). As selects it is ~40 operations whatever the mix; where the state is
 * wave-uniform (one channel per wavefront / workgroup) the same expressions run on the scalar unit. Only the record stores
 * remain predicated. Each line cites the statement of the reference it stands for.
 *
 * `o` is where the call's records go and how many there are so far: the kernels' StreamOut (lorahip_framemachine.h), or on the host
 * a OneCall (above). Of `s` only mtu is read. Everything the call is given arrives BY VALUE and the trace entry is written last of
 * the records, so a caller may pass members of the very lorahip_work_result that o.out points at (runRounds does: the first pass
 * leaves a call's detect results there) -- but only as copies made before the call, never through a reference to it. */
template <int N, class Out>
__host__ __device__ __forceinline__ void frameStep(StreamState &st, const StreamArgs &s, Out &o, const bool writer,
                                                   const int value, const float power, const float powerAvg, const float snr,
                                                   const float fIndex, const bool squelched, const bool syncd, const bool match0,
                                                   const bool match1, const int fineIdxBefore, const float fineErrBefore)
{
    const int stateBefore = st.state;
    const int fineIdxAfter = st.fineTuneIndex;      // the caller has committed window 0's steps (:160-162)
    const bool isFS = stateBefore == ST_FRAMESYNC, isD0 = stateBefore == ST_DOWNCHIRP0, isD1 = stateBefore == ST_DOWNCHIRP1;
    const bool isQC = stateBefore == ST_QUARTERCHIRP, isDA = stateBefore == ST_DATASYMBOLS;
    const bool sync3 = isFS && syncd && match0 && match1;                                                // :209
    const bool fsOpen = isFS && !sync3 && !squelched;                                                    // :217
    const bool fsQuiet = isFS && !sync3 && squelched;                                                    // :228
    const int error = value > N / 2 ? value - N : value;                                                 // :246-248, :262-264
    const int halfError = st.freqError / 2;                                                              // :278 (int division: towards zero)

    int total = N;
    total = sync3 ? 2 * N : total;                                                                       // :210
    total = fsOpen ? N - value : total;                                                                  // :219
    total = isQC ? N / 4 + halfError : total;                                                            // :278

    const int symCount = isQC ? 0 : st.symCount + (isDA ? 1 : 0);                                        // :279, out[_symCount++]  :290
    const bool post = isDA && ((unsigned)symCount >= s.mtu || squelched);                                // :291

    float ffe = st.finefreqError;
    ffe = fsOpen ? ffe + fIndex : ffe;                                                                   // :221
    ffe = isQC ? ffe + (float)halfError : ffe;                                                           // :277
    ffe = (fsQuiet || post) ? 0.0f : ffe;                                                                // :230, :299
    const int fti = fsQuiet ? 0 : st.fineTuneIndex;                                                      // :231
    const int freqError = isD0 ? error : (isD1 ? (st.freqError + error) / 2 : st.freqError);             // :249, :265
    // FRAMESYNC stays unless the sync words matched (:211); the chirp states and QUARTERCHIRP step on (:243, :256, :276); DATASYMBOLS
    // stays until the packet is posted (:300)
    const int next = isFS ? (sync3 ? ST_DOWNCHIRP0 : ST_FRAMESYNC) : (isDA ? (post ? ST_FRAMESYNC : ST_DATASYMBOLS) : stateBefore + 1);
    const int downTable = sync3 ? 1 : (isD1 ? 0 : st.downTable);                                        // :212, :257

    if (writer && isDA) o.symOut[o.nSym] = (short)value;                                                 // out[_symCount++] = value  :290
    // postMessage  :295-298; with it where the call ends in the stream (consume(total), :320) and the frame's frequency error
    if (writer && post) { StreamPacket q; q.callIndex = st.callCount; q.len = symCount; q.endPos = st.pos + total; q.freqError = st.freqError; q.pad = 0; o.pktOut[o.nPkt] = q; }
    if (o.sigOut)                                                                                        // uniform over the launch
    {
        // emitSignal("error" / "power" / "snr") as a record of its own (:267-269): the caller evaluated the logarithms for this call
        if (writer && isD1) { StreamSignal g; g.callIndex = st.callCount; g.error = freqError; g.power = power; g.snr = snr; g.pos = st.pos; o.sigOut[o.nSig] = g; }
        o.nSig += isD1 ? 1 : 0;
    }
    if (writer && o.out)
    {
        lorahip_work_result r;
        r.consumed = total;
        r.state_before = stateBefore;
        r.value = value;
        r.power = power; r.power_avg = powerAvg; r.snr = snr; r.f_index = fIndex;
        r.worked = 1;
        r.packet_len = post ? symCount : 0;
        r.signals = isD1 ? 1 : 0;
        r.sig_error = isD1 ? freqError : 0;
        r.sig_power = isD1 ? power : 0.0f;
        r.sig_snr = isD1 ? snr : 0.0f;
        r.fine_idx_before = fineIdxBefore; r.fine_idx_after = fineIdxAfter; r.fine_err_before = fineErrBefore; r.reserved = 0;
        o.out[o.calls] = r;
    }
    o.nSym += isDA ? 1 : 0;
    o.nPkt += post ? 1 : 0;
    o.calls++;
    st.state = next; st.downTable = downTable; st.freqError = freqError; st.fineTuneIndex = fti; st.finefreqError = ffe;
    st.symCount = symCount;
    st.prevValue = (short)value;                                                                         // :326
    st.pos += total;                                                                                     // consume(total)  :320
    st.callCount++;
}

} // namespace lorahip
