// Level 3 of the C ABI, the demod object: what the translation units that drive it share -- the object itself, the types of its
// members, and the functions that cross from one unit to another. HOST code only, private to those units:
//   lorahip_demod.cpp           the C entry points, the placement of a run's streams, runAny
//   lorahip_demod_rounds.cpp    the host-driven rounds (mode 2)
//   lorahip_demod_stream.cpp    the streaming run, its records and the Channel mirrors
//   lorahip_demod_pipe.cpp      the pipelined receiver (lorahip_demod_receive, async = 2)
//   lorahip_demod_resident.cpp  the resident receiver's host side (async = 3)
//   lorahip_demod_ports.cpp     the debug-port replay, the trace and its labels
#pragma once
#include "lorahip_own.h"
#include "lorahip_framestep.h"
#include "lorahip_demod_home.h"
#include <chrono>
#include <vector>

namespace lorahip { namespace demod {

struct Channel
{
    int state;
    bool downTable;         // _chirpTable == _downChirpTable
    short prevValue;
    int freqError;
    int fineTuneIndex;
    float finefreqError;
    size_t symCount;
    std::vector<int16_t> outSymbols;
    size_t base, len, pos;  // stream placement in the device buffer, read position
    int64_t callCount;      // work() calls since the stream began (a run that does not continue a stream starts it at 0)
    size_t runStart;        // read position when the last run began (append runs continue; the port replay starts there)
    std::vector<lorahip_work_result> trace;
    size_t traceStart;      // first trace entry of the last run
    size_t traceSymCount0;  // _symCount when the trace began (labels "S<n>" continue a packet that was open then)
    size_t portFft, portDec, portRaw;   // frames / samples the last run produced on the debug ports
};

//! the frame machine's members between a Channel mirror and the state the streaming kernels keep. `pos` and `callCount` are not
//! among them: the mirrors hold them wider, and whether they travel depends on the run (runStream, syncMirrors).
inline void toStreamState(const Channel &k, StreamState &st)
{
    st.state = k.state; st.downTable = k.downTable ? 1 : 0; st.prevValue = k.prevValue; st.freqError = k.freqError;
    st.fineTuneIndex = k.fineTuneIndex; st.finefreqError = k.finefreqError; st.symCount = int(k.symCount);
}
inline void fromStreamState(Channel &k, const StreamState &st)
{
    k.state = st.state; k.downTable = st.downTable != 0; k.prevValue = short(st.prevValue); k.freqError = st.freqError;
    k.fineTuneIndex = st.fineTuneIndex; k.finefreqError = st.finefreqError; k.symCount = size_t(st.symCount);
}

//! one posted packet: its symbols are pktSyms[off, off+len) of the owning demod (flat storage: tens of thousands of
//! packets per run must not cost an allocation each)
struct Packet
{
    int32_t channel;
    int64_t round;
    size_t off, len;
    int64_t endPos;         // lorahip_rx_info::end_pos and ::freq_error (the other two positions follow from these and len: rxInfo)
    int32_t freqError;
};

//! one emission of the block's "error" / "power" / "snr" signals (LoRaDemod.cpp:267-269)
struct Signal
{
    int32_t channel;
    int64_t round;
    int32_t error;
    float power, snr;
    int64_t pos;            // where the emitting call began (= the sync_pos of the frame's packet)
};

inline size_t align256(const size_t x) { return (x + 255) & ~size_t(255); }

//! where the pieces of one streaming launch live inside dm->sDev (device) / dm->sHost (host mirror of the head)
struct StreamLayout
{
    size_t B, cap, capPkt, symStride;
    bool tracing, signals;
    size_t oBase, oLen, oState, oN, oNSym, oNPkt, oNSig, oNear, oSum, oEnd, oPkt, oSym, oSig, oCalls, total;
    void make(const size_t B_, const size_t cap_, const size_t capPkt_, const bool tracing_, const size_t carryCap_ = 0, const bool signals_ = false)
    {
        B = B_; cap = cap_; capPkt = capPkt_; tracing = tracing_; signals = signals_;
        symStride = cap_ + carryCap_;                    // a channel's symbol row: what the launch may add behind what it was handed
        size_t cur = 0;
        auto carve = [&cur](const size_t bytes) { const size_t o = cur; cur += align256(bytes); return o; };
        oBase = carve(B * sizeof(long long)); oLen = carve(B * sizeof(long long));
        oState = carve(B * sizeof(StreamState));
        oN = carve(B * sizeof(int)); oNSym = carve(B * sizeof(int)); oNPkt = carve(B * sizeof(int)); oNSig = carve(B * sizeof(int));
        oNear = carve(2 * sizeof(unsigned));
        oSum = carve(sizeof(StreamSummary));
        oEnd = carve(B * sizeof(int2));
        oPkt = carve(B * capPkt * sizeof(StreamPacket));
        oSym = carve(B * symStride * sizeof(short));
        oSig = carve(signals ? B * capPkt * sizeof(StreamSignal) : 0);
        oCalls = carve(tracing ? B * cap * sizeof(lorahip_work_result) : 0);
        total = cur;
    }
};

//! The records of the LAST streaming launch of a run stay on the device until somebody needs them on the host: a receive chain
//! that hands the packets to the batched decoder (lorahip_demod_packets_to_device) never does, and then nothing but the
//! per-channel state and counts (52 B per channel) crosses PCIe per run.
struct PendingLaunch
{
    bool valid;
    StreamLayout lay;
    size_t firstNewPacket;          // index in dm->packets of the first packet of the run this launch belongs to
    int64_t rounds;
    size_t packets, packetSyms;     // what draining will append
    size_t signals;
    bool anyCarryIn, anyOpen;       // a channel entered the launch inside a packet / leaves it inside one
    double drainMs;                 // LORAHIP_DEMOD_TIMING
};

//! the PIPELINED receiver (lorahip_demod_receive, async = 2; see pipeStep): two record sets, their summaries and events
struct Pipe
{
    bool active;                    // steps are in flight: only receive / flush may touch the object
    unsigned k;                     // steps launched since the pipeline was entered
    Stream side;                    // step k's packets are packed HERE while step k + 1's kernel runs on the launch stream (declared before
                                    // the events and buffers used on it: they are released first)
    DevBuf<char> dev[2];            // record sets (a StreamLayout each; the state and the carry rows are the object's own)
    StreamLayout lay[2];
    HostBuf<StreamSummary> hSum;    // [2] pinned and mapped: the summary kernel writes here directly (no copy to enqueue)
    Event ev[2];
    bool pending[2];                // the set's kernel has been launched, its summary not read yet
    bool held[2];                   // the set's summary has been read, its packets are still in the set (rows too small: nothing is lost)
    size_t nPk[2]; int64_t nCalls[2];   // ... what that summary said
    size_t nSig[2]; bool sigs[2];       // ... and the signals kept in the set (the step ran with lorahip_demod_set_signals on)
    Event packDone;                 // the launch stream waits for this before anything later (the next kernel reuses the record set, the caller reads the rows)
    Event entry;                    // ... and the side stream for this: where the launch stream stood when the call began (the caller's
                                    // consumer of the rows handed out by the call before, earlier packing on the launch stream)
};

//! the RESIDENT receiver (lorahip_demod_receive, async = 3): one launch across the steps, lorahip_streamkernel.h (RES)
struct Resident
{
    bool active;                    // the kernel is on the device: only receive (async = 3) / flush may touch the object
    bool unavailable;               // tried and refused for this object (no instance, the grid not resident at once, a step timed out)
    unsigned seq;                   // steps rung
    unsigned reported;              // steps whose report the caller has had
    Stream run;                     // the kernel's stream (declared before what the kernel uses: released last)
    DevBuf<ResidentCtl> ctl;        // device: the mirror of the ring, the steps' counters
    HostBuf<ResidentHost> host;     // pinned and mapped: the ring the host writes, the steps' reports, the abort flag
    DevBuf<char> rec;               // the channels' records of a step (a StreamLayout; the state and the carry rows are the object's own)
    StreamLayout lay;
    Event ev;
    unsigned grid;
    size_t lastValid;
    bool lastMore;                  // the last reported step left a channel with samples it could not record
    bool sigs;                      // the launch keeps signal records
    bool tail;                      // the last step left fewer than 16 valid samples per row untouched (the flush's ordinary step takes them)
    unsigned nRep; size_t repPk[RES_DEPTH_MAX + 1], repSg[RES_DEPTH_MAX + 1];   // the steps the last call reported, oldest first (lorahip_demod_receive_steps)
    unsigned depth;                 // steps the caller lets the receiver run ahead of the last report (1 .. RES_DEPTH_MAX): it has depth + 1 sets of rows
    // LORAHIP_RESIDENT_DEBUG prints these at the flush: where the host's share of a step goes
    uint64_t dbgReports, dbgImmediate, dbgCalls;
    double dbgWaitNs, dbgBetweenNs;
    std::chrono::steady_clock::time_point dbgLast;
};

} } // namespace lorahip::demod

// Made by `new lorahip_demod()`, which value-initialises: a member without a default below starts at zero, false or null.
struct lorahip_demod
{
    int streamGrid;                  // lorahip_demod_set_stream_grid: 0 default, < 0 one workgroup per channel set, > 0 at most that many workgroups
    size_t streamCapMax;             // lorahip_demod_set_record_capacity: 0 = no bound beyond the library's own
    int streamLanes;                 // lorahip_demod_set_stream_lanes: 0 by channel count, < 0 always 16 points per lane, else log2 of the lanes per channel
    unsigned coWaves;                // a part of a mixed object: the wavefronts its sibling parts put on the same device (the automatic choice counts them)
    lorahip::Composite *comp;        // non-null: the handle is a container of (device, SF) parts (lorahip_rx.cpp); nothing below is used then
    lorahip_ctx *ctx;
    size_t N, B;
    unsigned char sync = 0x12;       // LoRaDemod.cpp:71-73
    float thresh = -30.0f;
    size_t mtu = 256;
    bool tracing;
    int64_t workCalls;
    std::vector<lorahip::demod::Channel> ch;
    std::vector<lorahip::demod::Packet> packets;
    std::vector<int16_t> pktSyms;
    bool wantSignals;                // keep a record per DOWNCHIRP1 call (lorahip_demod_set_signals)
    std::vector<lorahip::demod::Signal> signals;
    lorahip_signal_rows sigRows;     // lorahip_demod_receive_signal_rows: where receiver steps deliver the signals (all pointers null: they are dropped)
    bool sigRowsOn;
    size_t lastSignals;              // ... how many the last receive / receive_flush delivered there
    // per-round staging (host pinned + device), sized for B windows
    lorahip::HostBuf<char> h; lorahip::DevBuf<char> d;
    lorahip::DevBuf<float> dIq;      // owned upload buffer for lorahip_demod_run
    int mode;                        // 0 auto, 1 device streaming kernel, 2 host-driven rounds
    // streaming path: device + pinned-host mirrors, grown on demand
    lorahip::DevBuf<char> sDev; lorahip::HostBuf<char> sHost; // (the pinned one holds the head only)
    lorahip::DevBuf<char> dDense; lorahip::HostBuf<char> hDense; // the used part of the record arrays, packed for the copy back
    lorahip::Event evK0, evK1;       // around the streaming kernel launches of a run (lorahip_demod_kernel_ms)
    lorahip::Event evJoin;           // lorahip_demod_stream_wait
    lorahip::DevBuf<char> dSumScratch; // streamSummary's partial records (more than 32768 channels)
    double kernelMs;
    int lastLaunches;                // streaming kernel launches of the last run
    lorahip_demod_ports ports;       // level-3 debug ports (all pointers null: off); DEVICE pointers (the library's own when the caller's are host buffers)
    lorahip_demod_ports hostPorts;   // the caller's host buffers (host_buffers == 1)
    lorahip::DevBuf<float> ownFft, ownDec, ownRaw; // device mirrors owned by the library for host_buffers
    bool portsOn, userTracing;
    lorahip::DevBuf<char> dPort;     // scratch of the port replay: window descriptors, replayed fft / dec windows
    int64_t nNearSquelch, nNearStep; // decisions float rounding could flip, since activate() (lorahip_demod_near_threshold)
    // Streaming mode keeps the per-channel frame-machine state ON THE DEVICE between runs (its pinned copy in sHost is what the host
    // reads); the Channel mirrors above are brought up to date only when somebody needs them (host-driven rounds, ports, accessors).
    // The symbols of open packets stay in the carry rows below likewise. Which copy is current, and the placement of the next run's
    // streams: lorahip_demod_home.h
    lorahip::demod::Home home;
    lorahip::StreamSummary lastSum;  // of the last streaming launch (valid while home.deviceCurrent())
    unsigned nearSeen[2];            // the kernels' running near-threshold counters as last read
    bool portCountsDirty = true;     // ch[].portFft / portDec / portRaw may be non-zero
    // The symbols of the packet a channel is INSIDE when a streaming run ends stay on the device too: the kernel leaves them in dCarry
    // and copies them to the head of the channel's symbol row at the start of the next run, then appends behind them -- a packet
    // that spans runs is assembled without the host (the running receiver: lorahip_demod_run_device_segments + packets_to_device).
    lorahip::DevBuf<short> dCarry; size_t carryCap; // [B][carryCap]
    size_t callsPerWindowQ8 = 288;   // streaming runs: work() calls per N samples the record buffers are sized for, in 1/256 (adapts, see runStream;
                                     // 1.125 to begin with)
    lorahip::demod::PendingLaunch pending; // records of the last streaming launch still on the device
    lorahip::demod::Pipe pipe;       // the pipelined receiver (lorahip_demod_receive, async = 2) ...
    lorahip::demod::Resident res;    // ... and the resident one (async = 3): at most one of them is active
    const float *stepIq; size_t stepStride;   // the rows the steps of either read (a flush that has to resume a full channel continues on them)
    std::vector<size_t> carry;       // per channel: symbols of a packet begun before the launch being drained
};

namespace lorahip { namespace demod {

// lorahip_demod.cpp
int drained(const lorahip_demod *dm);

// lorahip_demod_rounds.cpp
size_t roundStagingBytes(size_t B);
void applyGeometry(lorahip_demod *dm);
int runRounds(lorahip_demod *dm, const float *iqDev, int64_t *roundsOut);

// lorahip_demod_stream.cpp
int growDense(lorahip_demod *dm, size_t bytes);
bool pipeBusy(const lorahip_demod *dm);
int refuseWhilePiped(const lorahip_demod *dm);
StreamLayout headLayout(const lorahip_demod *dm);
int ensureHead(lorahip_demod *dm);
int drainPending(lorahip_demod *dm);
StreamState *hostStates(lorahip_demod *dm);
int syncMirrors(lorahip_demod *dm);
bool usesStreamKernel(const lorahip_demod *dm);
void streamCapacity(const lorahip_demod *dm, size_t maxLen, size_t &cap, size_t &capPkt);
void foldNear(lorahip_demod *dm, unsigned squelch, unsigned step);
StreamArgs makeStreamArgs(const lorahip_demod *dm, const float *iqDev, const StreamLayout &L, char *rec);
int runStream(lorahip_demod *dm, const float *iqDev, int64_t *roundsOut);

// lorahip_demod_pipe.cpp
bool steadyAppend(const lorahip_demod *dm, size_t rowStride, size_t nValid);
bool stateOnDevice(const lorahip_demod *dm);
void noteSteadyStep(lorahip_demod *dm, size_t rowStride, size_t nValid);
void leaveStateOnDevice(lorahip_demod *dm);
hipError_t packPackets(const lorahip_demod *dm, const StreamLayout &L, const char *rec, size_t n, uint16_t *syms, size_t symStride, int32_t *nsyms, int32_t *chan,
                       lorahip_rx_info *info, hipStream_t st);
hipError_t packSignals(const lorahip_demod *dm, const StreamLayout &L, const char *rec, size_t first, hipStream_t st);
bool rowsHold(const lorahip_packet_rows *rows, size_t n);
int pipeFlush(lorahip_demod *dm, const lorahip_packet_rows *rows, size_t *nPackets, int64_t *calls);
int pipeStep(lorahip_demod *dm, const float *iqDev, size_t rowStride, size_t nValid, const lorahip_packet_rows *rows, size_t *nPackets, int64_t *calls, bool &handled);

// lorahip_demod_resident.cpp
void residentAbort(lorahip_demod *dm);
int residentFlush(lorahip_demod *dm, size_t *nPackets, int64_t *calls);
int residentStep(lorahip_demod *dm, const float *iqDev, size_t rowStride, size_t nValid, const lorahip_packet_rows *rows, size_t *nPackets, int64_t *calls, bool &handled);

// lorahip_demod_ports.cpp
int fillPorts(lorahip_demod *dm, const float *iqDev);

} } // namespace lorahip::demod
