// The LoRaDemod frame state machine (lorahip_framestep.h::frameStep) as the streaming kernels run it: per work() call, in the
// registers of every lane that owns the channel (replicated, so no broadcast is needed); the writer lane appends the
// symbol / packet / trace records -- into the arrays of StreamOut, below. Shared by lorahip_stream.hip (a channel per T <= 64
// lanes) and lorahip_stream_wide.hip (a channel per workgroup).
#pragma once
#include "lorahip_device.h"
#include "lorahip_framestep.h"

namespace lorahip {

//! where one channel's records of this launch go, and how many there are so far
struct StreamOut
{
    lorahip_work_result *out;
    short *symOut;
    StreamPacket *pktOut;
    StreamSignal *sigOut;
    int calls, nSym, nPkt, nSig;
    __device__ __forceinline__ void init(const StreamArgs &s, const unsigned channel)
    {
        out = s.calls ? s.calls + (size_t)channel * s.cap : nullptr;
        symOut = s.symOut + (size_t)channel * s.symStride;
        pktOut = s.pktOut + (size_t)channel * s.capPkt;
        sigOut = s.sigOut ? s.sigOut + (size_t)channel * s.capPkt : nullptr;
        calls = nSym = nPkt = nSig = 0;
    }
    //! The packet the channel is inside continues behind the symbols it has already (flag bit 2; `st` with the launch's flags
    //! applied): the channel's lanes (lane `t` of `T`) copy them from the carry rows to the head of the symbol row.
    //! `copy` false (the resident receiver): they stay where they are -- the symbol row holds only what the launch adds (nSym counts from
    //! 0), whoever packs the packet takes its first symbols from the carry row (residentPackOwn), and carryOut appends behind them.
    __device__ __forceinline__ void carryIn(const StreamArgs &s, const StreamState &st, const unsigned channel, const int t, const int T, const bool copy = true)
    {
        if (!copy || !(s.flags & 4) || st.state != ST_DATASYMBOLS) return;
        const int k = st.symCount < s.carryCap ? st.symCount : s.carryCap;
        const short *src = s.carry + (size_t)channel * s.carryCap;
        // (read at agent scope: in the resident receiver the row was written by this compute unit a step ago and an older copy of the
        // line may still sit in its L1)
        // (eight loads in flight per lane before the stores -- instead of a round trip to L2 per element, six per step with 8 lanes per
        // channel -- was measured in the resident receiver and LOST: 2.36 -> 1.79 Gsym/s at SF7, the registers it takes are spilled in the
        // window loop; profiles/r06/s26_*)
        for (int i = t; i < k; i += T) symOut[i] = __hip_atomic_load(const_cast<short *>(src) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nSym = st.symCount;
    }
    //! ... and a channel that ends the launch inside a packet leaves the packet's symbols in the carry rows (flag bit 3): the last
    //! k = min(symCount, nSym) entries of its row, written by the writer lane, are the packet's LAST k symbols and go to the entries
    //! symCount - k ... of the carry row. With carryIn's copy k = symCount (the whole packet, from entry 0); without it only what the
    //! launch added is appended -- with short receiver steps one turn of the loop instead of mtu / T, a round trip to L2 each.
    //! `acrossWaves`: the channel's lanes span several wavefronts (demodStreamWide): the other wavefronts must not load before the
    //! writer's wavefront has waited for its stores -- a workgroup barrier between the two (every thread of the workgroup calls this,
    //! the flags and the loop exit are workgroup-uniform).
    __device__ __forceinline__ void carryOut(const StreamArgs &s, const StreamState &st, const unsigned channel, const int t, const int T, const bool mine = true,
                                             const bool acrossWaves = false)
    {
        if (!(s.flags & 8)) return;                                 // uniform over the launch
        // The writer lane's stores have to be seen by its neighbours' loads. They are lanes of ONE wavefront, whose memory operations
        // go through one L1 in order: a fence -- the wait for the stores -- orders them, and the loads are made at agent scope (they
        // read L2, where the stores have landed), so no stale L1 line can be hit.
        // An agent-scope FENCE would do too, but it writes the whole L2 back (buffer_wbl2): 90 us per launch at 2048 wavefronts.
        // (the wait is spelled out: a workgroup-scope fence does not wait for global stores on this target -- the wavefronts of a workgroup
        // share an L1 --, and the loads below go past the L1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (acrossWaves) __syncthreads();                           // ... and the writer's wavefront has got here: its last symbol is in L2
        if (!mine || st.state != ST_DATASYMBOLS) return;
        int k = st.symCount < nSym ? st.symCount : nSym;
        int at = st.symCount - k;                                   // (0 with carryIn's copy: nSym >= symCount there)
        if (at + k > s.carryCap) { at = 0; k = k < s.carryCap ? k : s.carryCap; }     // (a packet longer than the carry row: as ever, its last k symbols from entry 0 -- such receivers keep the host path)
        short *dst = s.carry + (size_t)channel * s.carryCap + at;
        for (int i = t; i < k; i += T) dst[i] = __hip_atomic_load(symOut + (nSym - k + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

} // namespace lorahip
