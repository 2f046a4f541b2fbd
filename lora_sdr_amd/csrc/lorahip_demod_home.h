// Level 3, the demod object: WHERE the channels' frame-machine state and the symbols of the packets still open live, and which
// streams the next run reads. HOST code, nothing from HIP: the host compiler takes this header alone (tests/test_demod_home_cpu.py).
//
// | copy                               | where                          | made current by                                              | query                          |
// |------------------------------------|--------------------------------|--------------------------------------------------------------|--------------------------------|
// | frame state, the device block      | sDev (StreamLayout::oState)    | a completed streaming run; a receiver that gave it back      | deviceCurrent()                |
// | frame state, its pinned head copy  | sHost                          | ensureHead (headFetched); an upload from the mirrors         | !headLags()                    |
// | frame state, the Channel mirrors   | ch[].state .. ch[].callCount   | syncMirrors (mirrorsSynced); the host-driven rounds          | !mirrorsLag()                  |
// | read positions                     | the pinned copy's pos / ch[]   | a streaming run fills the first, a new placement voids it    | readPinnedPos(), pinnedPosCurrent(), placementUntouched() |
// | open packets, the carry rows       | dCarry                         | a streaming run of ONE launch; a receiver that gave it back  | carryRowsValid()               |
// | open packets, the mirrors          | ch[].outSymbols                | fetchCarry, drainPending, a resumed run, the rounds          | !openPacketsLag()              |
// | placement of uniform streams       | ch[].base / len / pos          | applyGeometry (geometryApplied)                              | geometryCurrent()              |
//
// Every change is a transition named after what happened; the units that drive the object (lorahip_demod*.cpp) call those and the
// queries and never see a flag.
#pragma once
#include <cstddef>

namespace lorahip { namespace demod {

class Home
{
public:
    //! how a streaming run left the open packets: in the carry rows with its records still on the device (the mirrors' symbols lag);
    //! in the carry rows, the records drained in the run (a traced run); or handed on through the mirrors (a resumed run, no carry rows)
    enum RunEnd { CARRY_RECORDS_PENDING, CARRY_RECORDS_DRAINED, THROUGH_MIRRORS };

    // ---- the placement of the next run's streams
    //! n_channels x spc samples, `stride` apart. An append run continues every channel's stream where the last append run left it
    //! (unless there was none: create, rewind, any other kind of run in between); any other run begins new streams at sample 0, and
    //! the positions in the pinned copy are not theirs
    void placedUniform(const size_t spc, const size_t stride, const bool appendRun)
    {
        uniform = true; uniSpc = spc; uniStride = stride; geomApplied = false;
        if (!appendRun || appendFresh) posOnDevice = false;
        if (!appendRun) appendFresh = true;
        append = appendRun;
    }
    void placedSegments() { uniform = false; geomApplied = true; posOnDevice = false; append = false; appendFresh = true; }   // each a new stream; the caller fills ch[]
    void geometryApplied() { geomApplied = true; }                                     // ch[].base / len / pos filled from the uniform placement
    void runCompleted() { if (append) { appendFresh = false; appendPrev = uniSpc; } }  // without error: the next append run continues an append run
    void rewound() { appendFresh = true; appendPrev = 0; }                             // the next append run starts new streams
    //! a pipelined or resident step over the first nValid samples of rows `stride` apart: an append run, after which the pinned copy and the mirrors lag
    void steadyStep(const size_t stride, const size_t nValid) { placedUniform(nValid, stride, true); appendPrev = nValid; mirrorsStale = true; headStale = true; }

    // ---- activate()
    void activateDeferred() { activatePending = true; }                                // the device holds the state: it travels with the next launch as a flag
    void activateRidesLaunch() { activatePending = false; }                            // ... the kernel resets the state when it loads it
    void activateAppliedToMirrors() { activatePending = false; devStateFresh = false; }    // ... or the mirrors were reset: the device lacks it, the next run uploads

    // ---- a streaming run
    void recordBuffersRegrown() { devStateFresh = false; headStale = false; }          // the pinned head goes with them; syncMirrors has read what there was
    void carryRowsRegrown() { devCarryValid = false; }                                 // syncMirrors has fetched what they held
    void stateUploaded() { headStale = false; }                                        // from the mirrors: the pinned copy IS what the device is given
    void carryRowsBypassed() { devCarryValid = false; }                                // packets longer than the rows: this run takes them from the mirrors
    void runBegins() { devStateFresh = false; mirrorsStale = true; }                   // BEFORE the first launch: a launch that fails leaves exactly this
    void launchSummarised() { headStale = true; }                                      // the pinned per-channel state and counts lag the device now
    void runEnded(const RunEnd how)                                                    // the device holds the state and this placement's read positions
    {
        devStateFresh = true; posOnDevice = true;
        devCarryValid = how != THROUGH_MIRRORS; hostCarryStale = how == CARRY_RECORDS_PENDING;
    }

    // ---- bringing copies to the host
    void headFetched() { headStale = false; }                                          // ensureHead
    void mirrorsSynced() { mirrorsStale = false; }                                     // syncMirrors, BEFORE it fetches the open packets (which can fail)
    void openPacketsFetched() { hostCarryStale = false; }                              // fetchCarry: the carry rows into the mirrors' outSymbols
    void pendingDrained() { hostCarryStale = false; }                                  // drainLaunch wrote the pending launch's open packets into the mirrors
    void roundsBegin() { devStateFresh = false; devCarryValid = false; }               // the rounds change the mirrors (synced, packets fetched): the device copies go stale

    // ---- the pipelined and the resident receiver
    void takenOver() { devStateFresh = false; }                                        // until it gives the state back only IT knows where the state stands
    //! flushed: as a streaming run of one launch leaves the object -- state, positions, open packets on the device, the pinned copy and the mirrors behind
    void givenBack() { devStateFresh = true; posOnDevice = true; mirrorsStale = true; headStale = true; devCarryValid = true; hostCarryStale = true; }
    //! the resident kernel was told to leave with its steps' bookkeeping incomplete. The device block is no longer taken as it stands:
    //! the next streaming run syncs the mirrors (from the pinned copy, fetched again where it lags) and uploads them. The two carry
    //! flags stay what they were at the takeover: rows that counted as valid then still feed that run's open packets, though the
    //! aborted steps may have rewritten them. Whether the open packets survive an abort can therefore not be read from here;
    //! ADVICE.md calls this doubtful. Kept exactly as it was.
    void aborted() { devStateFresh = false; }
    void censusFailed() { devStateFresh = true; }                                      // before any step was rung: the state on the device is what it was

    // ---- queries
    bool continues() const { return append && !appendFresh; }          //!< the run continues every channel's stream (callCount and pos go on)
    bool appendBegun() const { return !appendFresh; }                  //!< an append run has completed since create / rewind / another kind of run
    bool deviceCurrent() const { return devStateFresh; }               //!< a streaming run need not upload the state
    bool activateWaiting() const { return activatePending; }           //!< activate() applied neither to the device state nor to the mirrors yet
    bool headLags() const { return headStale; }
    bool mirrorsLag() const { return mirrorsStale; }
    bool pinnedPosCurrent() const { return posOnDevice; }              //!< the pinned copy's pos / callCount belong to the CURRENT placement
    bool readPinnedPos() const { return mirrorsStale && posOnDevice; } //!< the read positions are in the pinned copy, not in the mirrors
    bool placementUntouched() const { return !posOnDevice && uniform && !geomApplied; }    //!< nothing has run on this placement: every position is 0
    bool geometryCurrent() const { return geomApplied; }
    bool carryRowsValid() const { return devCarryValid; }
    bool openPacketsLag() const { return hostCarryStale; }             //!< ch[].outSymbols lack what the runs since the last drain received
    //! a pipelined or resident receiver may be entered: state and open packets on the device, no records of a launch left there
    bool mayEnter(const bool anyOpen, const bool recordsPending) const { return devStateFresh && (devCarryValid || !anyOpen) && !recordsPending; }
    bool isUniform() const { return uniform; }                         //!< n_channels x spc() samples, stride() apart
    size_t spc() const { return uniSpc; }
    size_t stride() const { return uniStride; }
    size_t prevValid() const { return appendPrev; }                    //!< samples per channel the last append run (or steady step) was given

    /*! What holds between two calls of the C ABI, error exits included. NOT among them, though they look true:
     *   deviceCurrent -> pinnedPosCurrent   a new non-append placement clears the latter alone
     *   carryRowsValid -> deviceCurrent     runBegins / takenOver / aborted leave the rows' flag (a failed launch exits so)
     *   openPacketsLag -> mirrorsLag        syncMirrors marks the mirrors synced before fetchCarry can fail
     *   headLags -> !deviceCurrent          a completed run leaves both; nor the reverse: consumed() fetches the head of a current state
     *   deviceCurrent -> mirrorsLag         an accessor that syncs the mirrors leaves the device current */
    bool consistent() const
    {
        return (!hostCarryStale || devCarryValid)    // what clears devCarryValid follows a syncMirrors that succeeded (it clears hostCarryStale), or clears both
            && (!activatePending || devStateFresh)   // set only while fresh; what clears fresh first syncs the mirrors (applying it) or needs steadyAppend (none waiting)
            && (!headStale || mirrorsStale)          // set together, or after runBegins; mirrorsSynced only behind an ensureHead that succeeded (sDev and sHost come as a pair)
            && (appendFresh || append)               // runCompleted clears appendFresh in an append run only; a placement of another kind sets it again
            && (!append || uniform)                  // placedUniform alone sets append; placedSegments clears both
            && (geomApplied || uniform);             // placedUniform alone clears geomApplied; placedSegments sets it
    }

    //! for the tests: bit 0 devStateFresh, 1 headStale, 2 mirrorsStale, 3 posOnDevice, 4 activatePending, 5 devCarryValid,
    //! 6 hostCarryStale, 7 append, 8 appendFresh, 9 geomApplied, 10 uniform
    unsigned bits() const
    {
        return unsigned(devStateFresh) | unsigned(headStale) << 1 | unsigned(mirrorsStale) << 2 | unsigned(posOnDevice) << 3 | unsigned(activatePending) << 4 |
               unsigned(devCarryValid) << 5 | unsigned(hostCarryStale) << 6 | unsigned(append) << 7 | unsigned(appendFresh) << 8 | unsigned(geomApplied) << 9 |
               unsigned(uniform) << 10;
    }

private:
    friend struct HomeProbe;            // the CPU test defines it, to start a transition from any value of the flags; the library does not
    // (value-initialised with the object: false / 0 unless said otherwise)
    bool devStateFresh, headStale, mirrorsStale, posOnDevice, activatePending, devCarryValid, hostCarryStale, append;
    bool appendFresh = true, geomApplied = true;
    bool uniform; size_t uniSpc, uniStride, appendPrev;
};

} } // namespace lorahip::demod
