"""lorahip_demod_home.h::Home -- which copy of the level-3 demod object's frame state and open packets is current, and which streams
the next run reads -- compiled for the HOST alone and driven without a GPU.

The transition table below was written from the units as they were BEFORE the type existed (the `file:line` of each row): the flags
a transition sets and clears, from every one of the 2^11 values of the flags. The walks replay, event by event, what the units do to
the type in the sequences of C ABI calls named in their docstrings; after every event the invariants (consistent()) hold and every
query equals its definition over the flags, and after every call the flags are the ones the units' code leaves."""
import ctypes as C
import os
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lora_sdr_amd", "csrc")
FLAGS = ["devStateFresh", "headStale", "mirrorsStale", "posOnDevice", "activatePending", "devCarryValid", "hostCarryStale", "append",
         "appendFresh", "geomApplied", "uniform"]                      # Home::bits(), bit 0 first
BIT = {n: 1 << i for i, n in enumerate(FLAGS)}
PENDING, DRAINED, THROUGH = 0, 1, 2                                    # Home::RunEnd

# (transition, arguments, start flags it applies to (None: all), sets, clears, where the writes stood)
TABLE = [
    ("placedUniform", (640, 700, 0), None, "uniform appendFresh", "geomApplied posOnDevice append", "lorahip_demod.cpp:25-28"),
    ("placedUniform", (640, 700, 1), lambda f: f("appendFresh"), "uniform append", "geomApplied posOnDevice", "lorahip_demod.cpp:25-28"),
    ("placedUniform", (640, 700, 1), lambda f: not f("appendFresh"), "uniform append", "geomApplied", "lorahip_demod.cpp:25-28"),
    ("placedSegments", (), None, "geomApplied appendFresh", "uniform posOnDevice append", "lorahip_demod.cpp:34-35"),
    ("geometryApplied", (), None, "geomApplied", "", "lorahip_demod_rounds.cpp:86"),
    ("runCompleted", (), lambda f: f("append"), "", "appendFresh", "lorahip_demod.cpp:65"),
    ("runCompleted", (), lambda f: not f("append"), "", "", "lorahip_demod.cpp:65"),
    ("rewound", (), None, "appendFresh", "", "lorahip_demod.cpp:364"),
    ("steadyStep", (700, 900), lambda f: f("appendFresh"), "uniform append mirrorsStale headStale", "geomApplied posOnDevice", "lorahip_demod_pipe.cpp:29-31"),
    ("steadyStep", (700, 900), lambda f: not f("appendFresh"), "uniform append mirrorsStale headStale", "geomApplied", "lorahip_demod_pipe.cpp:29-31"),
    ("activateDeferred", (), None, "activatePending", "", "lorahip_demod.cpp:325"),
    ("activateRidesLaunch", (), None, "", "activatePending", "lorahip_demod_stream.cpp:448"),
    ("activateAppliedToMirrors", (), None, "", "activatePending devStateFresh", "lorahip_demod_stream.cpp:237-238"),
    ("recordBuffersRegrown", (), None, "", "devStateFresh headStale", "lorahip_demod_stream.cpp:353-354"),
    ("carryRowsRegrown", (), None, "", "devCarryValid", "lorahip_demod_stream.cpp:342"),
    ("stateUploaded", (), None, "", "headStale", "lorahip_demod_stream.cpp:406"),
    ("carryRowsBypassed", (), None, "", "devCarryValid", "lorahip_demod_stream.cpp:433"),
    ("runBegins", (), None, "mirrorsStale", "devStateFresh", "lorahip_demod_stream.cpp:449-450"),
    ("launchSummarised", (), None, "headStale", "", "lorahip_demod_stream.cpp:477"),
    ("runEnded", (PENDING,), None, "devStateFresh posOnDevice devCarryValid hostCarryStale", "", "lorahip_demod_stream.cpp:514-520"),
    ("runEnded", (DRAINED,), None, "devStateFresh posOnDevice devCarryValid", "hostCarryStale", "lorahip_demod_stream.cpp:514-520"),
    ("runEnded", (THROUGH,), None, "devStateFresh posOnDevice", "devCarryValid hostCarryStale", "lorahip_demod_stream.cpp:514-515, 522"),
    ("headFetched", (), None, "", "headStale", "lorahip_demod_stream.cpp:77"),
    ("mirrorsSynced", (), None, "", "mirrorsStale", "lorahip_demod_stream.cpp:230"),
    ("openPacketsFetched", (), None, "", "hostCarryStale", "lorahip_demod_stream.cpp:210"),
    ("pendingDrained", (), None, "", "hostCarryStale", "lorahip_demod_stream.cpp:174"),
    ("roundsBegin", (), None, "", "devStateFresh devCarryValid", "lorahip_demod_rounds.cpp:116-117"),
    ("takenOver", (), None, "", "devStateFresh", "lorahip_demod_pipe.cpp:211, lorahip_demod_resident.cpp:256"),
    ("givenBack", (), None, "devStateFresh posOnDevice mirrorsStale headStale devCarryValid hostCarryStale", "", "lorahip_demod_pipe.cpp:40-41"),
    ("aborted", (), None, "", "devStateFresh", "lorahip_demod_resident.cpp:83"),
    ("censusFailed", (), None, "devStateFresh", "", "lorahip_demod_resident.cpp:251"),
]
ARGS = {"placedUniform": "size_t a, size_t b, int c", "steadyStep": "size_t a, size_t b", "runEnded": "int a"}
CALL = {"placedUniform": "a, b, c != 0", "steadyStep": "a, b", "runEnded": "Home::RunEnd(a)"}
# every query, as the units' expressions over the flags were
QUERIES = {
    "continues": lambda f: f("append") and not f("appendFresh"),
    "appendBegun": lambda f: not f("appendFresh"),
    "deviceCurrent": lambda f: f("devStateFresh"),
    "activateWaiting": lambda f: f("activatePending"),
    "headLags": lambda f: f("headStale"),
    "mirrorsLag": lambda f: f("mirrorsStale"),
    "pinnedPosCurrent": lambda f: f("posOnDevice"),
    "readPinnedPos": lambda f: f("mirrorsStale") and f("posOnDevice"),                              # lorahip_demod.cpp:817, :839
    "placementUntouched": lambda f: not f("posOnDevice") and f("uniform") and not f("geomApplied"),  # lorahip_demod.cpp:823
    "geometryCurrent": lambda f: f("geomApplied"),
    "carryRowsValid": lambda f: f("devCarryValid"),
    "openPacketsLag": lambda f: f("hostCarryStale"),
    "isUniform": lambda f: f("uniform"),
}
INVARIANTS = [lambda f: not f("hostCarryStale") or f("devCarryValid"), lambda f: not f("activatePending") or f("devStateFresh"),
              lambda f: not f("headStale") or f("mirrorsStale"), lambda f: f("appendFresh") or f("append"),
              lambda f: not f("append") or f("uniform"), lambda f: f("geomApplied") or f("uniform")]

SHIM = """
#include "lorahip_demod_home.h"
namespace lorahip { namespace demod {
struct HomeProbe
{
    static void set(Home &h, const unsigned b)
    {
        h.devStateFresh = b & 1; h.headStale = b & 2; h.mirrorsStale = b & 4; h.posOnDevice = b & 8; h.activatePending = b & 16; h.devCarryValid = b & 32;
        h.hostCarryStale = b & 64; h.append = b & 128; h.appendFresh = b & 256; h.geomApplied = b & 512; h.uniform = b & 1024;
    }
};
} }
using namespace lorahip::demod;
extern "C" {
Home *home_new() { return new Home(); }                     // value-initialised, as `new lorahip_demod()` makes its member
void home_free(Home *h) { delete h; }
void home_set(Home *h, unsigned b) { HomeProbe::set(*h, b); }
unsigned home_bits(const Home *h) { return h->bits(); }
int home_consistent(const Home *h) { return h->consistent(); }
int home_mayEnter(const Home *h, int anyOpen, int recordsPending) { return h->mayEnter(anyOpen != 0, recordsPending != 0); }
size_t home_spc(const Home *h) { return h->spc(); }
size_t home_stride(const Home *h) { return h->stride(); }
size_t home_prevValid(const Home *h) { return h->prevValid(); }
%s
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("home")
    src, so = str(d / "shim.cpp"), str(d / "libhome.so")
    fns = ["void home_%s(Home *h%s) { h->%s(%s); }" % (t, ", " + ARGS[t] if t in ARGS else "", t, CALL.get(t, "")) for t in dict.fromkeys(r[0] for r in TABLE)]
    fns += ["int home_%s(const Home *h) { return h->%s(); }" % (q, q) for q in QUERIES]
    with open(src, "w") as f:
        f.write(SHIM % "\n".join(fns))
    # no HIP include path and no HIP define: the header stands alone
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, src, "-o", so], check=True)
    L = C.CDLL(so)
    L.home_new.restype = C.c_void_p
    for name in ("spc", "stride", "prevValid"):
        getattr(L, "home_" + name).restype = C.c_size_t
    for t in dict.fromkeys(r[0] for r in TABLE):
        getattr(L, "home_" + t).restype = None
        getattr(L, "home_" + t).argtypes = [C.c_void_p] + {"placedUniform": [C.c_size_t, C.c_size_t, C.c_int], "steadyStep": [C.c_size_t, C.c_size_t], "runEnded": [C.c_int]}.get(t, [])
    for n in ["free", "set", "bits", "consistent", "mayEnter"] + list(QUERIES) + ["spc", "stride", "prevValid"]:
        fn = getattr(L, "home_" + n)
        fn.argtypes = [C.c_void_p] + {"set": [C.c_uint], "mayEnter": [C.c_int, C.c_int]}.get(n, [])
    return L


def mask(names):
    m = 0
    for n in names.split():
        m |= BIT[n]
    return m


def names(bits):
    return " ".join(n for n in FLAGS if bits & BIT[n])


def test_a_new_object_starts_as_before(lib):
    h = lib.home_new()
    assert names(lib.home_bits(h)) == "appendFresh geomApplied"
    assert lib.home_consistent(h) and lib.home_spc(h) == lib.home_stride(h) == lib.home_prevValid(h) == 0
    lib.home_free(h)


def test_every_transition_moves_exactly_the_flags_the_units_wrote(lib):
    h = lib.home_new()
    for name, args, when, sets, clears, where in TABLE:
        fn, s, c = getattr(lib, "home_" + name), mask(sets), mask(clears)
        assert s & c == 0
        for start in range(1 << len(FLAGS)):
            if when is not None and not when(lambda n: bool(start & BIT[n])):
                continue
            lib.home_set(h, start)
            fn(h, *args)
            got = lib.home_bits(h)
            assert got == (start | s) & ~c, "%s%r (%s) from [%s]: [%s]" % (name, args, where, names(start), names(got))
    # a start value is covered by exactly one row of a transition whose rows are conditional
    for name in ("placedUniform", "runCompleted", "steadyStep"):
        rows = [r for r in TABLE if r[0] == name and r[2] is not None]
        for start in range(1 << len(FLAGS)):
            hits = {}
            for r in rows:
                hits[r[1]] = hits.get(r[1], 0) + bool(r[2](lambda n: bool(start & BIT[n])))
            assert all(v == 1 for v in hits.values())
    lib.home_free(h)


def test_the_members_that_are_not_flags(lib):
    h = lib.home_new()
    lib.home_placedUniform(h, 640, 700, 1)
    assert (lib.home_spc(h), lib.home_stride(h), lib.home_prevValid(h)) == (640, 700, 0)
    lib.home_runCompleted(h)                                    # lorahip_demod.cpp:65: appendPrev = uniSpc
    assert lib.home_prevValid(h) == 640
    lib.home_steadyStep(h, 704, 900)                            # lorahip_demod_pipe.cpp:29-30
    assert (lib.home_spc(h), lib.home_stride(h), lib.home_prevValid(h)) == (900, 704, 900)
    lib.home_placedUniform(h, 100, 100, 0)
    lib.home_runCompleted(h)                                    # not an append run: nothing moves
    assert (lib.home_spc(h), lib.home_prevValid(h)) == (100, 900)
    lib.home_rewound(h)                                         # lorahip_demod.cpp:364
    assert lib.home_prevValid(h) == 0
    lib.home_free(h)


def test_queries_and_invariants_are_what_the_units_spelled_out(lib):
    h = lib.home_new()
    for start in range(1 << len(FLAGS)):
        lib.home_set(h, start)
        f = lambda n: bool(start & BIT[n])
        for q, want in QUERIES.items():
            assert bool(getattr(lib, "home_" + q)(h)) == bool(want(f)), "%s from [%s]" % (q, names(start))
        assert bool(lib.home_consistent(h)) == all(inv(f) for inv in INVARIANTS), names(start)
        for any_open in (0, 1):
            for pending in (0, 1):                              # lorahip_demod_pipe.cpp:23
                assert bool(lib.home_mayEnter(h, any_open, pending)) == (f("devStateFresh") and (f("devCarryValid") or not any_open) and not pending)
    lib.home_free(h)


class Obj:
    """The units' control flow around the type, event by event (what touches nothing of it is left out): every event is followed by
    the check of the invariants and of every query."""

    def __init__(self, lib):
        self.L, self.h = lib, lib.home_new()
        self.pending = types.SimpleNamespace(valid=False, any_open=False)      # PendingLaunch
        self.any_open = False                                                   # lastSum.anyOpen
        self.events = []

    def close(self):
        self.L.home_free(self.h)

    def q(self, name, *a):
        return bool(getattr(self.L, "home_" + name)(self.h, *a))

    def ev(self, name, *a):
        getattr(self.L, "home_" + name)(self.h, *a)
        self.events.append(name)
        bits = self.L.home_bits(self.h)
        f = lambda n: bool(bits & BIT[n])
        assert self.L.home_consistent(self.h), "%s left [%s]" % (name, names(bits))
        for k, want in QUERIES.items():
            assert self.q(k) == bool(want(f)), (name, k)

    def flags(self):
        return names(self.L.home_bits(self.h))

    # lorahip_demod_stream.cpp
    def ensure_head(self):
        if self.q("headLags"):
            self.ev("headFetched")

    def drain_pending(self):
        if self.pending.valid:
            self.ensure_head()                                  # drainLaunch
            self.pending.valid = False
            self.ev("pendingDrained")

    def sync_mirrors(self):
        if self.q("mirrorsLag"):
            self.ensure_head()
        self.ev("mirrorsSynced")
        if self.q("openPacketsLag"):                            # fetchCarry
            self.ev("openPacketsFetched")
        if self.q("activateWaiting"):
            self.ev("activateAppliedToMirrors")

    def run_stream(self, open_in, open_out, launches=1, tracing=False, long_packets=False, regrow_carry=False, regrow_records=False):
        """-> what the run did: resident (no upload), activate (as a flag), carry_uploaded (the mirrors' open packets sent up)"""
        self.drain_pending()
        if regrow_carry:
            self.sync_mirrors(); self.ev("carryRowsRegrown")
        if regrow_records:
            self.sync_mirrors(); self.ev("recordBuffersRegrown")
        resident = self.q("deviceCurrent")
        activate = resident and self.q("activateWaiting")
        carry_in = open_in and not activate
        if not resident:
            self.sync_mirrors(); self.ev("stateUploaded")
        use_carry = not long_packets
        uploaded = use_carry and carry_in and not self.q("carryRowsValid")
        if not use_carry:
            if self.q("openPacketsLag"):
                self.sync_mirrors()
            self.ev("carryRowsBypassed")
        if activate:
            self.ev("activateRidesLaunch")
        self.ev("runBegins")
        for i in range(launches):
            self.ev("launchSummarised")
            if i + 1 < launches or tracing:
                self.ensure_head()                              # drainLaunch
        last_pending = not tracing
        self.ev("runEnded", THROUGH if not (use_carry and launches == 1) else PENDING if last_pending else DRAINED)
        self.any_open = open_out
        self.pending.valid, self.pending.any_open = last_pending, open_out
        return dict(resident=resident, activate=activate, carry_uploaded=uploaded)

    # lorahip_demod_rounds.cpp
    def run_rounds(self):
        self.sync_mirrors()
        if not self.q("geometryCurrent"):
            self.ev("geometryApplied")
        self.ev("roundsBegin")

    # lorahip_demod.cpp
    def run(self, spc, stride=None, append=False, mode=1, **kw):
        self.ev("placedUniform", spc, stride or spc, int(append))
        self.drain_pending()
        cont = self.q("continues")
        r = self.run_stream(**kw) if mode == 1 else self.run_rounds()
        self.ev("runCompleted")
        return cont, r

    def activate(self):
        if self.q("deviceCurrent"):
            self.ev("activateDeferred")
        else:
            self.sync_mirrors()

    def clear_packets(self):
        if self.pending.valid:
            if self.pending.any_open and not self.q("carryRowsValid"):
                self.drain_pending()
            else:
                self.pending.valid = False

    def consumed_reads(self):
        """where lorahip_demod_consumed finds the positions"""
        if self.q("readPinnedPos"):
            self.ensure_head()
            return "pinned"
        return "zero" if self.q("placementUntouched") else "mirrors"

    # lorahip_demod_pipe.cpp / lorahip_demod_resident.cpp
    def may_enter(self):
        return self.q("continues") and not self.q("activateWaiting") and self.q("mayEnter", int(self.any_open), int(self.pending.valid))


@pytest.fixture
def obj(lib):
    o = Obj(lib)
    yield o
    o.close()


def test_walk_uniform_runs_and_a_deferred_activate(obj):
    """create; a uniform run; a second one, resident, no upload asked for; activate(); a run that applies it as a flag"""
    _, r = obj.run(4096, open_in=False, open_out=True)
    assert r == dict(resident=False, activate=False, carry_uploaded=False)
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale appendFresh uniform"
    n = len(obj.events)
    _, r = obj.run(4096, open_in=True, open_out=True)
    assert r == dict(resident=True, activate=False, carry_uploaded=False) and "stateUploaded" not in obj.events[n:] and "mirrorsSynced" not in obj.events[n:]
    obj.activate()
    assert obj.q("activateWaiting") and obj.q("deviceCurrent")
    _, r = obj.run(4096, open_in=True, open_out=False)
    assert r == dict(resident=True, activate=True, carry_uploaded=False) and not obj.q("activateWaiting")
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale appendFresh uniform"


def test_walk_streaming_then_rounds_then_streaming(obj):
    """a streaming run with an open packet; set_mode(2); rounds (the mirrors are synced, the carry fetched, the device copies go stale);
    a streaming run, which uploads the state and finds the carry rows not valid"""
    obj.run(4096, open_in=False, open_out=True)
    obj.clear_packets()                                         # (the records are dropped: the open packets are in the carry rows alone)
    n = len(obj.events)
    obj.run(4096, mode=2)
    assert obj.events[n:] == ["placedUniform", "headFetched", "mirrorsSynced", "openPacketsFetched", "geometryApplied", "roundsBegin", "runCompleted"]
    assert obj.flags() == "appendFresh geomApplied uniform"
    _, r = obj.run(4096, open_in=True, open_out=True)
    assert r == dict(resident=False, activate=False, carry_uploaded=True)
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale appendFresh uniform"


def test_walk_append_runs_and_a_rewind(obj):
    """append run, append run, rewind, append run: "continues" is false, true, false"""
    conts = [obj.run(1000, 4096, append=True, open_in=False, open_out=False)[0], obj.run(2000, 4096, append=True, open_in=False, open_out=False)[0]]
    assert obj.q("pinnedPosCurrent") and obj.L.home_prevValid(obj.h) == 2000
    obj.ev("rewound")
    assert obj.L.home_prevValid(obj.h) == 0
    conts.append(obj.run(500, 4096, append=True, open_in=False, open_out=False)[0])
    assert conts == [False, True, False]
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale append uniform"


@pytest.mark.parametrize("exit_", ["flush", "census", "abort"])
def test_walk_pipelined_and_resident_receivers(obj, exit_):
    """a streaming run; the pipeline (or the resident kernel) takes the state over; three steps; flush; an accessor drains. The resident
    receiver also with the census failing before any step, and with an abort after the steps."""
    obj.run(1000, 4096, append=True, open_in=False, open_out=True)
    assert not obj.may_enter()                                  # the run's records are still on the device
    obj.clear_packets()                                         # (lorahip_demod_receive clears after packing: dropped, the carry rows hold the open packets)
    assert obj.may_enter() and obj.q("openPacketsLag")
    before = obj.flags()
    obj.ev("takenOver")
    assert not obj.q("deviceCurrent") and not obj.may_enter()
    if exit_ == "census":
        obj.ev("aborted"); obj.ev("censusFailed")               # residentAbort, then lorahip_demod_resident.cpp:251
        assert obj.flags() == before and obj.may_enter()
        return
    for k in range(3):
        obj.ev("steadyStep", 4096, 1000 + 300 * (k + 1))
        assert obj.q("continues") and obj.consumed_reads() == "pinned" and not obj.q("headLags")
    assert obj.L.home_prevValid(obj.h) == 1900
    if exit_ == "abort":
        obj.ev("aborted")
        # the state is distrusted, the carry flags are what they were at the takeover (kept as the units had it)
        assert obj.flags() == "mirrorsStale posOnDevice devCarryValid hostCarryStale append uniform"
        _, r = obj.run(2200, 4096, append=True, open_in=True, open_out=False)
        assert r == dict(resident=False, activate=False, carry_uploaded=False)
        return
    obj.ev("givenBack"); obj.pending.valid = False              # leaveStateOnDevice
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale append uniform"
    assert obj.may_enter()
    obj.drain_pending()                                         # an accessor: nothing is pending after a flush
    obj.sync_mirrors()                                          # ... and one that reads the mirrors
    assert obj.flags() == "devStateFresh posOnDevice devCarryValid append uniform" and obj.consumed_reads() == "mirrors"


def test_walk_buffers_regrown_with_a_packet_open(obj):
    """the record buffers, then the carry rows, regrown between runs with a packet open"""
    obj.run(1000, 4096, append=True, open_in=False, open_out=True)
    _, r = obj.run(9000, 16384, append=True, open_in=True, open_out=True, regrow_records=True)
    assert r == dict(resident=False, activate=False, carry_uploaded=False)          # the state goes up again, the carry rows stayed valid
    assert obj.q("carryRowsValid")
    _, r = obj.run(9500, 16384, append=True, open_in=True, open_out=True, regrow_carry=True)
    assert r == dict(resident=True, activate=False, carry_uploaded=True)            # the state stayed, the open packets go up from the mirrors
    assert obj.flags() == "devStateFresh headStale mirrorsStale posOnDevice devCarryValid hostCarryStale append uniform"


def test_walk_a_resumed_run(obj):
    """more than one launch: the carry rows are not valid afterwards and the mirrors hold the symbols"""
    obj.run(1000, 4096, append=True, open_in=False, open_out=True)
    obj.run(3000, 4096, append=True, open_in=True, open_out=True, launches=3)
    assert not obj.q("carryRowsValid") and not obj.q("openPacketsLag") and obj.q("deviceCurrent")
    assert not obj.may_enter()
    obj.clear_packets()                                         # a packet is open and the rows are not valid: the records are drained, not dropped
    assert "pendingDrained" == obj.events[-1] and not obj.pending.valid
    _, r = obj.run(3500, 4096, append=True, open_in=True, open_out=False)
    assert r == dict(resident=True, activate=False, carry_uploaded=True)


def test_walk_a_placement_nothing_ran_on(obj):
    """placement set, nothing run: "nothing has run on this placement" is true and the positions read as zero; after the run it is false"""
    obj.run(1000, open_in=False, open_out=False)
    assert obj.consumed_reads() == "pinned"
    obj.ev("placedUniform", 2000, 2000, 0)
    assert obj.q("placementUntouched") and obj.consumed_reads() == "zero"
    obj.run_stream(open_in=False, open_out=False); obj.ev("runCompleted")
    assert not obj.q("placementUntouched") and obj.consumed_reads() == "pinned"
    obj.ev("placedSegments")
    assert not obj.q("placementUntouched") and obj.consumed_reads() == "mirrors"
