"""lorahip_rx_info without a GPU: (1) the identities the kernels rely on -- data_pos = end_pos - len * N and
sync_pos = data_pos - (N/4 + freq_error/2) - N -- hold on the reference's own call trace, for the restated block and, where it has
been built, the verbatim LoRaDemod.cpp; (2) lorahip_framestep.h::frameStep, compiled for the host, records the end position and the
frequency error of every packet and the position of every signal as the definition (tests/rx_info_def.py) has them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rx_info_def as D
from oracle.oracle import Oracle, Ref
from test_frame_machine_cpu import CSRC, MTU, N, SF, SYNC, THRESH, FRAMESYNC, Result, StreamState, make_stream, oracle_calls
from test_gpu_receiver import _streams

SEED = 902        # a seed of the recipe at which freq_error / 2 is non-zero with both signs at SF7 and at SF10 (asserted below)


def _cases(orc, sf):
    """(stream, mtu, threshold): the recipe of test_gpu_receiver._streams; MTU 8 ends every packet at the MTU, MTU 64 with the squelch
    at 3 dB ends them at the squelched padding window"""
    host = _streams(orc, np.random.default_rng(SEED), sf, 6)
    return [(host[c], mtu, th) for mtu, th in ((8, -30.0), (64, 3.0)) for c in range(host.shape[0])]


@pytest.mark.parametrize("sf", [7, 10])
def test_identities_hold_on_the_reference_trace(sf):
    orc = Oracle()
    ref = Ref() if Ref.available() else None
    n = 1 << sf
    half, by_mtu, by_squelch = set(), 0, 0
    for x, mtu, th in _cases(orc, sf):
        r = orc.demod_run(sf, x, mtu=mtu, thresh=th, keep=False)
        info, pos = D.from_oracle(r)
        lens = [len(q) for _, q in r["packets"]]
        assert D.identities(info, lens, n)
        # a packet's sync_pos is the position of exactly one signal of its channel: the join key
        assert all((pos == s).sum() == 1 for s in info[:, D.SYNC_POS]) and np.all(np.diff(pos) > 0)
        half |= set(np.trunc(info[:, D.FREQ_ERROR] / 2).astype(int).tolist())
        by_mtu += sum(ln == mtu for ln in lens)
        by_squelch += sum(ln < mtu for ln in lens)
        if ref is not None:
            v = ref.demod_run(sf, x, mtu=mtu, thresh=th)
            vinfo, vpos = D.from_ref(v)
            assert np.array_equal(vinfo, info) and np.array_equal(vpos, pos)
            assert D.identities(vinfo, [len(q) for _, q in v["packets"]], n)
    assert min(half) < 0 < max(half), "freq_error / 2 of both signs: %r" % sorted(half)
    assert by_mtu >= 6 and by_squelch >= 6, "packets ended by the MTU and by the squelch"


SHIM = r"""
#include "lorahip_framestep.h"
using namespace lorahip;
extern "C" void fm_step_info(StreamState *st, unsigned mtu, int value, float power, float powerAvg, float snr, float fIndex, int squelched, int syncd,
                             int match0, int match1, lorahip_work_result *r, long long *rec)
{
    StreamArgs s{};
    s.mtu = mtu;
    short sym = 0;
    StreamPacket pkt = {0, 0};
    StreamSignal sig = {0, 0, 0.0f, 0.0f};
    pkt.endPos = -1; pkt.freqError = 0x7fffffff; sig.pos = -1;
    OneCall o = {r, &sym, &pkt, &sig, 0, 0, 0, 0};
    frameStep<128>(*st, s, o, true, value, power, powerAvg, snr, fIndex, squelched != 0, syncd != 0, match0 != 0, match1 != 0, 0, 0.0f);
    const lorahip_rx_info q = rxInfo(pkt.endPos, pkt.len, pkt.freqError, 128);
    rec[0] = o.nPkt; rec[1] = o.nSig; rec[2] = pkt.len; rec[3] = sig.pos; rec[4] = sig.error;
    rec[5] = q.end_pos; rec[6] = q.data_pos; rec[7] = q.sync_pos; rec[8] = q.freq_error;
    rec[9] = (long long)sizeof(StreamState); rec[10] = (long long)sizeof(lorahip_rx_info);
}
"""


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    d = tmp_path_factory.mktemp("framestep_info")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-shared", "-fPIC", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + CSRC, src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.fm_step_info.restype = None
    lib.fm_step_info.argtypes = [C.POINTER(StreamState), C.c_uint, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.POINTER(Result), C.POINTER(C.c_longlong)]
    return lib.fm_step_info


def test_frame_step_records_positions_and_error(step):
    """the four-frame stream of test_frame_machine_cpu (packets ended by the MTU and by the squelch, a frame that posts nothing), call by
    call with the oracle's detects: what frameStep writes into the packet and signal records is the definition on the oracle's trace"""
    orc = Oracle()
    iq = make_stream(orc)
    want = oracle_calls(orc, iq)
    state = np.array([w["state"] for w in want])
    sig_calls = np.nonzero(state == D.DOWNCHIRP1)[0]
    info, sig_pos = D.rx_info([w["consumed"] for w in want], [i for i, w in enumerate(want) if w["packet_len"]], sig_calls,
                              [want[i]["sig_error"] for i in sig_calls], np.nonzero(state == D.DATASYMBOLS)[0])
    assert info.shape == (3, 4) and sig_pos.size == 3 and D.identities(info, [w["packet_len"] for w in want if w["packet_len"]], N)

    st, r, rec = StreamState(), Result(), (C.c_longlong * 11)()
    pos, got_info, got_pos = 0, [], []
    for w in want:
        before = st.state
        d0 = orc.detect_batch(SF, iq, offsets=[pos], chirp_sel=1 if st.downTable else 0, fine_idx0=st.fineTuneIndex, fine_err=st.finefreqError)
        value, power, pavg, findex = int(d0["sym"][0]), d0["power"][0], d0["powerAvg"][0], d0["fIndex"][0]
        snr = np.float32(power - pavg)
        squelched = bool(snr < np.float32(THRESH))
        st.fineTuneIndex = int(d0["fineIdxOut"][0])
        syncd = (not squelched) and (st.prevValue + 4) // 8 == 0
        match0 = (value + 4) // 8 == (SYNC >> 4)
        match1 = False
        if before == FRAMESYNC and syncd and match0:
            d1 = orc.detect_batch(SF, iq, offsets=[pos + N], chirp_sel=0, fine_idx0=st.fineTuneIndex, fine_err=st.finefreqError)
            match1 = (int(d1["sym"][0]) + 4) // 8 == (SYNC & 0xf)
            power, pavg, findex = d1["power"][0], d1["powerAvg"][0], d1["fIndex"][0]
        step(C.byref(st), MTU, value, power, pavg, snr, findex, squelched, syncd, match0, match1, C.byref(r), rec)
        assert r.consumed == w["consumed"] and before == w["state"]
        if rec[0]:
            assert rec[2] == w["packet_len"]
            got_info.append(list(rec[5:9]))
        if rec[1]:
            assert rec[4] == w["sig_error"]
            got_pos.append(rec[3])
        pos += r.consumed
    assert rec[9] == 40 and rec[10] == 32                 # StreamState keeps its layout; lorahip_rx_info is four int64
    assert got_pos == sig_pos.tolist()
    assert got_info == info.tolist()
