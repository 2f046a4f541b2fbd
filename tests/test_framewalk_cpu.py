"""lorahip_framewalk.h::FrameWalk -- the one copy of the transmit frame's float32 frequency / phase recurrence, which modFrames
(lorahip_tx.hip) and modFramesSched (lorahip_txsched.hip) both follow -- compiled for the HOST alone into a program of its own
(tests/framewalk_check.cpp), with the library's floating-point flags, and run without a GPU. The float32 phase of every body sample and
which samples are chirp samples at all must equal tests/modulator_def.py::mod_phases_def bit for bit. Phases only: the cos / sin of a
phase are the device's (tests/test_gpu_modulator_edges.py)."""
import os
import subprocess

import numpy as np
import pytest

from modulator_def import mod_phases_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lora_sdr_amd", "csrc")
S = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("framewalk") / "framewalk_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "framewalk_check.cpp"), "-o", path], check=True)
    return path


def frames_of(sf):
    """(symbols (F, S), counts (F,)): symbol 0, symbol N - 1 and a symbol >= N (not masked: f stays above fMax) in each of the three
    places, under every count -- none, one, all, a refused packet (-1) and more than the row holds (S + 1); the last two are silent"""
    N = 1 << sf
    rows = [[0, N - 1, N + 5], [N - 1, N + 5, 0], [N + 5, 0, N - 1]]
    syms, counts = [], []
    for count in (0, 1, S, -1, S + 1):
        for r in rows:
            syms.append(r)
            counts.append(count)
    return np.array(syms, np.uint16), np.array(counts, np.int32)


@pytest.mark.parametrize("sync", [0x12, 0x00, 0xff])
@pytest.mark.parametrize("sf", [6, 7])
def test_phases_and_live_samples_equal_the_definition(exe, tmp_path, sf, sync):
    syms, counts = frames_of(sf)
    F = len(counts)
    out = str(tmp_path / "walk.bin")
    args = [exe, out, str(sf), str(sync), str(S)]
    for f in range(F):
        args += [str(int(counts[f]))] + [str(int(s)) for s in syms[f]]
    run = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "framewalk_check: %d frames" % F

    want_phase, want_live = mod_phases_def(sf, syms, sync, counts)
    L = want_phase.shape[1]
    assert L == (14 + S) * (1 << sf) + (1 << sf) // 4
    raw = np.fromfile(out, np.uint8)
    assert raw.size == F * L * 5
    raw = raw.reshape(F, L * 5)
    phase = np.ascontiguousarray(raw[:, :L * 4]).view(np.float32)
    live = raw[:, L * 4:].astype(bool)

    assert np.array_equal(live, want_live)
    silent = (counts < 0) | (counts > S)
    assert not live[silent].any() and live[~silent, 0].all()
    for f in np.nonzero(~silent)[0]:                        # the body is live through the frame's own symbols and not behind them
        assert live[f].sum() == L - (S - counts[f]) * (1 << sf)
    # bit for bit, where there is a chirp (the definition's array holds a value behind the frame's own symbols too; the walker's is 0)
    assert np.array_equal(phase.view(np.uint32)[live], want_phase.view(np.uint32)[want_live])
    assert not phase.view(np.uint32)[~live].any()
