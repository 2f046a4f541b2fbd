"""The definition of lorahip_rx_info and of a signal's position, in numpy, from the call trace of ONE channel's stream -- what the
tests hold the library to. Nothing here knows how the library computes them.

With consumed[i] what call i of LoRaDemod::work() consumes, P(i) = consumed[0] + .. + consumed[i-1] is where call i starts. For a
packet posted by call k, whose frame's DOWNCHIRP1 call (the one that emits the signals, LoRaDemod.cpp:267-269) is j and whose first
DATASYMBOLS call is m:

    end_pos = P(k + 1)      data_pos = P(m)      sync_pos = P(j)      freq_error = the "error" call j emits

and a signal's position is P(j) of the call j that emits it."""
import numpy as np

END_POS, DATA_POS, SYNC_POS, FREQ_ERROR = range(4)
DOWNCHIRP1, DATASYMBOLS = 2, 4


def starts(consumed):
    """P(0) .. P(n): where every call starts, and where the last one ends"""
    return np.concatenate([[0], np.cumsum(np.asarray(consumed, np.int64))]).astype(np.int64)


def rx_info(consumed, post_calls, signal_calls, signal_errors, data_calls):
    """consumed: per call; post_calls: the calls that posted a packet, ascending; signal_calls / signal_errors: the calls that emitted
    the signals and the "error" each emitted; data_calls: the DATASYMBOLS calls. Returns ((P, 4) int64 info, (S,) int64 signal
    positions)."""
    P = starts(consumed)
    signal_calls, data_calls = np.asarray(signal_calls, np.int64), np.asarray(data_calls, np.int64)
    info = np.zeros((len(post_calls), 4), np.int64)
    for p, k in enumerate(post_calls):
        before = np.nonzero(signal_calls < k)[0]
        assert before.size, "a packet without a DOWNCHIRP1 call before it in this trace"
        j = int(signal_calls[before[-1]])                           # the frame's DOWNCHIRP1 call
        m = int(data_calls[data_calls > j][0])                      # its first DATASYMBOLS call
        assert m <= k
        info[p] = (P[k + 1], P[m], P[j], signal_errors[before[-1]])
    return info, P[signal_calls]


def from_oracle(run):
    """... of oracle.demod_run()'s dict (the restated block, pinned to the verbatim one)"""
    calls = run["calls"]
    state = np.array([c["state"] for c in calls], np.int64)
    return rx_info([c["consumed"] for c in calls], [k for k, _ in run["packets"]], np.nonzero(state == DOWNCHIRP1)[0],
                   [g[0] for g in run["signals"]], np.nonzero(state == DATASYMBOLS)[0])


def from_ref(run):
    """... of Ref.demod_run()'s dict (the verbatim LoRaDemod.cpp): its DOWNCHIRP1 call is the unlabelled one behind "DC" (:245, :259),
    its DATASYMBOLS calls are labelled "S<n> .." (:304), its signals come as ("error", v), ("power", v), ("snr", v) per emission"""
    labels = run["labels"]
    sig = [i for i in range(1, len(labels)) if labels[i - 1] == "DC"]
    data = [i for i, s in enumerate(labels) if s[:1] == "S" and s[1:2].isdigit()]        # ("SYNC" is FRAMESYNC's, :213)
    errors = [int(v) for name, v in run["signals"] if name == "error"]
    assert len(errors) == len(sig)
    return rx_info(run["consumed"], [k for k, _ in run["packets"]], sig, errors, data)


def identities(info, lens, N):
    """what the kernels rely on (include/lorahip.h): data_pos = end_pos - len * N, sync_pos = data_pos - (N/4 + freq_error/2) - N, with
    C's int division (towards zero)"""
    info, lens = np.asarray(info, np.int64), np.asarray(lens, np.int64)
    half = np.trunc(info[:, FREQ_ERROR] / 2).astype(np.int64)
    return (np.array_equal(info[:, DATA_POS], info[:, END_POS] - lens * N) and
            np.array_equal(info[:, SYNC_POS], info[:, DATA_POS] - (N // 4 + half) - N))
