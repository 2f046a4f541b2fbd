"""TEST INFRASTRUCTURE ONLY -- the crafted packet sets of tests/test_gpu_decoder_edges.py and their expected outcomes from the CPU oracle.

The sets are built with tests/codec_def.py, the outcomes come from oracle.decode alone; tests/test_codec_def_cpu.py asserts on the CPU that
every set holds what it was made for (every outcome class, the decode boundary straddled), so a set that degenerates is caught without
a GPU. Generators and tables are cached per process: a reference is computed once and shared; nobody writes into what they return.

A decoder configuration is the tuple of the golden file codec_kat.npz: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr,
data_length)."""
import functools

import numpy as np

import codec_def as D

RDD_TO_CR = {0: "4/4", 1: "4/5", 2: "4/6", 3: "4/7", 4: "4/8"}

H_CONFIGS = [(7, 0, 4), (9, 7, 1), (12, 0, 0), (8, 5, 3), (10, 0, 2)]        # (sf, ppm, rdd) of set H
E_SYMBOL_SIZES = [(7, 0), (9, 7), (12, 0), (8, 5)]                          # (sf, ppm) of set E
# payload bytes of set E: with 1 the decoded range ends with the first block (and its odd nibble) wherever that block is long enough, with
# 8 it ends behind it. Whether the nibble count is odd after the first block does not depend on the length: it is (PPM + 1) & 1 with a
# header and PPM & 1 without, so header on / off gives every symbol size one case of each (asserted in test_codec_def_cpu.py).
E_LENGTHS = (1, 8)
G_STRIDES = (16, 64, 160, 512)


def oracle_table(oracle, cfg, packets):
    """[(bytes or None, dropped)] per packet"""
    sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = cfg
    return [oracle.decode(sf, s, ppm=ppm, cr=RDD_TO_CR[rdd], crcc=bool(crcc), interleaving=bool(inter), error_check=bool(ec),
                          explicit=bool(explicit), hdr=bool(hdr), data_length=dlen) for s in packets]


def outcome(row):
    out, dropped = row
    return "dropped" if dropped else "nothing" if out is None else "bytes"


def table_arrays(table):
    """a table as (out_len (P,) int32 with -1 = nothing posted, dropped (P,) int32, bytes (P, W) uint8 zero-padded)"""
    n = np.array([-1 if o is None else o.size for o, _ in table], np.int32)
    d = np.array([dr for _, dr in table], np.int32)
    b = np.zeros((len(table), max(1, int(n.max()))), np.uint8)
    for i, (o, _) in enumerate(table):
        if o is not None:
            b[i, :o.size] = o
    return n, d, b


def as_rows(packets, stride):
    """zero-padded rows of `stride` symbols and each packet's own count"""
    rows = np.zeros((len(packets), stride), np.uint16)
    for i, s in enumerate(packets):
        rows[i, :min(len(s), stride)] = s[:stride]
    return rows, np.array([len(s) for s in packets], np.int32)


# ---- set H: one body under every header -------------------------------------------------------------------------------------
def header_grid(lengths):
    """every (length, crc flag, rate field 0..7): three flat arrays, length slowest"""
    ln, crc, rate = np.meshgrid(np.asarray(lengths), np.arange(2), np.arange(8), indexing="ij")
    return ln.reshape(-1), crc.reshape(-1), rate.reshape(-1)


@functools.lru_cache(maxsize=None)
def set_h(sf, ppm, rdd, max_len=255, true_len=20, n_symbols=None):
    """(H, n) packets: one body of true_len random bytes + its crc, coded at the decoder's rate and extended with zero-nibble blocks
    until a header announcing max_len + 5 bytes fits (2 * (max_len + 5) nibbles), under every header of header_grid(0..max_len).
    With n_symbols the body is cut or zero-padded to that many symbols instead."""
    P = ppm or sf
    rng = np.random.default_rng(1000 * sf + 10 * P + rdd)
    payload = rng.integers(0, 256, true_len).astype(np.uint8)
    have = -(-(2 * (true_len + 2) + 5) // P) * P
    extra = 0 if n_symbols else max(0, -(-(2 * (max_len + 5) - have) // P))
    body, _ = D.build(sf, payload, ppm, rdd, True, True, n_blocks=extra)
    if n_symbols:
        body = np.concatenate([body, np.zeros(n_symbols, np.uint16)])[:n_symbols]
    packets = D.set_header(body, sf, ppm, *header_grid(range(max_len + 1)))
    packets.setflags(write=False)
    return packets


@functools.lru_cache(maxsize=None)
def set_h_table(oracle, cfg, max_len=255, true_len=20, n_symbols=None):
    return oracle_table(oracle, cfg, set_h(cfg[0], cfg[1], cfg[2], max_len, true_len, n_symbols))


def check_set_h(tables_by_flags):
    """the conditions of set H on the oracle's results of one (sf, ppm, rdd): tables_by_flags[(hdr, crcc, ec)] -> table.
    Every configuration holds packets that produce bytes and packets that are dropped; without the header in the output (hdr = 0) also
    packets that post nothing without a drop; with crcc = 0 and error_check = 0 at least half produce bytes (the valid rate fields
    0..4 are 5 of 8)."""
    for (hdr, crcc, ec), table in tables_by_flags.items():
        kinds = [outcome(r) for r in table]
        assert kinds.count("bytes") > 0 and kinds.count("dropped") > 0, (hdr, crcc, ec)
        if not hdr:
            assert kinds.count("nothing") > 0, (hdr, crcc, ec)
        if not crcc and not ec:
            assert 2 * kinds.count("bytes") >= len(kinds), (hdr, crcc, ec, kinds.count("bytes"))


# ---- set E: one bit of damage around the end of the decoded range ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def set_e(sf, ppm, rdd, explicit, length):
    """-> (packets (n, S) uint16, labels, c_end, odd). Packet 0 is clean: `length` random bytes + crc at rate rdd, three zero-nibble
    blocks behind what the length needs. labels[i] = (kind, codeword, bit): ("clean", -1, -1); ("flip", c, b) for every bit b of the
    codewords c = first payload codeword, PPM - 1, PPM, PPM + 1, c_end - 2 .. c_end + 1, the packet's last, and with a header 0..4;
    ("two", c, b) for bits b and b + 1 together, in a 4/8 codeword of the first block and in codeword PPM + 1 behind it.
    c_end / odd: codec_def.decoded_end for the bytes the packet announces (length + crc, + 3 header bytes)."""
    P = ppm or sf
    rng = np.random.default_rng(((sf * 16 + P) * 8 + rdd) * 64 + 2 * length + explicit)
    payload = rng.integers(0, 256, length).astype(np.uint8)
    clean, cw = D.build(sf, payload, ppm, rdd, bool(explicit), True, n_blocks=3)
    c_end, odd = D.decoded_end(P, bool(explicit), length + (5 if explicit else 2))
    first = D.N_HDR_CODEWORDS if explicit else 0
    where = sorted(set([first, P - 1, P, P + 1, c_end - 2, c_end - 1, c_end, c_end + 1, cw.size - 1] + list(range(first))))
    assert where[0] >= 0 and c_end + 1 < cw.size
    packets, labels = [clean], [("clean", -1, -1)]
    for c in where:
        for b in range(8 if c < P else 4 + rdd):
            packets.append(D.flip(clean, sf, ppm, rdd, c, b)); labels.append(("flip", c, b))
    for c in (first if first < P else 1, P + 1):               # (PPM 5 with a header: the first block is all header, damage its length)
        for b in (0, 2):
            packets.append(D.flip(D.flip(clean, sf, ppm, rdd, c, b), sf, ppm, rdd, c, b + 1)); labels.append(("two", c, b))
    packets = np.stack(packets)
    packets.setflags(write=False)
    return packets, labels, c_end, odd


def e_cfg(sf, ppm, rdd, explicit, length, ec):
    return (sf, ppm, rdd, 1, 1, ec, explicit, 0, length)


@functools.lru_cache(maxsize=None)
def set_e_table(oracle, sf, ppm, rdd, explicit, length, ec):
    return oracle_table(oracle, e_cfg(sf, ppm, rdd, explicit, length, ec), set_e(sf, ppm, rdd, explicit, length)[0])


def check_set_e(labels, c_end, table_off, table_on):
    """the boundary is straddled, from the oracle's results alone: with error_check on every one-bit damage in codeword c_end - 1 is
    dropped and every one in c_end gives exactly what the clean packet gives -- as it does with error_check off --, and the clean packet
    decodes either way"""
    clean = table_on[0]
    assert clean[0] is not None and clean[1] == 0 and table_off[0][0] is not None and np.array_equal(table_off[0][0], clean[0])
    inside = [i for i, (k, c, _) in enumerate(labels) if k == "flip" and c == c_end - 1]
    outside = [i for i, (k, c, _) in enumerate(labels) if k == "flip" and c == c_end]
    assert len(inside) >= 5 and len(outside) >= 5
    for i in inside:
        assert table_on[i][1] == 1 and table_on[i][0] is None, labels[i]
    for i in outside:
        assert table_on[i][1] == 0 and np.array_equal(table_on[i][0], clean[0]), labels[i]
        assert table_off[i][1] == 0 and np.array_equal(table_off[i][0], clean[0]), labels[i]


def e_groups():
    """every (sf, ppm, rdd, explicit, length) of set E"""
    return [(sf, ppm, rdd, explicit, length) for sf, ppm in E_SYMBOL_SIZES for rdd in (1, 2, 3, 4) for explicit in (1, 0) for length in E_LENGTHS]


# ---- set R: rows shorter than their packet ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def set_r(sf, ppm, rdd, length):
    """-> (packets (3, S) uint16, need): the packets of test_set_r_rows_shorter_than_the_packet -- an explicit-header packet of `length`
    bytes + crc, two zero-nibble blocks longer than it needs, clean, with one bit flipped in the last decoded codeword and in the one
    behind it -- and the symbols (whole interleaver blocks) its announced bytes need"""
    P = ppm or sf
    clean, _ = D.build(sf, np.random.default_rng(length).integers(0, 256, length).astype(np.uint8), ppm, rdd, True, True, n_blocks=2)
    c_end, _ = D.decoded_end(P, True, length + 5)
    need = D.num_symbols_def(-(-c_end // P) * P, P, rdd)
    packets = np.stack([clean, D.flip(clean, sf, ppm, rdd, c_end - 1, 0), D.flip(clean, sf, ppm, rdd, c_end, 0)])
    packets.setflags(write=False)
    return packets, need


# ---- the launch shape, restated from lorahip_codec.hip (decodeCaps, launchDecode, launchDecodeGroup) -----------------------------
def launch_shape(sf, ppm, rdd, explicit, data_length, stride):
    """-> (lanes per packet G, LDS bytes per packet, packets per workgroup). The tests cannot observe any of the three; this restatement
    only lets them assert that their inputs are the ones that select every group size and the reduced packets-per-workgroup launch."""
    P, bs = ppm or sf, 4 + rdd
    c_end = max(2 * (260 if explicit else data_length + 2), P + 1)
    sym_need = 8 + (-(-c_end // P) + 1) * bs
    sym_row = ((stride + 15) // bs + 1) * bs + 8
    sym_cap = min(sym_need, sym_row)
    cw_cap = (sym_cap // bs + 2) * P + 16
    lds = (2 * sym_cap + 2 * cw_cap + 15) & ~15
    G = 8 if sym_cap <= 48 else 16 if sym_cap <= 96 else 32 if sym_cap <= 200 else 64
    return G, lds, min(256 // G, (160 * 1024) // lds)


# ---- set P: slices so long that fewer packets fit a workgroup than it has lane groups --------------------------------------------
P_ROW = 16384
P_LENGTH = 4096


@functools.lru_cache(maxsize=None)
def set_p(ppm):
    """seven rows of 16384 symbols at SF7, no header, data_length 4096, crc, 4/8 -> (rows, nsyms). Rows 0-4: built packets with different
    payloads, the rest of the row random symbols (what a demodulator appends up to its MTU); row 5: one payload byte changed behind the
    crc; row 6: cut to 4000 symbols, the row behind them random and not part of the packet. At PPM 5 a packet is 13120 symbols. At PPM
    4 and 2 it is 16392 and 32792: the rows then hold its first 16384 and the reference drops every one of them (4098 bytes do not fit)."""
    rng = np.random.default_rng(40 + ppm)
    rows = rng.integers(0, 128, (7, P_ROW)).astype(np.uint16)
    nsyms = np.full(7, P_ROW, np.int32)
    for r in range(7):
        payload = rng.integers(0, 256, P_LENGTH).astype(np.uint8)
        if r == 5:
            crc = D.data_checksum_def(payload)
            payload[1234] ^= 0x40
            s, _ = D.build(7, np.concatenate([payload, np.array([crc & 0xff, crc >> 8], np.uint8)]), ppm, 4, False, False)
        else:
            s, _ = D.build(7, payload, ppm, 4, False, True)
        s = s[:4000] if r == 6 else s[:P_ROW]
        rows[r, :s.size] = s
        if r == 6:
            nsyms[r] = 4000
    rows.setflags(write=False)
    return rows, nsyms


def p_cfg(ppm, ec):
    return (7, ppm, 4, 1, 1, ec, 0, 0, P_LENGTH)


@functools.lru_cache(maxsize=None)
def set_p_table(oracle, ppm, ec):
    rows, nsyms = set_p(ppm)
    return oracle_table(oracle, p_cfg(ppm, ec), [rows[r, :nsyms[r]] for r in range(7)])
