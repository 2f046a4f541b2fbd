"""TEST INFRASTRUCTURE ONLY -- the DEFINITION of a LoRa symbol packet as the codec kernels read it (include/lorahip.h: lorahip_decode_packets,
lorahip_encode_packets), restated in numpy from LoRaEncoder.cpp:161-233 on the primitives of LoRaCodes.hpp. No GPU, no library import.

A packet is a row of codewords, one nibble each:

    with an explicit header, five codewords  len >> 4, len & 15, flags, ck >> 4, ck & 15  (LoRaEncoder.cpp:188-200), flags = crc | rate << 1
        and ck = headerChecksum(len, flags) (LoRaCodes.hpp:31-55), Hamming(8,4) coded (:201-214), NOT whitened;
    then the payload (and its two crc bytes, LoRaEncoder.cpp:182-186 with LoRaCodes.hpp:80-93), low nibble of a byte first (:132-159);
    then pad nibbles up to a whole number of PPM codewords (:175). The reference reads them past the end of its byte vector; here they are 0.

The first PPM codewords (one interleaver block) are coded 4/8 whatever the coding rate, the rest at the rate `rdd` (:202, :209). A
codeword behind the header codewords is whitened with the low 4 + R bits of one of two byte-wide LFSRs (LoRaCodes.hpp:154-167; R = 4 in the
first block, rdd behind it; single parity, R = 1, has seeds of its own): the codeword at index p BEHIND THE HEADER CODEWORDS takes register
p mod 2 after p // 2 steps (LoRaEncoder.cpp:204, :211: the second call starts at PPM - header codewords). The encoder itself calls the
table form of the same sequence (LoRaCodes.hpp:128-148); tests/test_codec_def_cpu.py pins this file to its output.

A block of PPM codewords of 4 + R bits becomes 4 + R symbols of PPM bits: bit m of symbol k is bit k of codeword (m + k) mod PPM
(LoRaCodes.hpp:348-360). The first block makes 8 symbols. A symbol is then Gray -> binary (:187-194) and shifted left by sf - PPM
(LoRaEncoder.cpp:223-226).

What `build` adds to the encoder: the three header fields are free (a header may contradict its body), and the body may be extended by
whole blocks of zero nibbles, coded and whitened like pad nibbles. `flip` damages exactly one bit of one codeword, `set_header` swaps the
header codewords of a finished packet, `decoded_end` walks the decoder's loops (LoRaDecoder.cpp:315-361) to the first codeword they do
not read."""
import numpy as np

N_HDR_SYMBOLS = 8                                            # LoRaCodes.hpp:4-6
N_HDR_CODEWORDS = 5
HDR_RDD = 4

_SEEDS = ((0x6572D100E85C2EFF, 0xE85C2EFFFFFFFFFF), (0x05121100F8ECFEEF, 0xF8ECFEEFEFEFEFEF))   # LoRaCodes.hpp:155-156
_M64 = (1 << 64) - 1
_white_cache = {}


def _parity(v):
    v = np.asarray(v).astype(np.uint32)
    v = v ^ (v >> 16); v = v ^ (v >> 8); v = v ^ (v >> 4); v = v ^ (v >> 2); v = v ^ (v >> 1)
    return (v & 1).astype(np.uint8)


def whitening_def(single, n):
    """(2, n) uint8: the low byte of the even / odd register before each of its n steps (LoRaCodes.hpp:158-166, poly 0x1D on bytes)"""
    have = _white_cache.get(single)
    if have is None or have.shape[1] < n:
        n_make = max(n, 64)
        have = np.zeros((2, n_make), np.uint8)
        for o in (0, 1):
            r = _SEEDS[1 if single else 0][o]
            for k in range(n_make):
                have[o, k] = r & 0xff
                r = ((r >> 8) | ((((r >> 32) ^ (r >> 24) ^ (r >> 16) ^ r) & 0xff) << 56)) & _M64
        _white_cache[single] = have
    return have[:, :n]


def header_checksum_def(length, flags):
    """LoRaCodes.hpp:31-55: five parity bits over the 12 header bits w = len | flags << 8, spelled there as xor chains of named bits"""
    w = np.asarray(length).astype(np.uint32) | ((np.asarray(flags).astype(np.uint32) & 0xf) << 8)
    res = np.zeros(w.shape, np.uint8)
    for k, mask in enumerate((0xF12, 0x725, 0xA49, 0x18E, 0x0F0)):
        res |= _parity(w & mask) << k
    return res


def data_checksum_def(data):
    """LoRaCodes.hpp:80-93: CCITT crc, MSB first (:57-67), masked with two steps of an 8-bit LFSR (taps 0xB8) that steps once per byte"""
    res, v = 0, 0xff
    for byte in bytes(bytearray(np.asarray(data, np.uint8))):
        crc = res
        for _ in range(8):
            crc = ((crc << 1) ^ (0x1021 if crc & 0x8000 else 0)) & 0xffff
        v = ((v << 1) | (bin(v & 0xB8).count("1") & 1)) & 0xff
        res = crc ^ byte
    res ^= v
    v = ((v << 1) | (bin(v & 0xB8).count("1") & 1)) & 0xff
    return res ^ (v << 8)


def fec_def(nib, rdd):
    """one nibble -> a codeword of 4 + rdd bits: encodeHamming84sx / 74sx (LoRaCodes.hpp:201-214, :259-271), encodeParity64 / 54
    (:339-343, :319-323). 4/7 and 4/6 are the low bits of 4/8; 4/5 is one parity bit over the nibble."""
    x = np.asarray(nib).astype(np.uint8) & 0xf
    if rdd == 0:
        return x
    if rdd == 1:
        return x | (_parity(x) << 4)
    full = x | (_parity(x & 0x7) << 4) | (_parity(x & 0xE) << 5) | (_parity(x & 0xB) << 6) | (_parity(x & 0xD) << 7)
    return full & (0xff >> (4 - rdd))


def header_codewords_def(hdr_len, hdr_crc, hdr_rdd):
    """(..., 5) uint8: the header codewords of LoRaEncoder.cpp:189-199 for arrays of lengths, crc flags and rate fields (0..7: three bits)"""
    length = np.asarray(hdr_len).astype(np.uint8)
    flags = ((np.asarray(hdr_crc).astype(np.uint8) & 1) | ((np.asarray(hdr_rdd).astype(np.uint8) & 7) << 1)).astype(np.uint8)
    length, flags = np.broadcast_arrays(length, flags)
    ck = header_checksum_def(length, flags)
    return fec_def(np.stack([length >> 4, length & 15, flags, ck >> 4, ck & 15], axis=-1), HDR_RDD)


def interleave_def(codewords, ppm, width):
    """(..., B * ppm) codewords -> (..., B * width) Gray-domain symbols: LoRaCodes.hpp:348-360"""
    cw = np.asarray(codewords).astype(np.uint16)
    lead = cw.shape[:-1]
    cw = cw.reshape(lead + (-1, ppm))
    out = np.zeros(lead + (cw.shape[-2], width), np.uint16)
    for k in range(width):
        for m in range(ppm):
            out[..., k] |= ((cw[..., (m + k) % ppm] >> k) & 1) << m
    return out.reshape(lead + (-1,))


def deinterleave_def(gray, ppm, width):
    """the inverse (LoRaCodes.hpp:362-378): (..., B * width) Gray-domain symbols -> (..., B * ppm) codewords"""
    g = np.asarray(gray).astype(np.uint16)
    lead = g.shape[:-1]
    g = g.reshape(lead + (-1, width))
    out = np.zeros(lead + (g.shape[-2], ppm), np.uint8)
    for k in range(width):
        for m in range(ppm):
            out[..., (m + k) % ppm] |= (((g[..., k] >> m) & 1) << k).astype(np.uint8)
    return out.reshape(lead + (-1,))


def to_gray(symbols, sf, ppm):
    """what the decoder does first (LoRaDecoder.cpp:218-222) for symbols without low bits: shift right, binary -> Gray"""
    s = np.asarray(symbols).astype(np.uint16) >> (sf - ppm)
    return s ^ (s >> 1)


def from_gray(gray, sf, ppm):
    """LoRaEncoder.cpp:223-226: Gray -> binary (LoRaCodes.hpp:187-194), shift left"""
    g = np.asarray(gray).astype(np.uint16).copy()
    for s in (8, 4, 2, 1):
        g ^= g >> s
    return (g << (sf - ppm)).astype(np.uint16)


def codewords_of(symbols, sf, ppm, rdd):
    """every codeword of a packet of 8 + n * (4 + rdd) symbols, still whitened: the definition's own de-interleave"""
    P = ppm or sf
    g = to_gray(symbols, sf, P)
    head = deinterleave_def(g[..., :N_HDR_SYMBOLS], P, 4 + HDR_RDD)
    if g.shape[-1] == N_HDR_SYMBOLS:
        return head
    return np.concatenate([head, deinterleave_def(g[..., N_HDR_SYMBOLS:], P, 4 + rdd)], axis=-1)


def build(sf, payload, ppm, rdd, explicit, add_crc, hdr_len=None, hdr_crc=None, hdr_rdd=None, n_blocks=None):
    """-> (symbols uint16, codewords uint8) of one packet. ppm 0 = sf. The header announces hdr_len / hdr_crc / hdr_rdd where given, else what
    the body is (len(payload) & 255, add_crc, rdd). n_blocks further interleaver blocks of zero nibbles follow the body."""
    P = ppm or sf
    payload = np.asarray(payload, np.uint8).reshape(-1)
    data = payload
    if add_crc:                                                                          # LoRaEncoder.cpp:182-186
        crc = data_checksum_def(payload)
        data = np.concatenate([payload, np.array([crc & 0xff, crc >> 8], np.uint8)])
    n_hdr = N_HDR_CODEWORDS if explicit else 0
    n_cw = -(-(2 * data.size + n_hdr) // P) * P + (n_blocks or 0) * P                    # :175
    assert n_cw > 0, "no codewords: the reference's own count wraps (LoRaEncoder.cpp:176)"
    nib = np.zeros(n_cw - n_hdr, np.uint8)                                               # pad and extension nibbles are 0
    nib[0:2 * data.size:2] = data & 0xf                                                  # :132-159: low nibble first
    nib[1:2 * data.size:2] = data >> 4
    pos = np.arange(nib.size)                                                            # index behind the header codewords
    first = pos < P - n_hdr                                                              # the rest of the first block: 4/8 (:202)
    body = np.where(first, fec_def(nib, HDR_RDD), fec_def(nib, rdd)).astype(np.uint8)
    w4, wr = whitening_def(False, nib.size // 2 + 1), whitening_def(rdd == 1, nib.size // 2 + 1)
    body ^= np.where(first, w4[pos & 1, pos >> 1], wr[pos & 1, pos >> 1] & (0xff >> (4 - rdd))).astype(np.uint8)   # :204, :211
    head = np.zeros(0, np.uint8)
    if explicit:
        head = header_codewords_def(payload.size & 0xff if hdr_len is None else hdr_len, add_crc if hdr_crc is None else hdr_crc,
                                    rdd if hdr_rdd is None else hdr_rdd)
    codewords = np.concatenate([head, body]).astype(np.uint8)
    gray = np.concatenate([interleave_def(codewords[:P], P, 4 + HDR_RDD), interleave_def(codewords[P:], P, 4 + rdd)])   # :217-220
    return from_gray(gray, sf, P), codewords


def num_symbols_def(n_codewords, ppm, rdd):
    """LoRaEncoder.cpp:176"""
    return N_HDR_SYMBOLS + (n_codewords // ppm - 1) * (4 + rdd)


def flip(symbols, sf, ppm, rdd, codeword, bit):
    """a copy of the packet with bit `bit` of codeword `codeword` flipped: bit k of codeword i of a block sits in symbol k of the block at
    Gray-domain bit (i - k) mod PPM (LoRaCodes.hpp:354-356), so exactly one Gray bit of one symbol changes"""
    P = ppm or sf
    if codeword < P:
        sym_off, i, width = 0, codeword, 4 + HDR_RDD
    else:
        x, i = divmod(codeword - P, P)
        sym_off, width = N_HDR_SYMBOLS + x * (4 + rdd), 4 + rdd
    assert 0 <= bit < width, "codeword %d has %d bits" % (codeword, width)
    out = np.array(symbols, np.uint16)
    assert sym_off + width <= out.size
    g = to_gray(out[sym_off + bit], sf, P) ^ np.uint16(1 << ((i - bit) % P))
    out[sym_off + bit] = from_gray(g, sf, P)
    return out


def set_header(symbols, sf, ppm, hdr_len, hdr_crc, hdr_rdd):
    """(H, n) packets: the packet `symbols` (n,) under each of the H headers given as arrays. Only the eight symbols of the first block
    change: its PPM - 5 body codewords are kept, its five header codewords replaced, the block interleaved again."""
    P = ppm or sf
    symbols = np.asarray(symbols, np.uint16).reshape(-1)
    head = header_codewords_def(hdr_len, hdr_crc, hdr_rdd)
    head = head.reshape(-1, N_HDR_CODEWORDS)
    block = np.tile(deinterleave_def(to_gray(symbols[:N_HDR_SYMBOLS], sf, P), P, 4 + HDR_RDD), (head.shape[0], 1))
    block[:, :N_HDR_CODEWORDS] = head
    out = np.tile(symbols, (head.shape[0], 1))
    out[:, :N_HDR_SYMBOLS] = from_gray(interleave_def(block, P, 4 + HDR_RDD), sf, P)
    return out


def decoded_end(ppm, explicit, data_length):
    """the first codeword the decoder's loops do NOT read (LoRaDecoder.cpp:315-361), walked as written: the first block, the nibble
    that completes an odd byte, two per byte up to data_length (the bytes the header or the setter announces, header and crc bytes
    included). -> (codeword index, whether the nibble count was odd after the first block)"""
    c_ofs, d_ofs = (N_HDR_CODEWORDS, 6) if explicit else (0, 0)                          # :300-301
    while c_ofs < ppm:                                                                   # :315-320
        c_ofs += 1; d_ofs += 1
    odd = bool(d_ofs & 1)
    if odd:                                                                              # :322-339
        c_ofs += 1; d_ofs += 1
    d_ofs >>= 1
    for _ in range(d_ofs, data_length):                                                  # :346-361
        c_ofs += 2
    return c_ofs, odd
