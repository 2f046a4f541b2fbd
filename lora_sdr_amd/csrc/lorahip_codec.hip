// Batched LoRaDecoder: symbol packets -> bytes.
//
// What the LoRaDecoder block does for one message (LoRaDecoder.cpp:196-397 on LoRaCodes.hpp): Gray-code the demodulated
// symbols with rounding to the symbol size, de-interleave diagonally into codewords (the first block always 4/8), strip the
// whitening with the two interleaved LFSRs, Hamming / parity decode, parse and check the explicit header, check the
// payload CRC. Integer and bit work on a few hundred bytes per packet.
//
// Three kernel families, each as a uniform launch and over a table of per-packet settings (decodeGroupCfgs, decodePacketsCfgs; the soft
// decoder has the table form only), and the encoder (encodeGroup, encodeGroupCfgs) behind them.
//
// decodeGroup (the default): a GROUP of G = 8 / 16 / 32 / 64 lanes of a wavefront owns a packet (G by the row length of the
// launch), the packet's symbols, codewords and nibbles live in the group's slice of LDS, and every stage is data-parallel over
// the lanes of the group: a lane Gray-codes its symbols, builds its codewords bit by bit from the (at most eight) symbols of
// their interleaver block, whitens them from a precomputed table of the two LFSR sequences (they do not depend on the packet),
// decodes its nibbles, assembles its bytes; the CRC is a sum over the lanes of byte * x^(8 k) mod P (a 256-entry table), folded
// with lane shuffles. No per-lane arrays, no scratch. The order of the reference's decisions (what is decoded before which
// check, which coding rate applies where) is kept exactly; only the loops became lanes.
//
// decodeSoftCfgs (lorahip_decode_packets_soft): the same lane groups over rows of per-bit LLRs, which stay in global memory: a lane gathers
// its codeword's (at most eight) values and takes the maximum-likelihood nibble; LDS holds the nibbles alone.
//
// What the two group decoders share -- which packet a group owns, the counts at a rate, where a codeword lies, the header, the lengths,
// the row rule, the checksum, the output and the report -- is ONE set of stage functions (packetOf .. writePacket, in front of
// decodeGroupBody); the bodies are their own front ends and the workgroup barriers, with the stages between them.
//
// decodePackets (context variant 1): one lane walks one packet statement by statement in the reference's order, working arrays
// in per-lane scratch -- the round-1 kernel, kept as the A/B checker; it shares nothing with the group kernels.
#include "lorahip_internal.h"
#include <type_traits>

namespace lorahip {

#define LORAHIP_DEC_MAX_SYMBOLS 520            // symbols per packet incl. rounding to a block: the one-lane checker kernel (variant 1) only
#define LORAHIP_DEC_MAX_DATA_LENGTH 4096       // setDataLength without a header: bytes per packet the tables below reach (a LoRa length field is one byte)
#define LORAHIP_DEC_MAX_CODEWORDS ((LORAHIP_DEC_MAX_SYMBOLS / 4) * 12 + 4)
#define LORAHIP_HDR_RDD 4                      // LoRaCodes.hpp:103
#define LORAHIP_N_HDR_SYMBOLS 8                // :104
#define LORAHIP_N_HDR_CODEWORDS 5              // :105

namespace {

__device__ __forceinline__ int parityOf(const unsigned v) { return __popc(v) & 1; }

//! header checksum (LoRaCodes.hpp:131-156): five parity bits over the 12 header bits w = h[0] | (h[1] & 0xf) << 8, as masks
__device__ __forceinline__ unsigned char headerChecksum(const unsigned char *h)
{
    const unsigned w = h[0] | ((unsigned)(h[1] & 0xf) << 8);
    return (unsigned char)(parityOf(w & 0xF12) | (parityOf(w & 0x725) << 1) | (parityOf(w & 0xA49) << 2) | (parityOf(w & 0x18E) << 3) |
                           (parityOf(w & 0x0F0) << 4));
}

//! one byte position of the CCITT crc, MSB first (:158-168)
__device__ __forceinline__ unsigned short crc16sx(unsigned short crc, const unsigned short poly)
{
    for (int bit = 0; bit < 8; bit++)
    {
        const bool top = (crc & 0x8000) != 0;
        crc = (unsigned short)(crc << 1);
        if (top) crc ^= poly;
    }
    return crc;
}

//! payload checksum of the sx1272 (:170-194): crc over the bytes, masked with two steps of an 8-bit LFSR (taps 0xB8)
__device__ unsigned short dataChecksum(const unsigned char *data, const int length)
{
    unsigned short res = 0;
    unsigned char v = 0xff;
    for (int i = 0; i < length; i++)
    {
        const unsigned short crc = crc16sx(res, 0x1021);
        v = (unsigned char)((v << 1) | parityOf(v & 0xB8));
        res = crc ^ data[i];
    }
    res ^= v;
    v = (unsigned char)((v << 1) | parityOf(v & 0xB8));
    res ^= (unsigned short)(v << 8);
    return res;
}

//! one byte step of a whitening register: feedback byte b0^b2^b3^b4, shifted in at the top (:255-268)
__device__ __forceinline__ unsigned long long lfsrAdvance(const unsigned long long r)
{
    const unsigned long long fb = (r ^ (r >> 16) ^ (r >> 24) ^ (r >> 32)) & 0xff;
    return (r >> 8) | (fb << 56);
}

//! de-whitening with the two interleaved registers: codeword position p (counted from bitOfs) uses register p mod 2.
//! bufferSize is a uint16_t parameter in the reference.
__device__ void whiteningLfsr(unsigned char *buffer, const unsigned short bufferSize, const int bitOfs, const int RDD)
{
    unsigned long long even = (RDD == 1) ? 0x05121100F8ECFEEFull : 0x6572D100E85C2EFFull;   // single-parity mode has its own seeds
    unsigned long long odd = (RDD == 1) ? 0xF8ECFEEFEFEFEFEFull : 0xE85C2EFFFFFFFFFFull;
    const unsigned char keep = (unsigned char)(0xff >> (4 - RDD));
    for (int p = 0; p < bitOfs; p++)
    {
        if (p & 1) odd = lfsrAdvance(odd);
        else even = lfsrAdvance(even);
    }
    for (int j = 0; j < bufferSize; j++)
    {
        if ((bitOfs + j) & 1) { buffer[j] ^= (unsigned char)(odd & keep); odd = lfsrAdvance(odd); }
        else { buffer[j] ^= (unsigned char)(even & keep); even = lfsrAdvance(even); }
    }
}

// The sx Hamming codes (:222-259, :284-312) and parity checks (:318-323, :335-343) as syndrome masks: parity bit k covers
// the codeword bits in COVERk; a syndrome naming a data bit flips it, one naming a parity bit is ignored, anything else is
// uncorrectable (8,4 only). The flip tables are packed 4 bits per syndrome value (0xF = uncorrectable).
#define LORAHIP_COVER0 0x17u
#define LORAHIP_COVER1 0x2Eu
#define LORAHIP_COVER2 0x4Bu
#define LORAHIP_COVER3 0x8Du

__device__ __forceinline__ unsigned char decodeHamming84(const unsigned char b, bool &error, bool &bad)
{
    const unsigned syn = parityOf(b & LORAHIP_COVER0) | (parityOf(b & LORAHIP_COVER1) << 1) | (parityOf(b & LORAHIP_COVER2) << 2) |
                         (parityOf(b & LORAHIP_COVER3) << 3);
    // syndrome 0..15 -> data bit to flip: 0xD:1 0x7:2 0xB:4 0xE:8; 0,1,2,4,8 -> none; the rest uncorrectable
    const unsigned long long fix = 0xF81F4FF02FF0F000ull;
    const unsigned f = (unsigned)(fix >> (4 * syn)) & 0xf;
    if (syn) error = true;
    if (f == 0xf) { bad = true; return b & 0xf; }
    return (b ^ f) & 0xf;
}

__device__ __forceinline__ unsigned char decodeHamming74(const unsigned char b, bool &error)
{
    const unsigned syn = parityOf(b & LORAHIP_COVER0 & 0x7f) | (parityOf(b & LORAHIP_COVER1 & 0x7f) << 1) | (parityOf(b & LORAHIP_COVER2 & 0x7f) << 2);
    const unsigned fix = 0x28104000u;                  // syndrome 0..7 -> flip: 5:1 7:2 3:4 6:8
    if (syn) error = true;
    return (b ^ ((fix >> (4 * syn)) & 0xf)) & 0xf;
}

__device__ __forceinline__ unsigned char checkParity54(const unsigned char b, bool &error)
{
    if (parityOf(b & 0x1F)) error = true;              // one parity bit (b4) over the data bits
    return b & 0xf;
}

__device__ __forceinline__ unsigned char checkParity64(const unsigned char b, bool &error)
{
    if (parityOf(b & LORAHIP_COVER0) | parityOf(b & LORAHIP_COVER1)) error = true;   // the first two Hamming parity bits
    return b & 0xf;
}

//! one FEC nibble of the payload at coding rate rdd
__device__ __forceinline__ unsigned char decodeNibble(const unsigned char cw, const int rdd, bool &error, bool &bad)
{
    switch (rdd)
    {
    case 0: return cw;                            // the callers mask / shift exactly like the reference
    case 1: return checkParity54(cw, error);
    case 2: return checkParity64(cw, error);
    case 3: return decodeHamming74(cw, error);
    default: return decodeHamming84(cw, error, bad);
    }
}

__device__ void diagonalDeinterleave(const unsigned short *symbols, const int numSymbols, unsigned char *codewords,
                                     const int PPM, const int RDD)                                         // :366-381
{
    for (int x = 0; x < numSymbols / (4 + RDD); x++)
    {
        const int cwOff = x * PPM, symOff = x * (4 + RDD);
        for (int k = 0; k < 4 + RDD; k++)
        {
            const unsigned sym = symbols[symOff + k];
            int i = k % PPM;
            for (int m = 0; m < PPM; m++)
            {
                codewords[cwOff + i] |= (unsigned char)(((sym >> m) & 1) << k);
                if (++i == PPM) i = 0;
            }
        }
    }
}

} // namespace

/*! The settings of a table launch (lorahip_decode_packets_cfgs), by value in the kernel arguments: packet p runs under e[i], i = index[p], or
 * table[index[p]] with a table (a receiver: index = the channel the hand-off wrote, table = configuration of channel). An index[p] outside
 * the table, or an i outside [0, nCfgs), is outcome -3: the packet is not looked at. The caps are the slice entry i needs (decodePlan). */
struct DecodeCfgTable
{
    const int *index, *table;
    int nTable, nCfgs;
    DecodeCfg e[LORAHIP_DEC_MAX_CFGS];
};

//! packet p's entry of the table (DecodeCfgTable, or the encoder's EncodeCfgTable below), -1 where there is none
template <class Table>
__device__ __forceinline__ int cfgIndexOf(const Table &tab, const unsigned p)
{
    int i = tab.index[p];
    if (tab.table != nullptr)
    {
        if (i < 0 || i >= tab.nTable) return -1;
        i = tab.table[i];
    }
    return (i < 0 || i >= tab.nCfgs) ? -1 : i;
}

//! the rows of the launch with entry e as their settings: what the decoder bodies below read as `a`
__host__ __device__ __forceinline__ DecodeArgs withCfg(const DecodeArgs &rows, const DecodeCfg &e)
{
    DecodeArgs a = rows;
    a.sf = e.sf; a.ppm = e.ppm; a.rdd = e.rdd; a.crcc = e.crcc; a.interleaving = e.interleaving;
    a.errorCheck = e.errorCheck; a.explicitHdr = e.explicitHdr; a.hdr = e.hdr; a.dataLength = e.dataLength;
    return a;
}

//! the header report of packet p (struct lorahip_packet_info: length, rdd, crc, hdr_residue, fec_error, need_syms, two reserved words)
__device__ __forceinline__ void writePacketInfo(int *info, const unsigned p, const int length, const int rdd, const int crc, const int residue,
                                                const int fecError, const int needSyms)
{
    int *w = info + (size_t)p * 8;
    w[0] = length; w[1] = rdd; w[2] = crc; w[3] = residue; w[4] = fecError; w[5] = needSyms; w[6] = 0; w[7] = 0;
}

//! packet p under the settings in `a`: launch-uniform scalars in decodePackets, the packet's own in decodePacketsCfgs
__device__ __forceinline__ void decodeOnePacket(const DecodeArgs a, const unsigned p)
{
    const int nsyms = a.nsyms[p];
    const unsigned short *in = a.syms + (size_t)p * a.symStride;
    unsigned char *out = a.out + (size_t)p * a.outStride;
    int outLen = -1, dropped = 0;
    int iLen = -1, iRdd = -1, iCrc = 0, iRes = -1, iNeed = -1;                               // the report: "header not reached"
    bool error = false, bad = false;                                                         // :273-274

    unsigned short symbols[LORAHIP_DEC_MAX_SYMBOLS];
    unsigned char codewords[LORAHIP_DEC_MAX_CODEWORDS];
    unsigned char bytes[LORAHIP_DEC_MAX_CODEWORDS / 2 + 8];

    const int sf = a.sf;
    const int PPM = a.ppm == 0 ? sf : a.ppm;                                                 // LoRaDecoder.cpp:201
    do
    {
        if (PPM > sf || nsyms < LORAHIP_N_HDR_SYMBOLS) break;                                // :202 (throws), :208
        int cfgRdd = a.rdd;                                                                  // the rate the setter would have been given
        if (cfgRdd < 0)
        {
            // LORAHIP_RDD_FROM_HEADER: the header block by itself -- the first 8 symbols, Gray-coded, de-interleaved at 4/8, not whitened
            // (:228-255 do exactly this to them at every configured rate) -- names the rate the rest of the message is read at
            unsigned short hs[LORAHIP_N_HDR_SYMBOLS];
            unsigned char hc[LORAHIP_SF_MAX + 4];
            for (int i = 0; i < LORAHIP_N_HDR_SYMBOLS; i++)
            {
                unsigned short sym = i < a.symStride ? in[i] : 0;
                sym = (unsigned short)(sym + (1 << (sf - PPM)) / 2);
                sym = (unsigned short)(sym >> (sf - PPM));
                hs[i] = (unsigned short)(sym ^ (sym >> 1));
            }
            for (int i = 0; i < PPM; i++) hc[i] = 0;
            diagonalDeinterleave(hs, LORAHIP_N_HDR_SYMBOLS, hc, PPM, LORAHIP_HDR_RDD);
            bool hErr = false, hBad = false;
            unsigned char hb[3];
            hb[0] = (unsigned char)((decodeHamming84(hc[1], hErr, hBad) & 0xf) | (decodeHamming84(hc[0], hErr, hBad) << 4));
            hb[1] = decodeHamming84(hc[2], hErr, hBad) & 0xf;
            hb[2] = (unsigned char)((decodeHamming84(hc[4], hErr, hBad) & 0xf) | (decodeHamming84(hc[3], hErr, hBad) << 4));
            hb[2] ^= headerChecksum(hb);
            cfgRdd = (hb[1] >> 1) & 0x7;
            if (cfgRdd > 4)                                                                  // every rate setting drops it (:293 or :297)
            {
                // ... unless this kernel's own row rule comes first: a packet longer than its row, or than this build, is -2 at EVERY rate
                if (nsyms > a.symStride || nsyms > LORAHIP_DEC_MAX_SYMBOLS) { outLen = -2; break; }
                dropped = 1;
                iLen = hb[0]; iRdd = cfgRdd; iRes = hb[2]; error = hErr;
                break;
            }
        }
        const int numSymbols = ((nsyms + (4 + cfgRdd) - 1) / (4 + cfgRdd)) * (4 + cfgRdd);   // :210
        const int numCodewords = (numSymbols / (4 + cfgRdd)) * PPM;                          // :211
        if (numSymbols > LORAHIP_DEC_MAX_SYMBOLS || nsyms > a.symStride || numCodewords + 4 > LORAHIP_DEC_MAX_CODEWORDS) { outLen = -2; break; }   // larger than this build / this row supports
        int rdd = cfgRdd;                                                                    // :215
        for (int i = 0; i < numSymbols; i++)                                                 // :218-222
        {
            unsigned short sym = i < nsyms ? in[i] : 0;
            sym = (unsigned short)(sym + (1 << (sf - PPM)) / 2);
            sym = (unsigned short)(sym >> (sf - PPM));
            sym = (unsigned short)(sym ^ (sym >> 1));
            symbols[i] = sym;
        }
        if (!a.interleaving)                                                                 // :264-270
        {
            for (int i = 0; i < numSymbols; i++) reinterpret_cast<unsigned short *>(out)[i] = symbols[i];
            outLen = numSymbols;
            break;
        }
        for (int i = 0; i < numCodewords + 4; i++) codewords[i] = 0;
        {                                                                                    // :225-255
            int sOfs = 0, cOfs = 0;
            if (rdd != LORAHIP_HDR_RDD)
            {
                diagonalDeinterleave(symbols, LORAHIP_N_HDR_SYMBOLS, codewords, PPM, LORAHIP_HDR_RDD);
                if (a.explicitHdr) whiteningLfsr(codewords + LORAHIP_N_HDR_CODEWORDS, (unsigned short)(PPM - LORAHIP_N_HDR_CODEWORDS), 0, LORAHIP_HDR_RDD);
                else whiteningLfsr(codewords, (unsigned short)PPM, 0, LORAHIP_HDR_RDD);
                cOfs += PPM;
                sOfs += LORAHIP_N_HDR_SYMBOLS;
                if (numSymbols - sOfs > 0)
                {
                    diagonalDeinterleave(symbols + sOfs, numSymbols - sOfs, codewords + cOfs, PPM, rdd);
                    if (a.explicitHdr) whiteningLfsr(codewords + cOfs, (unsigned short)(numCodewords - cOfs), PPM - LORAHIP_N_HDR_CODEWORDS, rdd);
                    else whiteningLfsr(codewords + cOfs, (unsigned short)(numCodewords - cOfs), PPM, rdd);
                }
            }
            else
            {
                diagonalDeinterleave(symbols, numSymbols, codewords, PPM, rdd);
                if (a.explicitHdr) whiteningLfsr(codewords + LORAHIP_N_HDR_CODEWORDS, (unsigned short)(numCodewords - LORAHIP_N_HDR_CODEWORDS), 0, rdd);
                else whiteningLfsr(codewords, (unsigned short)numCodewords, 0, rdd);
            }
        }

        const int nbytes = (numCodewords + 1) / 2;
        for (int i = 0; i < nbytes + 8; i++) bytes[i] = 0;
        int dOfs = 0, cOfs = 0;
        long long packetLength = 0, dataLength = 0;
        bool checkCrc = a.crcc != 0;
        if (a.explicitHdr)                                                                   // :283-303
        {
            bytes[0] = decodeHamming84(codewords[1], error, bad) & 0xf;
            bytes[0] |= (unsigned char)(decodeHamming84(codewords[0], error, bad) << 4);     // length
            bytes[1] = decodeHamming84(codewords[2], error, bad) & 0xf;                      // coding rate and crc enable
            bytes[2] = decodeHamming84(codewords[4], error, bad) & 0xf;
            bytes[2] |= (unsigned char)(decodeHamming84(codewords[3], error, bad) << 4);     // checksum
            bytes[2] ^= headerChecksum(bytes);
            iLen = bytes[0]; iRdd = (bytes[1] >> 1) & 0x7; iRes = bytes[2];
            if (error && a.errorCheck) { dropped = 1; break; }
            if (0 == (bytes[1] & 1)) checkCrc = false;
            rdd = (bytes[1] >> 1) & 0x7;
            if (rdd > 4) { dropped = 1; break; }
            packetLength = bytes[0];
            dataLength = packetLength + ((bytes[1] & 1) ? 5 : 3);
            cOfs = LORAHIP_N_HDR_CODEWORDS;
            dOfs = 6;
        }
        else                                                                                 // :304-311
        {
            packetLength = a.dataLength;
            dataLength = a.crcc ? packetLength + 2 : packetLength;
            iLen = a.dataLength; iRdd = cfgRdd;
        }
        if (dataLength > nbytes) { dropped = 1; break; }                                     // :313
        {
            // the report's need_syms: the whole interleaver blocks that hold the codewords :315-361 decode for this length
            const int shift = a.explicitHdr ? 1 : 0;
            long long cEnd = 2 * dataLength - shift;
            const int fill = PPM + (((PPM + shift) & 1) ? 1 : 0);
            if (cEnd < fill) cEnd = fill;
            const long long nBlocks = (cEnd + PPM - 1) / PPM;
            iNeed = (int)(cfgRdd != LORAHIP_HDR_RDD ? LORAHIP_N_HDR_SYMBOLS + (nBlocks - 1) * (4 + cfgRdd) : nBlocks * (4 + cfgRdd));
        }
        for (; cOfs < PPM; cOfs++, dOfs++)                                                   // :315-320
        {
            if (dOfs & 1) bytes[dOfs >> 1] |= (unsigned char)(decodeHamming84(codewords[cOfs], error, bad) << 4);
            else bytes[dOfs >> 1] = decodeHamming84(codewords[cOfs], error, bad) & 0xf;
        }
        if (dOfs & 1)                                                                        // :322-339
        {
            bytes[dOfs >> 1] |= (unsigned char)(decodeNibble(codewords[cOfs++], rdd, error, bad) << 4);
            dOfs++;
        }
        dOfs >>= 1;
        if (error && a.errorCheck) { dropped = 1; break; }                                   // :342
        for (long long i = dOfs; i < dataLength; i++)                                        // :346-361
        {
            const unsigned char c0 = codewords[cOfs++], c1 = codewords[cOfs++];
            bytes[i] = decodeNibble(c0, rdd, error, bad) & 0xf;
            bytes[i] |= (unsigned char)(decodeNibble(c1, rdd, error, bad) << 4);
        }
        if (error && a.errorCheck) { dropped = 1; break; }                                   // :363
        dOfs = 0;
        if (a.explicitHdr)                                                                   // :367-379
        {
            if (bytes[1] & 1)
            {
                const unsigned short crc = dataChecksum(bytes + 3, (int)packetLength);
                const unsigned short packetCrc = (unsigned short)(bytes[3 + packetLength] | (bytes[4 + packetLength] << 8));
                iCrc = crc == packetCrc ? 1 : -1;
                if (crc != packetCrc && checkCrc) { dropped = 1; break; }
                bytes[3 + packetLength] ^= (unsigned char)crc;
                bytes[4 + packetLength] ^= (unsigned char)(crc >> 8);
            }
            if (!a.hdr) { dOfs = 3; dataLength -= 5; }
        }
        else if (checkCrc)                                                                   // :380-388
        {
            const unsigned short crc = dataChecksum(bytes, a.dataLength);
            const unsigned short packetCrc = (unsigned short)(bytes[a.dataLength] | (bytes[a.dataLength + 1] << 8));
            iCrc = crc == packetCrc ? 1 : -1;
            if (crc != packetCrc) { dropped = 1; break; }
            bytes[a.dataLength + 0] ^= (unsigned char)crc;
            bytes[a.dataLength + 1] ^= (unsigned char)(crc >> 8);
        }
        // `dataLength -= 5` on a size_t wraps for a header without the crc flag that announces fewer than 2 bytes; the
        // reference then fails to allocate its output and posts nothing
        if (dataLength < 0) break;
        for (long long i = 0; i < dataLength; i++) out[i] = bytes[dOfs + i];                 // :391-395
        outLen = (int)dataLength;
    } while (false);
    a.outLen[p] = outLen;
    a.dropped[p] = dropped;
    if (a.info != nullptr) writePacketInfo(a.info, p, iLen, iRdd, iCrc, iRes, error ? 1 : 0, iNeed);
}

__global__ void __launch_bounds__(64) decodePackets(const DecodeArgs a)
{
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.nPackets) return;
    decodeOnePacket(a, p);
}


/***********************************************************************
 * group-per-packet decoder
 **********************************************************************/
namespace {

#define LORAHIP_WHITEN_LEN 4104                // positions per register: the codewords that can reach the output (LORAHIP_DEC_MAX_DATA_LENGTH
                                               // bytes + crc = 8196 nibbles + the five header codewords) / 2, and the byte steps of the crc

//! the byte sequences of the two whitening registers for both seed sets, and the CRC helper tables -- none depends on the packet
struct CodecTables
{
    unsigned char white[2][2][LORAHIP_WHITEN_LEN];     // [single-parity seeds][odd register][step]: low byte before the step (:255-268)
    unsigned short xpow[LORAHIP_WHITEN_LEN];            // x^(8 k) mod (x^16 + x^12 + x^5 + 1): one byte position of crc16sx, k times
    unsigned char lfsr8[LORAHIP_WHITEN_LEN + 2];        // the 8-bit register of dataChecksum after k steps from 0xff (:170-194)
};

constexpr unsigned long long lfsrAdvanceC(const unsigned long long r)
{
    return (r >> 8) | ((((r ^ (r >> 16) ^ (r >> 24) ^ (r >> 32)) & 0xff)) << 56);
}
constexpr int parityC(unsigned v) { int p = 0; while (v) { p ^= 1; v &= v - 1; } return p; }

constexpr CodecTables makeCodecTables()
{
    CodecTables t = {};
    const unsigned long long seeds[2][2] = { { 0x6572D100E85C2EFFull, 0xE85C2EFFFFFFFFFFull }, { 0x05121100F8ECFEEFull, 0xF8ECFEEFEFEFEFEFull } };
    for (int c = 0; c < 2; c++)
        for (int o = 0; o < 2; o++)
        {
            unsigned long long r = seeds[c][o];
            for (int n = 0; n < LORAHIP_WHITEN_LEN; n++) { t.white[c][o][n] = (unsigned char)(r & 0xff); r = lfsrAdvanceC(r); }
        }
    unsigned v = 1;                                      // x^0
    for (int k = 0; k < LORAHIP_WHITEN_LEN; k++)
    {
        t.xpow[k] = (unsigned short)v;
        for (int b = 0; b < 8; b++) v = ((v << 1) ^ ((v & 0x8000) ? 0x1021 : 0)) & 0xffff;
    }
    unsigned char l = 0xff;
    for (int k = 0; k < LORAHIP_WHITEN_LEN + 2; k++) { t.lfsr8[k] = l; l = (unsigned char)((l << 1) | parityC(l & 0xB8)); }
    return t;
}

__device__ const CodecTables kCodec = makeCodecTables();

//! a * x^(8k) mod P for a byte a: the contribution of data byte a to the crc after k further byte steps
__device__ __forceinline__ unsigned crcShift(const unsigned a, const unsigned xk)
{
    unsigned acc = 0, t = xk;
#pragma unroll
    for (int b = 0; b < 8; b++)
    {
        acc ^= ((a >> b) & 1) ? t : 0u;
        t = ((t << 1) ^ ((t & 0x8000) ? 0x1021u : 0u)) & 0xffffu;
    }
    return acc;
}

template <int G> __device__ __forceinline__ unsigned groupXor(unsigned v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v ^= __shfl_xor(v, o, G);
    return v;
}
template <int G> __device__ __forceinline__ bool groupAny(const bool p)
{
    unsigned v = p ? 1u : 0u;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, G);
    return v != 0;
}

} // namespace

/*! What of a packet can reach the output. The reference de-interleaves and de-whitens EVERY codeword of the message (LoRaDecoder.cpp:
 * 225-255), but decodes only those the announced length needs (:315-361): the first PPM of them, the nibble that completes an odd
 * byte, then two per byte up to dataLength -- at most 2 * (255 + 5) with an explicit header (the length is one byte), 2 * (setDataLength
 * + 2) without. Codewords behind that, and the symbols they are made of, change nothing (numSymbols / numCodewords enter the checks
 * as numbers only). So the group's slice of LDS is sized by what the CONFIGURATION can need, not by the length of the row: a packet of
 * any length the demodulator can produce decodes like the reference decodes it. */
struct DecodeCaps { int symCap, cwCap; };

//! the slice a configuration at a FIXED rate needs (see DecodeCaps): the symbols / codewords that can reach the output, or the whole row if
//! that is less. On the host for the plan; on the device for a header-rate packet, whose decisions are those of the rate its header names.
__host__ __device__ __forceinline__ DecodeCaps decodeCapsAt(const int sf, const int ppm, const int rdd, const int explicitHdr, const int dataLength,
                                                            const int symStride)
{
    const int PPM = ppm == 0 ? sf : ppm, bs = 4 + rdd;
    long long nBlocks;
    if (explicitHdr)                                                 // (a length of one byte: 32-bit arithmetic -- the device takes this branch)
    {
        const int cEnd = 2 * (255 + 5) < PPM + 1 ? PPM + 1 : 2 * (255 + 5);
        nBlocks = (cEnd + PPM - 1) / PPM + 1;
    }
    else
    {
        long long cEnd = 2 * ((long long)dataLength + 2);
        if (cEnd < PPM + 1) cEnd = PPM + 1;
        nBlocks = (cEnd + PPM - 1) / PPM + 1;
    }
    const long long symNeed = LORAHIP_N_HDR_SYMBOLS + nBlocks * bs;
    const int rowBlocks = (symStride + 7 + 8) / bs + 1;
    const long long symRow = (long long)rowBlocks * bs + LORAHIP_N_HDR_SYMBOLS;                   // the row, rounded up to whole blocks
    DecodeCaps c;
    c.symCap = int(symNeed < symRow ? symNeed : symRow);
    // codewords of those symbols (+ the 4 zero entries behind numCodewords the nibble loop may read, + nibble offsets): symCap / bs blocks
    // + 2 -- symCap is 8 + a whole number of blocks of 4..8 symbols in BOTH branches (symNeed = 8 + nBlocks * bs, symRow = 8 + rowBlocks *
    // bs), so symCap / bs = (8 + B * bs) / bs = B + 8 / bs exactly, and 8 / bs is 2 for bs = 4 and 1 for bs = 5..8: no division needed
    const long long capBlocks = (symNeed < symRow ? nBlocks : (long long)rowBlocks) + (bs == 4 ? 2 : 1);
    c.cwCap = int((capBlocks + 2) * PPM + 16);
    return c;
}

__host__ __device__ __forceinline__ int decodeSliceOf(const DecodeCaps c) { return (c.symCap * 2 + 2 * c.cwCap + 15) & ~15; }

/***********************************************************************
 * The stages of the reference block that the two lane-group decoders share: decodeGroupBody (hard, below) and decodeSoftBody (soft, behind
 * the encoder) are their own front ends -- how a codeword's bits or LLRs are fetched and how a nibble is decided -- with these between
 * their barriers. Every rule of the reference about which packets exist, how long they are and what is reported is written here, once.
 * No stage holds a workgroup barrier: those stand in the two bodies, at top level, so the 256 threads of a table launch meet at every one
 * whatever their packets' settings are; a packet that is done only clears `go`. Everything here is the same for every lane of a group.
 **********************************************************************/
namespace {

//! one packet's way through the stages
struct PacketState
{
    bool go, error;                        // still decoding; the reference's error flag (:273), over the hard bits in both decoders
    int outLen, dropped;
    int rate, rdd;                         // the rate the message is laid out at (the setter's, or the one a header-rate entry's header names);
                                           // the rate the payload's nibbles are decoded at (the header's)
    bool checkCrc;                         // (rdd and checkCrc: from decodeHeader on)
    long long packetLength, dataLength, cEnd;   // cEnd: first codeword NOT needed by the bytes
    unsigned char h0, h1, h2;              // the explicit header: length, coding rate and crc enable, checksum residue
    int iLen, iRdd, iCrc, iRes, iNeed;     // the report (lorahip_packet_info)
};

//! which packet a lane works on: lane t of group g of the workgroup, packet p (pc: 0 in its place for a group that has none)
struct GroupPacket { int g, t; unsigned p, pc; bool have; int nsyms, PPM, rowSyms; unsigned char *out; };

//! interleaver blocks of a message at one rate
struct RateCounts { int bs, numSymbols, numCodewords; };

/*! Packet identity and the group-uniform early outs (:202 throws, :208 too short). A header-rate entry (a.rdd < 0) starts at 4/8: its
 * rate is known behind the bodies' first barrier. */
template <int G>
__device__ __forceinline__ GroupPacket packetOf(const DecodeArgs &a, const int perBlock, const bool known, PacketState &st)
{
    GroupPacket k;
    k.g = threadIdx.x / G; k.t = threadIdx.x % G;
    k.p = blockIdx.x * perBlock + k.g;
    k.have = k.g < perBlock && k.p < a.nPackets;                    // (long slices: fewer packets per workgroup than groups, the rest idle)
    k.pc = k.have ? k.p : 0;
    k.nsyms = k.have ? a.nsyms[k.pc] : 0;
    k.out = a.out + (size_t)k.pc * a.outStride;
    k.PPM = a.ppm == 0 ? a.sf : a.ppm;                                                       // LoRaDecoder.cpp:201
    // the row holds the first symStride symbols of a longer packet: whether that is enough is known once the length is (decodeNeeds)
    k.rowSyms = k.nsyms < a.symStride ? k.nsyms : a.symStride;
    st.go = k.have && known && !(k.PPM > a.sf || k.nsyms < LORAHIP_N_HDR_SYMBOLS);
    st.error = false; st.outLen = -1; st.dropped = 0;
    st.rate = a.rdd < 0 ? LORAHIP_HDR_RDD : a.rdd;
    st.packetLength = 0; st.dataLength = 0; st.cEnd = 0;
    st.h0 = 0; st.h1 = 0; st.h2 = 0;
    st.iLen = -1; st.iRdd = -1; st.iCrc = 0; st.iRes = -1; st.iNeed = -1;                    // "header not reached"
    return k;
}

__device__ __forceinline__ RateCounts countsAt(const int nsyms, const int PPM, const int rate)
{
    RateCounts n;
    n.bs = 4 + rate;                                                                         // symbols per interleaver block
    const int nBlocks = (nsyms + n.bs - 1) / n.bs;
    n.numSymbols = nBlocks * n.bs;                                                           // :210
    n.numCodewords = nBlocks * PPM;                                                          // :211
    return n;
}

//! where codeword c comes from: row i of the interleaver block whose symbols start at symOff and are coded at R, and its whitening byte
struct CodewordPlace { int i, symOff, R; bool whole; unsigned white; };

/*! Placement of codeword c < n.numCodewords (diagonal de-interleave :366-381, de-whitening :225-255). The first block is always 4/8 over
 * 8 symbols unless the whole packet is (then every block is). */
__device__ __forceinline__ CodewordPlace placeCodeword(const int c, const int PPM, const int rate, const RateCounts &n, const int explicitHdr)
{
    const bool hdrBlock = rate != LORAHIP_HDR_RDD;
    CodewordPlace w;
    int x;
    if (hdrBlock && c < PPM) { x = 0; w.i = c; w.symOff = 0; w.R = LORAHIP_HDR_RDD; }
    else if (hdrBlock) { x = (c - PPM) / PPM; w.i = (c - PPM) - x * PPM; w.symOff = LORAHIP_N_HDR_SYMBOLS + x * n.bs; w.R = rate; }
    else { x = c / PPM; w.i = c - x * PPM; w.symOff = x * n.bs; w.R = rate; }
    // with a header block the payload's symbols may end inside a block of `bs`: the reference de-interleaves
    // (numSymbols - 8) / bs whole blocks and leaves the rest of the codewords zero
    w.whole = !hdrBlock || c < PPM || (w.symOff + (4 + w.R) <= n.numSymbols);
    // position in the whitening sequence: codeword index, minus the five header codewords that are not whitened
    // (with a header block and nothing but it -- exactly 8 symbols -- the reference skips the payload's whitening call)
    const int pos = explicitHdr ? c - LORAHIP_N_HDR_CODEWORDS : c;
    w.white = 0;
    // (the tables end behind the last codeword any length can need: LORAHIP_DEC_MAX_DATA_LENGTH)
    if (pos >= 0 && (pos >> 1) < LORAHIP_WHITEN_LEN && !(hdrBlock && c >= PPM && n.numSymbols <= LORAHIP_N_HDR_SYMBOLS))
        w.white = kCodec.white[w.R == 1 ? 1 : 0][pos & 1][pos >> 1] & (0xffu >> (4 - w.R));
    return w;
}

/*! The header (:283-311), evaluated by every lane of the group alike: nib[c] is the decoded nibble of header codeword c, st.error what the
 * hard 4/8 decode of the five found (both only read with an explicit header). */
__device__ __forceinline__ void decodeHeader(PacketState &st, const DecodeArgs &a, const unsigned char (&nib)[LORAHIP_N_HDR_CODEWORDS], const int numCodewords)
{
    st.rdd = st.rate;                                                                        // :215
    st.checkCrc = a.crcc != 0;
    if (!st.go) return;
    const int nbytes = (numCodewords + 1) / 2;
    if (a.explicitHdr)
    {
        st.h0 = (unsigned char)(nib[1] | (nib[0] << 4));                                     // length
        st.h1 = nib[2];                                                                      // coding rate and crc enable
        st.h2 = (unsigned char)(nib[4] | (nib[3] << 4));                                     // checksum
        const unsigned char hb[2] = { st.h0, st.h1 };
        st.h2 ^= headerChecksum(hb);
        st.iLen = st.h0; st.iRdd = (st.h1 >> 1) & 0x7; st.iRes = st.h2;
        if (st.error && a.errorCheck) { st.dropped = 1; st.go = false; }
        if (st.go)
        {
            if (0 == (st.h1 & 1)) st.checkCrc = false;
            st.rdd = (st.h1 >> 1) & 0x7;
            if (st.rdd > 4) { st.dropped = 1; st.go = false; }
            st.packetLength = st.h0;
            st.dataLength = st.packetLength + ((st.h1 & 1) ? 5 : 3);
        }
    }
    else
    {
        st.packetLength = a.dataLength;
        st.dataLength = a.crcc ? st.packetLength + 2 : st.packetLength;
        st.iLen = a.dataLength; st.iRdd = st.rate;
    }
    if (st.go && st.dataLength > nbytes) { st.dropped = 1; st.go = false; }                  // :313
}

/*! What the bytes need. Nibbles (:315-361): codeword c -> nibble c (+1 after an explicit header); the first block is 4/8, the rest at the
 * coding rate the HEADER names; decoded are the first block, the nibble that completes its last byte, and what dataLength bytes need
 * -- [first payload codeword, st.cEnd); errors anywhere else do not count, exactly as in the reference's loops. symCap / cwCap: the
 * caps of the packet's rate in the hard plan, in both decoders: the same packets are -2 in both. */
__device__ __forceinline__ void decodeNeeds(PacketState &st, const DecodeArgs &a, const GroupPacket &k, const int bs, const int symCap, const int cwCap)
{
    if (!st.go) return;
    const int shift = a.explicitHdr ? 1 : 0;
    st.cEnd = 2 * st.dataLength - shift;
    const int fill = k.PPM + (((k.PPM + shift) & 1) ? 1 : 0);                                // first block + the odd nibble
    if (st.cEnd < fill) st.cEnd = fill;
    // the symbols those codewords are made of: whole interleaver blocks. A packet longer than its row decodes all the same while
    // they lie inside the row; if not, the caller's rows are too short for this packet (-2: reported, never guessed)
    const long long nBlocks = (st.cEnd + k.PPM - 1) / k.PPM;
    const long long needSyms = st.rate != LORAHIP_HDR_RDD ? LORAHIP_N_HDR_SYMBOLS + (nBlocks - 1) * bs : nBlocks * bs;
    st.iNeed = (int)needSyms;
    if ((k.nsyms > a.symStride && needSyms > a.symStride) || needSyms > symCap || st.cEnd + 4 > cwCap) { st.outLen = -2; st.go = false; }
}

//! the nibbles no codeword loop writes: the header's six in front, and zeros behind the decoded ones (the reference's buffer is zeroed)
template <int G>
__device__ __forceinline__ void frameNibbles(const PacketState &st, const DecodeArgs &a, const int t, unsigned char *sNib)
{
    if (!st.go) return;
    const int shift = a.explicitHdr ? 1 : 0;
    if (a.explicitHdr) { sNib[0] = st.h0 & 0xf; sNib[1] = st.h0 >> 4; sNib[2] = st.h1 & 0xf; sNib[3] = 0; sNib[4] = st.h2 & 0xf; sNib[5] = st.h2 >> 4; }
    for (long long v = st.cEnd + shift + t; v < 2 * (st.dataLength + 1); v += G) sNib[v] = 0;
}

/*! Behind the nibbles' barrier, st.error the whole group's: the error drop, then the checksum (:367-388): crc = sum over the bytes of
 * byte * x^(8 (len-1-i)), folded over the lanes, then the two LFSR masks; lane 0 un-masks the packet's two crc bytes in place. */
template <int G>
__device__ __forceinline__ void checkPayload(PacketState &st, const DecodeArgs &a, const int t, unsigned char *sNib)
{
    if (st.go && st.error && a.errorCheck) { st.dropped = 1; st.go = false; }                // :342, :363
    if (!(st.go && (a.explicitHdr ? (st.h1 & 1) != 0 : st.checkCrc))) return;
    const int base = a.explicitHdr ? 3 : 0;
    const int len = a.explicitHdr ? (int)st.packetLength : a.dataLength;
    unsigned acc = 0;
    for (int i = t; i < len; i += G)
    {
        const unsigned byte = sNib[2 * (base + i)] | (sNib[2 * (base + i) + 1] << 4);
        // res_{i+1} = S(res_i) ^ d_i: byte i is shifted by the len-1-i byte steps that follow it
        acc ^= crcShift(byte, kCodec.xpow[len - 1 - i]);
    }
    unsigned crc = groupXor<G>(acc);
    crc ^= kCodec.lfsr8[len];                                                                // res ^= v after len steps
    crc ^= (unsigned)kCodec.lfsr8[len + 1] << 8;                                             // ... and one step later, high byte
    crc &= 0xffff;
    const unsigned packetCrc = (sNib[2 * (base + len)] | (sNib[2 * (base + len) + 1] << 4)) |
                               ((sNib[2 * (base + len) + 2] | (sNib[2 * (base + len) + 3] << 4)) << 8);
    st.iCrc = crc == packetCrc ? 1 : -1;
    if (a.explicitHdr)
    {
        if (crc != packetCrc && st.checkCrc) { st.dropped = 1; st.go = false; }
    }
    else if (crc != packetCrc) { st.dropped = 1; st.go = false; }
    if (st.go && t == 0)
    {
        // bytes[len] ^= crc, bytes[len + 1] ^= crc >> 8 (:377-378, :386-387)
        const unsigned lo = (sNib[2 * (base + len)] | (sNib[2 * (base + len) + 1] << 4)) ^ (crc & 0xff);
        const unsigned hi = (sNib[2 * (base + len) + 2] | (sNib[2 * (base + len) + 3] << 4)) ^ (crc >> 8);
        sNib[2 * (base + len)] = lo & 0xf; sNib[2 * (base + len) + 1] = (lo >> 4) & 0xf;
        sNib[2 * (base + len) + 2] = hi & 0xf; sNib[2 * (base + len) + 3] = (hi >> 4) & 0xf;
    }
}

//! behind the last barrier: the bytes out of the nibbles, out_len, dropped and the report. known = false: -3, nothing else of the packet.
template <int G>
__device__ __forceinline__ void writePacket(PacketState &st, const DecodeArgs &a, const GroupPacket &k, const unsigned char *sNib, const bool known)
{
    int dOfs = 0;
    if (st.go && a.explicitHdr && !a.hdr) { dOfs = 3; st.dataLength -= 5; }                  // :379
    // `dataLength -= 5` on a size_t wraps for a header without the crc flag that announces fewer than 2 bytes; the
    // reference then fails to allocate its output and posts nothing
    if (st.go && st.dataLength >= 0)
    {
        for (long long i = k.t; i < st.dataLength; i += G) k.out[i] = (unsigned char)(sNib[2 * (dOfs + i)] | (sNib[2 * (dOfs + i) + 1] << 4));   // :391-395
        st.outLen = (int)st.dataLength;
    }
    if (k.have && k.t == 0)
    {
        a.outLen[k.p] = known ? st.outLen : -3;
        a.dropped[k.p] = st.dropped;
        // (error: every lane's own after the header, the group's after the nibbles -- where the decode ended, it is the reference's flag)
        if (a.info != nullptr) writePacketInfo(a.info, k.p, st.iLen, st.iRdd, st.iCrc, st.iRes, st.error ? 1 : 0, st.iNeed);
    }
}

} // namespace

/*! One packet per group of G lanes under the settings in `a` and the caps of THOSE settings; `slice` is the launch's distance between two
 * groups' LDS (>= what the caps need). decodeGroup hands in its kernel arguments, so every setting is a launch-uniform scalar there;
 * decodeGroupCfgs hands in the packet's own entry of the table, the same for every lane of a group (the lanes of a group share p): whatever
 * is group-uniform below stays so, and no barrier stands under a condition (the `go` flag), so the 256 threads meet at every one of them
 * whatever their packets' settings are. known = false (no such entry): the packet is reported as -3 and nothing of it is read or written.
 * a.rdd < 0 (LORAHIP_RDD_FROM_HEADER): `caps` are the largest of the entry's five rates; the packet's rate, and with it its own caps and
 * layout, are resolved behind the first barrier, and from there on it is a packet of the uniform launch at that rate. a.info, where set,
 * gets the packet's header report (struct lorahip_packet_info); it changes nothing else. */
template <int G>
__device__ __forceinline__ void decodeGroupBody(const DecodeArgs a, const DecodeCaps caps, const int slice, const int perBlock, const bool known)
{
    // per packet: symCap Gray-coded symbols (u16), then the codewords (u8), then the nibbles (u8), 16-byte aligned slices
    extern __shared__ __attribute__((aligned(16))) unsigned char smemDec[];
    PacketState st;
    const GroupPacket k = packetOf<G>(a, perBlock, known, st);
    const int t = k.t, nsyms = k.nsyms, PPM = k.PPM, sf = a.sf;
    int symCap = caps.symCap, cwCap = caps.cwCap;
    unsigned short *sSym = reinterpret_cast<unsigned short *>(smemDec + (size_t)k.g * slice);
    unsigned char *sCw = smemDec + (size_t)k.g * slice + symCap * 2;
    unsigned char *sNib = sCw + cwCap;
    const unsigned short *in = a.syms + (size_t)k.pc * a.symStride;
    // the coding rate of the setter. A header-rate entry (a.rdd < 0) has none: the packet's header names it, behind the first barrier, and
    // everything from the counts to `cwLoad` is worked out again there; until then only the Gray-code load runs, which does not depend on it
    RateCounts n = countsAt(nsyms, PPM, st.rate);
    int symLoad = n.numSymbols < symCap ? n.numSymbols : symCap;                             // what of it this slice holds
    int cwLoad = n.numCodewords + 4 < cwCap ? n.numCodewords + 4 : cwCap;

    // ---- Gray code with rounding to the symbol size (:218-222) --------------------------------------------------------
    if (st.go && !a.interleaving && nsyms > a.symStride) { st.outLen = -2; st.go = false; }  // every symbol is output: the row must hold them all
    // header rate: numSymbols is nsyms rounded up to a block of 4..8, so nsyms + 7 covers every rate (zeros behind the row, as always)
    const int grayLoad = !a.interleaving ? n.numSymbols : a.rdd < 0 ? (nsyms + 7 < symCap ? nsyms + 7 : symCap) : symLoad;
    if (st.go)
        for (int i = t; i < grayLoad; i += G)
        {
            unsigned short sym = i < k.rowSyms ? in[i] : 0;
            sym = (unsigned short)(sym + (1 << (sf - PPM)) / 2);
            sym = (unsigned short)(sym >> (sf - PPM));
            sym = (unsigned short)(sym ^ (sym >> 1));
            if (a.interleaving) sSym[i] = sym;
            else reinterpret_cast<unsigned short *>(k.out)[i] = sym;                        // :264-270
        }
    if (st.go && !a.interleaving) { st.outLen = n.numSymbols; st.go = false; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    // ---- header rate (LORAHIP_RDD_FROM_HEADER): every lane of the group reads the rate field out of the first eight symbols, alike ----
    // Codeword 2 of the first block holds it: de-interleaved at 4/8 over symbols 0..7 and never whitened at ANY configured rate (:228-255:
    // both branches give the first PPM codewords from exactly these symbols, and the explicit header's five are skipped by the whitening),
    // so the field does not depend on the rate the body below runs at. From here on the packet is a packet of the uniform launch at that
    // rate: its block size, its counts, and the caps and the slice layout of THAT rate's plan (they fit: the entry's slice is the
    // largest of the five; Gray-coded symbols behind symCap lie where its codewords go and are overwritten before anything reads them).
    // A field of 5..7 runs at 4/8 into the header stage, which drops it (the error check or :297) -- as it would under every setting.
    if (a.rdd < 0)                                                                           // (group-uniform; no barrier inside)
    {
        if (st.go)
        {
            unsigned cw2 = 0;
            for (int s = 0; s < LORAHIP_N_HDR_SYMBOLS; s++)
            {
                int m = 2 - (s < PPM ? s : s - PPM);                                        // 2 - s % PPM (5 <= PPM: a header-rate entry has a header)
                if (m < 0) m += PPM;
                cw2 |= ((sSym[s] >> m) & 1u) << s;
            }
            bool e2 = false, b2 = false;
            const int field = ((decodeHamming84((unsigned char)cw2, e2, b2) & 0xf) >> 1) & 0x7;
            st.rate = field > 4 ? LORAHIP_HDR_RDD : field;
        }
        const DecodeCaps cr = decodeCapsAt(sf, a.ppm, st.rate, 1, a.dataLength, a.symStride);   // (a header-rate entry has a header)
        symCap = cr.symCap; cwCap = cr.cwCap;
        sCw = smemDec + (size_t)k.g * slice + symCap * 2;
        sNib = sCw + cwCap;
        n = countsAt(nsyms, PPM, st.rate);
        symLoad = n.numSymbols < symCap ? n.numSymbols : symCap;
        cwLoad = n.numCodewords + 4 < cwCap ? n.numCodewords + 4 : cwCap;
    }

    // ---- de-interleave + de-whitening (placeCodeword), one codeword per lane and round, out of the Gray-coded symbols in LDS ----------
    if (st.go)
        for (int c = t; c < cwLoad; c += G)
        {
            unsigned cw = 0;
            if (c < n.numCodewords)
            {
                const CodewordPlace w = placeCodeword(c, PPM, st.rate, n, a.explicitHdr);
                // (a block whose symbols lie behind the slice is behind what any length can need: left zero, never read)
                if (w.whole && w.symOff + (4 + w.R) <= symLoad)
                    for (int s = 0; s < 4 + w.R; s++)
                    {
                        int m = w.i - (s % PPM);
                        if (m < 0) m += PPM;
                        cw |= ((sSym[w.symOff + s] >> m) & 1u) << s;
                    }
                cw ^= w.white;
            }
            sCw[c] = (unsigned char)cw;
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    // ---- header, needs, and the nibbles of the codewords the bytes need: the table FEC --------------------------------------------
    bool bad = false;
    unsigned char hn[LORAHIP_N_HDR_CODEWORDS] = { 0, 0, 0, 0, 0 };
    if (st.go && a.explicitHdr)
        for (int c = 0; c < LORAHIP_N_HDR_CODEWORDS; c++) hn[c] = decodeHamming84(sCw[c], st.error, bad);
    decodeHeader(st, a, hn, n.numCodewords);
    decodeNeeds(st, a, k, n.bs, symCap, cwCap);
    frameNibbles<G>(st, a, t, sNib);
    if (st.go)
        for (int c = (a.explicitHdr ? LORAHIP_N_HDR_CODEWORDS : 0) + t; c < st.cEnd; c += G)
        {
            const unsigned char cw = sCw[c];
            const unsigned char nib = c < PPM ? decodeHamming84(cw, st.error, bad) : decodeNibble(cw, st.rdd, st.error, bad);
            sNib[c + (a.explicitHdr ? 1 : 0)] = nib & 0xf;
        }
    st.error = groupAny<G>(st.error);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    checkPayload<G>(st, a, t, sNib);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();
    writePacket<G>(st, a, k, sNib, known);
}

template <int G>
__global__ void __launch_bounds__(256) decodeGroup(const DecodeArgs a, const DecodeCaps caps, const int slice, const int perBlock)
{
    decodeGroupBody<G>(a, caps, slice, perBlock, true);
}

//! What the four group kernels share on the host. The LDS a workgroup of theirs may ask for: the device's 160 KiB (the plans fit under it).
constexpr int kGroupLdsMax = 160 * 1024;

//! lanes per packet by the symbols of the longest row a launch can meet (a lane per symbol in the widest pass, about as many codewords)
static int lanesFor(const long rowSyms) { return rowSyms <= 48 ? 8 : rowSyms <= 96 ? 16 : rowSyms <= 200 ? 32 : 64; }

//! packets per workgroup of 256 threads: one per lane group, or as many slices as fit the LDS if that is fewer (0: not even one)
static int packetsPerBlock(const int lanes, const int slice)
{
    const int perBlock = 256 / lanes;
    return slice * perBlock > kGroupLdsMax ? kGroupLdsMax / slice : perBlock;
}

//! f(std::integral_constant<int, G>()) for the kernel instance of G = `lanes` lanes per packet
template <class F>
static hipError_t withLanes(const int lanes, F &&f)
{
    if (lanes == 8) return f(std::integral_constant<int, 8>());
    if (lanes == 16) return f(std::integral_constant<int, 16>());
    if (lanes == 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}

//! group kernel K over nPackets packets, perBlock of them per workgroup on `slice` bytes of LDS each; the attribute once per instance and device
template <auto K, class... Args>
static hipError_t launchGroup(const unsigned nPackets, const int perBlock, const int slice, hipStream_t stream, const Args &...args)
{
    static unsigned long long attrDone = 0;
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(K), kGroupLdsMax, attrDone);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(K, dim3((nPackets + perBlock - 1) / perBlock), dim3(256), size_t(slice) * perBlock, stream, args...);
    return hipGetLastError();
}

//! the slice a configuration needs (see DecodeCaps): the symbols / codewords that can reach the output, or the whole row if that is less
//! A header-rate entry (rdd < 0) runs each packet on the caps of the rate its header names: it gets the largest of the five in each component,
//! and the largest of their slices (which holds any of the five layouts, and the Gray-code load of min(nsyms + 7, symCap) symbols).
static DecodeCaps decodeCaps(const DecodeCfg &a, const int symStride, int &slice)
{
    DecodeCaps c = { 0, 0 };
    slice = 0;
    for (int r = a.rdd < 0 ? 0 : a.rdd; r <= (a.rdd < 0 ? 4 : a.rdd); r++)
    {
        const DecodeCaps cr = decodeCapsAt(a.sf, a.ppm, r, a.explicitHdr, a.dataLength, symStride);
        const int sr = decodeSliceOf(cr);
        c.symCap = cr.symCap > c.symCap ? cr.symCap : c.symCap;
        c.cwCap = cr.cwCap > c.cwCap ? cr.cwCap : c.cwCap;
        slice = sr > slice ? sr : slice;
    }
    return c;
}

/* What a launch over rows of symStride symbols under these settings runs on -- the one place that decides it, for the uniform launch (one
 * entry), the table launch and lorahip_decode_plan. Every entry gets the caps of ITS settings (its group lays out its slice with them); the
 * launch has ONE lane count and ONE slice: the lanes by the largest symCap (n symbols make about n * PPM / (4 + rdd) codewords), the slice
 * the largest entry's, and as many packets per workgroup as fit 160 KiB of LDS (0: not even one -- the entry points bound data_length, so
 * this cannot happen). A table with one long entry therefore runs few packets per workgroup for ALL its packets. */
DecodeTiling decodePlan(DecodeCfg *cfgs, const size_t nCfgs, const int symStride)
{
    DecodeTiling t = { 0, 0, 0, 0, 0 };
    for (size_t i = 0; i < nCfgs; i++)
    {
        int slice = 0;
        const DecodeCaps c = decodeCaps(cfgs[i], symStride, slice);
        cfgs[i].symCap = c.symCap; cfgs[i].cwCap = c.cwCap;
        t.symCap = c.symCap > t.symCap ? c.symCap : t.symCap;
        t.cwCap = c.cwCap > t.cwCap ? c.cwCap : t.cwCap;
        t.slice = slice > t.slice ? slice : t.slice;
    }
    t.lanes = lanesFor(t.symCap);
    t.perBlock = packetsPerBlock(t.lanes, t.slice);
    return t;
}

hipError_t launchDecode(const DecodeArgs &rows, const DecodeCfg &cfg, const int variant, hipStream_t stream)
{
    if (rows.nPackets == 0) return hipSuccess;
    const DecodeArgs a = withCfg(rows, cfg);
    if (variant == 1)
    {
        hipLaunchKernelGGL(decodePackets, dim3((a.nPackets + 63) / 64), dim3(64), 0, stream, a);
        return hipGetLastError();
    }
    DecodeCfg c = cfg;
    const DecodeTiling t = decodePlan(&c, 1, a.symStride);
    if (t.perBlock < 1) return hipErrorInvalidValue;                // (lorahip_decode_packets bounds data_length: cannot happen)
    const DecodeCaps caps = { t.symCap, t.cwCap };
    return withLanes(t.lanes, [&](auto g) { return launchGroup<decodeGroup<decltype(g)::value>>(a.nPackets, t.perBlock, t.slice, stream, a, caps, t.slice, t.perBlock); });
}

/***********************************************************************
 * group-per-packet encoder (LoRaEncoder.cpp:161-233 on LoRaCodes.hpp): bytes -> symbols
 **********************************************************************/
namespace {

//! the sx FEC of one nibble at coding rate rdd (LoRaCodes.hpp: encodeHamming84sx / 74sx, encodeParity64 / 54): the parity bits are
//! the decoder's cover masks over the data bits; 4/7 and 4/6 are prefixes of 4/8, 4/5 is one parity bit over the nibble
__device__ __forceinline__ unsigned encodeNibble(const unsigned nib, const int rdd)
{
    const unsigned x = nib & 0xf;
    if (rdd == 0) return x;
    if (rdd == 1) return x | ((unsigned)parityOf(x) << 4);
    const unsigned full = x | ((unsigned)parityOf(x & LORAHIP_COVER0 & 0xf) << 4) | ((unsigned)parityOf(x & LORAHIP_COVER1 & 0xf) << 5) |
                          ((unsigned)parityOf(x & LORAHIP_COVER2 & 0xf) << 6) | ((unsigned)parityOf(x & LORAHIP_COVER3 & 0xf) << 7);
    return full & (0xffu >> (4 - rdd));
}

} // namespace

/*! What a launch can need of a group's LDS slice: the payload + crc bytes, then the codewords. Both follow from the ROWS (a packet whose
 * bytes or symbols do not fit its rows is refused with -2 before it touches the slice), not from the packet. */
struct EncodeCaps { int byteCap, cwCap; };

/* A group of G lanes owns a packet. Pass 1: a lane per payload byte -- load (contiguous), keep in LDS, its term of the crc (byte * x^(8 k)
 * mod P, as decodeGroup sums it); the group's xor is the checksum, lane 0 appends it. Pass 2: a lane per codeword -- nibble from LDS, FEC,
 * whitening from the sequence table (the encoder's Sx1272ComputeWhitening and the decoder's two registers give the same bytes: position
 * = codeword index behind the header codewords, in both blocks). Pass 3: a lane per output symbol -- bit m = bit k of codeword
 * (m + k) % PPM of its interleaver block, Gray -> binary, shift; lanes store consecutive symbols of the row, zeros behind the packet.
 * Pad nibbles (codewords behind the last byte, up to a whole block) are 0: the reference reads them past the end of its vector.
 * encodeGroup hands in its kernel arguments (every setting a launch-uniform scalar); encodeGroupCfgs hands in the packet's own entry of its
 * table with that entry's caps, and `slice`, the launch's distance between two groups' LDS. No barrier stands under a condition.
 * known = false (no such entry): the row is zeroed and reported as -3, nothing of the packet is read. */
template <int G>
__device__ __forceinline__ void encodeGroupBody(const EncodeArgs a, const EncodeCaps caps, const int slice, const int perBlock, const bool known)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smemEnc[];
    const int g = threadIdx.x / G, t = threadIdx.x % G;
    unsigned char *sByte = smemEnc + (size_t)g * slice;
    unsigned char *sCw = sByte + caps.byteCap;
    const unsigned p = blockIdx.x * perBlock + g;
    const bool have = g < perBlock && p < a.nPackets;
    const unsigned pc = have ? p : 0;
    const int len = have ? a.nbytes[pc] : 0;
    const unsigned char *in = a.bytes + (size_t)pc * a.byteStride;
    unsigned short *out = a.syms + (size_t)pc * a.symStride;

    const int sf = a.sf;
    const int PPM = a.ppm == 0 ? sf : a.ppm;                                                 // LoRaEncoder.cpp:165
    const int bs = 4 + a.rdd;
    const int hdrCw = a.explicitHdr ? LORAHIP_N_HDR_CODEWORDS : 0;
    int outcome = known ? -1 : -3;                                                           // nothing defined / no such entry (see lorahip.h)
    bool go = have && known && len >= 0;
    if (go && len > a.byteStride) { outcome = -2; go = false; }
    const int nb = go ? len + (a.crc ? 2 : 0) : 0;                                           // :171
    const int numCodewords = ((2 * nb + hdrCw + PPM - 1) / PPM) * PPM;                       // :175
    const int numSymbols = LORAHIP_N_HDR_SYMBOLS + (numCodewords / PPM - 1) * bs;            // :176
    if (go && numCodewords == 0) go = false;                                                 // numCodewords / PPM - 1 wraps in the reference
    if (go && (numSymbols > a.symStride || numCodewords > caps.cwCap || nb > caps.byteCap)) { outcome = -2; go = false; }

    // ---- pass 1: bytes into LDS, checksum (:181-185; sx1272DataChecksum = the crc of decodeGroup) ---------------------------
    if (go)
    {
        unsigned acc = 0;
        for (int i = t; i < len; i += G)
        {
            const unsigned byte = in[i];
            sByte[i] = (unsigned char)byte;
            if (a.crc) acc ^= crcShift(byte, kCodec.xpow[len - 1 - i]);
        }
        if (a.crc)
        {
            unsigned crc = groupXor<G>(acc);
            crc ^= kCodec.lfsr8[len];
            crc ^= (unsigned)kCodec.lfsr8[len + 1] << 8;
            if (t == 0) { sByte[len] = (unsigned char)(crc & 0xff); sByte[len + 1] = (unsigned char)((crc >> 8) & 0xff); }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    // ---- pass 2: FEC + whitening, one codeword per lane and round (:187-212) -------------------------------------------------
    if (go)
    {
        unsigned char h[3] = { 0, 0, 0 };
        if (a.explicitHdr)
        {
            h[0] = (unsigned char)(len & 0xff);                                              // :189-192
            h[1] = (unsigned char)((a.crc ? 1 : 0) | (a.rdd << 1));
            h[2] = headerChecksum(h);
        }
        for (int c = t; c < numCodewords; c += G)
        {
            unsigned cw;
            if (c < hdrCw)                                                                   // :194-198, always 4/8, never whitened
            {
                const unsigned nib = c == 0 ? h[0] >> 4 : c == 1 ? h[0] & 0xf : c == 2 ? h[1] & 0xf : c == 3 ? h[2] >> 4 : h[2] & 0xf;
                cw = encodeNibble(nib, LORAHIP_HDR_RDD);
            }
            else
            {
                const int d = c - hdrCw;                                                     // data nibble, low nibble of a byte first
                const int R = c < PPM ? LORAHIP_HDR_RDD : a.rdd;                             // the first block is always 4/8
                const unsigned byte = (d >> 1) < nb ? sByte[d >> 1] : 0u;                    // pad nibbles are 0
                cw = encodeNibble((d & 1) ? byte >> 4 : byte & 0xf, R);
                if (a.whitening && (d >> 1) < LORAHIP_WHITEN_LEN)
                    cw ^= kCodec.white[R == 1 ? 1 : 0][d & 1][d >> 1] & (0xffu >> (4 - R));
            }
            sCw[c] = (unsigned char)cw;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    // ---- pass 3: diagonal interleave (LoRaCodes.hpp diagonalInterleaveSx), Gray -> binary, shift (:215-226) ------------------
    if (have)
    {
        const int nOut = go ? numSymbols : 0;
        for (int s = t; s < a.symStride; s += G)
        {
            unsigned sym = 0;
            if (s < nOut)
            {
                int cwOff = 0, k = s;
                if (s >= LORAHIP_N_HDR_SYMBOLS)
                {
                    const int x = (s - LORAHIP_N_HDR_SYMBOLS) / bs;
                    k = (s - LORAHIP_N_HDR_SYMBOLS) - x * bs;
                    cwOff = PPM + x * PPM;
                }
                int i = k % PPM;
                for (int m = 0; m < PPM; m++)
                {
                    sym |= ((sCw[cwOff + i] >> k) & 1u) << m;
                    if (++i == PPM) i = 0;
                }
                sym ^= sym >> 8; sym ^= sym >> 4; sym ^= sym >> 2; sym ^= sym >> 1;          // grayToBinary16
                sym = (sym << (sf - PPM)) & 0xffffu;
            }
            out[s] = (unsigned short)sym;
        }
        if (t == 0) a.nsyms[p] = go ? numSymbols : outcome;
    }
}

template <int G>
__global__ void __launch_bounds__(256) encodeGroup(const EncodeArgs a, const EncodeCaps caps, const int perBlock)
{
    encodeGroupBody<G>(a, caps, (caps.byteCap + caps.cwCap + 15) & ~15, perBlock, true);
}

//! symbols of a packet of n payload bytes (LoRaEncoder.cpp:171-176); -1 where the reference's own expression wraps
long encodeNumSymbols(const int sf, const int ppm, const int rdd, const int explicitHdr, const int crc, const size_t nBytes)
{
    const long PPM = ppm == 0 ? sf : ppm;
    const long nb = long(nBytes) + (crc ? 2 : 0);
    const long numCodewords = ((2 * nb + (explicitHdr ? LORAHIP_N_HDR_CODEWORDS : 0) + PPM - 1) / PPM) * PPM;
    if (numCodewords == 0) return -1;
    return LORAHIP_N_HDR_SYMBOLS + (numCodewords / PPM - 1) * (4 + rdd);
}

//! the slice an entry needs over rows of byteStride bytes and symStride symbols (see EncodeCaps)
static EncodeCaps encodeCaps(const EncodeCfg &e, const int byteStride, const int symStride)
{
    const long PPM = e.ppm == 0 ? e.sf : e.ppm, bs = 4 + e.rdd;
    const long nbMax = long(byteStride) + (e.crc ? 2 : 0);
    const long cwByBytes = ((2 * nbMax + (e.explicitHdr ? LORAHIP_N_HDR_CODEWORDS : 0) + PPM - 1) / PPM) * PPM;
    const long cwBySyms = symStride < LORAHIP_N_HDR_SYMBOLS ? 0 : ((symStride - LORAHIP_N_HDR_SYMBOLS) / bs + 1) * PPM;
    EncodeCaps c;
    c.cwCap = int(cwByBytes < cwBySyms ? cwByBytes : cwBySyms);
    c.byteCap = (c.cwCap / 2 + 2 + 3) & ~3;
    return c;
}

/* What a launch over rows of byteStride bytes and symStride symbols under these settings runs on -- the one place that decides it, for the
 * uniform launch (one entry) and the table launch, as decodePlan is for the decoder. Every entry gets the caps of ITS settings (its group lays
 * out its slice with them); the launch has ONE lane count and ONE slice: the lanes by the symbols a row can hold under the entry that makes
 * most of it, the slice the largest entry's, and as many packets per workgroup as fit the LDS (0: not even one -- the entry points bound
 * byte_stride, so this cannot happen). */
EncodeTiling encodePlan(EncodeCfg *cfgs, const size_t nCfgs, const int byteStride, const int symStride)
{
    EncodeTiling t = { 0, 0, 0, 0, 0 };
    long rowSyms = 0;
    for (size_t i = 0; i < nCfgs; i++)
    {
        EncodeCfg &e = cfgs[i];
        const EncodeCaps c = encodeCaps(e, byteStride, symStride);
        e.byteCap = c.byteCap; e.cwCap = c.cwCap;
        t.byteCap = c.byteCap > t.byteCap ? c.byteCap : t.byteCap;
        t.cwCap = c.cwCap > t.cwCap ? c.cwCap : t.cwCap;
        const long bySyms = c.cwCap == 0 ? 0 : LORAHIP_N_HDR_SYMBOLS + (c.cwCap / (e.ppm == 0 ? e.sf : e.ppm) - 1) * (4 + e.rdd);
        rowSyms = bySyms > rowSyms ? bySyms : rowSyms;
        const int slice = (c.byteCap + c.cwCap + 15) & ~15;
        t.slice = slice > t.slice ? slice : t.slice;
    }
    t.lanes = lanesFor(rowSyms);
    t.perBlock = packetsPerBlock(t.lanes, t.slice);
    return t;
}

//! (defined with the table kernels below)
__host__ __device__ __forceinline__ EncodeArgs withCfg(const EncodeArgs &rows, const EncodeCfg &e);

hipError_t launchEncode(const EncodeArgs &rows, const EncodeCfg &cfg, hipStream_t stream)
{
    if (rows.nPackets == 0) return hipSuccess;
    EncodeCfg c = cfg;
    const EncodeTiling t = encodePlan(&c, 1, rows.byteStride, rows.symStride);
    if (t.perBlock < 1) return hipErrorInvalidValue;                // (lorahip_encode_packets bounds byte_stride: cannot happen)
    const EncodeArgs a = withCfg(rows, c);
    const EncodeCaps caps = { t.byteCap, t.cwCap };
    // (encodeGroup works its slice out of the caps: the one entry's is the launch's)
    return withLanes(t.lanes, [&](auto g) { return launchGroup<encodeGroup<decltype(g)::value>>(a.nPackets, t.perBlock, t.slice, stream, a, caps, t.perBlock); });
}

/***********************************************************************
 * the decoder with the settings per packet (lorahip_decode_packets_cfgs): the kernels above over a table, and the hand-off's channel remap.
 * Behind the uniform kernels on purpose: those stay the functions they were, in the order they were.
 **********************************************************************/
__global__ void __launch_bounds__(64) decodePacketsCfgs(const DecodeArgs rows, const DecodeCfgTable tab)
{
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rows.nPackets) return;
    const int i = cfgIndexOf(tab, p);
    if (i < 0)
    {
        rows.outLen[p] = -3; rows.dropped[p] = 0;
        if (rows.info != nullptr) writePacketInfo(rows.info, p, -1, -1, 0, -1, 0, -1);
        return;
    }
    decodeOnePacket(withCfg(rows, tab.e[i]), p);
}


template <int G>
__global__ void __launch_bounds__(256) decodeGroupCfgs(const DecodeArgs rows, const DecodeCfgTable tab, const int slice, const int perBlock)
{
    const int g = threadIdx.x / G;
    const unsigned p = blockIdx.x * perBlock + g;
    const int i = (g < perBlock && p < rows.nPackets) ? cfgIndexOf(tab, p) : 0;     // (an idle group: any entry, it does nothing)
    const DecodeCfg &e = tab.e[i < 0 ? 0 : i];
    const DecodeCaps caps = { e.symCap, e.cwCap };
    decodeGroupBody<G>(withCfg(rows, e), caps, slice, perBlock, i >= 0);
}

//! the kernel argument of a table launch, hard or soft, over 1 <= nCfgs <= LORAHIP_DEC_MAX_CFGS entries
static DecodeCfgTable decodeTableOf(const DecodeCfg *cfgs, const size_t nCfgs, const int *index, const int *table, const int nTable)
{
    DecodeCfgTable tab;
    tab.index = index; tab.table = table; tab.nTable = nTable; tab.nCfgs = int(nCfgs);
    for (size_t i = 0; i < size_t(LORAHIP_DEC_MAX_CFGS); i++) tab.e[i] = cfgs[i < nCfgs ? i : 0];      // (no entry of the argument block is left unset)
    return tab;
}

hipError_t launchDecodeCfgs(const DecodeArgs &rows, const DecodeCfg *cfgs, const size_t nCfgs, const int *index, const int *table, const int nTable,
                            const int variant, hipStream_t stream)
{
    if (rows.nPackets == 0) return hipSuccess;
    if (nCfgs == 0 || nCfgs > size_t(LORAHIP_DEC_MAX_CFGS)) return hipErrorInvalidValue;
    DecodeCfgTable tab = decodeTableOf(cfgs, nCfgs, index, table, nTable);
    const DecodeTiling t = decodePlan(tab.e, nCfgs, rows.symStride);
    if (variant == 1)
    {
        hipLaunchKernelGGL(decodePacketsCfgs, dim3((rows.nPackets + 63) / 64), dim3(64), 0, stream, rows, tab);
        return hipGetLastError();
    }
    if (t.perBlock < 1) return hipErrorInvalidValue;                // (lorahip_decode_packets_cfgs bounds data_length: cannot happen)
    return withLanes(t.lanes, [&](auto g) { return launchGroup<decodeGroupCfgs<decltype(g)::value>>(rows.nPackets, t.perBlock, t.slice, stream, rows, tab, t.slice, t.perBlock); });
}

//! channel_dev[j] = globalOf[channel_dev[j]] for the n rows one part of a mixed handle packed (lorahip_rx.cpp: the hand-off speaks global channels)
__global__ void __launch_bounds__(256) remapChannels(int *chan, const int *globalOf, const unsigned n, const int nLocal)
{
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int c = chan[j];
    if (c >= 0 && c < nLocal) chan[j] = globalOf[c];
}

hipError_t launchRemapChannels(int *chan, const int *globalOf, const size_t n, const size_t nLocal, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(remapChannels, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, chan, globalOf, unsigned(n), int(nLocal));
    return hipGetLastError();
}

/***********************************************************************
 * the encoder with the settings per packet (lorahip_encode_packets_cfgs): encodeGroupBody over a table, as decodeGroupCfgs runs
 * decodeGroupBody. Behind the uniform kernels on purpose: those stay the functions they were, in the order they were.
 **********************************************************************/
/*! The settings of a table launch, by value in the kernel arguments: packet p runs under e[i], i = index[p] or table[index[p]] (cfgIndexOf);
 * without such an entry the outcome is -3 and the row is zeroed. The caps are the slice entry i needs over the rows of the launch. */
struct EncodeCfgTable
{
    const int *index, *table;
    int nTable, nCfgs;
    EncodeCfg e[LORAHIP_ENC_MAX_CFGS];
};

//! the rows of the launch with entry e as their settings: what encodeGroupBody reads as `a`
__host__ __device__ __forceinline__ EncodeArgs withCfg(const EncodeArgs &rows, const EncodeCfg &e)
{
    EncodeArgs a = rows;
    a.sf = e.sf; a.ppm = e.ppm; a.rdd = e.rdd; a.explicitHdr = e.explicitHdr; a.crc = e.crc; a.whitening = e.whitening;
    return a;
}

template <int G>
__global__ void __launch_bounds__(256) encodeGroupCfgs(const EncodeArgs rows, const EncodeCfgTable tab, const int slice, const int perBlock)
{
    const int g = threadIdx.x / G;
    const unsigned p = blockIdx.x * perBlock + g;
    const int i = (g < perBlock && p < rows.nPackets) ? cfgIndexOf(tab, p) : 0;     // (an idle group: any entry, it does nothing)
    const EncodeCfg &e = tab.e[i < 0 ? 0 : i];
    const EncodeCaps caps = { e.byteCap, e.cwCap };
    encodeGroupBody<G>(withCfg(rows, e), caps, slice, perBlock, i >= 0);
}

hipError_t launchEncodeCfgs(const EncodeArgs &rows, const EncodeCfg *cfgs, const size_t nCfgs, const int *index, const int *table, const int nTable,
                            hipStream_t stream)
{
    if (rows.nPackets == 0) return hipSuccess;
    if (nCfgs == 0 || nCfgs > size_t(LORAHIP_ENC_MAX_CFGS)) return hipErrorInvalidValue;
    EncodeCfgTable tab;
    tab.index = index; tab.table = table; tab.nTable = nTable; tab.nCfgs = int(nCfgs);
    for (size_t i = 0; i < nCfgs; i++) tab.e[i] = cfgs[i];
    const EncodeTiling t = encodePlan(tab.e, nCfgs, rows.byteStride, rows.symStride);
    for (size_t i = nCfgs; i < size_t(LORAHIP_ENC_MAX_CFGS); i++) tab.e[i] = tab.e[0];                  // (no entry of the argument block is left unset)
    if (t.perBlock < 1) return hipErrorInvalidValue;                // (lorahip_encode_packets_cfgs bounds byte_stride: cannot happen)
    return withLanes(t.lanes, [&](auto g) { return launchGroup<encodeGroupCfgs<decltype(g)::value>>(rows.nPackets, t.perBlock, t.slice, stream, rows, tab, t.slice, t.perBlock); });
}

/***********************************************************************
 * the soft-decision decoder (lorahip_decode_packets_soft): a symbol is its PPM log-likelihood ratios (positive: bit 1 of the Gray-coded,
 * rounded symbol value), and every FEC nibble is the x in 0..15 whose codeword correlates best with the codeword's LLRs. Behind the hard
 * kernels because it needs the encoder's encodeNibble. decodeSoftBody runs the stages decodeGroupBody runs (packetOf .. writePacket, in
 * front of decodeGroupBody) around its own front end; the `error` flag is still the hard decoders' over the hard bits (llr > 0). The LLRs
 * stay in global memory: a lane gathers the (at most eight) values of its codeword from the symbols of its interleaver block -- the same
 * diagonal the hard kernel walks in LDS -- so a packet's LDS slice holds its nibbles and nothing else, and no configuration outgrows it.
 **********************************************************************/
namespace {

/*! Codeword c of packet row `llr` (PPM floats per symbol, rowSyms symbols present): its hard bits, de-whitened, and in L[0..7] its LLRs with a
 * whitening bit of 1 negating the value. Bits the block does not carry, symbols behind the row, a block that is not whole and codewords
 * behind n.numCodewords are hard 0 / LLR 0, as decodeGroupBody's zero symbols and zero codewords are. */
__device__ __forceinline__ unsigned softCodeword(const float *llr, const int rowSyms, const int c, const int PPM, const int rate, const RateCounts &n,
                                                 const int explicitHdr, float (&L)[8])
{
#pragma unroll
    for (int s = 0; s < 8; s++) L[s] = 0.0f;
    if (c >= n.numCodewords) return 0u;
    const CodewordPlace w = placeCodeword(c, PPM, rate, n, explicitHdr);
    unsigned cw = 0;
    if (w.whole)
    {
#pragma unroll
        for (int s = 0; s < 8; s++)
        {
            int m = w.i - (s % PPM);
            if (m < 0) m += PPM;
            if (s < 4 + w.R && w.symOff + s < rowSyms) L[s] = llr[(size_t)(w.symOff + s) * PPM + m];
            cw |= (L[s] > 0.0f ? 1u : 0u) << s;
        }
    }
    cw ^= w.white;
#pragma unroll
    for (int s = 0; s < 8; s++) L[s] = ((w.white >> s) & 1u) ? -L[s] : L[s];
    return cw;
}

//! the nibble x that maximises M(x) = sum over k = 0..3+rdd ascending of (bit k of the rate's codeword of x ? +L[k] : -L[k]), in float;
//! the smallest x among equals
__device__ __forceinline__ unsigned softNibble(const float (&L)[8], const int rdd)
{
    unsigned best = 0;
    float bestM = 0.0f;
    for (unsigned x = 0; x < 16; x++)
    {
        const unsigned code = encodeNibble(x, rdd);
        float M = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < 4 + rdd) M = M + (((code >> k) & 1u) ? L[k] : -L[k]);
        if (x == 0 || M > bestM) { bestM = M; best = x; }
    }
    return best;
}

} // namespace

template <int G>
__device__ __forceinline__ void decodeSoftBody(const DecodeArgs a, const float *llrRows, const long long llrStride, const DecodeCaps caps, const int slice,
                                               const int perBlock, const bool known)
{
    // per packet: 16 bytes for the header block's five codewords (hard bits, then soft nibbles), then the nibbles
    extern __shared__ __attribute__((aligned(16))) unsigned char smemDec[];
    PacketState st;
    const GroupPacket k = packetOf<G>(a, perBlock, known, st);
    const int t = k.t, PPM = k.PPM;
    int symCap = caps.symCap, cwCap = caps.cwCap;                   // of the hard plan: they enter the row rule only
    unsigned char *sHdr = smemDec + (size_t)k.g * slice;
    unsigned char *sNib = sHdr + 16;
    const float *llr = llrRows + (size_t)k.pc * llrStride;
    RateCounts n = countsAt(k.nsyms, PPM, st.rate);

    // ---- the five header codewords: always the first block at 4/8 over symbols 0..7, never whitened ------------------------
    if (st.go && a.explicitHdr)
        for (int c = t; c < LORAHIP_N_HDR_CODEWORDS; c += G)
        {
            float L[8];
            sHdr[c] = (unsigned char)softCodeword(llr, k.rowSyms, c, PPM, LORAHIP_HDR_RDD, countsAt(LORAHIP_N_HDR_SYMBOLS, PPM, LORAHIP_HDR_RDD), 1, L);
            sHdr[8 + c] = (unsigned char)softNibble(L, LORAHIP_HDR_RDD);
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    // ---- header rate (LORAHIP_RDD_FROM_HEADER): the soft-decoded codeword 2 names it; from here on a packet of that rate -----------
    if (a.rdd < 0)                                                                           // (group-uniform; no barrier inside)
    {
        if (st.go)
        {
            const int field = (sHdr[8 + 2] >> 1) & 0x7;
            st.rate = field > 4 ? LORAHIP_HDR_RDD : field;
        }
        const DecodeCaps cr = decodeCapsAt(a.sf, a.ppm, st.rate, 1, a.dataLength, a.symStride);
        symCap = cr.symCap; cwCap = cr.cwCap;
        n = countsAt(k.nsyms, PPM, st.rate);
    }

    // ---- header (the nibbles soft, the error flag from the hard bits), needs, and the nibbles of the codewords the bytes need: a
    // codeword per lane and round, its LLRs gathered from the row, the maximum-likelihood nibble ------------------------------------
    bool bad = false;
    unsigned char hn[LORAHIP_N_HDR_CODEWORDS] = { 0, 0, 0, 0, 0 };
    if (st.go && a.explicitHdr)
        for (int c = 0; c < LORAHIP_N_HDR_CODEWORDS; c++) { (void)decodeHamming84(sHdr[c], st.error, bad); hn[c] = sHdr[8 + c]; }
    decodeHeader(st, a, hn, n.numCodewords);
    decodeNeeds(st, a, k, n.bs, symCap, cwCap);
    frameNibbles<G>(st, a, t, sNib);
    if (st.go)
        for (int c = (a.explicitHdr ? LORAHIP_N_HDR_CODEWORDS : 0) + t; c < st.cEnd; c += G)
        {
            float L[8];
            const unsigned char cw = (unsigned char)softCodeword(llr, k.rowSyms, c, PPM, st.rate, n, a.explicitHdr, L);
            if (c < PPM) (void)decodeHamming84(cw, st.error, bad);
            else (void)decodeNibble(cw, st.rdd, st.error, bad);
            sNib[c + (a.explicitHdr ? 1 : 0)] = (unsigned char)softNibble(L, c < PPM ? LORAHIP_HDR_RDD : st.rdd);
        }
    st.error = groupAny<G>(st.error);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();

    checkPayload<G>(st, a, t, sNib);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();
    writePacket<G>(st, a, k, sNib, known);
}

template <int G>
__global__ void __launch_bounds__(256) decodeSoftCfgs(const DecodeArgs rows, const float *llr, const long long llrStride, const DecodeCfgTable tab,
                                                      const int slice, const int perBlock)
{
    const int g = threadIdx.x / G;
    const unsigned p = blockIdx.x * perBlock + g;
    // index null: the uniform launch under the table's only entry
    const int i = (g < perBlock && p < rows.nPackets && tab.index != nullptr) ? cfgIndexOf(tab, p) : 0;
    const DecodeCfg &e = tab.e[i < 0 ? 0 : i];
    const DecodeCaps caps = { e.symCap, e.cwCap };
    decodeSoftBody<G>(withCfg(rows, e), llr, llrStride, caps, slice, perBlock, i >= 0);
}

hipError_t launchDecodeSoft(const DecodeArgs &rows, const float *llr, const long long llrStride, const DecodeCfg *cfgs, const size_t nCfgs,
                            const int *index, const int *table, const int nTable, hipStream_t stream)
{
    if (rows.nPackets == 0) return hipSuccess;
    if (nCfgs == 0 || nCfgs > size_t(LORAHIP_DEC_MAX_CFGS)) return hipErrorInvalidValue;
    DecodeCfgTable tab = decodeTableOf(cfgs, nCfgs, index, table, nTable);
    // lanes and caps of the hard plan (the caps enter the row rule); the slice is the nibbles' alone
    const DecodeTiling t = decodePlan(tab.e, nCfgs, rows.symStride);
    const int slice = (16 + t.cwCap + 15) & ~15;
    const int perBlock = packetsPerBlock(t.lanes, slice);
    if (perBlock < 1) return hipErrorInvalidValue;                  // (the entry points bound data_length: cannot happen)
    return withLanes(t.lanes, [&](auto g) { return launchGroup<decodeSoftCfgs<decltype(g)::value>>(rows.nPackets, perBlock, slice, stream, rows, llr, llrStride, tab, slice, perBlock); });
}

// rows: the de-whitening takes its length as a uint16_t in the reference (LoRaCodes.hpp: Sx1272ComputeWhiteningLfsr), i.e. messages of
// up to 65535 codewords are what the reference itself decodes as written; 16384 symbols stay below that at every setting
int decodeMaxSymbols() { return 16384; }
int decodeMaxDataLength() { return LORAHIP_DEC_MAX_DATA_LENGTH; }

} // namespace lorahip
