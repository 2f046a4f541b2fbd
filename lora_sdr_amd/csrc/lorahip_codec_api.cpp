// C ABI of the batched decoder and encoder (include/lorahip.h; kernels and launch plans: lorahip_codec.hip). Host-side only.
// Per direction there is ONE place for each of: what a call is refused for without a device (decodeCallOk / encodeCallOk), the settings
// of the public configuration as the kernels take them (decodeCfgOf / encodeCfgOf), and the launch (decodeRun / encodeRun). The four
// host-pointer forms share ONE trip through the context's staging pair (Staged). An entry point gathers its arguments into the call
// struct of its direction and says which form it is; decodeEntry / encodeEntry check once and run on the device or through the stage.
#include "lorahip_own.h"
#include <cstring>

using namespace lorahip;

namespace {

/*! One trip of a host-pointer entry point through the context's staging pair. The pieces are declared in the order they lie in the
 * stage, each 256-byte aligned: first those that only go in, then those that travel both ways, then those that only come out. A piece
 * without a host pointer or without bytes is absent: it takes no room and its device pointer is null. upload() grows the stage once,
 * copies the caller's data into the pinned buffer and queues ONE copy to the device over the leading pieces; download() queues ONE copy
 * back from the first piece that comes out to the end, waits for the stream and hands every such piece to the caller. */
class Staged
{
public:
    struct Piece { size_t off, bytes; };
    explicit Staged(lorahip_ctx *ctx) : ctx(ctx) {}
    Piece in(const void *host, const size_t bytes) { return add(const_cast<void *>(host), bytes, true, false); }
    Piece inout(void *host, const size_t bytes) { return add(host, bytes, true, true); }
    Piece out(void *host, const size_t bytes) { return add(host, bytes, false, true); }

    int upload()
    {
        { const int rc = growStage(ctx, cur, cur); if (rc != LORAHIP_OK) return rc; }
        char *d = ctx->dStage.get(), *h = ctx->hStage.get();
        for (int i = 0; i < n; i++)
            if (part[i].up) std::memcpy(h + part[i].off, part[i].host, part[i].bytes);
        LORAHIP_TRY(hipMemcpyAsync(d, h, upEnd, hipMemcpyHostToDevice, ctx->stream));
        return LORAHIP_OK;
    }

    //! after upload(): the piece on the device
    template <class T> T *dev(const Piece &p) const { return p.bytes ? reinterpret_cast<T *>(ctx->dStage.get() + p.off) : nullptr; }

    int download()
    {
        char *d = ctx->dStage.get(), *h = ctx->hStage.get();
        LORAHIP_TRY(hipMemcpyAsync(h + downBegin, d + downBegin, cur - downBegin, hipMemcpyDeviceToHost, ctx->stream));
        LORAHIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; i++)
            if (part[i].down) std::memcpy(part[i].host, h + part[i].off, part[i].bytes);
        return LORAHIP_OK;
    }

private:
    struct Part { void *host; size_t off, bytes; bool up, down; };
    static constexpr size_t NONE = ~size_t(0);
    lorahip_ctx *ctx;
    Part part[8];
    int n = 0;
    size_t cur = 0, upEnd = 0, downBegin = NONE;

    Piece add(void *host, const size_t bytes, const bool up, const bool down)
    {
        const Piece p = { cur, host ? bytes : 0 };
        if (p.bytes == 0) return p;
        const Part q = { host, p.off, p.bytes, up, down };
        part[n++] = q;
        if (down && downBegin == NONE) downBegin = p.off;
        cur += (p.bytes + 255) & ~size_t(255);
        // the copy to the device ends where the copy back begins, or with the last byte of the pieces that travel both ways
        if (up) upEnd = down ? p.off + p.bytes : cur;
        return p;
    }
};

//! where the arrays of a call are: on the device, or with the host -- its output rows copied out only, or in and out
enum class Where { Device, Host, HostRowsBothWays };

/***********************************************************************
 * batched decoder (lorahip_codec.hip: decodeGroup, decodeGroupCfgs)
 **********************************************************************/
//! what the decoder refuses of a configuration (host arithmetic only)
int decoderCfgOk(const lorahip_decoder_cfg *cfg)
{
    if (cfg->struct_size != sizeof(lorahip_decoder_cfg)) return LORAHIP_E_INVALID;
    if (cfg->sf < 1 || cfg->sf > LORAHIP_SF_MAX || cfg->ppm < 0 || cfg->ppm > cfg->sf || cfg->rdd < LORAHIP_RDD_FROM_HEADER || cfg->rdd > 4 || cfg->data_length < 0) return LORAHIP_E_INVALID;
    // the rate from the header: there has to be one, and the de-interleaver that reaches it
    if (cfg->rdd == LORAHIP_RDD_FROM_HEADER && !(cfg->explicit_hdr && cfg->interleaving))
    {
        setLastError("rdd = LORAHIP_RDD_FROM_HEADER needs explicit_hdr = 1 and interleaving = 1");
        return LORAHIP_E_INVALID;
    }
    // An explicit header occupies the first 5 codewords of the first (PPM-codeword) block: with fewer than 5 bits per symbol the
    // reference whitens `PPM - 5` (an unsigned short: ~65535) codewords past its buffer (LoRaDecoder.cpp:235, undefined behaviour).
    // There is nothing to be identical to; refuse the configuration instead of corrupting device memory.
    if (cfg->explicit_hdr && cfg->interleaving && (cfg->ppm ? cfg->ppm : cfg->sf) < 5)
    {
        setLastError("explicit header needs a symbol size (PPM) of at least 5 bits");
        return LORAHIP_E_INVALID;
    }
    // without a header the length of every packet is the setter's: what the decoder's tables reach bounds it (the reference has no bound;
    // a LoRa length field is one byte). Refused loudly -- never a packet silently not decoded.
    if (!cfg->explicit_hdr && cfg->interleaving && cfg->data_length > decodeMaxDataLength())
    {
        setLastError("data_length beyond what this build decodes (lorahip_decode_max_data_length())");
        return LORAHIP_E_INVALID;
    }
    return LORAHIP_OK;
}

//! the table of configurations of a launch, and of the plan query
int decodeCfgsOk(const lorahip_decoder_cfg *cfgs, const size_t n_cfgs)
{
    if (cfgs == nullptr || n_cfgs == 0 || n_cfgs > size_t(LORAHIP_DEC_MAX_CFGS)) return LORAHIP_E_INVALID;
    for (size_t i = 0; i < n_cfgs; i++) { const int rc = decoderCfgOk(cfgs + i); if (rc != LORAHIP_OK) return rc; }
    return LORAHIP_OK;
}

bool decodeRowsOk(const size_t sym_stride, const size_t out_stride)
{
    return !(sym_stride == 0 || sym_stride > size_t(decodeMaxSymbols()) || (out_stride & 1) || out_stride < 2 * (sym_stride + 8));
}

DecodeCfg decodeCfgOf(const lorahip_decoder_cfg &c)
{
    const DecodeCfg d = { c.sf, c.ppm, c.rdd, c.crcc, c.interleaving, c.error_check, c.explicit_hdr, c.hdr, c.data_length, 0, 0 };
    return d;
}

//! the arguments of a decoder entry point; the arrays are the caller's, of the host or of the device (index null: the uniform launch)
struct DecodeCall
{
    const lorahip_decoder_cfg *cfgs; size_t n_cfgs;
    const int32_t *index, *table; size_t n_table;
    const uint16_t *syms; size_t sym_stride;
    const int32_t *nsyms; size_t n_packets;
    uint8_t *out; size_t out_stride;
    int32_t *out_len, *dropped;
    lorahip_packet_info *info;
    const float *llr = nullptr; size_t llr_stride = 0;     // the soft forms: rows of LLRs in place of syms
};

//! The forms that take ONE configuration let a call without packets succeed before they look at the configuration: the device form
//! behind its struct_size, the host form without reading it. The table forms look at every entry first.
enum class Single { No, Device, Host };

/*! Every refusal of a decoder call that needs no device. *empty: the call has no packets and has succeeded. needIndex: a table form
 * that has no uniform launch (lorahip_decode_packets_cfgs and its host form); elsewhere a null index asks for the uniform launch. */
int decodeCallOk(const lorahip_ctx *ctx, const DecodeCall &c, const Single single, const bool needIndex, bool *empty)
{
    *empty = c.n_packets == 0;
    if (ctx == nullptr) return LORAHIP_E_INVALID;
    if (single != Single::No)
    {
        if (c.cfgs == nullptr || (single == Single::Device && c.cfgs->struct_size != sizeof(lorahip_decoder_cfg))) return LORAHIP_E_INVALID;
        if (c.n_packets == 0) return LORAHIP_OK;
    }
    { const int rc = decodeCfgsOk(c.cfgs, c.n_cfgs); if (rc != LORAHIP_OK) return rc; }
    if (!needIndex && c.index == nullptr && (c.n_cfgs != 1 || c.table != nullptr)) return LORAHIP_E_INVALID;
    if ((c.table != nullptr && c.n_table == 0) || c.n_table > 0x7fffffffu || !decodeRowsOk(c.sym_stride, c.out_stride)) return LORAHIP_E_INVALID;
    if (c.llr != nullptr || c.llr_stride != 0)
    {
        // the soft forms: no output of symbols, and every entry's symbols inside a row
        for (size_t i = 0; i < c.n_cfgs; i++)
        {
            if (!c.cfgs[i].interleaving) { setLastError("the soft decoder needs interleaving = 1"); return LORAHIP_E_INVALID; }
            if (c.llr_stride / size_t(c.cfgs[i].ppm ? c.cfgs[i].ppm : c.cfgs[i].sf) < c.sym_stride) return LORAHIP_E_INVALID;
        }
        // a row is at most sym_stride symbols of LORAHIP_SF_MAX values; padding up to eight times that is taken, more is a garbage stride
        // (and n_packets * llr_stride * sizeof(float), which the host form stages, stays far below 2^64: 2^31 * 2^21 * 4)
        if (c.llr_stride > c.sym_stride * size_t(LORAHIP_SF_MAX) * 8) return LORAHIP_E_INVALID;
    }
    if (c.n_packets == 0) return LORAHIP_OK;
    if ((needIndex && !c.index) || (!c.syms && !c.llr) || !c.nsyms || !c.out || !c.out_len || !c.dropped || c.n_packets > 0x7fffffffu) return LORAHIP_E_INVALID;
    return LORAHIP_OK;
}

/* The one launch behind every decoder entry point, on device pointers and checked arguments: a table of configurations (index null: the
 * uniform launch under its only entry) and, where asked for, the header report of every packet. */
int decodeRun(lorahip_ctx *ctx, const DecodeCall &c)
{
    static_assert(sizeof(lorahip_packet_info) == 32, "the kernels write eight int32 per packet");
    const DeviceGuard guard(ctx->device);
    DecodeArgs a = {};
    a.syms = c.syms; a.nsyms = c.nsyms; a.out = c.out; a.outLen = c.out_len; a.dropped = c.dropped;
    a.nPackets = unsigned(c.n_packets); a.symStride = int(c.sym_stride); a.outStride = int(c.out_stride);
    a.info = reinterpret_cast<int *>(c.info);
    DecodeCfg tab[LORAHIP_DEC_MAX_CFGS];
    for (size_t i = 0; i < c.n_cfgs; i++) tab[i] = decodeCfgOf(c.cfgs[i]);
    if (c.llr != nullptr) LORAHIP_TRY(launchDecodeSoft(a, c.llr, (long long)c.llr_stride, tab, c.n_cfgs, c.index, c.table, int(c.n_table), ctx->stream));
    else if (c.index == nullptr) LORAHIP_TRY(launchDecode(a, tab[0], ctx->variant, ctx->stream));
    else LORAHIP_TRY(launchDecodeCfgs(a, tab, c.n_cfgs, c.index, c.table, int(c.n_table), ctx->variant, ctx->stream));
    return LORAHIP_OK;
}

/* The host forms: the rows are staged through the context's pinned buffer, decoded, and the outputs copied back; synchronous. The table
 * forms upload the output rows too, so that a packet without an entry (-3) leaves its row as the caller had it; the uniform form has no
 * such packet and sends them one way. */
int decodeStaged(lorahip_ctx *ctx, const DecodeCall &c, const bool rowsBothWays)
{
    const DeviceGuard guard(ctx->device);
    Staged st(ctx);
    const Staged::Piece pSym = c.llr ? st.in(c.llr, c.n_packets * c.llr_stride * sizeof(float)) : st.in(c.syms, c.n_packets * c.sym_stride * sizeof(uint16_t)), pN = st.in(c.nsyms, c.n_packets * sizeof(int32_t));
    const Staged::Piece pIdx = st.in(c.index, c.n_packets * sizeof(int32_t)), pTab = st.in(c.table, c.n_table * sizeof(int32_t));
    const Staged::Piece pOut = rowsBothWays ? st.inout(c.out, c.n_packets * c.out_stride) : st.out(c.out, c.n_packets * c.out_stride);
    const Staged::Piece pLen = st.out(c.out_len, c.n_packets * sizeof(int32_t)), pDrop = st.out(c.dropped, c.n_packets * sizeof(int32_t));
    const Staged::Piece pInfo = st.out(c.info, c.n_packets * sizeof(lorahip_packet_info));
    { const int rc = st.upload(); if (rc != LORAHIP_OK) return rc; }
    const DecodeCall d = { c.cfgs, c.n_cfgs, st.dev<const int32_t>(pIdx), st.dev<const int32_t>(pTab), c.n_table, c.llr ? nullptr : st.dev<const uint16_t>(pSym), c.sym_stride,
                           st.dev<const int32_t>(pN), c.n_packets, st.dev<uint8_t>(pOut), c.out_stride, st.dev<int32_t>(pLen), st.dev<int32_t>(pDrop),
                           st.dev<lorahip_packet_info>(pInfo), c.llr ? st.dev<const float>(pSym) : nullptr, c.llr_stride };
    { const int rc = decodeRun(ctx, d); if (rc != LORAHIP_OK) return rc; }
    return st.download();
}

int decodeEntry(lorahip_ctx *ctx, const DecodeCall &c, const Single single, const bool needIndex, const Where where)
{
    bool empty;
    const int rc = decodeCallOk(ctx, c, single, needIndex, &empty);
    if (rc != LORAHIP_OK || empty) return rc;
    return where == Where::Device ? decodeRun(ctx, c) : decodeStaged(ctx, c, where == Where::HostRowsBothWays);
}

/***********************************************************************
 * batched encoder (lorahip_codec.hip: encodeGroup, encodeGroupCfgs)
 **********************************************************************/
//! what LoRaEncoder::work() cannot do either: PPM > SF throws (LoRaEncoder.cpp:166); an explicit header with PPM < 5 makes `PPM - cOfs`
//! wrap (:200). sf as the decoder configuration accepts it.
bool encoderCfgOk(const lorahip_encoder_cfg *cfg)
{
    if (cfg == nullptr || cfg->struct_size != sizeof(lorahip_encoder_cfg)) return false;
    if (cfg->sf < 1 || cfg->sf > LORAHIP_SF_MAX || cfg->ppm < 0 || cfg->ppm > cfg->sf || cfg->rdd < 0 || cfg->rdd > 4) return false;
    if (cfg->explicit_hdr && (cfg->ppm ? cfg->ppm : cfg->sf) < 5)
    {
        setLastError("explicit header needs a symbol size (PPM) of at least 5 bits");
        return false;
    }
    return true;
}

EncodeCfg encodeCfgOf(const lorahip_encoder_cfg &c)
{
    const EncodeCfg e = { c.sf, c.ppm, c.rdd, c.explicit_hdr ? 1 : 0, c.crc ? 1 : 0, c.whitening ? 1 : 0, 0, 0 };
    return e;
}

//! the arguments of an encoder entry point; the arrays are the caller's, of the host or of the device (index null: the uniform launch)
struct EncodeCall
{
    const lorahip_encoder_cfg *cfgs; size_t n_cfgs;
    const int32_t *index, *table; size_t n_table;
    const uint8_t *bytes; size_t byte_stride;
    const int32_t *nbytes; size_t n_packets;
    uint16_t *syms; size_t sym_stride;
    int32_t *nsyms;
};

//! every refusal of an encoder call that needs no device, in the order decodeCallOk makes its own; needIndex: the table forms
int encodeCallOk(const lorahip_ctx *ctx, const EncodeCall &c, const bool needIndex, bool *empty)
{
    *empty = c.n_packets == 0;
    if (ctx == nullptr || c.cfgs == nullptr || c.n_cfgs == 0 || c.n_cfgs > size_t(LORAHIP_ENC_MAX_CFGS)) return LORAHIP_E_INVALID;
    for (size_t i = 0; i < c.n_cfgs; i++)
        if (!encoderCfgOk(c.cfgs + i)) return LORAHIP_E_INVALID;
    if ((c.table != nullptr && c.n_table == 0) || c.n_table > 0x7fffffffu) return LORAHIP_E_INVALID;
    if (c.byte_stride > size_t(lorahip_encode_max_bytes()) || c.sym_stride == 0 || c.sym_stride > size_t(decodeMaxSymbols())) return LORAHIP_E_INVALID;
    if (c.n_packets == 0) return LORAHIP_OK;
    if ((needIndex && !c.index) || (c.byte_stride && !c.bytes) || !c.nbytes || !c.syms || !c.nsyms || c.n_packets > 0x7fffffffu) return LORAHIP_E_INVALID;
    return LORAHIP_OK;
}

//! the one launch behind every encoder entry point, on device pointers and checked arguments (index null: the uniform launch)
int encodeRun(lorahip_ctx *ctx, const EncodeCall &c)
{
    const DeviceGuard guard(ctx->device);
    EncodeArgs a = {};
    a.bytes = c.bytes; a.nbytes = c.nbytes; a.syms = c.syms; a.nsyms = c.nsyms;
    a.nPackets = unsigned(c.n_packets); a.byteStride = int(c.byte_stride); a.symStride = int(c.sym_stride);
    EncodeCfg tab[LORAHIP_ENC_MAX_CFGS];
    for (size_t i = 0; i < c.n_cfgs; i++) tab[i] = encodeCfgOf(c.cfgs[i]);
    if (c.index == nullptr) LORAHIP_TRY(launchEncode(a, tab[0], ctx->stream));
    else LORAHIP_TRY(launchEncodeCfgs(a, tab, c.n_cfgs, c.index, c.table, int(c.n_table), ctx->stream));
    return LORAHIP_OK;
}

//! the host forms: staged through the context's pinned buffer like the decoder's, the symbol rows one way; synchronous
int encodeStaged(lorahip_ctx *ctx, const EncodeCall &c)
{
    const DeviceGuard guard(ctx->device);
    Staged st(ctx);
    const Staged::Piece pByte = st.in(c.bytes, c.n_packets * c.byte_stride), pN = st.in(c.nbytes, c.n_packets * sizeof(int32_t));
    const Staged::Piece pIdx = st.in(c.index, c.n_packets * sizeof(int32_t)), pTab = st.in(c.table, c.n_table * sizeof(int32_t));
    const Staged::Piece pSym = st.out(c.syms, c.n_packets * c.sym_stride * sizeof(uint16_t)), pLen = st.out(c.nsyms, c.n_packets * sizeof(int32_t));
    { const int rc = st.upload(); if (rc != LORAHIP_OK) return rc; }
    const EncodeCall d = { c.cfgs, c.n_cfgs, st.dev<const int32_t>(pIdx), st.dev<const int32_t>(pTab), c.n_table, st.dev<const uint8_t>(pByte), c.byte_stride,
                           st.dev<const int32_t>(pN), c.n_packets, st.dev<uint16_t>(pSym), c.sym_stride, st.dev<int32_t>(pLen) };
    { const int rc = encodeRun(ctx, d); if (rc != LORAHIP_OK) return rc; }
    return st.download();
}

int encodeEntry(lorahip_ctx *ctx, const EncodeCall &c, const bool needIndex, const Where where)
{
    bool empty;
    const int rc = encodeCallOk(ctx, c, needIndex, &empty);
    if (rc != LORAHIP_OK || empty) return rc;
    return where == Where::Device ? encodeRun(ctx, c) : encodeStaged(ctx, c);
}

} // namespace

extern "C" {

int lorahip_decode_packets(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfg, const uint16_t *syms_dev, const size_t sym_stride,
                           const int32_t *nsyms_dev, const size_t n_packets, uint8_t *out_dev, const size_t out_stride,
                           int32_t *out_len_dev, int32_t *dropped_dev)
{
    const DecodeCall c = { cfg, 1, nullptr, nullptr, 0, syms_dev, sym_stride, nsyms_dev, n_packets, out_dev, out_stride, out_len_dev, dropped_dev, nullptr };
    return decodeEntry(ctx, c, Single::Device, false, Where::Device);
}

int lorahip_decode_packets_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfg, const uint16_t *syms, const size_t sym_stride,
                                const int32_t *nsyms, const size_t n_packets, uint8_t *out, const size_t out_stride, int32_t *out_len,
                                int32_t *dropped)
{
    const DecodeCall c = { cfg, 1, nullptr, nullptr, 0, syms, sym_stride, nsyms, n_packets, out, out_stride, out_len, dropped, nullptr };
    return decodeEntry(ctx, c, Single::Host, false, Where::Host);
}

int lorahip_decode_packets_cfgs(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, const size_t n_table, const uint16_t *syms_dev, const size_t sym_stride,
                                const int32_t *nsyms_dev, const size_t n_packets, uint8_t *out_dev, const size_t out_stride,
                                int32_t *out_len_dev, int32_t *dropped_dev)
{
    const DecodeCall c = { cfgs, n_cfgs, index_dev, table_dev, n_table, syms_dev, sym_stride, nsyms_dev, n_packets, out_dev, out_stride, out_len_dev, dropped_dev, nullptr };
    return decodeEntry(ctx, c, Single::No, true, Where::Device);
}

int lorahip_decode_packets_info(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, const size_t n_table, const uint16_t *syms_dev, const size_t sym_stride,
                                const int32_t *nsyms_dev, const size_t n_packets, uint8_t *out_dev, const size_t out_stride,
                                int32_t *out_len_dev, int32_t *dropped_dev, lorahip_packet_info *info_dev)
{
    const DecodeCall c = { cfgs, n_cfgs, index_dev, table_dev, n_table, syms_dev, sym_stride, nsyms_dev, n_packets, out_dev, out_stride, out_len_dev, dropped_dev, info_dev };
    return decodeEntry(ctx, c, Single::No, false, Where::Device);
}

int lorahip_decode_packets_cfgs_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, const size_t n_table, const uint16_t *syms, const size_t sym_stride,
                                     const int32_t *nsyms, const size_t n_packets, uint8_t *out, const size_t out_stride, int32_t *out_len,
                                     int32_t *dropped)
{
    const DecodeCall c = { cfgs, n_cfgs, index, table, n_table, syms, sym_stride, nsyms, n_packets, out, out_stride, out_len, dropped, nullptr };
    return decodeEntry(ctx, c, Single::No, true, Where::HostRowsBothWays);
}

int lorahip_decode_packets_info_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, const size_t n_table, const uint16_t *syms, const size_t sym_stride,
                                     const int32_t *nsyms, const size_t n_packets, uint8_t *out, const size_t out_stride, int32_t *out_len,
                                     int32_t *dropped, lorahip_packet_info *info)
{
    const DecodeCall c = { cfgs, n_cfgs, index, table, n_table, syms, sym_stride, nsyms, n_packets, out, out_stride, out_len, dropped, info };
    return decodeEntry(ctx, c, Single::No, false, Where::HostRowsBothWays);
}

int lorahip_decode_packets_soft(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, const size_t n_table, const float *llr_dev, const size_t llr_stride, const size_t sym_stride,
                                const int32_t *nsyms_dev, const size_t n_packets, uint8_t *out_dev, const size_t out_stride,
                                int32_t *out_len_dev, int32_t *dropped_dev, lorahip_packet_info *info_dev)
{
    if (llr_stride == 0) return LORAHIP_E_INVALID;
    const DecodeCall c = { cfgs, n_cfgs, index_dev, table_dev, n_table, nullptr, sym_stride, nsyms_dev, n_packets, out_dev, out_stride, out_len_dev, dropped_dev, info_dev,
                           llr_dev, llr_stride };
    return decodeEntry(ctx, c, Single::No, false, Where::Device);
}

int lorahip_decode_packets_soft_host(lorahip_ctx *ctx, const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, const size_t n_table, const float *llr, const size_t llr_stride, const size_t sym_stride,
                                     const int32_t *nsyms, const size_t n_packets, uint8_t *out, const size_t out_stride, int32_t *out_len,
                                     int32_t *dropped, lorahip_packet_info *info)
{
    if (llr_stride == 0) return LORAHIP_E_INVALID;
    const DecodeCall c = { cfgs, n_cfgs, index, table, n_table, nullptr, sym_stride, nsyms, n_packets, out, out_stride, out_len, dropped, info, llr, llr_stride };
    return decodeEntry(ctx, c, Single::No, false, Where::HostRowsBothWays);
}

int lorahip_decode_plan(const lorahip_decoder_cfg *cfgs, const size_t n_cfgs, const size_t sym_stride, lorahip_decode_tiling *plan)
{
    if (plan == nullptr || plan->struct_size != sizeof(lorahip_decode_tiling)) return LORAHIP_E_INVALID;
    *plan = lorahip_decode_tiling();
    plan->struct_size = sizeof(lorahip_decode_tiling);
    { const int rc = decodeCfgsOk(cfgs, n_cfgs); if (rc != LORAHIP_OK) return rc; }
    if (sym_stride == 0 || sym_stride > size_t(decodeMaxSymbols())) return LORAHIP_E_INVALID;
    DecodeCfg tab[LORAHIP_DEC_MAX_CFGS];
    for (size_t i = 0; i < n_cfgs; i++) tab[i] = decodeCfgOf(cfgs[i]);
    const DecodeTiling t = decodePlan(tab, n_cfgs, int(sym_stride));
    plan->lanes_per_packet = t.lanes; plan->sym_cap = t.symCap; plan->cw_cap = t.cwCap; plan->lds_slice_bytes = t.slice; plan->packets_per_workgroup = t.perBlock;
    return LORAHIP_OK;
}

int lorahip_decode_max_symbols(void) { return decodeMaxSymbols(); }
int lorahip_decode_max_data_length(void) { return decodeMaxDataLength(); }

long lorahip_encode_num_symbols(const lorahip_encoder_cfg *cfg, const size_t n_bytes)
{
    if (!encoderCfgOk(cfg) || n_bytes > size_t(decodeMaxDataLength())) return -1;
    return encodeNumSymbols(cfg->sf, cfg->ppm, cfg->rdd, cfg->explicit_hdr, cfg->crc, n_bytes);
}

int lorahip_encode_max_bytes(void) { return decodeMaxDataLength(); }

int lorahip_encode_packets(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfg, const uint8_t *bytes_dev, const size_t byte_stride,
                           const int32_t *nbytes_dev, const size_t n_packets, uint16_t *syms_dev, const size_t sym_stride,
                           int32_t *nsyms_dev)
{
    const EncodeCall c = { cfg, 1, nullptr, nullptr, 0, bytes_dev, byte_stride, nbytes_dev, n_packets, syms_dev, sym_stride, nsyms_dev };
    return encodeEntry(ctx, c, false, Where::Device);
}

int lorahip_encode_packets_host(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfg, const uint8_t *bytes, const size_t byte_stride,
                                const int32_t *nbytes, const size_t n_packets, uint16_t *syms, const size_t sym_stride, int32_t *nsyms)
{
    const EncodeCall c = { cfg, 1, nullptr, nullptr, 0, bytes, byte_stride, nbytes, n_packets, syms, sym_stride, nsyms };
    return encodeEntry(ctx, c, false, Where::Host);
}

int lorahip_encode_packets_cfgs(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index_dev,
                                const int32_t *table_dev, const size_t n_table, const uint8_t *bytes_dev, const size_t byte_stride,
                                const int32_t *nbytes_dev, const size_t n_packets, uint16_t *syms_dev, const size_t sym_stride,
                                int32_t *nsyms_dev)
{
    const EncodeCall c = { cfgs, n_cfgs, index_dev, table_dev, n_table, bytes_dev, byte_stride, nbytes_dev, n_packets, syms_dev, sym_stride, nsyms_dev };
    return encodeEntry(ctx, c, true, Where::Device);
}

int lorahip_encode_packets_cfgs_host(lorahip_ctx *ctx, const lorahip_encoder_cfg *cfgs, const size_t n_cfgs, const int32_t *index,
                                     const int32_t *table, const size_t n_table, const uint8_t *bytes, const size_t byte_stride,
                                     const int32_t *nbytes, const size_t n_packets, uint16_t *syms, const size_t sym_stride, int32_t *nsyms)
{
    const EncodeCall c = { cfgs, n_cfgs, index, table, n_table, bytes, byte_stride, nbytes, n_packets, syms, sym_stride, nsyms };
    return encodeEntry(ctx, c, true, Where::Host);
}

} // extern "C"
