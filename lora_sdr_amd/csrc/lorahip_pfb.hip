// Polyphase filter-bank channeliser: the front end for a UNIFORM channel plan -- K channels on the grid fs/M, M a power of two
// 8..1024 or 5 * 2^a, a = 0..6 (include/lorahip.h has the definition; DESIGN.md section 8c the shape and the measurements). Row i is,
// by definition, what the direct-form channeliser (lorahip_chan.hip) defines for freq = bins[i] / M with the exact phase (for a
// power of two that frequency is exact in the 64-bit phase counter; for 5 * 2^a it is not, and the formula below is the definition):
// the mixer phase of sample n is exp(-2 pi i b (n mod M) / M) and the L products of an output fold, by absolute sample time modulo M,
// into M sums that one forward M-point DFT turns into every bin at once:
//
//     v_s[m] = sum_{j<L, (n_m - j) mod M == s} h[j] x[n_m - j]            n_m = (m + 1) D - 1
//     y_b[m] = sum_{s<M} v_s[m] exp(-2 pi i b s / M)
//
// L real-by-complex multiply-adds and one FFT per output time, whatever K is (the direct form: K L complex multiply-adds).
//
// One workgroup = one tile of T consecutive output times (T = the largest power of two with T M <= 4096, 16 at least and 256 at most),
// three stages in one launch:
//   * polyphase: lane = s (consecutive lanes read consecutive samples and consecutive taps), the fold runs over j = r + M q in
//     ascending q with r = (n_m - s) mod M, one fused multiply-add per component and tap, ceil((L - r) / M) rounds: the taps the
//     filter has and no others (the table is padded with zeros to Q = ceil(L / M) whole rounds, but no product is formed with the
//     padding: a NaN or Inf reaches the L outputs of the definition). The samples come from an LDS copy of the tile's input span
//     where that fits beside the sums, and straight from global memory / L2 where it does not (large D). Tiles sit on absolute
//     multiples of T and every sum has one fixed order, so a result does not depend on where a call or a tile starts;
//   * FFT: T transforms of M points in place in the LDS, decimation in frequency, 2 to 4 radix-2 stages per pass in registers
//     (passes of 16 / 8 points a lane), twiddles from a host table computed in double. The result is left in bit-reversed order:
//     the host reverses the selected bins instead. M = 5 * 2^a: one radix-5 stage first, then five such transforms of M / 5 points
//     (lorahip_pfbfft5.h; bin 5 k + r is left at r M / 5 + bitrev(k));
//   * store: only the selected bins leave the LDS; lane = output time, so a row's run of a tile is T * 8 >= 128 bytes. Rows of the
//     sums are M + 1 samples apart: the T lanes that read one bin of T rows hit T different banks (M + 1 odd; M = 5: 6 samples =
//     12 banks apart, lanes 16 apart share a bank: two-way).
// The chunk of a call is cf32, sc16 or sc8 (template argument S; lorahip_frontend.h has the definition): a staged span is converted
// when it is copied, so the LDS holds cf32 for every format and the staging rule does not depend on it; an unstaged fold converts at
// every tap read. The cf32 instances are the code they were before the formats.
// The phase is the stream position modulo M -- integer arithmetic, no drift. M is a template constant: for the power-of-two banks
// the divisions and remainders by it are shifts and masks, for the others multiplications.
#include "lorahip_bank.h"
#include <new>

struct lorahip_pfb
{
    lorahip_ctx *ctx;
    int M, D, L, Lp, Q, K, T, logT, staged, span, HC;
    size_t ldsBytes;
    lorahip::DevBuf<float> dTaps;               // [Lp] h[j], zeros from L on
    lorahip::DevBuf<float2> dTw;                // [bankTwiddles(M)] exp(-2 pi i k / M), k < M / 2; 5 * 2^a: the same for M / 5, then exp(-2 pi i n / M), n < M
    lorahip::DevBuf<int> dSel;                  // [K] where row i's bin stands after the transform: bankPlace(M, bins[i] mod M)
    lorahip::StreamCarry carry;                 // the HC samples before n0
};

namespace lorahip {

constexpr size_t PFB_STAGE_LDS = 80u << 10;     // sums + twiddles + input span up to this: two workgroups a compute unit

template <class S> struct PfbArgs
{
    const S *chunk;                 // this call's samples in their format (lorahip_frontend.h)
    long long nChunk;
    const float2 *hist;
    int histLen;
    long long n0;                   // absolute index of chunk[0]
    const float *taps;
    const float2 *tw;
    const int *sel;
    float2 *out;
    long long outStride;
    long long mLo;                  // absolute index of the first output of this call
    long long nOut;
    int D, L, Lp, K, T, logT, span;
    float scale;                    // of the integer formats
};

//! one folded sum from samples that lie in a row: xp = the newest sample of residue s, the older ones M apart below it; rounds = the
//! number of taps r, r + M, ... below L. S = float2 for the LDS copy (converted when it was staged), the chunk's format for the chunk
template <int M, class S>
__device__ __forceinline__ float2 pfbFold(const S *xp, const float *hp, const int rounds, const float scale)
{
    float re = 0.0f, im = 0.0f;
#pragma unroll 4
    for (int q = 0; q < rounds; q++)
    {
        float2 x;
        if constexpr (std::is_same<S, float2>::value) x = xp[-q * M];
        else x = iqLoad(xp - q * M, scale);
        const float h = hp[q * M];
        re = __builtin_fmaf(h, x.x, re);
        im = __builtin_fmaf(h, x.y, im);
    }
    return make_float2(re, im);
}

template <int M, bool STAGED, class S>
__global__ __launch_bounds__(PFB_THREADS) void pfbChannelize(const PfbArgs<S> a)
{
    extern __shared__ float2 pfbLds[];
    constexpr bool POW2 = bankIsPow2(M);
    constexpr int LOGN = bankLog2(bankPow2Part(M)), TW = bankTwiddles(M);
    const int tid = threadIdx.x;
    const int T = a.T, D = a.D, Lp = a.Lp;
    float2 *v = pfbLds;                             // [T][M + 1]
    float2 *tw = v + T * (M + 1);                   // [TW]
    float2 *xs = tw + TW;                           // [span] (STAGED)
    const long long mTile = ((a.mLo >> a.logT) + (long long)blockIdx.x) << a.logT;
    const long long nFirst = (mTile + 1) * D - 1;   // n_m of the tile's first output
    const long long tileStart = nFirst - (Lp - 1);  // oldest sample of the tile's first output
    const long long rel = tileStart - a.n0;
    const bool inside = rel >= 0 && rel + a.span <= a.nChunk;       // the tile's whole input lies in this call's chunk

    for (int k = tid; k < TW; k += PFB_THREADS) tw[k] = a.tw[k];
    if constexpr (STAGED)
    {
        if (inside)
        {
            const S *__restrict__ src = a.chunk + rel;
#pragma unroll 8
            for (int i = tid; i < a.span; i += PFB_THREADS)
            {
                if constexpr (std::is_same<S, float2>::value) xs[i] = src[i];
                else xs[i] = iqLoad(src + i, a.scale);
            }
        }
        else
        {
#pragma unroll 4
            for (int i = tid; i < a.span; i += PFB_THREADS) xs[i] = carriedSample(a.chunk, a.nChunk, a.hist, a.histLen, a.n0, tileStart + i, a.scale);
        }
        __syncthreads();
    }

    // polyphase stage: lane = residue s
    [[maybe_unused]] const int nFirstModM = int((unsigned long long)nFirst % unsigned(M)), dModM = D % M;    // nFirst >= 0
    for (int idx = tid; idx < T * M; idx += PFB_THREADS)
    {
        int s, t, r;                                // r = (n - s) mod M, the floor remainder (n - s < 0 at the start of a stream when D < M)
        if constexpr (POW2) { s = idx & (M - 1); t = idx >> LOGN; }
        else { t = int(unsigned(idx) / unsigned(M)); s = idx - t * M; }
        const long long n = nFirst + (long long)t * D;
        if constexpr (POW2) r = int((n - s) & (M - 1));
        else
        {
            r = int(unsigned(nFirstModM + t * dModM) % unsigned(M)) - s;
            if (r < 0) r += M;
        }                                           // the newest sample of residue s is r samples old: taps r, r + M, ...
        const int at = t * D + Lp - 1 - r;          // ... and stands here in the tile's span
        const float *hp = a.taps + r;
        const int rounds = POW2 ? (a.L - r + M - 1) >> LOGN : int(unsigned(a.L - r + M - 1) / unsigned(M));   // taps r, r + M, ... < L: the padding of the table is never multiplied (0 where r >= L)
        float2 acc;
        if constexpr (STAGED) acc = pfbFold<M>(xs + at, hp, rounds, 1.0f);
        else if (inside) acc = pfbFold<M>(a.chunk + rel + at, hp, rounds, a.scale);
        else
        {
            float re = 0.0f, im = 0.0f;
            for (int q = 0; q < rounds; q++)
            {
                const float2 x = carriedSample(a.chunk, a.nChunk, a.hist, a.histLen, a.n0, n - r - (long long)q * M, a.scale);
                const float h = hp[q * M];
                re = __builtin_fmaf(h, x.x, re);
                im = __builtin_fmaf(h, x.y, im);
            }
            acc = make_float2(re, im);
        }
        v[t * (M + 1) + s] = acc;
    }
    __syncthreads();

    if constexpr (POW2) pfbFft<LOGN, 0>(v, tw, T, tid);
    else pfbFft5<LOGN>(v, tw, tw + (M / 10), T, tid);

    // store stage: lane = output time
    const long long mTileLoc = mTile - a.mLo;       // the tile's first output in this call (< 0: the call starts inside the tile)
    const int nItems = a.K << a.logT;
    for (int item = tid; item < nItems; item += PFB_THREADS)
    {
        const int t = item & (T - 1), i = item >> a.logT;
        const long long ml = mTileLoc + t;
        if (ml >= 0 && ml < a.nOut) a.out[(long long)i * a.outStride + ml] = v[t * (M + 1) + a.sel[i]];
    }
}

template <int M, class S>
static hipError_t pfbLaunch(const lorahip_pfb *p, const PfbArgs<S> &a, const unsigned grid)
{
    static unsigned long long ldsMask[2];
    if (p->staged)
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(&pfbChannelize<M, true, S>), 160 * 1024, ldsMask[1]);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((pfbChannelize<M, true, S>), dim3(grid), dim3(PFB_THREADS), p->ldsBytes, p->ctx->stream, a);
    }
    else
    {
        const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(&pfbChannelize<M, false, S>), 160 * 1024, ldsMask[0]);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((pfbChannelize<M, false, S>), dim3(grid), dim3(PFB_THREADS), p->ldsBytes, p->ctx->stream, a);
    }
    return hipGetLastError();
}

template <class S>
static int pfbRun(lorahip_pfb *p, const S *wide, const float scale, const size_t nIn, float2 *out, const size_t outStride, size_t *nOutP)
{
    lorahip_ctx *ctx = p->ctx;
    const unsigned long long mLo = p->carry.n0 / (unsigned long long)p->D;
    const size_t nOut = decimatedCount(p->carry.n0, nIn, p->D);
    if (nOutP) *nOutP = nOut;
    if (nIn == 0) return LORAHIP_OK;
    if (nOut && (out == nullptr || outStride < nOut)) { setLastError("polyphase channeliser: no output rows, or out_stride below the outputs of this call"); return LORAHIP_E_INVALID; }
    if (nOut > (size_t(1) << 30)) { setLastError("polyphase channeliser: more than 2^30 outputs per channel in one call"); return LORAHIP_E_INVALID; }
    const size_t nTiles = nOut ? size_t((mLo & (unsigned long long)(p->T - 1)) + nOut + size_t(p->T) - 1) >> p->logT : 0;
    if (nTiles > 0x7fffffffu) { setLastError("polyphase channeliser: the outputs of one call exceed the launch grid"); return LORAHIP_E_INVALID; }
    const DeviceGuard guard(ctx->device);
    PfbArgs<S> a;
    a.chunk = wide; a.scale = scale; a.nChunk = (long long)nIn;
    a.hist = p->carry.current(); a.histLen = p->HC;
    a.n0 = (long long)p->carry.n0;
    a.taps = p->dTaps.get(); a.tw = p->dTw.get(); a.sel = p->dSel.get();
    a.out = out; a.outStride = (long long)outStride;
    a.mLo = (long long)mLo; a.nOut = (long long)nOut;
    a.D = p->D; a.L = p->L; a.Lp = p->Lp; a.K = p->K; a.T = p->T; a.logT = p->logT; a.span = p->span;
    if (nOut)
    {
        const hipError_t e = bankDispatch(p->M, BankCounts(), [&](const auto m) { return pfbLaunch<decltype(m)::value>(p, a, unsigned(nTiles)); });
        LORAHIP_TRY(e);
    }
    hipLaunchKernelGGL(carryHistory<S>, dim3((p->HC + 255) / 256), dim3(256), 0, ctx->stream, a.chunk, a.nChunk, a.hist, a.histLen, a.n0, p->carry.next(), a.scale);
    LORAHIP_TRY(hipGetLastError());
    p->carry.advance(nIn);
    return LORAHIP_OK;
}

static int pfbCheck(const bool radix5, const size_t n_bins, const size_t decim, const size_t n_taps, const size_t n_sel)
{
    return bankCheck("polyphase channeliser", "decim", radix5, n_bins, decim, n_taps, n_sel);
}

//! lorahip_pfb_create (power-of-two bin counts) and lorahip_pfb_create_radix5 (5 * 2^a): the same object
static int pfbCreate(const bool radix5, lorahip_pfb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel,
                     const size_t decim, const float *taps, const size_t n_taps)
{
    if (out == nullptr) return LORAHIP_E_INVALID;
    *out = nullptr;
    if (ctx == nullptr || taps == nullptr) { setLastError("polyphase channeliser: no context or no taps"); return LORAHIP_E_INVALID; }
    if (pfbCheck(radix5, n_bins, decim, n_taps, n_sel) != LORAHIP_OK) return LORAHIP_E_INVALID;
    if (bins == nullptr && n_sel != n_bins) { setLastError("polyphase channeliser: without a bin list n_sel must be n_bins"); return LORAHIP_E_INVALID; }

    lorahip_pfb *p = new (std::nothrow) lorahip_pfb();
    if (p == nullptr) return LORAHIP_E_NOMEM;
    const int M = int(n_bins);
    p->ctx = ctx; p->M = M; p->D = int(decim); p->L = int(n_taps); p->K = int(n_sel);
    p->Q = (p->L + M - 1) / M; p->Lp = p->Q * M;
    p->HC = p->Lp - 1;
    p->logT = bankLogT(M, 4);                   // T = 16 at least
    p->T = 1 << p->logT;
    const size_t fixedLds = (size_t(p->T) * size_t(M + 1) + size_t(bankTwiddles(M))) * sizeof(float2);
    const size_t span = size_t(p->T - 1) * size_t(p->D) + size_t(p->Lp);
    p->span = int(span);                        // < 2^21
    p->staged = fixedLds + span * sizeof(float2) <= PFB_STAGE_LDS;
    p->ldsBytes = fixedLds + (p->staged ? span * sizeof(float2) : 0);

    std::vector<float> h;
    std::vector<float2> tw;
    std::vector<int> sel;
    try
    {
        h.assign(size_t(p->Lp), 0.0f);
        tw = bankTwiddleTable(M, false);
        sel.resize(n_sel);
    }
    catch (const std::bad_alloc &) { delete p; return LORAHIP_E_NOMEM; }
    for (size_t j = 0; j < n_taps; j++) h[j] = taps[j];
    for (size_t i = 0; i < n_sel; i++) sel[i] = bankPlace(M, bins ? bankBin(M, bins[i]) : int(i));
    return uploadTables(out, p, "polyphase channeliser", size_t(p->HC), p->dTaps, h.data(), h.size(), p->dTw, tw.data(), tw.size(),
                        p->dSel, sel.data(), sel.size());
}

} // namespace lorahip

using namespace lorahip;

extern "C" {

int lorahip_pfb_check(const size_t n_bins, const size_t decim, const size_t n_taps, const size_t n_sel)
{
    return pfbCheck(false, n_bins, decim, n_taps, n_sel);
}

int lorahip_pfb_check_radix5(const size_t n_bins, const size_t decim, const size_t n_taps, const size_t n_sel)
{
    return pfbCheck(true, n_bins, decim, n_taps, n_sel);
}

int lorahip_pfb_create(lorahip_pfb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel,
                       const size_t decim, const float *taps, const size_t n_taps)
{
    return pfbCreate(false, out, ctx, n_bins, bins, n_sel, decim, taps, n_taps);
}

int lorahip_pfb_create_radix5(lorahip_pfb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel,
                              const size_t decim, const float *taps, const size_t n_taps)
{
    return pfbCreate(true, out, ctx, n_bins, bins, n_sel, decim, taps, n_taps);
}

void lorahip_pfb_destroy(lorahip_pfb *p)
{
    if (p == nullptr) return;
    const DeviceGuard guard(p->ctx->device);
    delete p;
}

int lorahip_pfb_reset(lorahip_pfb *p)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(p->ctx->device);
    LORAHIP_TRY(p->carry.reset(p->ctx->stream));
    return LORAHIP_OK;
}

size_t lorahip_pfb_out_count(const lorahip_pfb *p, const size_t n_in)
{
    return p == nullptr ? 0 : decimatedCount(p->carry.n0, n_in, p->D);
}

int lorahip_pfb_run(lorahip_pfb *p, const float *wide_dev, const size_t n_in, float *out_dev, const size_t out_stride, size_t *n_out)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    if (n_in && wide_dev == nullptr) { setLastError("polyphase channeliser: no input"); return LORAHIP_E_INVALID; }
    return pfbRun(p, reinterpret_cast<const float2 *>(wide_dev), 1.0f, n_in, reinterpret_cast<float2 *>(out_dev), out_stride, n_out);
}

int lorahip_pfb_run_iq(lorahip_pfb *p, const void *wide_dev, const int format, const float scale, const size_t n_in, float *out_dev, const size_t out_stride,
                       size_t *n_out)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    if (n_in && wide_dev == nullptr) { setLastError("polyphase channeliser: no input"); return LORAHIP_E_INVALID; }
    if (iqCheck("polyphase channeliser", wide_dev, format, scale) != LORAHIP_OK) return LORAHIP_E_INVALID;
    return iqDispatch(wide_dev, format, [&](const auto *wide) { return pfbRun(p, wide, scale, n_in, reinterpret_cast<float2 *>(out_dev), out_stride, n_out); });
}

} // extern "C"
