// Polyphase synthesis filter bank: the transmit front end for a UNIFORM channel plan -- K channel streams onto the grid fs/M, M a power
// of two 8..1024 or 5 * 2^a, a = 0..6 (include/lorahip.h has the definition; DESIGN.md section 8d the shape and the measurements). The
// mirror image of lorahip_pfb.hip. The output is, by definition, what the direct-form synthesiser (lorahip_synth.hip) defines for
// freq[k] = bins[k] / M with the exact phase (for a power of two that frequency is exact in the 64-bit phase counter; for 5 * 2^a it is
// not, and the formulas below are the definition): the mixer phase of output n is exp(+2 pi i b (n mod M) / M) and the K mixers
// collapse into one inverse M-point DFT per INPUT time:
//
//     X_b[m] = sum_{k : b_k mod M == b} g_k x_k[m]
//     u_s[m] = sum_{b<M} X_b[m] exp(+2 pi i b s / M)
//     y[n]   = sum_{i : p + iU < L} h[p + iU] u_{n mod M}[n/U - i]             p = n mod U
//
// one FFT per U outputs and at most ceil(L/U) real-by-complex multiply-adds per output, whatever K is (the direct form: K ceil(L/U)
// complex multiply-adds).
//
// A call is cut into segments of input times whose transforms fit a workspace of PSB_WS_POINTS samples (small enough to stay in the
// last-level cache between the two launches of a segment):
//   * psbTransform: one workgroup = T consecutive input times (T = the largest power of two with T M <= 4096, 8 at least and 256 at
//     most). Gather: lane = time (a row's
//     run of a tile is contiguous), the rows of a bin are summed in ascending k with one fused multiply-add per component, the gain
//     applied there; a bin without a row is 0. Then T transforms of M points in place in the LDS -- the pass structure of the receive
//     bank (lorahip_pfbfft.h) with conjugated twiddles from a host table computed in double. The result stands in bit-reversed order
//     and is put straight while it is stored: the workspace row of a time holds u_0 .. u_{M-1};
//   * psbFold: lane = output sample, so consecutive lanes read consecutive taps and consecutive residues of a workspace row and their
//     stores are contiguous. The fold runs over i in ascending order, over the taps below L and no others: no product with padding
//     is formed, so a NaN or Inf in x_k[m] reaches the outputs mU .. mU + L - 1 of the definition and no other. A phase without a tap
//     (p >= L) is an exact zero;
//   * psbHistory: the transforms of the last ceil(L/U) - 1 input times, which the next outputs reach back to, are carried (not
//     recomputed) in one of two small buffers. Before the start of the stream they are zeros.
// Every u_s[m] depends on the inputs of time m alone and every sum has one fixed order, so an output does not depend on how the
// stream was cut into calls or segments. The phase is the stream position modulo M -- integer arithmetic, no drift.
// The three kernels are templates on M, like the receive bank's. M = 5 * 2^a: the transform is lorahip_pfbfft5.h with the conjugate
// tables -- one radix-5 stage, then five radix-2 transforms of N = M / 5 points, residue 5 k + r left at r N + bitrev(k) --, and the
// divisions and remainders by M are by a compile-time constant where the powers of two have shifts and masks.
// psbFold is also a template on the output sample type S (lorahip_frontend.h: float2, short2 = sc16, char2 = sc8): the fold is the same
// sequence of FMAs, the lane's one output becomes an 8-, 4- or 2-byte store, quantised by the definition in include/lorahip.h, and the
// integer instances add their clipped components to the object's counter, one atomic per wavefront at most. The workspace and the
// history stay cf32, and a segment's output pointer advances in samples of S.
#include "lorahip_bank.h"
#include <new>

struct lorahip_psb
{
    lorahip_ctx *ctx;
    int M, U, L, I, HC, K, T, logT;
    size_t seg;                                 // input times per segment at most
    size_t ldsBytes;
    lorahip::DevBuf<float> dTaps;               // [L] h[j]
    lorahip::DevBuf<float2> dTw;                // [bankTwiddles(M)] exp(+2 pi i k / M), k < M / 2; 5 * 2^a: the same for M / 5, then exp(+2 pi i n / M), n < M
    lorahip::DevBuf<int> dBinStart;             // [M + 1] the rows of bin b are dBinRow[dBinStart[b] .. dBinStart[b + 1]), ascending
    lorahip::DevBuf<int> dBinRow;               // [K]
    lorahip::DevBuf<float> dBinGain;            // [K] the gain of that row
    lorahip::DevBuf<float2> dWs;                // [segment][M] u_s[m] of the segment in flight
    lorahip::StreamCarry carry;                 // [HC][M] u_s[m] of the HC input times before n0
    lorahip::ClipCount clipped;                 // components the integer runs clipped since create / reset
};

namespace lorahip {

constexpr int PSB_FOLD_THREADS = 256;
constexpr size_t PSB_WS_POINTS = size_t(1) << 22;       // 32 MiB of transforms per segment
constexpr size_t PSB_SEG_OUTPUTS = size_t(1) << 30;     // the outputs of a segment are indexed with 32 bits

struct PsbArgs
{
    const float2 *in;               // the segment's first sample of row 0
    long long inStride;
    int cnt;                        // input times in this segment
    long long m0;                   // absolute index of the segment's first input time
    const int *binStart, *binRow;
    const float *binGain;
    const float *taps;
    const float2 *tw;
    float2 *ws;
    const float2 *hist;
    void *out;                      // the segment's first output, samples of psbFold's S
    int U, L, HC, T, logT;
    unsigned long long *clipped;    // the integer instances of psbFold count here; float2 ignores both
    float scale;
};

//! u_s of input time m0 + c (c >= -HC): from this segment's workspace or from the history kept from earlier segments and calls
template <int M>
__device__ __forceinline__ float2 psbU(const PsbArgs &a, const int c, const int s)
{
    const float2 *src = c >= 0 ? a.ws + (long long)c * M + s : a.hist + (long long)(c + a.HC) * M + s;
    return *src;
}

template <int M>
__global__ __launch_bounds__(PFB_THREADS) void psbTransform(const PsbArgs a)
{
    extern __shared__ float2 psbLds[];
    constexpr bool POW2 = bankIsPow2(M);
    constexpr int LOGN = bankLog2(bankPow2Part(M)), TW = bankTwiddles(M);
    const int tid = threadIdx.x;
    const int T = a.T;
    float2 *v = psbLds;                             // [T][M + 1]
    float2 *tw = v + T * (M + 1);                   // [TW]
    const int c0 = int(blockIdx.x) << a.logT;       // the tile's first input time in the segment

    for (int k = tid; k < TW; k += PFB_THREADS) tw[k] = a.tw[k];

    // gather: lane = input time
    for (int item = tid; item < T * M; item += PFB_THREADS)
    {
        const int t = item & (T - 1), b = item >> a.logT;
        float re = 0.0f, im = 0.0f;
        if (c0 + t < a.cnt)
        {
            const float2 *col = a.in + (c0 + t);
            const int e1 = a.binStart[b + 1];
            for (int e = a.binStart[b]; e < e1; e++)
            {
                const float2 x = col[(long long)a.binRow[e] * a.inStride];
                const float g = a.binGain[e];
                re = __builtin_fmaf(g, x.x, re);
                im = __builtin_fmaf(g, x.y, im);
            }
        }
        v[t * (M + 1) + b] = make_float2(re, im);
    }
    __syncthreads();

    if constexpr (POW2) pfbFft<LOGN, 0>(v, tw, T, tid);
    else pfbFft5<LOGN>(v, tw, tw + M / 10, T, tid);

    // store: lane = residue s, which is put straight from its place in the row
    for (int item = tid; item < T * M; item += PFB_THREADS)
    {
        const int t = int(unsigned(item) / unsigned(M)), s = item - t * M;
        const int at = bankPlaceDev<M>(s);
        if (c0 + t < a.cnt) a.ws[(long long)(c0 + t) * M + s] = v[t * (M + 1) + at];
    }
}

template <int M, class S>
__global__ __launch_bounds__(PSB_FOLD_THREADS) void psbFold(const PsbArgs a)
{
    const unsigned U = unsigned(a.U);
    const unsigned long long o64 = (unsigned long long)blockIdx.x * PSB_FOLD_THREADS + threadIdx.x;
    if (o64 >= (unsigned long long)a.cnt * U) return;
    const unsigned o = unsigned(o64);               // < 2^31
    const unsigned c = o / U, p = o - c * U;        // input time in the segment, output phase
    const unsigned m0 = unsigned((unsigned long long)a.m0 % unsigned(M));      // the same in every lane
    const int s = int((((m0 + c) % unsigned(M)) * U + p) % unsigned(M));       // (m U + p) mod M; 319 * 4096 + 4095 fits
    const int rounds = int(p) < a.L ? (a.L - int(p) + int(U) - 1) / int(U) : 0;    // taps p, p + U, ... < L
    const float *hp = a.taps + p;
    float re = 0.0f, im = 0.0f;
#pragma unroll 4
    for (int i = 0; i < rounds; i++)
    {
        const float2 u = psbU<M>(a, int(c) - i, s);
        const float h = hp[(long long)i * U];
        re = __builtin_fmaf(h, u.x, re);
        im = __builtin_fmaf(h, u.y, im);
    }
    if constexpr (std::is_same<S, float2>::value) static_cast<float2 *>(a.out)[o] = make_float2(re, im);
    else
    {
        unsigned clipped = 0;                       // <= 2 a lane; the lanes past the end have left and count nothing
        iqStore(static_cast<S *>(a.out) + o, make_float2(re, im), a.scale, clipped);
        iqCountClipped<2>(a.clipped, clipped);
    }
}

//! the transforms of the HC input times that precede the next segment
template <int M>
__global__ void psbHistory(const PsbArgs a, float2 *newHist)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)a.HC * M) return;
    int h, s;                                       // HC M < 2^26; the powers of two shift all 64 bits, as they always have
    if constexpr (bankIsPow2(M)) { h = int(idx >> bankLog2(M)); s = int(idx & (M - 1)); }
    else { h = int(unsigned(idx) / unsigned(M)); s = int(unsigned(idx)) - h * M; }
    newHist[idx] = psbU<M>(a, a.cnt - a.HC + h, s);         // >= -HC
}

template <int M, class S>
static hipError_t psbLaunch(const lorahip_psb *p, const PsbArgs &a, float2 *newHist)
{
    static unsigned long long ldsMask;
    hipStream_t st = p->ctx->stream;
    hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(&psbTransform<M>), 160 * 1024, ldsMask);
    if (e != hipSuccess) return e;
    const unsigned tiles = unsigned((a.cnt + a.T - 1) >> a.logT);
    hipLaunchKernelGGL((psbTransform<M>), dim3(tiles), dim3(PFB_THREADS), p->ldsBytes, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const unsigned long long nOut = (unsigned long long)a.cnt * (unsigned long long)a.U;        // <= 2^30
    hipLaunchKernelGGL((psbFold<M, S>), dim3(unsigned((nOut + PSB_FOLD_THREADS - 1) / PSB_FOLD_THREADS)), dim3(PSB_FOLD_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.HC)
    {
        const unsigned long long n = (unsigned long long)a.HC * M;                              // < 2^26
        hipLaunchKernelGGL((psbHistory<M>), dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, a, newHist);
        e = hipGetLastError();
    }
    return e;
}

//! out in the format S; scale is what the integer formats multiply by
template <class S>
static int psbRun(lorahip_psb *p, const float2 *in, const size_t inStride, const size_t nIn, S *out, const float scale, size_t *nOutP)
{
    lorahip_ctx *ctx = p->ctx;
    if (nOutP) *nOutP = 0;
    if (nIn == 0) return LORAHIP_OK;
    if (in == nullptr || out == nullptr) { setLastError("polyphase synthesiser: a device pointer is NULL"); return LORAHIP_E_INVALID; }
    if (inStride < nIn) { setLastError("polyphase synthesiser: in_stride is shorter than n_in"); return LORAHIP_E_INVALID; }
    const size_t U = size_t(p->U);
    if (nIn > (size_t(1) << 30) / U) { setLastError("polyphase synthesiser: more than 2^30 outputs in one call"); return LORAHIP_E_INVALID; }
    const size_t seg = nIn < p->seg ? nIn : p->seg;
    // (the launch grids: seg / T tiles and seg * U / 256 <= 2^22 fold blocks, both far below 2^31 - 1)
    const DeviceGuard guard(ctx->device);
    if (p->dWs.grow(seg * size_t(p->M) * sizeof(float2)) != hipSuccess)
    {
        (void)hipGetLastError();
        setLastError("polyphase synthesiser: no device memory for the workspace");
        return LORAHIP_E_NOMEM;
    }
    PsbArgs a;
    a.inStride = (long long)inStride;
    a.binStart = p->dBinStart.get(); a.binRow = p->dBinRow.get(); a.binGain = p->dBinGain.get();
    a.taps = p->dTaps.get(); a.tw = p->dTw.get(); a.ws = p->dWs.get();
    a.U = p->U; a.L = p->L; a.HC = p->HC; a.T = p->T; a.logT = p->logT;
    if constexpr (!std::is_same<S, float2>::value) LORAHIP_TRY(p->clipped.ensure(ctx->stream));
    a.clipped = p->clipped.dev.get(); a.scale = scale;
    for (size_t done = 0; done < nIn; )
    {
        const size_t cnt = nIn - done < seg ? nIn - done : seg;
        a.in = in + done; a.cnt = int(cnt); a.m0 = (long long)p->carry.n0;
        a.hist = p->carry.current();
        a.out = out + done * U;
        float2 *newHist = p->carry.next();
        const hipError_t e = bankDispatch(p->M, BankCounts(), [&](const auto m) { return psbLaunch<decltype(m)::value, S>(p, a, newHist); });
        LORAHIP_TRY(e);
        p->carry.advance(cnt);
        done += cnt;
    }
    if (nOutP) *nOutP = nIn * U;
    return LORAHIP_OK;
}

static int psbCheck(const bool radix5, const size_t n_bins, const size_t interp, const size_t n_taps, const size_t n_sel)
{
    return bankCheck("polyphase synthesiser", "interp", radix5, n_bins, interp, n_taps, n_sel);
}

//! lorahip_psb_create (power-of-two bin counts) and lorahip_psb_create_radix5 (5 * 2^a): the same object
static int psbCreate(const bool radix5, lorahip_psb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel,
                     const float *gain, const size_t interp, const float *taps, const size_t n_taps)
{
    if (out == nullptr) return LORAHIP_E_INVALID;
    *out = nullptr;
    if (ctx == nullptr || taps == nullptr) { setLastError("polyphase synthesiser: no context or no taps"); return LORAHIP_E_INVALID; }
    if (psbCheck(radix5, n_bins, interp, n_taps, n_sel) != LORAHIP_OK) return LORAHIP_E_INVALID;
    if (bins == nullptr && n_sel != n_bins) { setLastError("polyphase synthesiser: without a bin list n_sel must be n_bins"); return LORAHIP_E_INVALID; }
    if (gain)
        for (size_t k = 0; k < n_sel; k++)
            if (!std::isfinite(gain[k])) { setLastError("polyphase synthesiser: a gain is not finite"); return LORAHIP_E_INVALID; }

    lorahip_psb *p = new (std::nothrow) lorahip_psb();
    if (p == nullptr) return LORAHIP_E_NOMEM;
    const int M = int(n_bins);
    p->ctx = ctx; p->M = M; p->U = int(interp); p->L = int(n_taps); p->K = int(n_sel);
    p->I = (p->L + p->U - 1) / p->U;
    p->HC = p->I - 1;
    p->logT = bankLogT(M, 3);                   // T = 8 at least
    p->T = 1 << p->logT;
    p->ldsBytes = (size_t(p->T) * size_t(M + 1) + size_t(bankTwiddles(M))) * sizeof(float2);
    const size_t byWs = PSB_WS_POINTS / size_t(M), byOut = PSB_SEG_OUTPUTS / interp;
    p->seg = byWs < byOut ? byWs : byOut;

    std::vector<float2> tw;
    std::vector<int> start, row;
    std::vector<float> g;
    try
    {
        tw = bankTwiddleTable(M, true);
        start.assign(size_t(M) + 1, 0);
        row.resize(n_sel);
        g.resize(n_sel);
    }
    catch (const std::bad_alloc &) { delete p; return LORAHIP_E_NOMEM; }
    // the rows of every bin, in ascending k (a counting sort is stable)
    const auto binOf = [&](const size_t k) { return bins ? size_t(bankBin(M, bins[k])) : k; };
    for (size_t k = 0; k < n_sel; k++) start[binOf(k) + 1]++;
    for (int b = 0; b < M; b++) start[size_t(b) + 1] += start[size_t(b)];
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (size_t k = 0; k < n_sel; k++)
        {
            const int e = at[binOf(k)]++;
            row[size_t(e)] = int(k);
            g[size_t(e)] = gain ? gain[k] : 1.0f;
        }
    }
    return uploadTables(out, p, "polyphase synthesiser", size_t(p->HC) * size_t(M), p->dTaps, taps, n_taps, p->dTw, tw.data(), tw.size(),
                        p->dBinStart, start.data(), start.size(), p->dBinRow, row.data(), row.size(), p->dBinGain, g.data(), g.size());
}

} // namespace lorahip

using namespace lorahip;

extern "C" {

int lorahip_psb_check(const size_t n_bins, const size_t interp, const size_t n_taps, const size_t n_sel)
{
    return psbCheck(false, n_bins, interp, n_taps, n_sel);
}

int lorahip_psb_check_radix5(const size_t n_bins, const size_t interp, const size_t n_taps, const size_t n_sel)
{
    return psbCheck(true, n_bins, interp, n_taps, n_sel);
}

int lorahip_psb_create(lorahip_psb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel, const float *gain,
                       const size_t interp, const float *taps, const size_t n_taps)
{
    return psbCreate(false, out, ctx, n_bins, bins, n_sel, gain, interp, taps, n_taps);
}

int lorahip_psb_create_radix5(lorahip_psb **out, lorahip_ctx *ctx, const size_t n_bins, const int32_t *bins, const size_t n_sel,
                              const float *gain, const size_t interp, const float *taps, const size_t n_taps)
{
    return psbCreate(true, out, ctx, n_bins, bins, n_sel, gain, interp, taps, n_taps);
}

void lorahip_psb_destroy(lorahip_psb *p)
{
    if (p == nullptr) return;
    const DeviceGuard guard(p->ctx->device);
    delete p;
}

int lorahip_psb_reset(lorahip_psb *p)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(p->ctx->device);
    LORAHIP_TRY(p->carry.reset(p->ctx->stream));
    LORAHIP_TRY(p->clipped.reset(p->ctx->stream));
    return LORAHIP_OK;
}

size_t lorahip_psb_out_count(const lorahip_psb *p, const size_t n_in)
{
    return p == nullptr ? 0 : n_in * size_t(p->U);
}

int lorahip_psb_run(lorahip_psb *p, const float *in_dev, const size_t in_stride, const size_t n_in, float *wide_dev, size_t *n_out)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    return psbRun(p, reinterpret_cast<const float2 *>(in_dev), in_stride, n_in, reinterpret_cast<float2 *>(wide_dev), 1.0f, n_out);
}

int lorahip_psb_run_iq(lorahip_psb *p, const float *in_dev, const size_t in_stride, const size_t n_in, void *wide_dev, const int format,
                       const float scale, size_t *n_out)
{
    if (p == nullptr) return LORAHIP_E_INVALID;
    if (n_out) *n_out = 0;
    if (iqCheck("polyphase synthesiser", wide_dev, format, scale) != LORAHIP_OK) return LORAHIP_E_INVALID;
    return iqDispatch(wide_dev, format, [&](auto *wide) { return psbRun(p, reinterpret_cast<const float2 *>(in_dev), in_stride, n_in, wide, scale, n_out); });
}

int lorahip_psb_clipped(lorahip_psb *p, unsigned long long *count)
{
    if (p == nullptr || count == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(p->ctx->device);
    LORAHIP_TRY(p->clipped.read(p->ctx->stream, count));
    return LORAHIP_OK;
}

} // extern "C"
