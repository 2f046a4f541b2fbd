// Rational-rate resampler: K rows at one rate -> the same K rows at U / D times that rate (include/lorahip.h has the definition). The
// block between a radio's sample rate and the rates the four front ends take: zero-stuff by U, low-pass with real taps, keep every
// D-th sample. Not a reference component: the tests check against a float64 restatement of the definition.
//
// Output m stands at instant t_m = (m + 1) D - 1 of the zero-stuffed stream: its tap phase is p = t_m mod U, its newest input sample
// c = floor(t_m / U), and y[m] = sum_{i < T} h[p + i U] x[c - i] with T = ceil(L / U) (taps padded with zeros to T rounds). With
// g = gcd(U, D), U' = U / g, D' = D / g: m -> m + U' moves t_m by U D', so the outputs m = u, u + U', u + 2 U' ... share ONE phase p
// and their newest sample advances by exactly D' -- the resampler is U' decimators by D' with T-tap branches, interleaved at the
// output. The kernel is built on that:
//   * a wavefront computes 64 consecutive outputs of one such subsequence ("steps", one per lane): the T branch taps are wave-uniform
//     and come through the scalar cache, and lane s reads sample c + s D' - i;
//   * the tile's input span is staged once into LDS split by D' phase (sample j of the span at [j mod D'][j / D'], the [p][q] layout of
//     lorahip_chan.hip), so the lanes of a wavefront read consecutive addresses for every tap;
//   * a workgroup = one tile of NS steps (a power of two, 64 .. 512 where the LDS allows) x one block of PB <= 32 neighbouring
//     subsequences u x RG rows. Its wavefronts share the (subsequence, block of 64 steps) items out; a lane keeps one accumulator per
//     row, so one tap fetch serves all RG rows;
//   * the outputs go through LDS as [row][step][u]: the tile's outputs m = (tile NS + s) U' + u are then stored in runs of PB
//     consecutive samples (the whole tile contiguous where PB = U'), not strided by U'.
// Every output is one chain of T fused multiply-adds per component in ascending i from 0: nothing depends on the tile an output falls
// into or on how the stream was cut into calls. All of m, t_m, c and the row addressing are 64-bit; inside a tile 32 bits do.
// The chunk of a call is cf32, sc16 or sc8 (template argument S; lorahip_frontend.h): converted in the staging load, the LDS, the
// carried history and everything after them hold cf32.
#include "lorahip_frontend.h"
#include <cmath>
#include <new>
#include <vector>

namespace lorahip {

constexpr int RS_PB = 32;                           // subsequences (output phases) per workgroup at most
constexpr int RS_WAVES = 8;                         // wavefronts per workgroup at most
constexpr size_t RS_LDS_SMALL = 64u << 10, RS_LDS_MAX = 160u << 10;
constexpr unsigned long long RS_POS_MAX = 1ull << 52;    // (position + n_in) * 1024 stays far below 2^63
typedef __attribute__((address_space(4))) float ConstFloat;     // a load through it at a wave-uniform address is a scalar load

//! how one (U, D, L, K) is cut into tiles; filled by resampPlan
struct ResampPlan
{
    int U, D, L, T, Up, Dp, PB, nPB, nWaves, NS, sbShift, RG, TI, QP, TP, HC;    // NS steps = 2^sbShift blocks of 64 (one block of NS < 64)
    size_t ldsBytes;
};

} // namespace lorahip

struct lorahip_resampler
{
    lorahip_ctx *ctx;
    int K;
    lorahip::ResampPlan plan;
    lorahip::DevBuf<float> dTaps;                   // [U][TP]: h[p + i U] at [p][i], zero where p + i U >= L
    lorahip::StreamCarry carry;                     // [K][HC] the HC = T - 1 samples of every row before n0
};

namespace lorahip {

template <class S> struct ResampArgs
{
    const S *in;                    // this call's rows in their format
    long long inStride, nIn;
    const float2 *hist;
    long long n0;                   // absolute index of in[0] of every row
    const float *taps;
    float2 *out;
    long long outStride;
    long long mLo, nOut;            // absolute index of the first output of this call, and how many
    long long tile0;                // the tile mLo falls into
    int K, U, D, L, T, Up, Dp, PB, nPB, NS, sbShift, TI, QP, TP, HC;
    float scale;
};

static int gcdInt(int a, int b) { while (b) { const int r = a % b; a = b; b = r; } return a; }

//! The tiling of (U, D, L) for K rows, or false and the reason. The LDS holds, per row of the group, the tile's input span
//! D' * QP >= TI = (NS - 1) D' + T + ceil((PB - 1) D / U) + 1 samples and its NS * PB outputs. Preferred: the tiling within 64 KiB (two
//! workgroups share a compute unit) with the most work, RG * NS for RG = 8, 4, 2, 1 rows (no group wider than the rows need) and
//! NS = 512 .. 64 steps, the wider row group where two are level (its tap fetches serve more rows); then one row and 64 steps within
//! the 160 KiB of a workgroup; then fewer steps (32 .. 1: lanes idle, but every ratio with D' up to 1024 is served). What no tiling can
//! shrink is the span of ONE step, T + ceil((PB - 1) D / U) + 1 <= T + 993 samples (PB <= U' and PB <= 32), rounded up to D' * QP
//! (at most 2 D' <= 2048 more), and its PB <= 32 outputs: within 160 KiB / 8 bytes = 20480 samples for every T = ceil(L / U) <= 16384,
//! whatever U and D; beyond that it depends on D', and what does not fit is refused.
static bool resampPlan(const size_t up, const size_t down, const size_t nTaps, const size_t nRows, ResampPlan &p, std::string &why)
{
    if (up == 0 || up > 1024 || down == 0 || down > 1024) { why = "up and down must be 1..1024"; return false; }
    if (nTaps == 0 || nTaps > (1u << 16)) { why = "n_taps must be 1..65536"; return false; }
    if (nRows == 0 || nRows > 65535u * 8u) { why = "n_rows must be 1..65535*8"; return false; }
    p.U = int(up); p.D = int(down); p.L = int(nTaps);
    const int g = gcdInt(p.U, p.D);
    p.Up = p.U / g; p.Dp = p.D / g;
    p.T = (p.L + p.U - 1) / p.U;
    p.HC = p.T - 1;
    p.TP = (p.T + 15) & ~15;                        // whole rounds of 16: what the tap loop fetches at a time
    p.PB = p.Up < RS_PB ? p.Up : RS_PB;
    p.nPB = (p.Up + p.PB - 1) / p.PB;
    const auto fits = [&p](const int NS, const int RG, const size_t cap)
    {
        const long long TI = (long long)(NS - 1) * p.Dp + p.T + ((long long)(p.PB - 1) * p.D + p.U - 1) / p.U + 1;
        const long long QP = ((TI + p.Dp - 1) / p.Dp) | 1;
        const unsigned long long lds = (unsigned long long)RG * ((unsigned long long)p.Dp * (unsigned long long)QP + (unsigned long long)NS * p.PB) * sizeof(float2);
        if (lds > cap) return false;
        p.NS = NS; p.RG = RG; p.TI = int(TI); p.QP = int(QP); p.ldsBytes = size_t(lds);
        p.sbShift = 0;
        while ((64 << p.sbShift) < NS) p.sbShift++;
        const int items = p.PB << p.sbShift, rounds = (items + RS_WAVES - 1) / RS_WAVES;
        p.nWaves = (items + rounds - 1) / rounds;
        return true;
    };
    int bestNS = 0, bestRG = 0;
    for (int RG = 8; RG >= 1; RG >>= 1)
        for (int NS = 512; NS >= 64 && size_t(RG) < 2 * nRows; NS >>= 1)
            if (RG * NS > bestRG * bestNS && fits(NS, RG, RS_LDS_SMALL)) { bestNS = NS; bestRG = RG; }
    if (bestNS) return fits(bestNS, bestRG, RS_LDS_SMALL);
    for (int NS = 64; NS >= 1; NS >>= 1)
        if (fits(NS, 1, RS_LDS_MAX)) return true;
    why = "ceil(n_taps / up) samples of a row, and the span of one tile round them, do not fit the LDS (20480 samples; 16384 always fit)";
    return false;
}

//! one tile x one phase block x RG rows; blockIdx.x = tile * nPB + phase block (the phase blocks of a tile are neighbours in launch
//! order and share the tile's input in L2), blockIdx.y + 65535 blockIdx.z = row group
template <int RG, class S>
__global__ __launch_bounds__(RS_WAVES * 64) void resample(const ResampArgs<S> a)
{
    extern __shared__ float2 rsLds[];
    const int tid = threadIdx.x, nT = blockDim.x;
    const int Dp = a.Dp, QP = a.QP, T = a.T, NS = a.NS, PB = a.PB;
    const int RS = Dp * QP;                                     // samples of one row's span in LDS
    float2 *xs = rsLds;                                         // [RG][Dp][QP]
    float2 *ys = rsLds + RG * RS;                               // [RG][NS][PB]
    const int pb = int(blockIdx.x % unsigned(a.nPB));
    const long long tile = a.tile0 + (long long)(blockIdx.x / unsigned(a.nPB));
    const int u0 = pb * PB, nU = min(PB, a.Up - u0);
    const long long mTile = tile * NS * a.Up + u0;              // the block's first output (absolute)
    const long long rowBase = ((long long)blockIdx.y + (long long)blockIdx.z * 65535) * RG;
    // the block's first output: its instant t, newest sample c0 and tap phase p0 -- the one 64-bit division. Subsequence ul stands ul D
    // instants later, which 32 bits hold (p0 + 31 D < 2^16). The oldest sample of the block is T - 1 before c0.
    const unsigned long long t0 = (unsigned long long)(mTile + 1) * unsigned(a.D) - 1;
    const long long c0 = (long long)(t0 / unsigned(a.U));
    const int p0 = int(t0 - (unsigned long long)c0 * unsigned(a.U));
    const long long cMin = c0 - (T - 1);

    {
        const int dq = nT / Dp, dp = nT - dq * Dp;
        int q = tid / Dp, p = tid - q * Dp;
        const long long rel = cMin - a.n0;
        if (rel >= 0 && rel + a.TI <= a.nIn && rowBase + RG <= a.K)
        {
            // the common tile: wholly inside this call's rows. 8 loads in flight per lane and round, then their LDS stores (a load past
            // the span reads its last sample again and is not stored)
            constexpr int B = 8 / RG;
            const S *src = a.in + rowBase * a.inStride + rel;
            for (int jj = tid; jj < a.TI; jj += B * nT)
            {
                float2 v[B][RG];
#pragma unroll
                for (int u = 0; u < B; u++)
#pragma unroll
                    for (int r = 0; r < RG; r++) v[u][r] = iqLoad(src + r * a.inStride + min(jj + u * nT, a.TI - 1), a.scale);
#pragma unroll
                for (int u = 0; u < B; u++)
                {
                    if (jj + u * nT < a.TI)
                    {
#pragma unroll
                        for (int r = 0; r < RG; r++) xs[r * RS + p * QP + q] = v[u][r];
                    }
                    p += dp; q += dq;
                    if (p >= Dp) { p -= Dp; q++; }
                }
            }
        }
        else
        {
            for (int j = tid; j < a.TI; j += nT)
            {
#pragma unroll
                for (int r = 0; r < RG; r++)
                {
                    const long long row = rowBase + r;
                    float2 v = make_float2(0.0f, 0.0f);
                    if (row < a.K) v = carriedSample(a.in + row * a.inStride, a.nIn, a.hist + row * a.HC, a.HC, a.n0, cMin + j, a.scale);
                    xs[r * RS + p * QP + q] = v;
                }
                p += dp; q += dq;
                if (p >= Dp) { p -= Dp; q++; }
            }
        }
    }
    __syncthreads();

    // items = (subsequence, block of 64 steps), shared out among the wavefronts; everything but the lane's step is wave-uniform
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nWaves = nT >> 6;
    const int lane = tid & 63;
    const int items = nU << a.sbShift;
    for (int it = wave; it < items; it += nWaves)
    {
        const int ul = it >> a.sbShift, sb = it - (ul << a.sbShift);
        const unsigned tu = unsigned(p0) + unsigned(ul) * unsigned(a.D);
        const int dc = int(tu / unsigned(a.U));
        const int p = __builtin_amdgcn_readfirstlane(int(tu) - dc * a.U);
        const int j0 = __builtin_amdgcn_readfirstlane(dc + T - 1);     // the newest sample of step 0 in the span; j0 + (NS-1) D' < TI
        const int step = sb * 64 + (lane < NS ? lane : 0);             // idle lanes (NS < 64) read what lane 0 reads and store nothing
        int pp = __builtin_amdgcn_readfirstlane(j0 % Dp);              // (the quotient and remainder come out of the vector unit)
        int off = (pp * QP + __builtin_amdgcn_readfirstlane(j0 / Dp) + step) * int(sizeof(float2));    // in bytes: one add a tap
        const ConstFloat *hp = (const ConstFloat *)(a.taps + (size_t)p * a.TP);
        float2 acc[RG];
#pragma unroll
        for (int r = 0; r < RG; r++) acc[r] = make_float2(0.0f, 0.0f);
        // acc = fma(h[i], x[c - i], acc) for i = 0 .. T - 1. From one tap to the next the sample is one older: the D' phase below, or
        // the last phase one slot earlier (pp and the step of off are wave-uniform).
        const int wrapBytes = ((Dp - 1) * QP - 1) * int(sizeof(float2)), downBytes = -QP * int(sizeof(float2));
        const char *xb = reinterpret_cast<const char *>(xs);
        const auto older = [&]()
        {
            off += pp == 0 ? wrapBytes : downBytes;
            pp = pp == 0 ? Dp - 1 : pp - 1;
        };
        // R taps a round. Their coefficients are read through the constant address space at a wave-uniform address: one scalar load
        // of R dwords into SGPRs (s_load_dwordx16 at RG = 1 .. x2 at RG = 8), which the packed multiply-adds take as their scalar
        // operand. The round's R * RG = 16 LDS reads are issued beside it. The last round holds n < R taps: it reads and multiplies
        // only n samples -- the span in LDS ends with tap T - 1, and a product with a tap behind it would carry a non-finite sample
        // further than the definition says -- but its coefficient fetches are not cut to n (up to R - 1 dwords, some of them behind
        // tap T - 1): every row of the table is padded with zeros to whole rounds of 16 so that they stay inside it.
        constexpr int R = 16 / RG;
        const auto round = [&](const int i, const int n)
        {
            float h[R];
            float2 x[R][RG];
#pragma unroll
            for (int k = 0; k < R; k++) h[k] = hp[i + k];
#pragma unroll
            for (int k = 0; k < R; k++)
                if (k < n)
                {
#pragma unroll
                    for (int r = 0; r < RG; r++) x[k][r] = *reinterpret_cast<const float2 *>(xb + r * RS * int(sizeof(float2)) + off);
                    older();
                }
            // Keeps the scheduler from pairing every read with its add (one read in flight). It does not put all 16 reads before
            // the first add: instruction selection has moved the adds of the round's first taps ahead of it by then. As compiled
            // (RG = 1): 4 reads, a wait for them and the coefficients, then adds and reads interleaved with up to 7 reads in flight.
            // Forcing all 16 reads ahead of the first add was measured and is slower on one row.
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < R; k++)
                if (k < n)
                {
#pragma unroll
                    for (int r = 0; r < RG; r++)
                    {
                        acc[r].x = __builtin_fmaf(h[k], x[k][r].x, acc[r].x);
                        acc[r].y = __builtin_fmaf(h[k], x[k][r].y, acc[r].y);
                    }
                }
        };
        int i = 0;
        for (; i + R <= T; i += R) round(i, R);
        if (i < T) round(i, T - i);
        if (lane < NS)
        {
#pragma unroll
            for (int r = 0; r < RG; r++)
                ys[(r * NS + step) * PB + ul] = p < a.L ? acc[r] : make_float2(0.0f, 0.0f);     // a phase without a tap: exactly 0
        }
    }
    __syncthreads();

    // step s of the block holds the nU consecutive outputs mTile + s U' ..: consecutive threads store consecutive samples
    {
        const int total = NS * nU;
        const int ds = nT / nU, du = nT - ds * nU;
        int s = tid / nU, ul = tid - s * nU;
        const long long mRel = mTile - a.mLo;                   // the block's first output in this call (< 0: the call starts inside it)
        for (int idx = tid; idx < total; idx += nT)
        {
            const long long ml = mRel + (long long)s * a.Up + ul;
            if (ml >= 0 && ml < a.nOut)
            {
#pragma unroll
                for (int r = 0; r < RG; r++)
                    if (rowBase + r < a.K) a.out[(rowBase + r) * a.outStride + ml] = ys[(r * NS + s) * PB + ul];
            }
            ul += du; s += ds;
            if (ul >= nU) { ul -= nU; s++; }
        }
    }
}

//! the HC samples of every row that precede the next call
template <class S> __global__ void resampHistory(const ResampArgs<S> a, float2 *newHist)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = (long long)blockIdx.y + (long long)blockIdx.z * 65535;
    if (h < a.HC && row < a.K)
        newHist[row * a.HC + h] = carriedSample(a.in + row * a.inStride, a.nIn, a.hist + row * a.HC, a.HC, a.n0, a.n0 + a.nIn - a.HC + h, a.scale);
}

//! floor(n U / D) for a stream position (128-bit product: n is the caller's)
static unsigned long long resampOutputsBefore(const ResampPlan &p, const unsigned long long n)
{
    return (unsigned long long)((unsigned __int128)n * unsigned(p.U) / unsigned(p.D));
}

template <int RG, class S> static hipError_t resampLaunch(const lorahip_resampler *r, const ResampArgs<S> &a, const dim3 grid)
{
    static unsigned long long ldsMask;
    const hipError_t e = ensureDynamicLds(reinterpret_cast<const void *>(&resample<RG, S>), RS_LDS_MAX, ldsMask);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((resample<RG, S>), grid, dim3(unsigned(r->plan.nWaves) * 64u), r->plan.ldsBytes, r->ctx->stream, a);
    return hipGetLastError();
}

//! the next nIn samples of every row; in of the format S, scale what the integer formats multiply by
template <class S>
static int resampRun(lorahip_resampler *r, const S *in, const float scale, const size_t inStride, const size_t nIn, float2 *out, const size_t outStride,
                     size_t *nOutP)
{
    lorahip_ctx *ctx = r->ctx;
    const ResampPlan &p = r->plan;
    const DeviceGuard guard(ctx->device);
    if (nOutP) *nOutP = 0;
    if (nIn == 0) return LORAHIP_OK;
    const unsigned long long n0 = r->carry.n0;
    if (nIn > RS_POS_MAX || n0 + nIn > RS_POS_MAX) { setLastError("resampler: the stream position would pass 2^52"); return LORAHIP_E_INVALID; }
    const unsigned long long mLo = resampOutputsBefore(p, n0);
    const size_t nOut = size_t(resampOutputsBefore(p, n0 + nIn) - mLo);
    if (nOut > (size_t(1) << 30)) { setLastError("resampler: more than 2^30 outputs per row in one call"); return LORAHIP_E_INVALID; }
    if (in == nullptr || (nOut && out == nullptr)) { setLastError("resampler: a device pointer is NULL"); return LORAHIP_E_INVALID; }
    if (inStride < nIn) { setLastError("resampler: in_stride is shorter than n_in"); return LORAHIP_E_INVALID; }
    if (outStride < nOut) { setLastError("resampler: out_stride is shorter than the output count"); return LORAHIP_E_INVALID; }
    ResampArgs<S> a;
    a.in = in; a.inStride = (long long)inStride; a.nIn = (long long)nIn;
    a.hist = r->carry.current();
    a.n0 = (long long)n0;
    a.taps = r->dTaps.get();
    a.out = out; a.outStride = (long long)outStride;
    a.mLo = (long long)mLo; a.nOut = (long long)nOut;
    const unsigned long long perTile = (unsigned long long)p.NS * unsigned(p.Up);
    a.tile0 = (long long)(mLo / perTile);
    a.K = r->K; a.U = p.U; a.D = p.D; a.L = p.L; a.T = p.T; a.Up = p.Up; a.Dp = p.Dp; a.PB = p.PB; a.nPB = p.nPB; a.NS = p.NS; a.sbShift = p.sbShift; a.TI = p.TI;
    a.QP = p.QP; a.TP = p.TP; a.HC = p.HC;
    a.scale = scale;
    const unsigned groups = unsigned((r->K + p.RG - 1) / p.RG);
    const unsigned gy = groups < 65535u ? groups : 65535u, gz = (groups + 65534u) / 65535u;
    if (nOut)
    {
        const unsigned long long tiles = (mLo + nOut - 1) / perTile - mLo / perTile + 1;
        const unsigned long long nBlocks = tiles * unsigned(p.nPB);
        if (nBlocks > 0x7fffffffu || nBlocks * (unsigned(p.nWaves) * 64u) > 0xffffffffu)     // the runtime refuses 2^32 threads in x
        {
            setLastError("resampler: tiles x phase blocks of one call exceed the launch grid");
            return LORAHIP_E_INVALID;
        }
        const dim3 grid((unsigned)nBlocks, gy, gz);
        LORAHIP_TRY(p.RG == 8 ? resampLaunch<8>(r, a, grid) : p.RG == 4 ? resampLaunch<4>(r, a, grid) : p.RG == 2 ? resampLaunch<2>(r, a, grid)
                                                                                                                   : resampLaunch<1>(r, a, grid));
    }
    if (p.HC)
    {
        const unsigned ky = unsigned(r->K < 65535 ? r->K : 65535), kz = unsigned((r->K + 65534) / 65535);
        hipLaunchKernelGGL(resampHistory<S>, dim3((p.HC + 255) / 256, ky, kz), dim3(256), 0, ctx->stream, a, r->carry.next());
        LORAHIP_TRY(hipGetLastError());
    }
    r->carry.advance(nIn);
    if (nOutP) *nOutP = nOut;
    return LORAHIP_OK;
}

} // namespace lorahip

using namespace lorahip;

extern "C" {

int lorahip_resampler_check(const size_t up, const size_t down, const size_t n_taps, const size_t n_rows)
{
    ResampPlan p;
    std::string why;
    if (resampPlan(up, down, n_taps, n_rows, p, why)) return LORAHIP_OK;
    setLastError("resampler: " + why);
    return LORAHIP_E_INVALID;
}

int lorahip_resampler_plan(const size_t up, const size_t down, const size_t n_taps, const size_t n_rows, lorahip_resampler_tiling *plan)
{
    if (plan == nullptr) { setLastError("resampler: NULL argument"); return LORAHIP_E_INVALID; }
    *plan = lorahip_resampler_tiling();
    ResampPlan p;
    std::string why;
    if (!resampPlan(up, down, n_taps, n_rows, p, why)) { setLastError("resampler: " + why); return LORAHIP_E_INVALID; }
    plan->ns = size_t(p.NS); plan->rg = size_t(p.RG); plan->pb = size_t(p.PB); plan->n_phase_blocks = size_t(p.nPB);
    plan->ti = size_t(p.TI); plan->qp = size_t(p.QP); plan->waves = size_t(p.nWaves); plan->lds_bytes = p.ldsBytes;
    plan->t = size_t(p.T); plan->up_reduced = size_t(p.Up); plan->down_reduced = size_t(p.Dp);
    return LORAHIP_OK;
}

int lorahip_resampler_create(lorahip_resampler **out, lorahip_ctx *ctx, const size_t n_rows, const size_t up, const size_t down, const float *taps,
                             const size_t n_taps)
{
    if (out == nullptr) return LORAHIP_E_INVALID;
    *out = nullptr;
    if (ctx == nullptr || taps == nullptr) { setLastError("resampler: NULL argument"); return LORAHIP_E_INVALID; }
    ResampPlan p;
    std::string why;
    if (!resampPlan(up, down, n_taps, n_rows, p, why)) { setLastError("resampler: " + why); return LORAHIP_E_INVALID; }
    lorahip_resampler *r = new (std::nothrow) lorahip_resampler();
    if (r == nullptr) return LORAHIP_E_NOMEM;
    r->ctx = ctx; r->K = int(n_rows); r->plan = p;
    std::vector<float> h;
    try { h.assign(size_t(p.U) * size_t(p.TP), 0.0f); }
    catch (const std::bad_alloc &) { delete r; return LORAHIP_E_NOMEM; }
    for (int j = 0; j < p.L; j++) h[size_t(j % p.U) * size_t(p.TP) + size_t(j / p.U)] = taps[j];
    return uploadTables(out, r, "resampler", n_rows * size_t(p.HC), r->dTaps, h.data(), h.size());
}

void lorahip_resampler_destroy(lorahip_resampler *r)
{
    if (r == nullptr) return;
    const DeviceGuard guard(r->ctx->device);
    delete r;
}

int lorahip_resampler_reset_at(lorahip_resampler *r, const uint64_t position)
{
    if (r == nullptr) return LORAHIP_E_INVALID;
    if (position > RS_POS_MAX) { setLastError("resampler: a stream position beyond 2^52"); return LORAHIP_E_INVALID; }
    const DeviceGuard guard(r->ctx->device);
    LORAHIP_TRY(r->carry.reset(r->ctx->stream));
    r->carry.n0 = position;
    return LORAHIP_OK;
}

int lorahip_resampler_reset(lorahip_resampler *r) { return lorahip_resampler_reset_at(r, 0); }

size_t lorahip_resampler_out_count(const lorahip_resampler *r, const size_t n_in)
{
    if (r == nullptr || n_in > RS_POS_MAX || r->carry.n0 + n_in > RS_POS_MAX) return 0;      // what run() refuses
    return size_t(resampOutputsBefore(r->plan, r->carry.n0 + n_in) - resampOutputsBefore(r->plan, r->carry.n0));
}

int lorahip_resampler_run(lorahip_resampler *r, const float *in_dev, const size_t in_stride, const size_t n_in, float *out_dev, const size_t out_stride,
                          size_t *n_out)
{
    if (r == nullptr) return LORAHIP_E_INVALID;
    return resampRun(r, reinterpret_cast<const float2 *>(in_dev), 1.0f, in_stride, n_in, reinterpret_cast<float2 *>(out_dev), out_stride, n_out);
}

int lorahip_resampler_run_iq(lorahip_resampler *r, const void *in_dev, const int format, const float scale, const size_t in_stride, const size_t n_in,
                             float *out_dev, const size_t out_stride, size_t *n_out)
{
    if (r == nullptr) return LORAHIP_E_INVALID;
    if (n_out) *n_out = 0;
    if (iqCheck("resampler", in_dev, format, scale) != LORAHIP_OK) return LORAHIP_E_INVALID;
    return iqDispatch(in_dev, format, [&](const auto *in) { return resampRun(r, in, scale, in_stride, n_in, reinterpret_cast<float2 *>(out_dev), out_stride, n_out); });
}

} // extern "C"
