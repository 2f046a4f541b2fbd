// Front-end synthesiser: K channel streams at the channel rate -> one wideband stream (include/lorahip.h has the definition). The mirror
// image of lorahip_chan.hip: zero-stuff by U, low-pass, mix each channel up to its centre, scale, sum. Like the channeliser it is not a
// reference component, so there is nothing to be bit-exact with: the tests check against a float64 restatement of the definition.
//
// The mixer factors exactly in the 64-bit phase (w n = w j + w (n - j) mod 2^64), so with n = m U + p and j = p + i U
//     y[m U + p] = sum_k sum_i g_k[p + i U] xr_k[m - i],    g_k[j] = gain_k h[j] e^{+i theta_k j},    xr_k[m] = x_k[m] e^{+i theta_k U m}
//   * the host pre-rotates (and pre-scales) the taps per channel in double;
//   * the device rotates every INPUT sample once while it stages it into LDS: K rotations per input time, not K per output;
//   * what is left is K ceil(L/U) complex multiply-adds per output with wave-uniform coefficients: fp32 VALU work (v_pk_fma_f32), as in
//     the channeliser.
// One workgroup = one tile of 256 input times m x one block of 8 output phases p, all channels. Lane = input time: it holds its 8
// outputs in registers and walks the channels in ascending order, 8 at a time through LDS (one ds_read_b64 of xr_k[m - i] feeds
// 16 v_pk_fma_f32 whose coefficients arrive through the scalar cache), so the channel sum has one fixed order. Tiles sit on absolute
// multiples of 256 input times and the rotation is (phase at the start of a 256-block, evaluated from the 64-bit counter) x (table over
// the 256 places inside it): nothing depends on how the stream was cut into calls, and nothing drifts.
// Stores: a lane's 8 outputs are 64 contiguous bytes, lanes lie U * 8 bytes apart: four 16-byte stores per lane, back to back
// (DESIGN.md has the reasoning and what was measured).
// The kernel is a template on the output sample type S (`Out` inside the kernel; lorahip_frontend.h: float2, short2 = sc16, char2 =
// sc8); nothing before the store depends on it. A lane's 8 outputs are 8 * sizeof(S) contiguous bytes = 64 / 32 / 16, lanes lie
// U * sizeof(S) bytes apart. The rule of the wide path, for every S: vec16 = (U * sizeof(S)) % 16 == 0 and the output pointer is
// 16-byte aligned -- then every lane's first output of a full phase block is, and the lane writes four / two / one 16-byte stores.
// U even (cf32), U % 4 == 0 (sc16), U % 8 == 0 (sc8). Otherwise, and in a partial phase block, one store per sample, guarded by
// p0 + p < U. The integer instances quantise by the definition in include/lorahip.h (iqPack) and add their clipped components to the
// object's counter, one atomic per wavefront at most (iqCountClipped).
#include "lorahip_frontend.h"
#include "lorahip_mixer.h"
#include <cmath>
#include <new>
#include <vector>

struct lorahip_synthesizer
{
    lorahip_ctx *ctx;
    int K, L, U, I, UP, nPB, TS, nBlk, HC, nGroups;
    size_t ldsBytes;
    lorahip::DevBuf<float2> dTaps;              // [nGroups*8][I][UP] (+ a pad row): g_k[p + i U] at [k][i][p], zero where p + i U >= L or p >= U
    lorahip::DevBuf<unsigned long long> dWU;    // [nGroups*8] w_k * U mod 2^64: the phase step of one input time
    lorahip::DevBuf<float2> dRot;               // [nGroups*8][256] e^{+2 pi i frac(w_k U t / 2^64)}
    lorahip::StreamCarry carry;                 // [K][HC] the HC input samples of every channel before n0
    lorahip::ClipCount clipped;                 // components the integer runs clipped since create / reset
};

namespace lorahip {

constexpr int SYN_THREADS = 256;    // input times per tile
constexpr int SYN_KG = 8;           // channels staged together
constexpr int SYN_P = 8;            // output phases per lane

struct SynthArgs
{
    const float2 *in;
    long long inStride, nIn;
    const float2 *hist;
    long long n0;                   // absolute index of in[0] of every row
    const v2f *taps;
    const unsigned long long *wU;
    const v2f *laneRot;
    void *out;                      // samples of the kernel's S
    int K, L, U, I, UP, nPB, TS, nBlk, HC, nGroups, vec16;
    unsigned long long *clipped;    // the integer instances count here; float2 ignores both
    float scale;
};

//! sample m of channel ch (absolute index): from this call's rows, from the history kept from earlier calls, or 0
__device__ __forceinline__ float2 synthSample(const SynthArgs &a, const int ch, const long long m)
{
    const long long c = m - a.n0, h = c + a.HC;
    const float2 *src = c >= 0 ? a.in + (long long)ch * a.inStride + c : a.hist + (long long)ch * a.HC + h;
    const bool ok = ch < a.K && (c >= 0 ? c < a.nIn : h >= 0);
    float2 v = make_float2(0.0f, 0.0f);
    if (ok) v = *src;
    return v;
}

typedef float v16f __attribute__((ext_vector_type(16)));

//! start the loads of one tap block: the 8 phase coefficients of one channel (wave-uniform, 64 bytes through the scalar cache) and this
//! lane's rotated sample
__device__ __forceinline__ void synthIssue(v16f &G, v2f &X, const v2f *gp, const unsigned ldsAddr)
{
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\tds_read_b64 %1, %3" : "=&s"(G), "=&v"(X) : "s"(gp), "v"(ldsAddr) : "memory");
}
//! the loads have landed; both pass through so that no use can be scheduled above the wait
__device__ __forceinline__ void synthWait(v16f &G, v2f &X)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(G), "+v"(X));
}
//! acc[p] += g[p] * x for the 8 phases of a lane. All first halves of the complex multiply-adds, then all second halves, so that no
//! packed FMA waits for the one issued just before it
__device__ __forceinline__ void synthFma(v2f (&acc)[SYN_P], const v16f &G, const v2f x)
{
    v2f c[SYN_P];
#pragma unroll
    for (int p = 0; p < SYN_P; p++) c[p] = (v2f){G[2 * p], G[2 * p + 1]};
#pragma unroll
    for (int p = 0; p < SYN_P; p++)
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc[p]) : "s"(c[p]), "v"(x));                  // (g.x*x.x, g.x*x.y)
#pragma unroll
    for (int p = 0; p < SYN_P; p++)
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(acc[p]) : "s"(c[p]), "v"(x));   // (-g.y*x.y, g.y*x.x)
}

// blockIdx.x = tile * nPB + phase block: the phase blocks of a tile are neighbours in launch order and share the tile's input in L2
template <class Out> __global__ __launch_bounds__(SYN_THREADS) void synthesize(const SynthArgs a)
{
    extern __shared__ float2 synLds[];
    v2f *xs = reinterpret_cast<v2f *>(synLds);                  // [8][TS] rotated samples, then [nBlk][8] block phases
    const int t = threadIdx.x;
    const int I = a.I, TS = a.TS, HC = a.HC, UP = a.UP;
    const int pb = int(blockIdx.x % unsigned(a.nPB));
    // tiles sit on absolute multiples of 256 input times, so a sample's place in its tile -- and with it every rounding -- does not
    // depend on how the stream was cut into calls
    const long long mTile = ((a.n0 >> 8) + (long long)(blockIdx.x / unsigned(a.nPB))) * SYN_THREADS;
    const long long mStart = mTile - HC;                        // oldest sample the tile needs (may be < 0: reads as 0)
    const long long blk0 = mStart >> 8;                         // floor, also below 0
    v2f *base = xs + SYN_KG * TS;

    v2f acc[SYN_P];
#pragma unroll
    for (int p = 0; p < SYN_P; p++) acc[p] = (v2f){0.0f, 0.0f};

    for (int g = 0; g < a.nGroups; g++)
    {
        const int chBase = g * SYN_KG;                          // wU, laneRot and taps are padded to whole groups
        if (g) __syncthreads();                                 // the previous group's reads are done
        // e^{+i theta_k U m} = (phase at the first sample of m's 256-block) x (phase over m mod 256 more): one sine/cosine per channel
        // and block, evaluated from the 64-bit counter, the rest from a per-channel table of 256 entries
        if (t < SYN_KG * a.nBlk)
        {
            const unsigned long long mb = (unsigned long long)((blk0 + (t >> 3)) * SYN_THREADS);    // wraps like the counter below 0
            const v2f r = mixerPhase(unsigned((a.wU[chBase + (t & 7)] * mb) >> 32));
            base[t] = (v2f){r.x, -r.y};                         // mixerPhase is e^{-i ...}
        }
        __syncthreads();
        for (int c = 0; c < SYN_KG; c++)
        {
            const int ch = chBase + c;
            for (int j = t; j < TS; j += SYN_THREADS)
            {
                const long long m = mStart + j;
                const float2 v = synthSample(a, ch, m);
                const v2f rot = cmulF(a.laneRot[ch * SYN_THREADS + int(m & 255)], base[int((m >> 8) - blk0) * SYN_KG + c]);
                xs[c * TS + j] = cmulF((v2f){v.x, v.y}, rot);
            }
        }
        __syncthreads();
        // One tap block (channel c, taps p + i U of the 8 phases) per step, channels ascending, software-pipelined by hand: while the 16
        // packed FMAs of a step run, the next step's LDS read and scalar coefficient load are in flight. Both return through lgkmcnt
        // and scalar loads complete out of order, so the only safe wait is lgkmcnt(0), placed before the next issue. The prefetch of
        // the last step reads the next group's first coefficients (or the pad row behind the table) and is dropped.
        // (the 64-bit product is evaluated on the vector side: hand the scalar loads a pointer that is in scalar registers for sure)
        const uintptr_t gu = uintptr_t(a.taps + ((size_t)chBase * I) * UP + pb * SYN_P);
        const unsigned gLo = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(gu)))), gHi = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(gu >> 32))));
        const v2f *gp = reinterpret_cast<const v2f *>(uintptr_t(gLo) | (uintptr_t(gHi) << 32));    // (unsigned: the builtin returns int, which would sign-extend)
        const unsigned lds0 = unsigned(uintptr_t(xs)) + unsigned(HC + t) * 8u;      // xr_c[m] of channel 0; low half of a flat LDS address = the LDS offset
        const unsigned wrap = unsigned(TS + HC) * 8u;                               // from (c, I - 1) to (c + 1, 0)
        const int S = SYN_KG * I;                                                   // even
        unsigned addr = lds0;
        int i = 0;
        v16f gA, gB;
        v2f xA, xB;
        asm volatile("s_nop 4" ::: "memory");                    // the pointer has just come out of the vector unit
        synthIssue(gA, xA, gp, addr);
        for (int st = 0; st < S; st += 2)
        {
            gp += UP;
            if (++i == I) { i = 0; addr += wrap; } else addr -= 8u;
            synthWait(gA, xA);
            synthIssue(gB, xB, gp, addr);
            synthFma(acc, gA, xA);
            gp += UP;
            if (++i == I) { i = 0; addr += wrap; } else addr -= 8u;
            synthWait(gB, xB);
            synthIssue(gA, xA, gp, st + 2 < S ? addr : lds0);
            synthFma(acc, gB, xB);
        }
        synthWait(gA, xA);                                      // nothing may still be in flight when the registers are reused
    }

    const long long mLoc = mTile + t - a.n0;                    // this lane's input time in this call
    if (mLoc < 0 || mLoc >= a.nIn) return;
    const int p0 = pb * SYN_P;
#pragma unroll
    for (int p = 0; p < SYN_P; p++)
        if (p0 + p >= a.L) acc[p] = (v2f){0.0f, 0.0f};          // a phase without a tap: exactly 0 whatever the input holds
    Out *o = static_cast<Out *>(a.out) + (mLoc * a.U + p0);         // 64-bit: 2^30 outputs are 2^33 bytes
    if constexpr (std::is_same<Out, float2>::value)
    {
        if (a.vec16 && p0 + SYN_P <= a.U)
        {
#pragma unroll
            for (int p = 0; p < SYN_P; p += 2)
                *reinterpret_cast<float4 *>(o + p) = make_float4(acc[p].x, acc[p].y, acc[p + 1].x, acc[p + 1].y);
        }
        else
        {
#pragma unroll
            for (int p = 0; p < SYN_P; p++)
                if (p0 + p < a.U) o[p] = make_float2(acc[p].x, acc[p].y);
        }
    }
    else
    {
        unsigned clipped = 0;                                   // <= 16 a lane
        if (a.vec16 && p0 + SYN_P <= a.U)
        {
            constexpr int PER = 16 / int(sizeof(Out));            // samples per 16-byte store: 4 (sc16), 8 (sc8)
            struct alignas(16) Line { Out v[PER]; };
#pragma unroll
            for (int p = 0; p < SYN_P; p += PER)
            {
                Line line;
#pragma unroll
                for (int q = 0; q < PER; q++) line.v[q] = iqPack(o, make_float2(acc[p + q].x, acc[p + q].y), a.scale, clipped);
                *reinterpret_cast<Line *>(o + p) = line;
            }
        }
        else
        {
#pragma unroll
            for (int p = 0; p < SYN_P; p++)
                if (p0 + p < a.U) iqStore(o + p, make_float2(acc[p].x, acc[p].y), a.scale, clipped);
        }
        iqCountClipped<5>(a.clipped, clipped);                  // the lanes of both paths are together again (the path is the block's)
    }
}

//! the HC samples of every channel that precede the next call
__global__ void synthHistory(const SynthArgs a, float2 *newHist)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = blockIdx.y + blockIdx.z * 65535;
    if (h < a.HC && ch < a.K) newHist[(long long)ch * a.HC + h] = synthSample(a, ch, a.n0 + a.nIn - a.HC + h);
}

//! out in the format S; scale is what the integer formats multiply by
template <class S>
static int synthRun(lorahip_synthesizer *s, const float2 *in, const size_t inStride, const size_t nIn, S *out, const float scale, size_t *nOutP)
{
    static unsigned long long ldsMask = 0;
    lorahip_ctx *ctx = s->ctx;
    const DeviceGuard guard(ctx->device);
    if (nOutP) *nOutP = 0;
    if (nIn == 0) return LORAHIP_OK;
    if (in == nullptr || out == nullptr) { setLastError("synthesiser: a device pointer is NULL"); return LORAHIP_E_INVALID; }
    if (inStride < nIn) { setLastError("synthesiser: in_stride is shorter than n_in"); return LORAHIP_E_INVALID; }
    const size_t nOut = nIn * size_t(s->U);
    if (nOut > (size_t(1) << 30)) { setLastError("synthesiser: more than 2^30 outputs in one call"); return LORAHIP_E_INVALID; }
    const size_t nBlocks = size_t(s->nPB) * ((s->carry.n0 % SYN_THREADS + nIn + SYN_THREADS - 1) / SYN_THREADS);
    if (nBlocks > 0x7fffffffu) { setLastError("synthesiser: tiles x phase blocks of one call exceed the launch grid"); return LORAHIP_E_INVALID; }
    SynthArgs a;
    a.in = in; a.inStride = (long long)inStride; a.nIn = (long long)nIn;
    a.hist = s->carry.current();
    a.n0 = (long long)s->carry.n0;
    a.taps = reinterpret_cast<const v2f *>(s->dTaps.get());
    a.wU = s->dWU.get();
    a.laneRot = reinterpret_cast<const v2f *>(s->dRot.get());
    a.out = out;
    a.K = s->K; a.L = s->L; a.U = s->U; a.I = s->I; a.UP = s->UP; a.nPB = s->nPB; a.TS = s->TS; a.nBlk = s->nBlk; a.HC = s->HC;
    a.nGroups = s->nGroups;
    a.vec16 = ((size_t(s->U) * sizeof(S)) % 16 == 0 && uintptr_t(out) % 16 == 0) ? 1 : 0;
    if constexpr (!std::is_same<S, float2>::value) LORAHIP_TRY(s->clipped.ensure(ctx->stream));
    a.clipped = s->clipped.dev.get(); a.scale = scale;
    LORAHIP_TRY(ensureDynamicLds(reinterpret_cast<const void *>(&synthesize<S>), 160 * 1024, ldsMask));
    hipLaunchKernelGGL(synthesize<S>, dim3((unsigned)nBlocks), dim3(SYN_THREADS), s->ldsBytes, ctx->stream, a);
    LORAHIP_TRY(hipGetLastError());
    if (s->HC)
    {
        const unsigned ky = unsigned(s->K < 65535 ? s->K : 65535), kz = unsigned((s->K + 65534) / 65535);
        hipLaunchKernelGGL(synthHistory, dim3((s->HC + 255) / 256, ky, kz), dim3(256), 0, ctx->stream, a, s->carry.next());
        LORAHIP_TRY(hipGetLastError());
    }
    s->carry.advance(nIn);
    if (nOutP) *nOutP = nOut;
    return LORAHIP_OK;
}

} // namespace lorahip

using namespace lorahip;

extern "C" {

int lorahip_synthesizer_create(lorahip_synthesizer **out, lorahip_ctx *ctx, const size_t n_channels, const double *freq, const float *gain,
                               const size_t interp, const float *taps, const size_t n_taps)
{
    if (out == nullptr) return LORAHIP_E_INVALID;
    *out = nullptr;
    if (ctx == nullptr || freq == nullptr || taps == nullptr || n_channels == 0 || n_channels > 65535u * SYN_KG ||
        interp == 0 || interp > 256 || n_taps == 0 || n_taps > (1u << 16))
    {
        setLastError("synthesiser: NULL argument, or n_channels outside 1..65535*8, interp outside 1..256, n_taps outside 1..65536");
        return LORAHIP_E_INVALID;
    }
    if (gain)
        for (size_t k = 0; k < n_channels; k++)
            if (!std::isfinite(gain[k])) { setLastError("synthesiser: a gain is not finite"); return LORAHIP_E_INVALID; }
    const int U = int(interp), L = int(n_taps);
    const int I = (L + U - 1) / U;                               // taps per output phase
    const int HC = I - 1, TS = SYN_THREADS + HC, nBlk = (HC + SYN_THREADS - 1) / SYN_THREADS + 1;
    const size_t lds = (size_t(SYN_KG) * size_t(TS) + size_t(SYN_KG) * size_t(nBlk)) * sizeof(float2);
    if (lds > (160u << 10) || SYN_KG * nBlk > SYN_THREADS)
    {
        setLastError("synthesiser: 8 * (256 + n_taps/interp) samples do not fit the LDS");
        return LORAHIP_E_INVALID;
    }
    lorahip_synthesizer *s = new (std::nothrow) lorahip_synthesizer();
    if (s == nullptr) return LORAHIP_E_NOMEM;
    s->ctx = ctx; s->K = int(n_channels); s->L = L; s->U = U; s->I = I; s->HC = HC; s->TS = TS; s->nBlk = nBlk;
    s->nPB = (U + SYN_P - 1) / SYN_P; s->UP = s->nPB * SYN_P;
    s->nGroups = int((n_channels + SYN_KG - 1) / SYN_KG);
    s->ldsBytes = lds;

    const size_t KP = size_t(s->nGroups) * SYN_KG, UP = size_t(s->UP);
    std::vector<unsigned long long> wU;
    std::vector<float2> g, rot;
    try
    {
        wU.assign(KP, 0);
        g.assign((KP * size_t(I) + 1) * UP, make_float2(0.0f, 0.0f));     // + a pad row for the last prefetch
        rot.assign(KP * SYN_THREADS, make_float2(1.0f, 0.0f));
    }
    catch (const std::bad_alloc &) { delete s; return LORAHIP_E_NOMEM; }
    for (size_t k = 0; k < n_channels; k++)
    {
        const unsigned long long w = lorahip_channelizer_phase_inc(freq[k]);
        const double gk = gain ? double(gain[k]) : 1.0;
        wU[k] = w * (unsigned long long)U;
        for (int j = 0; j < L; j++)
        {
            const double ang = 2.0 * M_PI * std::ldexp(double((long long)(w * (unsigned long long)j)), -64);    // turns in [-0.5, 0.5)
            g[(k * size_t(I) + size_t(j / U)) * UP + size_t(j % U)] =
                make_float2(float(gk * double(taps[j]) * std::cos(ang)), float(gk * double(taps[j]) * std::sin(ang)));
        }
        for (int t = 0; t < SYN_THREADS; t++)
        {
            const double ang = 2.0 * M_PI * std::ldexp(double((long long)(wU[k] * (unsigned long long)t)), -64);
            rot[k * SYN_THREADS + size_t(t)] = make_float2(float(std::cos(ang)), float(std::sin(ang)));
        }
    }
    return uploadTables(out, s, "synthesiser", size_t(n_channels) * size_t(HC), s->dTaps, g.data(), g.size(), s->dWU, wU.data(), wU.size(),
                        s->dRot, rot.data(), rot.size());
}

void lorahip_synthesizer_destroy(lorahip_synthesizer *s)
{
    if (s == nullptr) return;
    const DeviceGuard guard(s->ctx->device);
    delete s;
}

int lorahip_synthesizer_reset(lorahip_synthesizer *s)
{
    if (s == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(s->ctx->device);
    LORAHIP_TRY(s->carry.reset(s->ctx->stream));
    LORAHIP_TRY(s->clipped.reset(s->ctx->stream));
    return LORAHIP_OK;
}

size_t lorahip_synthesizer_out_count(const lorahip_synthesizer *s, const size_t n_in)
{
    return s == nullptr ? 0 : n_in * size_t(s->U);
}

int lorahip_synthesizer_run(lorahip_synthesizer *s, const float *in_dev, const size_t in_stride, const size_t n_in, float *wide_dev,
                            size_t *n_out)
{
    if (s == nullptr) return LORAHIP_E_INVALID;
    return synthRun(s, reinterpret_cast<const float2 *>(in_dev), in_stride, n_in, reinterpret_cast<float2 *>(wide_dev), 1.0f, n_out);
}

int lorahip_synthesizer_run_iq(lorahip_synthesizer *s, const float *in_dev, const size_t in_stride, const size_t n_in, void *wide_dev,
                               const int format, const float scale, size_t *n_out)
{
    if (s == nullptr) return LORAHIP_E_INVALID;
    if (n_out) *n_out = 0;
    if (iqCheck("synthesiser", wide_dev, format, scale) != LORAHIP_OK) return LORAHIP_E_INVALID;
    return iqDispatch(wide_dev, format, [&](auto *wide) { return synthRun(s, reinterpret_cast<const float2 *>(in_dev), in_stride, n_in, wide, scale, n_out); });
}

int lorahip_synthesizer_clipped(lorahip_synthesizer *s, unsigned long long *count)
{
    if (s == nullptr || count == nullptr) return LORAHIP_E_INVALID;
    const DeviceGuard guard(s->ctx->device);
    LORAHIP_TRY(s->clipped.read(s->ctx->stream, count));
    return LORAHIP_OK;
}

} // extern "C"
