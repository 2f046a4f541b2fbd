// The radix-2 transform the two polyphase banks share: lorahip_pfb.hip runs it forward (twiddles exp(-2 pi i k / M)) and
// lorahip_psb.hip inverse (the conjugate table; lorahip_bank.h builds both). T rows of M points, M + 1 samples apart, in place in the
// LDS; the result is left in bit-reversed order. With SUBS > 1 a row of STRIDE samples holds SUBS independent sub-rows of M points
// side by side, each transformed on its own (the 5 * 2^a banks of lorahip_pfbfft5.h); the defaults are the power-of-two banks' layout.
#pragma once
#include <hip/hip_runtime.h>

namespace lorahip {

constexpr int PFB_THREADS = 256;

//! (a - b) * w with the rounding fixed: one product, one fused multiply-add per component
__device__ __forceinline__ float2 pfbTwiddle(const float2 d, const float2 w)
{
    return make_float2(__builtin_fmaf(-d.y, w.y, d.x * w.x), __builtin_fmaf(d.y, w.x, d.x * w.y));
}

constexpr int pfbPassBits(const int left) { return (left + (left + 3) / 4 - 1) / ((left + 3) / 4); }   // ceil(left / passes left), passes of <= 4 stages

//! the stages DONE .. LOGM - 1 of the decimation-in-frequency transform of every (sub-)row, R stages per pass: a lane takes the 2^R
//! points hs apart that those stages combine with each other
template <int LOGM, int DONE, int STRIDE = (1 << LOGM) + 1, int SUBS = 1>
__device__ __forceinline__ void pfbFft(float2 *v, const float2 *tw, const int T, const int tid)
{
    if constexpr (DONE < LOGM)
    {
        constexpr int M = 1 << LOGM, R = pfbPassBits(LOGM - DONE), P = 1 << R;
        constexpr int LOGHS = LOGM - DONE - R, HS = 1 << LOGHS;     // distance of the lane's points = half span of the pass's last stage
        constexpr int PER = M >> R;                                 // lanes a row
        for (int item = tid; item < T * SUBS * PER; item += PFB_THREADS)
        {
            const int sr = item >> (LOGM - R), w = item & (PER - 1);    // sub-row sr = t * SUBS + sub
            const int t = int(unsigned(sr) / unsigned(SUBS)), sub = sr - t * SUBS;
            const int j = w & (HS - 1), grp = w >> LOGHS;
            float2 *row = v + t * STRIDE + sub * M + (grp << (LOGHS + R)) + j;
            float2 e[P];
#pragma unroll
            for (int u = 0; u < P; u++) e[u] = row[u * HS];
#pragma unroll
            for (int rho = 0; rho < R; rho++)
            {
                const int hu = 1 << (R - 1 - rho);                  // half span of this stage in the lane's points
                const int twStep = M >> (R - rho + LOGHS);          // M / (2 * hu * HS)
#pragma unroll
                for (int u = 0; u < P; u++)
                {
                    if (u & hu) continue;
                    const float2 x = e[u], y = e[u + hu];
                    e[u] = make_float2(x.x + y.x, x.y + y.y);
                    e[u + hu] = pfbTwiddle(make_float2(x.x - y.x, x.y - y.y), tw[(j + (u & (hu - 1)) * HS) * twStep]);
                }
            }
#pragma unroll
            for (int u = 0; u < P; u++) row[u * HS] = e[u];
        }
        __syncthreads();
        pfbFft<LOGM, DONE + R, STRIDE, SUBS>(v, tw, T, tid);
    }
}

} // namespace lorahip
