// The transform of the two polyphase banks on 5 * 2^a bins (lorahip_pfb.hip forward, lorahip_psb.hip inverse: the same code with the
// conjugate tables; lorahip_bank.h builds both): M = 5 N points, N = 2^a, a = 0..6, T rows M + 1 samples apart, in place in the LDS.
// One radix-5 decimation-in-frequency stage, then five independent radix-2 transforms of N points (lorahip_pfbfft.h with five
// sub-rows a row):
//
//     X[5 k + r] = sum_{n<N} ( W_M^(r n) sum_{q<5} x[n + N q] W_5^(r q) ) W_N^(k n)            W_P = exp(-2 pi i / P)
//
// The radix-5 stage leaves the inner sum of (r, n) at r N + n, so sub-row r holds the bins 5 k + r, k in bit-reversed order: bin
// 5 k + r stands at r N + bitrev_a(k). The table w5[n] = exp(-2 pi i n / M), n < M, computed in double on the host, holds the
// twiddles W_M^(r n) (r n < 4 N) and the constants of the 5-point transform, W_5 = w5[N] and W_5^2 = w5[2 N].
#pragma once
#include "lorahip_pfbfft.h"

namespace lorahip {

//! the 5-point transform of the points N apart of every row and the twiddles of the five sub-transforms that follow; the order of
//! every sum is fixed, every product is fused into its sum
template <int A>
__device__ __forceinline__ void pfbRadix5(float2 *v, const float2 *w5, const int T, const int tid)
{
    constexpr int N = 1 << A, M = 5 * N;
    const float2 k1 = w5[N], k2 = w5[2 * N];        // (cos, -sin) of 2 pi / 5 and of 4 pi / 5
    for (int item = tid; item < T * N; item += PFB_THREADS)
    {
        const int t = item >> A, n = item & (N - 1);
        float2 *p = v + t * (M + 1) + n;
        const float2 x0 = p[0], x1 = p[N], x2 = p[2 * N], x3 = p[3 * N], x4 = p[4 * N];
        const float2 a1 = make_float2(x1.x + x4.x, x1.y + x4.y), a2 = make_float2(x2.x + x3.x, x2.y + x3.y);
        const float2 d1 = make_float2(x1.x - x4.x, x1.y - x4.y), d2 = make_float2(x2.x - x3.x, x2.y - x3.y);
        // X[1], X[4] = m1 -+ i (s1 d1 + s2 d2) and X[2], X[3] = m2 -+ i (s2 d1 - s1 d2), s = sin = -k.y: u = -(the bracket)
        const float2 m1 = make_float2(__builtin_fmaf(k2.x, a2.x, __builtin_fmaf(k1.x, a1.x, x0.x)), __builtin_fmaf(k2.x, a2.y, __builtin_fmaf(k1.x, a1.y, x0.y)));
        const float2 m2 = make_float2(__builtin_fmaf(k1.x, a2.x, __builtin_fmaf(k2.x, a1.x, x0.x)), __builtin_fmaf(k1.x, a2.y, __builtin_fmaf(k2.x, a1.y, x0.y)));
        const float2 u1 = make_float2(__builtin_fmaf(k2.y, d2.x, k1.y * d1.x), __builtin_fmaf(k2.y, d2.y, k1.y * d1.y));
        const float2 u2 = make_float2(__builtin_fmaf(-k1.y, d2.x, k2.y * d1.x), __builtin_fmaf(-k1.y, d2.y, k2.y * d1.y));
        p[0] = make_float2(x0.x + (a1.x + a2.x), x0.y + (a1.y + a2.y));
        p[N] = pfbTwiddle(make_float2(m1.x - u1.y, m1.y + u1.x), w5[n]);
        p[2 * N] = pfbTwiddle(make_float2(m2.x - u2.y, m2.y + u2.x), w5[2 * n]);
        p[3 * N] = pfbTwiddle(make_float2(m2.x + u2.y, m2.y - u2.x), w5[3 * n]);
        p[4 * N] = pfbTwiddle(make_float2(m1.x + u1.y, m1.y - u1.x), w5[4 * n]);
    }
    __syncthreads();
}

//! T transforms of 5 * 2^A points: tw = the radix-2 table of the N-point sub-transforms (N / 2 entries), w5 as above
template <int A>
__device__ __forceinline__ void pfbFft5(float2 *v, const float2 *tw, const float2 *w5, const int T, const int tid)
{
    pfbRadix5<A>(v, w5, T, tid);
    pfbFft<A, 0, 5 * (1 << A) + 1, 5>(v, tw, T, tid);
}

} // namespace lorahip
