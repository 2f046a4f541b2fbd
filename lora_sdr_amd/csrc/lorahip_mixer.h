// What the front-end kernels share (lorahip_chan.hip: wideband -> channels; lorahip_synth.hip: channels -> wideband): the fp32 evaluation
// of a 32-bit mixer phase and the complex multiply / multiply-add they are built from. DEVICE code only.
#pragma once
#include <hip/hip_runtime.h>

namespace lorahip {

typedef float v2f __attribute__((ext_vector_type(2)));

//! acc += g * x, complex, two packed FMAs; g is wave-uniform (SGPR pair)
__device__ __forceinline__ void cmacS(v2f &acc, const v2f g, const v2f x)
{
    asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(g), "v"(x));                   // (g.x*x.x, g.x*x.y)
    asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(acc) : "s"(g), "v"(x));    // (-g.y*x.y, g.y*x.x)
}

//! complex product with fused multiply-adds
__device__ __forceinline__ v2f cmulF(const v2f a, const v2f b)
{
    return (v2f){fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)};
}

//! e^{-2 pi i ph / 2^32}: nearest quarter turn taken out exactly, then the fp32 sine / cosine kernels on [-pi/4, pi/4]
//! (minimax polynomials, error ~1e-7); the phase bits below 2^-32 turn (1.5e-9 rad) are dropped
__device__ __forceinline__ v2f mixerPhase(const unsigned ph)
{
    const unsigned q = (ph + 0x20000000u) >> 30;                                    // quadrant 0..3 (4 wraps to 0 below)
    const float x = float(int(ph - (q << 30))) * 1.4629180792671596e-09f;           // 2 pi / 2^32
    const float z = x * x;
    const float sn = fmaf(x * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), x);
    const float cs = fmaf(z, fmaf(z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f), -0.5f), 1.0f);
    // angle = q * pi/2 + x; the result is (cos, -sin) of it
    const float c1 = (q & 1) ? -sn : cs, s1 = (q & 1) ? cs : sn;                    // cos/sin of (x + pi/2) = (-sin x, cos x)
    const bool neg = (q & 2) != 0;
    return (v2f){neg ? -c1 : c1, neg ? s1 : -s1};
}

} // namespace lorahip
