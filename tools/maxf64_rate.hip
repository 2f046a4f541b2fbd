// issue rate of v_max_f64 against v_pk_mul_f32 / v_pk_add_f32 / v_cndmask_b32 / v_cmp_gt_f32 + v_cndmask_b32 (run on the GPU):
// what one key maximum of the bin scan (lorahip_device.h, laneScanKeys) costs beside the compare-and-select it replaces.
//   hipcc --offload-arch=gfx950 -O3 tools/maxf64_rate.hip -o maxf64_rate && ./maxf64_rate
// Every kernel runs 64 instructions per loop round on CHAINS accumulators: CHAINS = 1 is one dependent chain (latency), CHAINS = 8
// eight independent ones (issue rate). Cycles are the wavefront's own shader clock (s_memtime) over its loop, per instruction; with
// W wavefronts on a SIMD the SIMD's issue cost of one instruction is that figure / W.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float v2f __attribute__((ext_vector_type(2)));
enum { MAXF64, PKMUL, PKADD, CNDMASK, CMPSEL, NOPS };
static const char *kNames[NOPS] = { "v_max_f64", "v_pk_mul_f32", "v_pk_add_f32", "v_cndmask_b32", "v_cmp_gt_f32 + v_cndmask_b32 (2 instr)" };

template <int OP, int CHAINS>
__global__ __launch_bounds__(256) void k(unsigned long long *cyc, float *out, const float *in, const int iters)
{
    double d[CHAINS];
    v2f p[CHAINS];
    float f[CHAINS];
    for (int i = 0; i < CHAINS; i++)
    {
        d[i] = (double)in[i] + threadIdx.x;
        p[i] = (v2f){in[i], in[i + 1]};
        f[i] = in[i + 2];
    }
    const double dx = (double)in[9] + (threadIdx.x & 7);
    const v2f px = {in[5], in[6]};                                      // 1.0f: the chain's values stay finite
    const float fx = in[7];
    const unsigned long long mask = 0x5555555555555555ull + (unsigned long long)(iters & 1);
    const unsigned long long t0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int it = 0; it < iters; it++)
    {
#pragma unroll
        for (int u = 0; u < 64; u++)
        {
            const int i = u % CHAINS;
            if (OP == MAXF64) asm volatile("v_max_f64 %0, %0, %1" : "+v"(d[i]) : "v"(dx));
            if (OP == PKMUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[i]) : "v"(px));
            if (OP == PKADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(p[i]) : "v"(px));
            if (OP == CNDMASK) asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(f[i]) : "v"(fx), "s"(mask));
            if (OP == CMPSEL) asm volatile("v_cmp_gt_f32_e32 vcc, %1, %0\n\tv_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(f[i]) : "v"(fx) : "vcc");
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    float s = 0;
    for (int i = 0; i < CHAINS; i++) s += (float)d[i] + p[i].x + p[i].y + f[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0)
    {
        cyc[2 * (blockIdx.x * 4 + (threadIdx.x >> 6))] = t1 - t0;
        cyc[2 * (blockIdx.x * 4 + (threadIdx.x >> 6)) + 1] = w1 - w0;
    }
}

template <int OP, int CHAINS>
static void run(unsigned long long *cyc, float *out, const float *in, const int wavesPerSimd)
{
    const int iters = 20000, blocks = 256 * wavesPerSimd;         // 256 CUs x (4 wavefronts per block = 1 per SIMD) x wavesPerSimd
    k<OP, CHAINS><<<blocks, 256>>>(cyc, out, in, 200);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a);
    k<OP, CHAINS><<<blocks, 256>>>(cyc, out, in, iters);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    std::vector<unsigned long long> h(size_t(blocks) * 8);
    hipMemcpy(h.data(), cyc, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost);
    double c = 0, w = 0;
    for (size_t i = 0; i < h.size(); i += 2) { c += double(h[i]); w += double(h[i + 1]); }
    const double n = double(iters) * 64, waves = double(h.size() / 2);
    const double perWave = c / waves / n;
    printf("%-40s chains %d, %d waves/SIMD: %7.3f ms, %6.2f clk per instr per wave, %6.2f clk of the SIMD per instr (clock %.2f GHz)\n",
           kNames[OP], CHAINS, wavesPerSimd, ms, perWave, perWave / wavesPerSimd, c / w * 0.1);
    hipEventDestroy(a); hipEventDestroy(b);
}

int main()
{
    float *in, *out;
    unsigned long long *cyc;
    hipMalloc(&in, 4096); hipMalloc(&out, 256 * 4 * 256 * 4); hipMalloc(&cyc, 256 * 4 * 8 * sizeof(unsigned long long));
    float h[64];
    for (int i = 0; i < 64; i++) h[i] = 1.0f + 1.0f / (i + 3);
    h[5] = h[6] = 1.0f;
    hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice);
    for (int w : {1, 3})
    {
        run<MAXF64, 1>(cyc, out, in, w); run<MAXF64, 8>(cyc, out, in, w);
        run<PKMUL, 1>(cyc, out, in, w); run<PKMUL, 8>(cyc, out, in, w);
        run<PKADD, 1>(cyc, out, in, w); run<PKADD, 8>(cyc, out, in, w);
        run<CNDMASK, 1>(cyc, out, in, w); run<CNDMASK, 8>(cyc, out, in, w);
        run<CMPSEL, 1>(cyc, out, in, w); run<CMPSEL, 8>(cyc, out, in, w);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
