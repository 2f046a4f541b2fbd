// LDS per workgroup of the SF11 / SF12 streaming kernels and what it allows per compute unit (host program; no GPU needed):
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -ffp-contract=off -Ilora_sdr_amd/csrc -Iinclude -x hip tools/lds_budget.hip -o /tmp/lds_budget && /tmp/lds_budget
#include "lorahip_widecore.h"
#include "lorahip_residentproto.h"
#include <cstdio>
using namespace lorahip;
template <class C> static void wide(const char *name)
{
    typedef typename WideSmem<C>::Stream S;
    const size_t smem = WideSmem<C>::streamBytes();
    printf("%-14s threads %4d  LDS per workgroup %6zu B = exchange %6zu + stage twiddles %6zu + split fine-tune tables %6zu + rest %zu -> %d workgroups per CU by LDS (160 KiB) = %d wavefronts per SIMD; resident receiver %zu B\n",
           name, C::T, smem, sizeof(S::x), sizeof(S::tw), size_t(FineDims<C::LOG2N>::BYTES),
           sizeof(S) - sizeof(S::x) - sizeof(S::tw), int(163840 / smem), int(163840 / smem) * (C::T / 64) / 4, WideSmem<C>::streamBytes(sizeof(ResLds)));
}
int main()
{
    wide<StreamWide11>("StreamWide11");
    wide<StreamWide12>("StreamWide12");
    return 0;
}
