// fmha_fwd_mla.hip — the MLA prefill forward (head size 192 for Q K^T, 128 for V) for one dtype.
// Compiled once per dtype with -DXFA_DTN=<bf16|f16> (see build.py): a translation unit of its
// own, so the code objects of the other forwards stay as they are.
#include "fmha_fwd_mla_kernel.h"
#include "fmha_launch.h"

#define XFA_CAT2(a, b) a##b
#define XFA_CAT(a, b) XFA_CAT2(a, b)

namespace xfa {

#if XFA_DT_BF16
typedef __bf16 elem_t;
#else
typedef _Float16 elem_t;
#endif

// 8 waves x 32 rows: 256-row items, two waves per SIMD
#ifndef XFA_MLA_WAVES
#define XFA_MLA_WAVES 8
#endif
constexpr int kFwdMlaWaves = XFA_MLA_WAVES;

hipError_t XFA_CAT(launch_fwd_mla_, XFA_DTN)(const FwdParams& p, hipStream_t st) {
    constexpr int NW = kFwdMlaWaves;
    const bool mask = p.wl >= 0 || p.wr >= 0;
    const FwdPlan s = plan_fwd(p, NW * 32, p.num_cus * (p.persist_per_cu > 0 ? 1 : 0), 1, kFwdMlaQueue);
    allow_lds<fmha_fwd_mla_kernel<elem_t, NW, true>, fmha_fwd_mla_kernel<elem_t, NW, false>>(p.device, kMlaSmem);
    return launch_planned("fmha_fwd_mla_kernel", mask ? fmha_fwd_mla_kernel<elem_t, NW, true> : fmha_fwd_mla_kernel<elem_t, NW, false>,
                          s, NW * 64, kMlaSmem, st);
}

}  // namespace xfa
