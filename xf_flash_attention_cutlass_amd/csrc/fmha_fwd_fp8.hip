// fmha_fwd_fp8.hip — launches of the fp8 (e4m3fn) Q/K/V forward (fmha_fwd_fp8_kernel.h), D = 128,
// bf16 or fp16 output; the item schedules are planned by plan_fwd and walked by fwd_walk.
#include <algorithm>

#include "fmha_fwd_fp8_kernel.h"
#include "fmha_fwd8w_kernel.h"
#if XFA_VARIANTS
#include "fmha_fwd8pp_kernel.h"   // (fp8_w4 = 2: the variants build only, build.py --variants)
#endif
#include "fmha_launch.h"

namespace xfa {

// 4-wave fp8 forward (fmha_fwd8w_kernel.h): no left window (the 8-wave kernel's masked loop
// handles those).  VARLEN: the instantiation that reads cu_seqlens / seqused_k (a dense launch
// runs the one without, whose code the packed path does not touch).  DSC, here and below: the
// instantiation that reads its items' descales from device tensors (the _ex entries; a by-value
// launch runs the one without)
template <bool F16, bool VARLEN, bool DSC>
static hipError_t launch_fp8_w4(const FwdParams& p, hipStream_t st) {
    allow_lds<fmha_fwd8w_kernel<F16, VARLEN, DSC>>(p.device, kFwd8wSmem);
    return launch_planned("fmha_fwd8w_kernel", fmha_fwd8w_kernel<F16, VARLEN, DSC>,
                          plan_fwd(p, kFwd8wRows, p.num_cus, 1, kFwd8wQueue), 256, kFwd8wSmem, st);
}

#if XFA_VARIANTS
// 8-wave ping-pong fp8 forward (fmha_fwd8pp_kernel.h): the same items, schedules, eligibility
template <bool F16, bool DSC>
static hipError_t launch_fp8_pp(const FwdParams& p, hipStream_t st) {
    allow_lds<fmha_fwd8pp_kernel<F16, DSC>>(p.device, kFwd8ppSmem);
    return launch_planned("fmha_fwd8pp_kernel", fmha_fwd8pp_kernel<F16, DSC>,
                          plan_fwd(p, kFwd8ppRows, p.num_cus, 1, kFwd8ppQueue), 512, kFwd8ppSmem, st);
}
#endif

// 8-wave fp8 forward.  Its schedules differ from the other launchers': a dense launch never
// takes the dynamic queue (static schedules only, whatever fwd_dyn says), and a packed one with
// the item counter follows the ragged rule (plan_fwd, kQueueRagged: more items than CUs =>
// mode 3 on min(items, slots) workgroups, never per-XCD queues).
template <typename T, bool VARLEN, bool DSC>
static hipError_t launch_fp8_t(const FwdParams& p, hipStream_t st) {
    constexpr int NW = 8;
    const bool mask = p.wl >= 0 || p.wr >= 0;
    const FwdPlan s = plan_fwd(p, NW * 32, p.num_cus * p.persist_per_cu, 1,
                               p.work_ctr ? kFwdFp8Queue<VARLEN> : kQueueStatic);
    const size_t smem = 8 * (size_t)kFp8Tile;     // K and V, four buffers each
    allow_lds<fmha_fwd_fp8_kernel<T, NW, true, VARLEN, DSC>, fmha_fwd_fp8_kernel<T, NW, false, VARLEN, DSC>>(p.device, (int)smem);
    return launch_planned("fmha_fwd_fp8_kernel<8 waves>",
                          mask ? fmha_fwd_fp8_kernel<T, NW, true, VARLEN, DSC> : fmha_fwd_fp8_kernel<T, NW, false, VARLEN, DSC>,
                          s, NW * 64, smem, st);
}

template <bool DSC>
static hipError_t launch_fwd_fp8_t(const FwdParams& p, bool out_fp16, hipStream_t st) {
#if XFA_VARIANTS
    // (the ping-pong kernel's prologue is dense only: a varlen launch goes to the 4-wave kernel)
    if (p.fwd4 == 2 && !p.cu_seqlens_q && p.k_row == p.v_row && (p.wl < 0 || p.wl >= p.seqlen_k))
        return out_fp16 ? launch_fp8_pp<true, DSC>(p, st) : launch_fp8_pp<false, DSC>(p, st);
#endif
    const bool w4 = p.fwd4 && p.k_row == p.v_row && (p.wl < 0 || p.wl >= p.seqlen_k);
    if (p.cu_seqlens_q) {
        if (w4) return out_fp16 ? launch_fp8_w4<true, true, DSC>(p, st) : launch_fp8_w4<false, true, DSC>(p, st);
        return out_fp16 ? launch_fp8_t<_Float16, true, DSC>(p, st) : launch_fp8_t<__bf16, true, DSC>(p, st);
    }
    if (w4) return out_fp16 ? launch_fp8_w4<true, false, DSC>(p, st) : launch_fp8_w4<false, false, DSC>(p, st);
    return out_fp16 ? launch_fp8_t<_Float16, false, DSC>(p, st) : launch_fp8_t<__bf16, false, DSC>(p, st);
}

hipError_t launch_fwd_fp8(const FwdParams& p, bool out_fp16, hipStream_t st) {
    return p.q_descale ? launch_fwd_fp8_t<true>(p, out_fp16, st) : launch_fwd_fp8_t<false>(p, out_fp16, st);
}

}  // namespace xfa

#ifdef XFA_FWD8_STAMPS
// diagnostic builds only: copy out (and optionally clear) the 4-wave fp8 phase stamps
extern "C" int fmha_fwd8_stamps(unsigned long long* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(xfa::g_fwd8_stamps), sizeof(xfa::g_fwd8_stamps)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[4 * 8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(xfa::g_fwd8_stamps), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
