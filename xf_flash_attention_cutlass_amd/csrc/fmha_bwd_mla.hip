// fmha_bwd_mla.hip — the MLA prefill backward (head size 192 for Q K^T, 128 for V) for one dtype.
// Compiled once per dtype with -DXFA_DTN=<bf16|f16> (see build.py): a translation unit of its
// own, so the code objects of the other backwards stay as they are.
// Launch sequence: preprocess (D = rowsum(dO*O)) -> dK/dV -> dQ, on the caller's stream.
#include "fmha_bwd_mla_kernel.h"
#include "fmha_launch.h"

#define XFA_CAT2(a, b) a##b
#define XFA_CAT(a, b) XFA_CAT2(a, b)

namespace xfa {

#if XFA_DT_BF16
typedef __bf16 elem_t;
#else
typedef _Float16 elem_t;
#endif

// p.dsum: fp32 [like the LSE]; tokens: the query rows of the whole batch
hipError_t XFA_CAT(launch_bwd_mla_, XFA_DTN)(const BwdParams& p, int64_t tokens, hipStream_t st) {
    typedef elem_t T;
    const int total_rows = (int)(tokens * p.h);
    const unsigned blocks = (unsigned)(((int64_t)total_rows * (kBwdMlaHdv / 8) + 255) / 256);
    hipLaunchKernelGGL((fmha_bwd_mla_pre_kernel<T>), dim3(blocks), dim3(256), 0, st, p, total_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    const bool mask = p.wl >= 0 || p.wr >= 0;
    const bool packed = p.cu_seqlens_q != nullptr;
    void (*const dkdv[2][2])(const BwdParams) = {
        {fmha_bwd_mla_dkdv_kernel<T, false, false>, fmha_bwd_mla_dkdv_kernel<T, false, true>},
        {fmha_bwd_mla_dkdv_kernel<T, true, false>, fmha_bwd_mla_dkdv_kernel<T, true, true>}};
    void (*const dq[2][2])(const BwdParams) = {
        {fmha_bwd_mla_dq_kernel<T, false, false>, fmha_bwd_mla_dq_kernel<T, false, true>},
        {fmha_bwd_mla_dq_kernel<T, true, false>, fmha_bwd_mla_dq_kernel<T, true, true>}};
    allow_lds<fmha_bwd_mla_dq_kernel<T, false, false>, fmha_bwd_mla_dq_kernel<T, false, true>,
              fmha_bwd_mla_dq_kernel<T, true, false>, fmha_bwd_mla_dq_kernel<T, true, true>>(p.device, kBwdMlaDqSmem);

    const dim3 gk((p.seqlen_k + kBwdMlaBlockN - 1) / kBwdMlaBlockN, p.b * p.hk);
    hipLaunchKernelGGL(dkdv[mask][packed], gk, dim3(kBwdMlaWaves * 64), kBwdMlaDkdvSmem, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gq((p.seqlen_q + kBwdMlaBlockM - 1) / kBwdMlaBlockM, p.b * p.h);
    // the record for fmha_last_kernel(): the three kernels of the sequence, the dQ kernel's grid
    note_launch("fmha_bwd_mla_pre_kernel+fmha_bwd_mla_dkdv_kernel+fmha_bwd_mla_dq_kernel", 0, 0, gq.x, gq.y, gq.z,
                kBwdMlaWaves * 64);
    hipLaunchKernelGGL(dq[mask][packed], gq, dim3(kBwdMlaWaves * 64), kBwdMlaDqSmem, st, p);
    return hipGetLastError();
}

}  // namespace xfa
