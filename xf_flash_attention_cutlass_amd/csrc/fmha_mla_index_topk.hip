// fmha_mla_index_topk.hip — the MLA indexer's top-k selection (fmha_mla_index_topk; DESIGN.md
// §3.13.1): one launch of fmha_mla_index_topk_kernel (fmha_mla_index_topk_kernel.h), one workgroup
// per logits row.  A translation unit of its own: the code objects of the other kernels stay as
// they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fmha_mla_index_topk_kernel.h"

namespace xfa {

hipError_t launch_mla_index_topk(const MlaIndexTopkParams& p, hipStream_t st) {
    if (p.rows <= 0) return hipSuccess;
    allow_lds<fmha_mla_index_topk_kernel>(p.device, topk_lds_bytes(kMlaTopkStage));
    // LDS for the longest row this launch can stage: none where no row can be longer than topk
    const int keep = p.max_seqlen_k > p.topk ? std::min(p.max_seqlen_k, kMlaTopkStage) : 0;
    const dim3 grid((unsigned)p.rows), block(kTopkThreads);
    note_launch("fmha_mla_index_topk_kernel", 0, 0, grid.x, grid.y, grid.z, kTopkThreads);
    hipLaunchKernelGGL(fmha_mla_index_topk_kernel, grid, block, topk_lds_bytes(keep), st, p);
    return hipGetLastError();
}

}  // namespace xfa
