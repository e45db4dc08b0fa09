// fmha_mla_index_topk_split.hip — the MLA indexer's top-k selection with every row split over
// several workgroups (fmha_mla_index_topk_split): fmha_mla_index_topk_part_kernel,
// one workgroup per (row, chunk), then fmha_mla_index_topk_merge_kernel, one per row
// (fmha_mla_index_topk_split_kernel.h).  A translation unit of its own: the code objects of the
// other kernels stay as they are.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_mla_index_topk_split_kernel.h"

namespace xfa {

hipError_t launch_mla_index_topk_split(const MlaIndexTopkSplitParams& p, hipStream_t st) {
    if (p.rows <= 0) return hipSuccess;
    allow_lds<fmha_mla_index_topk_part_kernel, fmha_mla_index_topk_merge_kernel>(p.device, topk_split_lds_bytes(kMlaTopkStage));
    // LDS of a chunk: none where no chunk can be longer than topk
    const int keep = p.chunk > p.topk ? p.chunk : 0;
    const dim3 parts((unsigned)((int64_t)p.rows * p.splits)), rows((unsigned)p.rows), block(kTopkSplitThreads);
    hipLaunchKernelGGL(fmha_mla_index_topk_part_kernel, parts, block, topk_split_lds_bytes(keep), st, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    note_launch("fmha_mla_index_topk_merge_kernel", 0, 0, rows.x, rows.y, rows.z, kTopkSplitThreads);
    hipLaunchKernelGGL(fmha_mla_index_topk_merge_kernel, rows, block, topk_split_lds_bytes(p.splits * p.topk), st, p);
    return hipGetLastError();
}

}  // namespace xfa
