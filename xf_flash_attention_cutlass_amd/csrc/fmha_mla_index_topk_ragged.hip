// fmha_mla_index_topk_ragged.hip — the MLA indexer's top-k selection for prefill rows
// (fmha_mla_index_topk_ragged): one launch of fmha_mla_index_topk_ragged_kernel
// (fmha_mla_index_topk_ragged_kernel.h), one workgroup of 4 waves per logits row.  A translation
// unit of its own: the code objects of the other kernels stay as they are.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_mla_index_topk_ragged_kernel.h"

namespace xfa {

hipError_t launch_mla_index_topk_ragged(const MlaIndexTopkRaggedParams& p, hipStream_t st) {
    if (p.rows <= 0) return hipSuccess;
    MlaIndexTopkRaggedParams q = p;
    // LDS for what a row of this launch can need: no histogram and no list where none is longer than topk
    q.cap = ragtopk_cap(p.keys, p.topk);
    const dim3 grid((unsigned)p.rows), block(kMlaTopkRaggedThreads);
    note_launch("fmha_mla_index_topk_ragged_kernel", 0, 0, grid.x, grid.y, grid.z, kMlaTopkRaggedThreads);
    hipLaunchKernelGGL(fmha_mla_index_topk_ragged_kernel, grid, block, ragtopk_lds_bytes(p.keys, p.topk), st, q);
    return hipGetLastError();
}

}  // namespace xfa
