// fmha_mla_index_ragged.hip — the MLA indexer's prefill logits (fmha_mla_index_logits_ragged;
// DESIGN.md §3.13.2): one launch of fmha_mla_index_ragged_kernel (fmha_mla_index_ragged_kernel.h).
// A translation unit of its own: the code objects of the other indexer kernels stay as they are.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_mla_index_ragged_kernel.h"

namespace xfa {

template <int HEADS>
static hipError_t launch_ragged_t(const MlaIndexRaggedParams& p, hipStream_t st, const char* name) {
    constexpr int NP = kRagRowsPerWave, THREADS = 64 * (kMlaRaggedRows / NP);
    const int chunks = (p.n + kMlaRaggedChunk - 1) / kMlaRaggedChunk;
    const dim3 grid((unsigned)((int64_t)p.row_blocks * chunks)), block(THREADS);
    if (grid.x == 0) return hipSuccess;
    note_launch(name, 0, 0, grid.x, grid.y, grid.z, THREADS);
    hipLaunchKernelGGL((fmha_mla_index_ragged_kernel<HEADS, NP>), grid, block, 0, st, p);
    return hipGetLastError();
}

hipError_t launch_mla_index_logits_ragged(const MlaIndexRaggedParams& p, hipStream_t st) {
    return p.heads == 64 ? launch_ragged_t<64>(p, st, "fmha_mla_index_ragged_kernel<64>")
                         : launch_ragged_t<32>(p, st, "fmha_mla_index_ragged_kernel<32>");
}

}  // namespace xfa
