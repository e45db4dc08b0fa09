// fmha_mla_index.hip — the MLA indexer (DeepSeek-V3.2's lightning indexer): the
// fused index logits over the paged fp8 index-key cache (fmha_mla_index_logits,
// fmha_mla_index_kernel.h) and the append into that cache (fmha_mla_index_cache_append_fp8, below).
// A translation unit of its own: the code objects of the other MLA kernels stay as they are.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_mla_index_kernel.h"
#include "fmha_row8.h"

namespace xfa {

template <int HEADS>
static hipError_t launch_index_t(const MlaIndexParams& p, hipStream_t st, const char* name) {
    const int chunks = (p.max_seqlen_k + kMlaIndexChunk - 1) / kMlaIndexChunk;
    const dim3 grid((unsigned)((int64_t)p.b * chunks)), block(kIdxWaves * 64);
    if (grid.x == 0) return hipSuccess;
    note_launch(name, 0, 0, grid.x, grid.y, grid.z, kIdxWaves * 64);
    if (p.seqlen_q == 1) hipLaunchKernelGGL((fmha_mla_index_logits_kernel<HEADS, 1, false>), grid, block, 0, st, p);
    else if (p.seqlen_q == 2) hipLaunchKernelGGL((fmha_mla_index_logits_kernel<HEADS, 2, false>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((fmha_mla_index_logits_kernel<HEADS, 2, true>), grid, block, 0, st, p);
    return hipGetLastError();
}

hipError_t launch_mla_index_logits(const MlaIndexParams& p, hipStream_t st) {
    return p.heads == 64 ? launch_index_t<64>(p, st, "fmha_mla_index_logits_kernel<64>")
                         : launch_index_t<32>(p, st, "fmha_mla_index_logits_kernel<32>");
}

// ---------------------------------------------------------------- index-key cache append
// A quarter wave per token, one pass: lane c of the 16 holds features 8 c .. +7, amax by a
// butterfly over them, then the words of fmha_mla_cache_append_fp8 with one scale for the whole
// row: descale = amax / 448 (1 where amax == 0), bytes = e4m3(clamp(x * (1 / descale))).  ue8m0:
// the descale becomes the smallest power of two >= amax / 448, at least 2^-126, on the exponent
// bits (exponent + 1 unless the mantissa is zero).  The 128 bytes and the descale of a slot
// outside the cache are not written.
template <typename T>
__global__ void __launch_bounds__(256) fmha_mla_index_append_fp8_kernel(const MlaIndexAppendParams p) {
    const int c = threadIdx.x & 15;
    const int t = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = t < p.tokens;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) load8(reinterpret_cast<const T*>(p.k) + (int64_t)t * p.k_row + 8 * c, x);
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));       // (every lane takes part)
    float descale = m == 0.f ? 1.f : m / 448.f;
    if (p.ue8m0) {
        const unsigned bits = __float_as_uint(descale);
        const unsigned e = (bits >> 23) + ((bits & 0x7fffffu) != 0);
        descale = __uint_as_float((e < 1u ? 1u : e) << 23);
    }
    if (!live) return;
    const int64_t slot = p.slot[t];
    if (slot < 0 || slot >= p.slots) return;
    const int64_t blk = slot / p.page;
    const int row = (int)(slot - blk * p.page);
    uint8_t* block = reinterpret_cast<uint8_t*>(p.cache) + blk * p.page * 132;
    store8(block + row * 128 + 8 * c, x, 1.f / descale);
    if (c == 0) *reinterpret_cast<float*>(block + (int64_t)p.page * 128 + 4 * row) = descale;
}

hipError_t launch_mla_index_append_fp8(const MlaIndexAppendParams& p, bool fp16, hipStream_t st) {
    if (p.tokens <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.tokens + 15) / 16));
    if (fp16) hipLaunchKernelGGL(fmha_mla_index_append_fp8_kernel<_Float16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(fmha_mla_index_append_fp8_kernel<__bf16>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace xfa
