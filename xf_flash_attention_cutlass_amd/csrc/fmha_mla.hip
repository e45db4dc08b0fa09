// fmha_mla.hip — MLA decode over a paged latent cache (fmha_mla_decode): the decode kernel
// (fmha_mla_decode_kernel.h) for bf16 and fp16, its twin over an fp8 latent cache
// (fmha_mla_decode_fp8, fmha_mla_decode_fp8_kernel.h), the two over index-selected tokens
// (fmha_mla_decode_sparse[_fp8], fmha_mla_decode_sparse[_fp8]_kernel.h), and the split combine at head size 512
// (fmha_combine_kernel<512, T>, the forward's template, instantiated here).  A translation unit of
// its own: the kernels run one wave per SIMD with 147,456 B of LDS, unlike anything in
// fmha_fwd.hip.
#include "fmha_fwd_kernel.h"
#include "fmha_mla_decode_kernel.h"
#include "fmha_mla_decode_fp8_kernel.h"
#include "fmha_mla_decode_sparse_kernel.h"
#include "fmha_mla_decode_sparse_fp8_kernel.h"
#include "fmha_launch.h"

namespace xfa {

// kernel: fmha_mla_decode_kernel<T>, fmha_mla_decode_fp8_kernel<T> or one of their sparse twins
template <typename T, void (*kernel)(const MlaParams), int kSmem>
static hipError_t launch_mla_t(const MlaParams& p, hipStream_t st, const char* tiles, const char* splits) {
    allow_lds<kernel>(p.device, kSmem);
    const int64_t items = (int64_t)p.b * p.num_splits * p.row_tiles;
    const dim3 grid((unsigned)((items + kMlaWaves - 1) / kMlaWaves));
    // the mapping: the waves of a workgroup are row tiles of one (batch, split), or key splits
    note_launch(p.row_tiles > 1 ? tiles : splits, 0, 0, grid.x, grid.y, grid.z, kMlaWaves * 64);
    hipLaunchKernelGGL(kernel, grid, dim3(kMlaWaves * 64), kSmem, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.num_splits <= 1) return e;
    CombineParams cp{};
    cp.oaccum = p.oaccum;
    cp.lseaccum = p.lseaccum;
    cp.o = p.o;
    cp.lse = p.lse;
    cp.o_batch = p.o_batch; cp.o_row = p.o_row; cp.o_head = p.o_head;
    cp.lse_batch = (int64_t)p.h * p.seqlen_q; cp.lse_head = p.seqlen_q;
    cp.b = p.b; cp.h = p.h; cp.seqlen_q = p.seqlen_q; cp.d = kMlaDV; cp.hd = kMlaDV;
    cp.num_splits = p.num_splits;
    const int64_t crow = (int64_t)p.b * p.h * p.seqlen_q;
    hipLaunchKernelGGL((fmha_combine_kernel<kMlaDV, T>), dim3((unsigned)((crow + 3) / 4)), dim3(256), 0, st, cp);
    return hipGetLastError();
}

hipError_t launch_mla_decode(const MlaParams& p, bool fp16, hipStream_t st) {
    const char *tiles = "fmha_mla_decode_kernel<tiles>", *splits = "fmha_mla_decode_kernel<splits>";
    return fp16 ? launch_mla_t<_Float16, fmha_mla_decode_kernel<_Float16>, kMlaSmem>(p, st, tiles, splits)
                : launch_mla_t<__bf16, fmha_mla_decode_kernel<__bf16>, kMlaSmem>(p, st, tiles, splits);
}

hipError_t launch_mla_decode_fp8(const MlaParams& p, bool fp16, hipStream_t st) {
    const char *tiles = "fmha_mla_decode_fp8_kernel<tiles>", *splits = "fmha_mla_decode_fp8_kernel<splits>";
    return fp16 ? launch_mla_t<_Float16, fmha_mla_decode_fp8_kernel<_Float16>, kMlaSmem>(p, st, tiles, splits)
                : launch_mla_t<__bf16, fmha_mla_decode_fp8_kernel<__bf16>, kMlaSmem>(p, st, tiles, splits);
}

hipError_t launch_mla_decode_sparse(const MlaParams& p, bool fp8, bool fp16, hipStream_t st) {
    if (fp8) {
        const char *tiles = "fmha_mla_decode_sparse_fp8_kernel<tiles>", *splits = "fmha_mla_decode_sparse_fp8_kernel<splits>";
        return fp16 ? launch_mla_t<_Float16, fmha_mla_decode_sparse_fp8_kernel<_Float16>, kMlaSmem>(p, st, tiles, splits)
                    : launch_mla_t<__bf16, fmha_mla_decode_sparse_fp8_kernel<__bf16>, kMlaSmem>(p, st, tiles, splits);
    }
    const char *tiles = "fmha_mla_decode_sparse_kernel<tiles>", *splits = "fmha_mla_decode_sparse_kernel<splits>";
    return fp16 ? launch_mla_t<_Float16, fmha_mla_decode_sparse_kernel<_Float16>, kMlaSmem>(p, st, tiles, splits)
                : launch_mla_t<__bf16, fmha_mla_decode_sparse_kernel<__bf16>, kMlaSmem>(p, st, tiles, splits);
}

}  // namespace xfa
