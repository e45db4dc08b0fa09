// fmha_append.hip — append new K/V rows to a (paged) KV cache with optional rotary embedding,
// the KV-cache write step of `mha_fwd_kvcache`.
//
// The reference validates k/v/rotary arguments (export.cpp:1585-1669) and its kernel has the
// append + rotary code (flash_fwd_kernel_hip.h:817-934, rotary_hip.h:21-152), but its C path
// never enables it (csrc/paged_attn.cpp:513-525 forces rotary_dim 0, knew_ptr unset).  Here it
// is a separate, HBM-bound pass in front of the attention:
//
//   pos = cache_seqlens[b] + j                       (j < seqlen_new)
//   kcache[page(b, pos)][pos % page][h] = rotary(knew[b][j][h], pos)
//   vcache[...same slot...]             = vnew[b][j][h]
//   q_out[b][s][h]  = rotary(q[b][s][h], cache_seqlens[b] + (per_token ? s : 0))
//   seqlens_out[b]  = cache_seqlens[b] + seqlen_new
//
// rotary(x, pos) over the first `rdim` elements (cos/sin [seqlen_ro][rdim/2]):
//   non-interleaved (GPT-NeoX): x1 = x[i], x2 = x[i + rdim/2]  -> (x1 c - x2 s, x1 s + x2 c)
//   interleaved (GPT-J):        x1 = x[2i], x2 = x[2i + 1]      -> same, with c = cos[pos][i]
// computed in fp32 and rounded once.  One thread owns 8 output elements (16 bytes); in the
// non-interleaved case a thread of the first half also writes the partner chunk.
//
// An fp8 cache (fmha_kvcache_append_fp8; cache element type uint8_t = OCP e4m3fn bytes): the
// fp32 value (K after its rotary, V as read) is multiplied by 1 / k_scale or 1 / v_scale,
// clamped to +-448 and rounded once to e4m3 (no 16-bit step in between), 8 bytes per store.
//
// The fp8 latent cache of the MLA decode has an append of its own (fmha_mla_cache_append_fp8,
// below): rows of 656 bytes with a scale per 128 features, through a slot_mapping.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_launch.h"

namespace xfa {


template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&x)[8]) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    const T8 v = *reinterpret_cast<const T8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (float)v[i];
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&x)[8]) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    T8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (T)x[i];
    *reinterpret_cast<T8*>(p) = v;
}

// 8 fp32 values x inv -> 8 e4m3fn bytes (v_cvt_pk_fp8_f32: round to nearest even), one store
__device__ __forceinline__ void store8(uint8_t* p, const float (&x)[8], const float inv) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = x[i] * inv;
        f[i] = v < -448.f ? -448.f : (v > 448.f ? 448.f : v);
    }
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *reinterpret_cast<u32x2*>(p) = u32x2{(unsigned)lo, (unsigned)hi};
}
// (a cache in q's dtype: no scale)
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&x)[8], const float) { store8(p, x); }

// rotate-and-store one row (8 elements per thread; chunk c of the row); C: the destination's
// element type (T, or uint8_t for an fp8 cache, then scaled by inv)
template <typename T, typename C>
__device__ __forceinline__ void rotate_row(const AppendParams& p, const T* src, C* dst, int c,
                                           int pos, const float inv) {
    const int e0 = 8 * c;
    if (e0 >= p.d) return;
    const T* cs = reinterpret_cast<const T*>(p.cos) + (int64_t)pos * (p.rdim / 2);
    const T* sn = reinterpret_cast<const T*>(p.sin) + (int64_t)pos * (p.rdim / 2);
    float x[8];
    load8(src + e0, x);
    if (e0 >= p.rdim) {                 // past the rotary part: copy
        store8(dst + e0, x, inv);
        return;
    }
    if (p.interleaved) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float c0 = (float)cs[e0 / 2 + i], s0 = (float)sn[e0 / 2 + i];
            const float x1 = x[2 * i], x2 = x[2 * i + 1];
            x[2 * i] = x1 * c0 - x2 * s0;
            x[2 * i + 1] = x1 * s0 + x2 * c0;
        }
        store8(dst + e0, x, inv);
        return;
    }
    const int half = p.rdim / 2;
    if (e0 >= half) return;             // written by the partner thread of the first half
    float y[8];
    load8(src + e0 + half, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float c0 = (float)cs[e0 + i], s0 = (float)sn[e0 + i];
        const float x1 = x[i], x2 = y[i];
        x[i] = x1 * c0 - x2 * s0;
        y[i] = x1 * s0 + x2 * c0;
    }
    store8(dst + e0, x, inv);
    store8(dst + e0 + half, y, inv);
}

// rows [0, n_kv) are new K/V rows (b, j, hk); rows [n_kv, n_kv + n_q) are q rows (b, s, h)
template <typename T, typename C>
__global__ void __launch_bounds__(256) fmha_append_kernel(const AppendParams p) {
    constexpr bool kFp8 = !std::is_same<T, C>::value;
    const int cpr = p.d / 8;                           // 16-byte chunks per row
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / cpr;
    const int c = (int)(t - row * cpr);
    const int64_t n_kv = (int64_t)p.b * p.snew * p.hk;
    const int64_t n_q = p.rdim > 0 ? (int64_t)p.b * p.sq * p.h : 0;
    if (t < p.b && p.seqlens_out) p.seqlens_out[t] = p.cache_seqlens[t] + p.snew;
    if (row < n_kv) {
        const int hki = (int)(row % p.hk);
        const int64_t bj = row / p.hk;
        const int j = (int)(bj % p.snew);
        const int bi = (int)(bj / p.snew);
        const int pos = p.cache_seqlens[bi] + j;
        // a slot past the block table's row (cache full) is dropped, never written into
        // another sequence's page
        if (pos < 0 || pos / p.page >= p.bt_stride) return;
        const int pg = p.block_table[(int64_t)bi * p.bt_stride + pos / p.page];
        const int64_t slot = (int64_t)pg * p.page_stride + (int64_t)(pos % p.page) * p.row_stride +
                             (int64_t)hki * p.head_stride;
        const int64_t src = (int64_t)bi * p.kn_batch + (int64_t)j * p.kn_row + (int64_t)hki * p.kn_head;
        const T* kn = reinterpret_cast<const T*>(p.knew) + src;
        const T* vn = reinterpret_cast<const T*>(p.vnew) + src;
        C* kc = reinterpret_cast<C*>(p.kcache) + slot;
        C* vc = reinterpret_cast<C*>(p.vcache) + slot;
        if (8 * c < p.d) {
            typedef __attribute__((ext_vector_type(8))) T T8;
            if constexpr (kFp8) {
                float x[8];
                load8(vn + 8 * c, x);
                store8(vc + 8 * c, x, p.v_inv);
                if (p.rdim > 0) {
                    rotate_row<T, C>(p, kn, kc, c, pos, p.k_inv);
                } else {
                    load8(kn + 8 * c, x);
                    store8(kc + 8 * c, x, p.k_inv);
                }
            } else {
                *reinterpret_cast<T8*>(vc + 8 * c) = *reinterpret_cast<const T8*>(vn + 8 * c);
                if (p.rdim > 0) rotate_row<T, C>(p, kn, kc, c, pos, 1.f);
                else *reinterpret_cast<T8*>(kc + 8 * c) = *reinterpret_cast<const T8*>(kn + 8 * c);
            }
        }
    } else if (row < n_kv + n_q) {
        const int64_t r = row - n_kv;
        const int hi = (int)(r % p.h);
        const int64_t bs = r / p.h;
        const int s = (int)(bs % p.sq);
        const int bi = (int)(bs / p.sq);
        const int pos = p.cache_seqlens[bi] + (p.q_per_token ? s : 0);
        const int64_t off = (int64_t)bi * p.q_batch + (int64_t)s * p.q_row + (int64_t)hi * p.q_head;
        rotate_row<T, T>(p, reinterpret_cast<const T*>(p.q) + off, reinterpret_cast<T*>(p.q_out) + off, c, pos, 1.f);
    }
}

hipError_t launch_append(const AppendParams& p, bool fp16, hipStream_t st) {
    const int cpr = p.d / 8;
    const int64_t rows = (int64_t)p.b * p.snew * p.hk + (p.rdim > 0 ? (int64_t)p.b * p.sq * p.h : 0);
    const int64_t threads = rows * cpr > p.b ? rows * cpr : p.b;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (p.cache_fp8) {
        if (fp16) hipLaunchKernelGGL((fmha_append_kernel<_Float16, uint8_t>), dim3(blocks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((fmha_append_kernel<__bf16, uint8_t>), dim3(blocks), dim3(256), 0, st, p);
    } else {
        if (fp16) hipLaunchKernelGGL((fmha_append_kernel<_Float16, _Float16>), dim3(blocks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((fmha_append_kernel<__bf16, __bf16>), dim3(blocks), dim3(256), 0, st, p);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- fp8 latent cache append
// fmha_mla_cache_append_fp8: one wave per token, one pass.  Lane l holds latent features 8 l .. +7,
// so the 16 lanes l / 16 == g hold the 128-feature group g: amax by a butterfly over them,
// descale = amax / 448 (1 where amax == 0), bytes = e4m3(clamp(x * (1 / descale))) - the words of
// fmha_quantize_fp8 at a finer grain.  The row (656 bytes: 512 e4m3, 4 fp32 descales, the 64
// rotary features as they come) is written whole or, for a slot outside the cache, not at all.
template <typename T>
__global__ void __launch_bounds__(256) fmha_mla_append_fp8_kernel(const MlaAppendParams p) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.tokens) return;
    const int64_t slot = p.slot[t];
    if (slot < 0 || slot >= p.slots) return;
    uint8_t* row = reinterpret_cast<uint8_t*>(p.cache) + slot * 656;
    float x[8];
    load8(reinterpret_cast<const T*>(p.latent) + (int64_t)t * p.latent_row + 8 * lane, x);
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float descale = m == 0.f ? 1.f : m / 448.f;
    store8(row + 8 * lane, x, 1.f / descale);
    if ((lane & 15) == 0) *reinterpret_cast<float*>(row + 512 + 4 * (lane >> 4)) = descale;
    if (lane < 8)
        *reinterpret_cast<T8*>(row + 528 + 16 * lane) =
            *reinterpret_cast<const T8*>(reinterpret_cast<const T*>(p.k_pe) + (int64_t)t * p.pe_row + 8 * lane);
}

hipError_t launch_mla_append_fp8(const MlaAppendParams& p, bool fp16, hipStream_t st) {
    if (p.tokens <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.tokens + 3) / 4));
    if (fp16) hipLaunchKernelGGL(fmha_mla_append_fp8_kernel<_Float16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(fmha_mla_append_fp8_kernel<__bf16>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- causal ALiBi LSE ------
__global__ void __launch_bounds__(256) fmha_lse_alibi_kernel(const LseAlibiParams p) {
    const int bh = blockIdx.x;
    const int bidx = bh / p.h, head = bh - bidx * p.h;
    int q_off = 0, sq = p.seqlen_q, sk = p.seqlen_k;
    if (p.cu_seqlens_q) { q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off; }
    if (p.cu_seqlens_k) sk = p.cu_seqlens_k[bidx + 1] - p.cu_seqlens_k[bidx];
    if (p.seqused_k) sk = p.seqused_k[bidx];
    if (p.leftpad_k) sk -= p.leftpad_k[bidx];
    const int pos = blockIdx.y * 256 + threadIdx.x;
    if (pos >= sq) return;
    const float slope = p.alibi[bidx * p.alibi_bstride + head];
    const int64_t i = (int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + q_off + pos;
    const float x = p.src[i];
    p.dst[i] = isfinite(x) ? x + p.sign * slope * (float)(pos + sk - sq) : x;
}

hipError_t launch_lse_alibi(const LseAlibiParams& p, hipStream_t st) {
    const int max_sq = p.seqlen_q;     // (varlen: max_seqlen_q)
    if (max_sq <= 0 || p.b * p.h <= 0) return hipSuccess;
    hipLaunchKernelGGL(fmha_lse_alibi_kernel, dim3(p.b * p.h, (max_sq + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- attention-sink post-pass
// One thread per 16-byte chunk of an O row, d / 8 threads per (row, head), 256 / (d / 8) rows per
// workgroup; the row's LSE and sink[head] are one address for all of its threads (one request per
// wave).  fp32 arithmetic, rounded once to T.  The barrier orders every read of a row's LSE
// before its one write (the threads of a row may sit in two waves when d / 8 does not divide 64).
template <typename T>
__global__ void __launch_bounds__(256) fmha_sink_kernel(const SinkPassParams p) {
    const int cpr = p.d >> 3, rpb = 256 / cpr;
    const int t = threadIdx.x, ri = t / cpr, c = t - ri * cpr;
    const int64_t rh = (int64_t)blockIdx.x * rpb + ri;
    const bool ok = ri < rpb && rh < (int64_t)p.b * p.rows * p.h;
    float l0 = INFINITY, s = 0.f;
    int64_t li = 0;
    T* orow = nullptr;
    if (ok) {
        const int head = (int)(rh % p.h);
        const int64_t r = rh / p.h;
        const int64_t bi = r / p.rows, pos = r - bi * p.rows;
        li = bi * p.lse_batch + (int64_t)head * p.lse_head + pos;
        orow = reinterpret_cast<T*>(p.o) + bi * p.o_batch + pos * p.o_row + (int64_t)head * p.o_head;
        l0 = p.lse[li];
        s = p.sink[head];
    }
    __syncthreads();
    if (!ok || l0 == INFINITY) return;       // no visible key: O = 0 and LSE = +inf stay
    const SinkMerge sm = sink_merge(l0, s);
    if (c == 0) p.lse[li] = sm.lse;
    if (sm.f == 1.f) return;                 // (a sink of -inf leaves O untouched)
    float x[8];
    load8(orow + 8 * c, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] *= sm.f;
    store8(orow + 8 * c, x);
}

hipError_t launch_sink_pass(const SinkPassParams& p, bool fp16, hipStream_t st) {
    const int rpb = 256 / (p.d / 8);
    const int64_t rh = (int64_t)p.b * p.rows * p.h;
    if (rh <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rh + rpb - 1) / rpb));
    if (fp16) hipLaunchKernelGGL(fmha_sink_kernel<_Float16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(fmha_sink_kernel<__bf16>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace xfa
