/*
 * paged_attn.h — C ABI of libpaged-attention.so, MI355X (gfx950) build.
 *
 * Drop-in for the reference's public header `csrc/paged_attn.h` (installed to
 * include/ by CMakeLists.txt:78-81): the three reference entry points keep their
 * exact names, parameter order and types.  Everything else here is new.
 *
 * Conventions shared by every entry point (reference semantics):
 *   - all pointers are caller-owned DEVICE pointers on the current HIP device;
 *     tensors are contiguous: dense  [batch, seqlen, heads, head_size],
 *     varlen [total_tokens, heads, head_size], paged [num_blocks, page, heads_k, head_size];
 *   - head_size must be a multiple of 8 (callers pad, export.cpp:539-547) and <= 256;
 *   - `is_fp16 == false` means bf16;
 *   - causality is carried ONLY by the windows: causal <=> window_left < 0 && window_right == 0
 *     (paged_attn.cpp:116); the `is_causal` flags of the varlen/paged entries are ignored,
 *     exactly as in the reference;
 *   - work is enqueued asynchronously on `stream`; nothing synchronises;
 *   - errors never throw or exit: the call returns without launching and the reason is
 *     readable from fmha_last_error() on the calling thread (""/NULL-free on success).
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

/* ABI 2.1: the entries whose argument lists changed in 2.0 are exported under _v2 names; these
 * macros keep sources that call the plain names compiling unchanged, while a binary built
 * against the 1.0 header fails to link instead of calling them with a stale argument list
 * (the pattern of the CUDA driver API's cuMemAlloc -> cuMemAlloc_v2). */
#define fmha_varlen_fwd_ex fmha_varlen_fwd_ex_v2
#define fmha_page_kvcache_fwd_ex fmha_page_kvcache_fwd_ex_v2
#define fmha_bwd_workspace_size fmha_bwd_workspace_size_v2
#define fmha_varlen_bwd_workspace_size fmha_varlen_bwd_workspace_size_v2
#define fmha_varlen_bwd fmha_varlen_bwd_v2

#ifdef __cplusplus
#define FMHA_DEFAULT(x) = x
extern "C" {
#else
#define FMHA_DEFAULT(x)
#endif

/* Dense forward.  Replaces csrc/paged_attn.h:8-31 (impl paged_attn.cpp:310-383).
 * Writes o and, when softmax_lse_ptr != NULL, the fp32 log-sum-exp [batch, heads, seqlen_q]
 * (the reference leaves it unwritten; bwd needs it).  alibi_slopes_ptr: fp32 [heads] or
 * [batch, heads] (the latter when batch > 1, as paged_attn.cpp:375 assumes).  p_dropout in
 * [0, 1): P is dropped with Philox keep bits drawn from this thread's RNG state
 * (fmha_set_rng_state) and the kept values scaled by 1 / (1 - p_dropout), as the reference's
 * dropout forward (dropout_hip.h:14-109, whose C path never runs it); no KV
 * split with dropout.  return_softmax (needs p_dropout > 0, p_ptr and softmax_lse_ptr): p_ptr
 * receives the dropped-out softmax [batch, heads, round128(seqlen_q), round128(seqlen_k)] in q's
 * dtype, dropped entries with the sign bit set (the reference's S_dmask encoding; here P is
 * normalised).  num_splits <= 0 picks a split count; 1 forces the single-pass kernel. */
void fmha_fwd(void* q_ptr, void* k_ptr, void* v_ptr, void* o_ptr, void* alibi_slopes_ptr,
              const int32_t seqlen_q, const int32_t seqlen_k, const int32_t batch_size,
              const int32_t num_heads, const int32_t num_heads_k, const int32_t head_size,
              const float p_dropout, hipStream_t stream, hipDeviceProp_t* dprops,
              const float softmax_scale, void* p_ptr, void* softmax_lse_ptr,
              int window_size_left, int window_size_right, const float softcap,
              const bool return_softmax, bool is_fp16, int num_splits FMHA_DEFAULT(0));

/* Varlen (packed, ragged) forward.  Replaces csrc/paged_attn.h:33-53 (impl
 * paged_attn.cpp:385-440).  cu_seqlens_{q,k}: int32 [batch+1], cumulative. */
void fmha_varlen_fwd(void* q_ptrs, void* k_ptrs, void* v_ptrs, void* o_ptrs,
                     void* cu_seqlens_q_ptrs, void* cu_seqlens_k_ptrs,
                     const int32_t max_seqlen_q, const int32_t max_seqlen_k,
                     const int32_t batch_size, const int32_t num_heads,
                     const int32_t num_heads_k, const int32_t head_size, hipStream_t stream,
                     const float softmax_scale, const bool is_causal, const bool is_fp16,
                     int window_size_left FMHA_DEFAULT(-1), int window_size_right FMHA_DEFAULT(-1));

/* Paged-KV forward (decode / chunked prefill over a block table).  Replaces
 * csrc/paged_attn.h:55-84 (impl paged_attn.cpp:442-568).
 * kcache/vcache [num_blocks, page_block_size, heads_k, head_size]; block_table int32
 * [batch, max_cache_seq_k / page_block_size]; cache_seqlens_k int32 [batch] = per-sequence
 * lengths (non-cumulative).  k/v (append), cache_batch_idx and rotary are ignored exactly
 * as in the reference C path (paged_attn.cpp:513-525).  Split scratch comes from a cached
 * per-device pool (no per-call hipMalloc, no leak — cf. paged_attn.cpp:186-189,557-561). */
void fmha_page_kvcache_fwd(void* q_ptr, void* kcache_ptr, void* vcache_ptr, void* k_ptr,
                           void* v_ptr, void* o_ptr, void* block_table_ptr,
                           void* cache_seqlens_k_ptr, const int32_t max_cache_seq_k,
                           const int32_t seqlen_q, const int32_t seqlen_k,
                           const int32_t batch_size, const int32_t num_heads,
                           const int32_t num_heads_k, const int32_t head_size,
                           const int32_t page_block_size, hipStream_t stream,
                           const float softmax_scale, int window_size_left,
                           int window_size_right, const int32_t num_splits,
                           void* cache_batch_idx_ptr, void* rotary_cos_ptr, void* rotary_sin_ptr,
                           bool is_causal, bool is_rotary_interleaved, bool is_fp16);

/* ---------------------------------------------------------------- new entry points --- */

/* Thread-local description of the last failed call on this thread ("" if none). */
const char* fmha_last_error(void);
/* 0 if the last call on this thread succeeded, a nonzero code otherwise. */
int fmha_last_status(void);

/* KV split count the last forward call on this thread launched with (1 = single pass; decode
 * kernel: one split per wave; 0 if that call launched nothing).  Diagnostic, for tests and
 * tuning. */
int fmha_last_num_splits(void);

/* The forward kernel the last forward call on this thread launched, with its schedule, e.g.
 * "fmha_fwd4_kernel persistent=2 xcdq=0 grid=256x1x1 block=256" ("" if the call launched no
 * forward kernel).  persistent: 0 one workgroup per item, 1 boustrophedon, 2 XCD-grouped item
 * pairs, 3 dynamic queue (xcdq=1: one queue per XCD).  Diagnostic (ABI 2.3), for tests and the
 * bench line; the combine launch of a split forward is not named. */
const char* fmha_last_kernel(void);

/* Dropout RNG state of the calling thread: the following forward / backward calls with
 * p_dropout > 0 draw their keep bits from Philox4x32-7 keyed by (seed, offset) over the score
 * coordinates (batch x head, query position, key) - a forward and the backward of the same
 * scores with the same state drop the same entries (flash-attn's rng_state = {seed, offset}). */
void fmha_set_rng_state(uint64_t seed, uint64_t offset);

/* Graph-capturable dropout key (ABI 2.2): the next dropout call on this thread reads its key
 * on the device when it runs - seed = *seed_ptr, offset = *offset_ptr + offset_add (torch's
 * philox_cuda_state under stream capture: seed_.ptr, offset_.ptr, offset_intragraph_, which the
 * reference unpacks in its kernels, flash_api_hip.cpp:509) - and a forward writes the key it used
 * to rng_out[0..1] (device int64 x 2, may be NULL; the reference's params.rng_state).  The
 * backward of that forward: fmha_set_rng_state_device(rng_out, rng_out + 1, 0, NULL).
 * seed_ptr == NULL keeps the host key of fmha_set_rng_state (rng_out still receives it).
 * One-shot: consumed by the next entry that takes p_dropout, whatever its value or outcome
 * (fmha_set_rng_state clears it too). */
void fmha_set_rng_state_device(const int64_t* seed_ptr, const int64_t* offset_ptr,
                               uint64_t offset_add, int64_t* rng_out);

/* Library version / build identification, e.g. "xf-fmha-gfx950 2.13".  2.0 (round 3) changed
 * argument lists of existing symbols; 2.1 exports those under _v2 names (see INTEGRATION.md
 * "ABI history"). */
const char* fmha_version(void);

/* Process-wide schedule knobs; every setting computes the same results (the parity suite runs
 * under any of them).  Each knob is an atomic value read once per call, so setting one while
 * another thread launches is safe (that launch sees the old or the new value).  Returns 0, or
 * -1 for an unknown name / out-of-range value.  Knobs: fwd_waves (4 | 8 waves = 128 | 256
 * query rows per forward workgroup), fwd_prio (0/1), fwd_persistent (workgroups per CU, 0 =
 * one workgroup per item), fwd_slack (0..16; an fp16 launch runs with at most 15 and an fp8 one
 * with at most 8, since P <= 2^slack must fit the type it is rounded to), fwd_order (0/1),
 * fwd_dyn (0..2), fwd_xcdq (0/1),
 * fwd_pipe (0..2), fwd_decode (0/1), dec_wg_per_cu (1..16), dec_hmaj (0..2), dec_mr (16/32),
 * fwd_w4 (D = 128 forward where eligible — dense, varlen, or a paged cache whose page size is a
 * power of two >= 8: 4 auto, the default = 3 where no row has a right window and the cache is
 * not paged, else 2; 3 the 8-wave ping-pong kernel on the 16x16x32 MFMA (not paged); 2 the
 * 8-wave ping-pong kernel on 32x32x16; 1 the 4-wave kernel (variants build); 0 neither), fp8_w4 (fp8 forward: 1 the 4-wave kernel, the default; 2 the
 * 8-wave ping-pong kernel, dense launches only; 0 the 8-wave compiler-scheduled one), comb_row (0/1), bwd_order (0/1),
 * bwd_desc (0/1), dec_fold (0/1: the decode split combine folded into the split launch),
 * fwd_plain (0/1: the 32x32x16 ping-pong body without the score-feature and left-window code for
 * the launches with neither; same results; fmha_last_kernel names the body, " body=plain"). */
int fmha_set_option(const char* name, int value);
/* Current value of a knob, or -1 (with fmha_last_error set) for an unknown name. */
int fmha_get_option(const char* name);

/* fp8 forward (extension; north_star "the two back-to-back GEMMs on ... fp8 MFMA"): q, k, v in
 * OCP fp8 e4m3fn ([batch, seqlen, heads, 128] contiguous bytes, as fmha_fwd's layout) with
 * per-tensor fp32 dequant scales (value = stored x scale, FA3's descale_q/k/v); both GEMMs on
 * the gfx950 block-scaled fp8 MFMA (2x the bf16 rate), P rounded to e4m3 for the PV product.
 * o: bf16 (out_fp16 = false) or fp16 [batch, seqlen_q, heads, 128]; softmax_lse fp32
 * [batch, heads, seqlen_q] or NULL.  Causality / windows as fmha_fwd (causal <=> wl < 0 &&
 * wr == 0).  head_size must be 128; no ALiBi / softcap / dropout. */
/* fmha_fwd with explicit ELEMENT strides for q, k, v, o (batch, row, head; the last dimension
 * is contiguous): head- or batch-sliced views run without a copy (the reference's C ABI assumes
 * contiguous tensors, csrc/paged_attn.cpp:46-60).  strides[12] = {q_batch, q_row, q_head,
 * k_batch, k_row, k_head, v_batch, v_row, v_head, o_batch, o_row, o_head}.  softmax_lse is
 * [batch, num_heads, seqlen_q] contiguous (or NULL).  head_size must be a multiple of 8.
 * p_dropout / s_dmask: dropout and return_softmax as fmha_fwd (s_dmask = its p_ptr, or NULL). */
void fmha_fwd_strided(void* q, void* k, void* v, void* o, void* alibi_slopes, void* softmax_lse,
                      int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                      int32_t num_heads_k, int32_t head_size, const int64_t* strides,
                      float softmax_scale, int window_size_left, int window_size_right,
                      float softcap, bool is_fp16, int num_splits, hipStream_t stream,
                      float p_dropout, void* s_dmask);

void fmha_fwd_fp8(void* q, void* k, void* v, void* o, void* softmax_lse, float q_scale,
                  float k_scale, float v_scale, int32_t seqlen_q, int32_t seqlen_k,
                  int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                  float softmax_scale, int window_size_left, int window_size_right, bool out_fp16,
                  hipStream_t stream);

/* fmha_fwd_fp8 over packed variable-length sequences (2.5): q [total_q, heads, 128] and k/v
 * [total_k, heads_k, 128] in OCP fp8 e4m3fn bytes, cu_seqlens_q / cu_seqlens_k int32
 * [batch + 1] (both required), seqused_k int32 [batch] or NULL (keys [0, seqused_k[b]) of the
 * slot cu_seqlens_k describes).  o: bf16 or fp16 [total_q, heads, 128]; softmax_lse fp32
 * [heads, total_q] (unpadded, as fmha_varlen_fwd_ex; total_q addresses it) or NULL.  A sequence
 * without keys gets O = 0 and LSE = +inf, one without queries writes nothing.  Windows are
 * normalised against max_seqlen_k.  head_size must be 128; no ALiBi / softcap / dropout / paged
 * K/V. */
void fmha_varlen_fwd_fp8(void* q, void* k, void* v, void* o, void* softmax_lse,
                         void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                         float q_scale, float k_scale, float v_scale,
                         int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                         int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                         float softmax_scale, int window_size_left, int window_size_right,
                         bool out_fp16, hipStream_t stream);

/* fmha_fwd_fp8 / fmha_varlen_fwd_fp8 with the descales read on the device (2.6): the three
 * floats become device pointers q_descale, k_descale, v_descale (fp32) and two ELEMENT strides
 * that index each of them by (batch, kv head): the descale of batch b (packed input: sequence
 * b), kv head g is ptr[b * descale_batch_stride + g * descale_head_stride]; q's applies to the
 * whole group of query heads of kv head g.  (0, 0) is a one-element per-tensor scale,
 * (heads_k, 1) FA3's [batch, heads_k] tensors.  No host sync, so a scale computed on the device
 * (fmha_quantize_fp8) can be used inside a captured graph.  Caller contract: the values cannot be
 * checked on the host, so "descale > 0" is the caller's to keep - a non-positive or non-finite
 * descale spoils the output of that (batch, kv head) only, never addressing.  Everything else as
 * the by-value entries, which give bit-identical results for equal scales. */
void fmha_fwd_fp8_ex(void* q, void* k, void* v, void* o, void* softmax_lse, const float* q_descale,
                     const float* k_descale, const float* v_descale, int32_t descale_batch_stride,
                     int32_t descale_head_stride, int32_t seqlen_q, int32_t seqlen_k,
                     int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                     float softmax_scale, int window_size_left, int window_size_right, bool out_fp16,
                     hipStream_t stream);

void fmha_varlen_fwd_fp8_ex(void* q, void* k, void* v, void* o, void* softmax_lse,
                            void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                            const float* q_descale, const float* k_descale, const float* v_descale,
                            int32_t descale_batch_stride, int32_t descale_head_stride,
                            int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                            int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                            float softmax_scale, int window_size_left, int window_size_right,
                            bool out_fp16, hipStream_t stream);

/* bf16 / fp16 -> OCP fp8 e4m3fn with the descales the fp8 entries take (2.6).  x: [batch, seqlen,
 * heads, head_size] by ELEMENT strides {batch, row, head} (last dimension contiguous, as
 * fmha_fwd_strided), or with cu_seqlens (int32 [batch + 1]) packed [total, heads, head_size]:
 * then seqlen is the longest sequence and the batch stride is ignored.  x8: contiguous bytes of
 * the same logical shape.  granularity 0: one scale, descale[1]; 1: one per (batch or sequence,
 * group of `group` consecutive heads), descale [batch, num_heads / group] contiguous - group =
 * heads / heads_k for q (a forward item covers one kv head and all its query heads), 1 for k, v.
 *   amax = max |float(x)| over the scale's set;  descale = amax / 448.0f (1.0f when amax == 0 or
 *   the set is empty);  byte = e4m3fn round-to-nearest-even of clamp(float(x) * (1.0f / descale),
 *   -448, 448).
 * Two passes over x (an order-independent maximum, then the conversion), no allocation per call
 * and no host sync: capturable in a graph.  head_size a multiple of 8 and <= 256; x 16-byte and
 * x8 8-byte aligned; strides multiples of 8. */
void fmha_quantize_fp8(const void* x, void* x8, float* descale, const void* cu_seqlens,
                       int32_t batch_size, int32_t seqlen, int32_t num_heads, int32_t group,
                       int32_t head_size, const int64_t* strides, int32_t granularity, bool is_fp16,
                       hipStream_t stream);

/* Varlen forward with the fields the reference's varlen C entry drops (paged_attn.cpp:423-433):
 * LSE out (fp32 [num_heads, total_q], unpadded as export.cpp:827; total_q = cu_seqlens_q[batch]
 * must be passed by the caller, it is only used to address the LSE), ALiBi, softcap,
 * seqused_k (int32 [batch], optional), and an optional paged K/V (block_table != NULL: k/v are
 * [num_blocks, page, heads_k, head_size], block_table [batch, block_table_stride]).
 * p_dropout / s_dmask: as fmha_fwd (non-paged only; s_dmask [batch, heads,
 * round128(max_seqlen_q), round128(max_seqlen_k)], each sequence's rows from 0). */
void fmha_varlen_fwd_ex_v2(void* q, void* k, void* v, void* o, void* softmax_lse,
                        void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                        void* block_table, int32_t block_table_stride, int32_t page_block_size,
                        void* alibi_slopes, int32_t alibi_batch_stride,
                        int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                        int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                        int32_t head_size, float softmax_scale, int window_size_left,
                        int window_size_right, float softcap, bool is_fp16, hipStream_t stream,
                        float p_dropout, void* s_dmask);

/* Paged-KV forward that also returns LSE (fp32 [batch, num_heads, seqlen_q]) and takes ALiBi
 * and an fp8 (OCP e4m3fn) K/V cache with per-tensor dequant scales.
 * kv_dtype: 0 = same as q (fp16/bf16), 1 = fp8 e4m3fn (k_scale/v_scale multiply the stored
 * values).  num_splits <= 0 picks a split count.
 * cache_leftpad: optional int32 [batch_size] (flash-attn's leftpad_k, block_info.h; commented
 * out in export.cpp:1627-1634): batch b attends over cache rows [cache_leftpad[b],
 * cache_seqlens[b]), key positions counted from cache_leftpad[b].  Only for one page per
 * sequence (max_seqlen_k <= page_block_size), as the reference: no paged KV with leftpad. */
void fmha_page_kvcache_fwd_ex_v2(void* q, void* kcache, void* vcache, void* o, void* softmax_lse,
                              void* block_table, int32_t block_table_stride, void* cache_seqlens,
                              int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                              int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                              int32_t page_block_size, float softmax_scale,
                              int window_size_left, int window_size_right, float softcap,
                              void* alibi_slopes, int32_t alibi_batch_stride, int32_t num_splits,
                              int32_t kv_dtype, float k_scale, float v_scale,
                              void* cache_leftpad, bool is_fp16, hipStream_t stream);

/* KV-cache append with optional rotary embedding: the write step of mha_fwd_kvcache with new
 * k/v (export.cpp:1585-1669, kernel flash_fwd_kernel_hip.h:817-934 / rotary_hip.h:21-152 - never
 * enabled by the reference's C path, csrc/paged_attn.cpp:513-525).  For each batch b and new
 * token j: pos = cache_seqlens[b] + j; kcache/vcache slot (block_table[b][pos / page],
 * pos % page) <- rotary(knew[b][j]) / vnew[b][j]; seqlens_out[b] = cache_seqlens[b] +
 * seqlen_new.  With rotary_dim > 0 also q_out = rotary(q) at position cache_seqlens[b] + s
 * (q_rotary_per_token, the causal/local case) or cache_seqlens[b] (otherwise).  rotary_cos /
 * rotary_sin: [seqlen_ro, rotary_dim / 2] in q's dtype; interleaved = GPT-J pairs (2i, 2i+1),
 * else GPT-NeoX halves (i, i + rotary_dim/2).  knew/vnew contiguous [b, seqlen_new, hk, d];
 * caches contiguous [num_blocks, page, hk, d]; q/q_out contiguous [b, seqlen_q, h, d].
 * seqlens_out must be a different buffer from cache_seqlens (rejected otherwise: the kernel
 * reads the old lengths while writing the new ones).  New rows whose slot falls past the
 * block table's row (pos >= block_table_stride * page) are dropped.
 * Stream-ordered; run the attention (fmha_page_kvcache_fwd_ex with seqlens_out) after it. */
void fmha_kvcache_append(void* q, void* q_out, void* kcache, void* vcache, const void* knew,
                         const void* vnew, int32_t seqlen_new, const void* block_table,
                         int32_t block_table_stride, int32_t page_block_size,
                         const void* cache_seqlens, void* seqlens_out, const void* rotary_cos,
                         const void* rotary_sin, int32_t rotary_dim, bool is_rotary_interleaved,
                         bool q_rotary_per_token, int32_t batch_size, int32_t seqlen_q,
                         int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                         bool is_fp16, hipStream_t stream);

/* fmha_kvcache_append into an fp8 (OCP e4m3fn) cache (2.6): kcache / vcache are bytes
 * [num_blocks, page, hk, d], knew / vnew / q / q_out stay in q's dtype; k_scale / v_scale are the
 * cache's descales (positive), as fmha_page_kvcache_fwd_ex takes them with kv_dtype = 1.  K: the
 * rotary in fp32 as above, x (1 / k_scale), clamped to +-448 and rounded once to e4m3; V:
 * x (1 / v_scale), clamped, rounded.  Everything else (seqlens_out, dropped rows, q_out) as
 * fmha_kvcache_append. */
void fmha_kvcache_append_fp8(void* q, void* q_out, void* kcache, void* vcache, const void* knew,
                             const void* vnew, int32_t seqlen_new, const void* block_table,
                             int32_t block_table_stride, int32_t page_block_size,
                             const void* cache_seqlens, void* seqlens_out, const void* rotary_cos,
                             const void* rotary_sin, int32_t rotary_dim, bool is_rotary_interleaved,
                             bool q_rotary_per_token, int32_t batch_size, int32_t seqlen_q,
                             int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                             bool is_fp16, hipStream_t stream, float k_scale, float v_scale);

/* Dense backward: the C form of mha_bwd (export.cpp:948-1176, live twin flash_api_hip.cpp:
 * 815-1043), which the reference never built.  Inputs dout/q/k/v/out as the fwd layout,
 * softmax_lse fp32 [batch, heads, seqlen_q] from fmha_fwd; outputs dq [b,sq,h,d],
 * dk/dv [b,sk,hk,d] (GQA groups reduced in-kernel, no host sum_out), softmax_d fp32
 * [batch, heads, seqlen_q] (may be NULL: then pool scratch is used).  p_dropout: the forward's,
 * with the same fmha_set_rng_state (the keep bits are regenerated, not stored).
 * deterministic: S = min(ceil(CUs / (b * hk)), key blocks) fp32 dQ slices (the bound of
 * export.cpp:1086-1092), each owned by one workgroup that walks its key blocks in a fixed order
 * and adds by plain read-modify-write (D <= 128; D > 128: float atomics into the slice), then
 * summed in slice order: bitwise reproducible for a given S, instead of float atomics into one
 * accumulator.  S also stops at 1 + 8 GiB / (one slice's bytes).
 * workspace: optional caller scratch of fmha_bwd_workspace_size(..., deterministic) bytes;
 * NULL = pool.  A shorter workspace (at least one slice) is accepted and runs with as many
 * slices as it holds: still reproducible, but the dQ bits then depend on that slice count, so
 * pass the full size when results must match across callers.  One sequence's slab of any tensor must stay under 2 GiB - 256 bytes (32-bit
 * buffer offsets); larger inputs fail with an error, never a wrong result. */
void fmha_bwd(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
              void* dq, void* dk, void* dv, void* alibi_slopes, void* softmax_d,
              int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
              int32_t num_heads_k, int32_t head_size, float p_dropout, float softmax_scale,
              int window_size_left, int window_size_right, float softcap, bool deterministic,
              bool is_fp16, hipStream_t stream, void* workspace, size_t workspace_bytes);

size_t fmha_bwd_workspace_size_v2(int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size,
                               int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                               bool deterministic);

/* Varlen backward (mha_varlen_bwd semantics, flash_api_hip.cpp:1045-1298): packed q/k/v/out/
 * dout, cu_seqlens int32 [batch+1], softmax_lse fp32 [num_heads, total_q]; softmax_d fp32
 * [num_heads, total_q] receives rowsum(dO*O) (may be NULL: pool scratch).  deterministic and
 * workspace as fmha_bwd (fmha_varlen_bwd_workspace_size(..., deterministic) bytes); p_dropout as
 * fmha_bwd. */
void fmha_varlen_bwd_v2(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
                     void* dq, void* dk, void* dv, void* cu_seqlens_q, void* cu_seqlens_k,
                     void* alibi_slopes, int32_t alibi_batch_stride, int32_t max_seqlen_q,
                     int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                     int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                     int32_t head_size, float softmax_scale, int window_size_left,
                     int window_size_right, float softcap, bool deterministic, bool is_fp16,
                     hipStream_t stream, void* workspace, size_t workspace_bytes,
                     void* softmax_d, float p_dropout);

size_t fmha_varlen_bwd_workspace_size_v2(int32_t total_q, int32_t max_seqlen_k, int32_t batch_size,
                                      int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                                      bool deterministic);

/* ------------------------------------------------------------ attention sinks (2.7) --- */

/* Attention sink (gpt-oss; other builds' s_aux / learnable_sink): `sink` is fp32 [num_heads] on
 * the device, one logit per QUERY head that joins the softmax denominator and carries no value.
 * It is in the units of the scaled scores: not multiplied by softmax_scale, not soft-capped.
 * For row i of head h over its visible keys j (scores S after scale, softcap and masks):
 *   P_ij = exp(S_ij) / (sum_j exp(S_ij) + exp(sink[h])),  O_i = sum_j P_ij V_j,
 *   LSE_i = log(sum_j exp(S_ij) + exp(sink[h])).
 * A row without a visible key keeps O = 0 and LSE = +inf; sink[h] = -inf is no sink for head h
 * (bit-identical to the base entry); sink == NULL is the base entry, bit for bit.  Refused with
 * an error, outputs untouched: a sink with ALiBi, with p_dropout > 0 or with s_dmask.  Causal
 * and left / right windows, softcap, GQA / MQA, seqused_k, paged and fp8 caches, cache_leftpad,
 * split-KV and every head size of the base entries are allowed.  fmha_last_kernel() ends in
 * " sink=epilogue" (applied in the forward kernel), " sink=combine" (in the split combine) or
 * " sink=pass" (a pass over O and LSE after a launch whose kernel cannot apply it; when
 * softmax_lse is NULL the LSE it needs lives in pool scratch).  No allocation per call, no host
 * sync.
 *
 * fmha_fwd_sink: fmha_fwd_strided plus sink. */
void fmha_fwd_sink(void* q, void* k, void* v, void* o, void* alibi_slopes, void* softmax_lse,
                   int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                   int32_t num_heads_k, int32_t head_size, const int64_t* strides,
                   float softmax_scale, int window_size_left, int window_size_right,
                   float softcap, bool is_fp16, int num_splits, hipStream_t stream,
                   float p_dropout, void* s_dmask, const float* sink);

/* fmha_varlen_fwd_ex plus sink; total_q must be given with a sink. */
void fmha_varlen_fwd_sink(void* q, void* k, void* v, void* o, void* softmax_lse,
                          void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                          void* block_table, int32_t block_table_stride, int32_t page_block_size,
                          void* alibi_slopes, int32_t alibi_batch_stride,
                          int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                          int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                          int32_t head_size, float softmax_scale, int window_size_left,
                          int window_size_right, float softcap, bool is_fp16, hipStream_t stream,
                          float p_dropout, void* s_dmask, const float* sink);

/* fmha_page_kvcache_fwd_ex plus sink (bf16 / fp16 and fp8 caches alike). */
void fmha_page_kvcache_fwd_sink(void* q, void* kcache, void* vcache, void* o, void* softmax_lse,
                                void* block_table, int32_t block_table_stride, void* cache_seqlens,
                                int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                                int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                                int32_t page_block_size, float softmax_scale,
                                int window_size_left, int window_size_right, float softcap,
                                void* alibi_slopes, int32_t alibi_batch_stride, int32_t num_splits,
                                int32_t kv_dtype, float k_scale, float v_scale,
                                void* cache_leftpad, bool is_fp16, hipStream_t stream,
                                const float* sink);

/* Gradient of the sink.  fmha_bwd / fmha_varlen_bwd need no change for a sink forward: given its
 * out and softmax_lse, P = exp(S - LSE) and D = rowsum(dO * O) are already those of the sink
 * softmax (the sink column has V = 0, hence dP = 0), so dq / dk / dv come out right.  This entry
 * adds dsink[h] = - sum over (batch, row) of exp(sink[h] - LSE) * D; rows with LSE = +inf add 0.
 * Run it after fmha_bwd / fmha_varlen_bwd called with a non-NULL softmax_d.  softmax_lse and
 * softmax_d: element (b, h, row) at b * batch_stride + h * head_stride + row - dense
 * [batch, heads, seqlen_q]: (heads * seqlen_q, seqlen_q); packed: batch = 1, rows = total_q,
 * head_stride = total_q.  dsink: fp32 [num_heads].  One workgroup per head sums in a fixed
 * order without atomics: bitwise reproducible. */
void fmha_bwd_sink(const float* softmax_lse, const float* softmax_d, const float* sink, float* dsink,
                   int32_t batch, int32_t num_heads, int32_t rows, int64_t batch_stride,
                   int64_t head_stride, hipStream_t stream);

/* ------------------------------------------------- merge of partial attention states (2.8) --- */

/* Most parts one fmha_merge_states call takes. */
#define FMHA_MERGE_MAX_PARTS 16

/* Merge num_parts partial results (O_i, LSE_i) of the same queries, each computed over its own
 * keys (a cached prefix and a new suffix; the K/V chunks of ring attention), into the (O, LSE) of
 * one softmax over all of those keys (other libraries' merge_attn_states / merge_state).
 * o_parts / lse_parts: HOST arrays of num_parts DEVICE pointers, 1 <= num_parts <=
 * FMHA_MERGE_MAX_PARTS; the pointers are copied by value into the kernel's arguments: no device
 * table, no copy, no allocation, no host sync (capturable in a graph).
 * strides[10], in ELEMENTS: the parts' O {batch, row, head}, the output's O {batch, row, head},
 * the parts' LSE {batch, head}, the output's LSE {batch, head}.  O's last dimension is contiguous
 * (fmha_fwd_strided's convention), an LSE row is contiguous (fmha_bwd_sink's): element (b, h, row)
 * at b * batch + h * head + row; all parts share one stride set.  Dense: O [batch, rows, heads,
 * head_size], LSE [batch, heads, rows]; packed: batch = 1, rows = total_q, LSE [heads, total_q].
 * head_size a multiple of 8 and <= 256; O pointers 16-byte aligned, O strides multiples of 8.
 * Per (batch, row, head), in fp32:
 *   a part whose LSE is +inf (this library's "no visible key") or -inf (other libraries') is
 *   absent, and its O never enters the sum (it may hold anything, NaN included);
 *   over the present parts  m = max LSE_i, w_i = exp(LSE_i - m), den = sum w_i,
 *   O = sum (w_i / den) O_i  rounded once to the dtype,  LSE = m + log(den);
 *   sink != NULL (fp32 [num_heads], as in 2.7): the sink joins afterwards - O is scaled by
 *   f = 1 / (1 + exp(sink[h] - LSE)) and LSE becomes log(exp(LSE) + exp(sink[h])); sink[h] = -inf
 *   gives the bits of the call without a sink;
 *   no part present: O = 0 and LSE = +inf, whatever the sink.
 * o and lse may be exactly part 0's buffers (same pointer and strides) for in-place accumulation;
 * lse may be NULL.  The parts are summed in index order without atomics: bitwise reproducible.
 * rows == 0 or batch == 0 launches nothing and succeeds.  Refused with an error, outputs
 * untouched: num_parts out of range, a NULL part pointer, a bad head_size, bad strides or
 * alignment, o (or lse) overlapping a part other than part 0 or part 0 only partly (judged on the
 * byte ranges the strides span). */
void fmha_merge_states(const void* const* o_parts, const float* const* lse_parts, int32_t num_parts,
                       void* o, float* lse, const float* sink,
                       int32_t batch, int32_t rows, int32_t num_heads, int32_t head_size,
                       const int64_t* strides, bool is_fp16, hipStream_t stream);

/* ------------------------------------------------- MLA decode over a latent cache (2.9) ------ */

/* Decode attention for multi-head latent attention (DeepSeek-V2/V3/R1, Kimi) in its "absorbed"
 * form: every query head attends over ONE shared latent row per token, head_size = 576 wide (512
 * compressed-KV features + 64 rotary features), and the value is the first head_size_v = 512
 * features of the same row.  bf16 or fp16.
 *   q          [batch, seqlen_q, num_heads, 576] by element strides {batch, row, head}, last
 *              dimension contiguous (fmha_fwd_strided's convention)
 *   kv_cache   [num_blocks, page_block_size, 1, 576], contiguous; page_block_size % 16 == 0
 *   block_table int32 [batch, block_table_stride], required; cache_seqlens int32 [batch]
 *   o          [batch, seqlen_q, num_heads, 512] by element strides {batch, row, head}
 *   softmax_lse fp32 [batch, num_heads, seqlen_q], or NULL
 *   strides[6], in ELEMENTS: q {batch, row, head}, then o {batch, row, head}
 * For sequence b with n = min(cache_seqlens[b], max_seqlen_k) keys K (n x 576, through the table)
 * and V = K[:, :512]:  S = softmax_scale q K^T (all 576 features), O = softmax(S) V,
 * LSE = logsumexp(S).  softmax_scale is the caller's (DeepSeek's is not 576^-1/2).
 * Windows: (-1, -1) full attention; (-1, 0) causal, bottom-right aligned (the query at position s
 * sees keys < n - seqlen_q + s + 1); any other window is refused.  A row without a visible key
 * (n = 0; n < seqlen_q under causal) gives O = 0 and LSE = +inf.
 * max_seqlen_k: an upper bound of the lengths, at most block_table_stride * page_block_size; it
 * sizes the automatic split count.  num_splits <= 0: chosen from the workgroups against the CU
 * count, at most the key tiles and 128; 1: a single pass without scratch or combine; up to 128.
 * The split scratch comes from the per-stream pool: no allocation once it is warm, no host sync
 * (capturable in a graph).  fmha_last_kernel() names fmha_mla_decode_kernel with its mapping
 * (<tiles>: the waves of a workgroup are 16-row tiles of one (batch, key split); <splits>: one
 * row tile, the waves are key splits), fmha_last_num_splits() the split count.
 * batch_size == 0 launches nothing and succeeds.  Refused with an error, outputs untouched: a NULL
 * q / kv_cache / o / block_table / cache_seqlens / strides, (head_size, head_size_v) other than
 * (576, 512), a page size that is no multiple of 16, another window, num_heads < 1 or
 * seqlen_q < 1, num_splits > 128, strides that are no multiples of 8 or pointers that are not
 * 16-byte aligned, a page slab beyond the 32-bit offset limit.
 * Partial results over two caches (a shared prefix and a suffix) are merged with
 * fmha_merge_states, 256 of the 512 columns per call. */
void fmha_mla_decode(void* q, void* kv_cache, void* o, void* softmax_lse,
                     void* block_table, int32_t block_table_stride, void* cache_seqlens,
                     int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                     int32_t num_heads, int32_t head_size, int32_t head_size_v,
                     int32_t page_block_size, const int64_t* strides /* q then o: batch,row,head */,
                     float softmax_scale, int window_size_left, int window_size_right,
                     int32_t num_splits, bool is_fp16, hipStream_t stream);

/* ------------------------------------- MLA decode over an fp8 latent cache, its append (2.10) */

/* The fp8 latent cache (FlashMLA's fp8 KV cache, vLLM's fp8_ds_mla): kv_cache8 holds BYTES
 * [num_blocks, page_block_size, 1, 656], contiguous, page_block_size % 16 == 0, 0.569 of the
 * 16-bit row.  The row of one token:
 *   bytes   0 .. 511   latent features 0 .. 511, OCP e4m3fn
 *   bytes 512 .. 527   four fp32 descales; descale j belongs to features 128 j .. 128 j + 127
 *   bytes 528 .. 655   rotary features 512 .. 575 in q's dtype (bf16, or fp16 for an fp16 call),
 *                      not quantised
 * The operand the kernel attends over: feature i < 512 is T(float(e4m3[i]) * descale[i / 128]) -
 * one fp32 product, rounded once to q's dtype T (FlashMLA's own dequantisation) - and features
 * 512 .. 575 are the stored 16-bit values.  With K (n x 576) so defined and V = K[:, :512],
 * fmha_mla_decode_fp8 is fmha_mla_decode word for word: S over all 576 features, the windows
 * (-1, -1) and (-1, 0), the empty-row rule, max_seqlen_k and the automatic split count, the LSE
 * layout, the strides, the scratch pool and graph capturability, every check and refusal (the
 * page slab judged at 656 bytes a row), fmha_last_num_splits().  fmha_last_kernel() names
 * fmha_mla_decode_fp8_kernel<tiles> or <splits>.  (The scales are applied to the operands, not to
 * S and O as the fp8 paged decode does: a scale per (key, 128 features) does not factor out of
 * O after the PV product.) */
void fmha_mla_decode_fp8(void* q, void* kv_cache8, void* o, void* softmax_lse,
                         void* block_table, int32_t block_table_stride, void* cache_seqlens,
                         int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                         int32_t num_heads, int32_t head_size /* 576 */, int32_t head_size_v /* 512 */,
                         int32_t page_block_size, const int64_t* strides /* q then o: batch,row,head */,
                         float softmax_scale, int window_size_left, int window_size_right,
                         int32_t num_splits, bool is_fp16, hipStream_t stream);

/* Append tokens to the fp8 latent cache: one launch, one pass, no scratch, no host sync
 * (capturable in a graph).
 *   latent [num_tokens, 512] and k_pe [num_tokens, 64] in bf16 (fp16 for is_fp16), each by its own
 *          row stride in ELEMENTS (two views of one 576-wide tensor are the common case); k_pe
 *          arrives rotated and is copied
 *   slot_mapping int64 [num_tokens]: slot = block * page_block_size + row (vLLM's
 *          concat_and_cache_mla convention).  A negative slot, or one >= num_blocks *
 *          page_block_size, writes nothing; a row is written whole (656 bytes) or not at all.
 * The quantiser, for each 128-feature group of a row (fmha_quantize_fp8's words at a finer
 * grain): amax = max |float(x)|; descale = amax / 448.0f, and 1.0f when amax == 0; byte = e4m3fn
 * round-to-nearest-even of clamp(float(x) * (1.0f / descale), -448, 448).
 * num_tokens == 0 launches nothing and succeeds.  Refused with an error, the cache untouched: a
 * NULL pointer, a row stride that is negative or no multiple of 8, latent / k_pe / kv_cache8 not
 * 16-byte aligned or slot_mapping not 8-byte aligned, a page size that is no multiple of 16, a
 * negative count. */
void fmha_mla_cache_append_fp8(const void* latent, int64_t latent_row_stride, const void* k_pe,
                               int64_t k_pe_row_stride, void* kv_cache8, const void* slot_mapping,
                               int32_t num_tokens, int32_t num_blocks, int32_t page_block_size,
                               bool is_fp16, hipStream_t stream);

/* --------------------------- MLA decode over index-selected tokens: sparse attention (2.11) */

/* MLA decode where an indexer has chosen the tokens (DeepSeek-V3.2's sparse attention; FlashMLA's
 * flash_mla_with_kvcache(..., indices=...)): the decode attends over exactly the selected rows of
 * the paged latent cache, gathered inside the kernel.  fmha_mla_decode_sparse reads the 16-bit
 * cache of fmha_mla_decode, fmha_mla_decode_sparse_fp8 the 656-byte rows of fmha_mla_decode_fp8
 * (the operand is that entry's rounded row, unchanged).
 *   q, o, softmax_lse, strides, softmax_scale, num_splits, is_fp16: as fmha_mla_decode
 *   kv_cache   contiguous [num_blocks, page_block_size, 1, 576] of q's type, or bytes
 *              [num_blocks, page_block_size, 1, 656]; num_blocks >= 1, page_block_size % 16 == 0.
 *              The cache may be larger than 4 GiB: slot-to-byte arithmetic is done in 64 bits.
 *   indices    int32 [batch, seqlen_q, topk], last dimension contiguous, 4-byte aligned;
 *              indices_batch_stride and indices_row_stride in ELEMENTS, non-negative; topk >= 1
 * An entry is a PHYSICAL SLOT, block * page_block_size + row (FlashMLA's convention, the one
 * fmha_mla_cache_append_fp8 writes): the row of slot s starts at byte s * 1152 (s * 656).  An entry
 * is valid iff 0 <= entry < num_blocks * page_block_size; every other value (-1, FlashMLA's
 * padding; INT32_MIN; INT32_MAX; num_blocks * page_block_size) contributes nothing and is never
 * turned into an address.  The kernel validates: the host cannot without a sync, and no index
 * value, however wild, produces a load outside [kv_cache, kv_cache + num_blocks *
 * page_block_size * row bytes).
 * For query (b, pos, head), K is the rows at the valid entries of indices[b, pos, :], in that
 * order, duplicates as often as they occur, V = K[:, :512]:  S = softmax_scale q K^T (all 576
 * features), O = softmax(S) V, LSE = logsumexp(S).  A row whose entries are all invalid gives O = 0
 * and LSE = +inf.  There is no block table, no cache_seqlens and no mask: visibility is what the
 * indexer chose.  Per-batch topk lengths are expressed by padding with -1.
 * A 16-row tile is 16 heads of ONE position (row tiles = seqlen_q * ceil(num_heads / 16)); a split
 * is an equal range of the ceil(topk / 32) index tiles.  num_splits <= 0: fmha_mla_decode's rule
 * over these row tiles, at most ceil(topk / 32) and 128.  The split scratch comes from the
 * per-stream pool; no host sync (capturable in a graph).  fmha_last_kernel() names
 * fmha_mla_decode_sparse_kernel<tiles> or <splits> (fmha_mla_decode_sparse_fp8_kernel<...>),
 * fmha_last_num_splits() the split count.  With indices[b, 0, :] the slots of a dense sequence in
 * order, the result equals fmha_mla_decode[_fp8] over that sequence bit for bit at the same split
 * count.
 * batch_size == 0 validates in full, launches nothing and succeeds.  Refused with an error, outputs
 * untouched: a NULL q / kv_cache / o / indices / strides, (head_size, head_size_v) other than
 * (576, 512), topk < 1, num_blocks < 1, a page size that is no positive multiple of 16,
 * num_heads < 1 or seqlen_q < 1, a negative batch, num_splits > 128, q / o strides that are no
 * multiples of 8 or pointers that are not 16-byte aligned (indices, softmax_lse: 4-byte), a
 * negative indices stride, a launch larger than one grid covers. */
void fmha_mla_decode_sparse(void* q, void* kv_cache, void* o, void* softmax_lse,
                            void* indices, int64_t indices_batch_stride, int64_t indices_row_stride,
                            int32_t topk, int32_t seqlen_q, int32_t batch_size, int32_t num_heads,
                            int32_t head_size /* 576 */, int32_t head_size_v /* 512 */,
                            int32_t num_blocks, int32_t page_block_size,
                            const int64_t* strides /* q then o: batch,row,head */,
                            float softmax_scale, int32_t num_splits, bool is_fp16, hipStream_t stream);
void fmha_mla_decode_sparse_fp8(void* q, void* kv_cache8, void* o, void* softmax_lse,
                                void* indices, int64_t indices_batch_stride, int64_t indices_row_stride,
                                int32_t topk, int32_t seqlen_q, int32_t batch_size, int32_t num_heads,
                                int32_t head_size /* 576 */, int32_t head_size_v /* 512 */,
                                int32_t num_blocks, int32_t page_block_size,
                                const int64_t* strides /* q then o: batch,row,head */,
                                float softmax_scale, int32_t num_splits, bool is_fp16, hipStream_t stream);

/* ------------------------- MLA prefill: head size 192 for Q K^T, 128 for V (2.12) */

/* The prefill half of multi-head latent attention in its un-absorbed form (DeepSeek-V2/V3/R1,
 * Kimi): q and k carry 192 features a head (128 "nope" + 64 rotary), v and o 128.
 *   S = softmax_scale q K^T over all 192 features, O = softmax(S) V, LSE = logsumexp(S) in fp32.
 * One pass of fmha_fwd_mla_kernel (fmha_last_kernel() names it with its schedule); no ALiBi,
 * softcap, dropout, sink, paged or fp8 K/V and no KV split.  Windows as every forward here:
 * bottom-right aligned, causal <=> (-1, 0); a row without a visible key gives O = 0 and
 * LSE = +inf.  GQA: num_heads % num_heads_k == 0.  The default softmax_scale of the models is
 * 192^-1/2 (possibly times a YaRN factor); it is the caller's.
 * Nothing is copied or padded: every tensor goes by its own strides, in ELEMENTS, last dimension
 * contiguous; V's row and head pitch are independent of K's.  Loads go through descriptors sized
 * to each sequence: nothing outside a sequence's rows and columns reaches a result, and nothing
 * but o's and softmax_lse's own elements is written.  No scratch and no host sync; the first
 * forward call on a stream allocates that stream's item-queue counters, so warm a stream up
 * before capturing a graph on it.
 *
 * fmha_fwd_mla: dense q [batch, seqlen_q, heads, 192], k [batch, seqlen_k, heads_k, 192],
 * v [batch, seqlen_k, heads_k, 128], o [batch, seqlen_q, heads, 128]; strides[12] = {batch, row,
 * head} of q, k, v, o; softmax_lse fp32 [batch, heads, seqlen_q] contiguous, or NULL.
 *
 * fmha_varlen_fwd_mla: packed q [total_q, heads, 192], k [total_k, heads_k, 192], v [total_k,
 * heads_k, 128], o [total_q, heads, 128]; strides[8] = {row, head} of q, k, v, o; cu_seqlens_q /
 * cu_seqlens_k int32 [batch + 1]; seqused_k int32 [batch] or NULL: the keys of sequence b are the
 * first seqused_k[b] rows at cu_seqlens_k[b]; softmax_lse fp32 [heads, total_q], or NULL.  A
 * sequence without keys (or without queries) is fine; max_seqlen_k == 0 is refused.
 *
 * Refused with an error, outputs untouched: (head_size_qk, head_size_v) other than (192, 128); a
 * NULL q / k / v / o / strides (varlen: cu_seqlens_q / cu_seqlens_k); batch_size < 1;
 * num_heads % num_heads_k != 0; q / k / v / o not 16-byte aligned; a stride that is negative or,
 * over an extent above 1, no multiple of 8; a k (v) row stride below 192 (128); non-positive
 * lengths; one sequence's slab beyond the 32-bit offset limit. */
void fmha_fwd_mla(void* q, void* k, void* v, void* o, void* softmax_lse,
                  int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                  int32_t num_heads_k, int32_t head_size_qk /* 192 */, int32_t head_size_v /* 128 */,
                  const int64_t* strides /* q, k, v, o: batch,row,head */, float softmax_scale,
                  int window_size_left, int window_size_right, bool is_fp16, hipStream_t stream);
void fmha_varlen_fwd_mla(void* q, void* k, void* v, void* o, void* softmax_lse,
                         void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k /* nullable */,
                         int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                         int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                         int32_t head_size_qk /* 192 */, int32_t head_size_v /* 128 */,
                         const int64_t* strides /* q, k, v, o: row,head */, float softmax_scale,
                         int window_size_left, int window_size_right, bool is_fp16, hipStream_t stream);

/* ------------------------- MLA prefill backward: dq, dk (192 wide), dv (128 wide) (2.13) */

/* The gradient of fmha_fwd_mla / fmha_varlen_fwd_mla from dout (like o), the forward's inputs, its
 * o and its softmax_lse: dq (like q), dk (like k), dv (like v).  Three launches on `stream`:
 *   fmha_bwd_mla_pre_kernel   D[row] = sum over the 128 columns of dout * o (fp32);
 *   fmha_bwd_mla_dkdv_kernel  one workgroup a 128-key block of one (batch, kv head): dk, dv;
 *   fmha_bwd_mla_dq_kernel    one workgroup a 128-row block of one (batch, head): dq.
 * No atomics: every output element has one writer and one summation order, so results are
 * bitwise reproducible and there is no deterministic flag, no fp32 dq accumulator and no
 * workspace.  The only scratch is D, num_heads x tokens fp32 laid out like softmax_lse: the
 * caller's softmax_d, or with softmax_d == NULL the stream's scratch pool (the first call on a
 * stream allocates it: warm a stream up before capturing a graph on it).
 * Every dq / dk / dv element of every sequence is written, exact zeros for rows without a visible
 * key and keys no row sees; nothing else is.  Windows as the forward; no ALiBi, softcap, dropout,
 * sink or seqused_k.  fmha_last_kernel() names the three kernels and the dq grid.
 *
 * fmha_bwd_mla: dense tensors as fmha_fwd_mla; strides[24] = {batch, row, head} of q, k, v, out,
 * dout, dq, dk, dv; softmax_lse (and softmax_d) fp32 [batch, heads, seqlen_q] contiguous.
 * fmha_varlen_bwd_mla: packed tensors as fmha_varlen_fwd_mla; strides[16] = {row, head} of the
 * same eight; softmax_lse (and softmax_d) fp32 [heads, total_q].
 *
 * Refused with an error, nothing launched, outputs untouched: what fmha_fwd_mla refuses (for
 * all eight tensors: dq as q, dk as k, dv as v, out and dout as o), and a NULL dout /
 * softmax_lse / dq / dk / dv; the message names the argument. */
void fmha_bwd_mla(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
                  void* dq, void* dk, void* dv, void* softmax_d /* nullable: pool */,
                  int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                  int32_t num_heads_k, int32_t head_size_qk /* 192 */, int32_t head_size_v /* 128 */,
                  const int64_t* strides /* q,k,v,out,dout,dq,dk,dv: batch,row,head */,
                  float softmax_scale, int window_size_left, int window_size_right, bool is_fp16,
                  hipStream_t stream);
void fmha_varlen_bwd_mla(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
                         void* dq, void* dk, void* dv, void* softmax_d /* nullable: pool */,
                         void* cu_seqlens_q, void* cu_seqlens_k, int32_t max_seqlen_q,
                         int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t batch_size,
                         int32_t num_heads, int32_t num_heads_k, int32_t head_size_qk /* 192 */,
                         int32_t head_size_v /* 128 */,
                         const int64_t* strides /* q,k,v,out,dout,dq,dk,dv: row,head */,
                         float softmax_scale, int window_size_left, int window_size_right,
                         bool is_fp16, hipStream_t stream);

#ifdef __cplusplus
} /* extern "C" */
#endif
#undef FMHA_DEFAULT
