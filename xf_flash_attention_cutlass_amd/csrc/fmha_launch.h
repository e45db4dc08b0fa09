// fmha_launch.h — internal host-side launch interface (one object file per head dim x dtype).
// Replaces the reference's template fan-out run_mha_fwd_splitkv_dispatch / run_flash_splitkv_fwd
// (flash_fwd_launch_template_hip.h:106-189) and the bwd launch template
// (flash_bwd_launch_template_hip.h:76-136).
#pragma once

#include "fmha_common.h"
#include "fmha_fwd_sched.h"

#include <atomic>

#ifndef XFA_VARIANTS
// 0: the product library.  1 (build.py --variants, lib/variants/): also the kernels no default
// path runs, kept for A/B and the bit-identity tests: the 4-wave D = 128 forward (fwd_w4 = 1) and
// the 8-wave ping-pong fp8 forward (fp8_w4 = 2)
#define XFA_VARIANTS 0
#endif

namespace xfa {

// Tuning knobs, settable through fmha_set_option() (schedule choices with equal results; the
// parity suite runs under any of them via XFA_TEST_OPTIONS).  The one list of them: Options,
// fmha_set_option and fmha_get_option all expand it.  X(name, default, lo, hi); two knobs take
// only the ends of their range (fwd_waves 4 | 8, dec_mr 16 | 32: fmha_set_option).
#define XFA_KNOBS(X)                                                                              \
    /* D = 128 forward where eligible: 4 auto (3 where no row has a right window, else 2); 3 the  \
       ping-pong on the 16x16x32 MFMA (r6: non-causal C2 +1.5-2.8 %, causal -1.3-3.4 % against 2, \
       same box); 2 the 8-wave ping-pong kernel (fmha_fwdpp_kernel.h; round 5, same box: C2       \
       causal +2-3 %, C4 +3 %, non-causal equal), 1 the 4-wave kernel (fmha_fwd4_kernel.h, the    \
       variants build only), 0 neither (8-wave fmha_fwd_kernel) */                                \
    X(fwd_w4, 4, 0, 4)                                                                            \
    /* the 32x32x16 ping-pong body generated without the score features and the left window       \
       (fwdpp_plain_item_*) for the launches with neither; 0 the full body everywhere.  Same bits \
       (tests/test_fwdpp_plain_gpu.py).  Same box, alternating with the library before it, 9      \
       rounds: C2 causal 1159-1162 vs 1129-1134 TFLOP/s (+2.4 %), C4 +2.3 %, sq 2048 / sk 4096    \
       +2.3 %; VALU 87.2 M vs 92.0 M, SALU 16.5 M vs 19.6 M per C2 launch */     \
    X(fwd_plain, 1, 0, 1)                                                                         \
    /* 4-wave fp8 forward (fmha_fwd8w_kernel.h) where eligible (C2 shape, same box: 1610 vs 1576  \
       TFLOP/s causal, 1852 vs 1799 non-causal); 2 the ping-pong one (the variants build only) */ \
    X(fp8_w4, 1, 0, 2)                                                                            \
    /* waves per forward workgroup (4 or 8); 32 query rows per wave */                            \
    X(fwd_waves, 8, 4, 8)                                                                         \
    /* static s_setprio 1 for the younger half of the workgroup */                                \
    X(fwd_prio, 0, 0, 1)                                                                          \
    /* persistent grid (workgroups per CU; 0 = one workgroup per item) */                         \
    X(fwd_persistent, 1, 0, 8)                                                                    \
    /* deferred rescale: running max may lag by this many log2 units */                           \
    X(fwd_slack, 8, 0, 16)                                                                        \
    /* persistent item order: 0 boustrophedon, 1 XCD-grouped pairs */                             \
    X(fwd_order, 1, 0, 1)                                                                         \
    /* dynamic item queue: 0 never, 1 varlen only, 2 every persistent launch */                   \
    X(fwd_dyn, 1, 0, 2)                                                                           \
    /* dynamic queue kind: 1 one unit-major queue per XCD, 0 one global heaviest-row-block-first  \
       queue */                                                                                   \
    X(fwd_xcdq, 1, 0, 1)                                                                          \
    /* software-pipelined loop over the unmasked key tiles */                                     \
    X(fwd_pipe, 1, 0, 2)                                                                          \
    /* split-KV decode kernel when seqlen_q * H/Hk <= 32 */                                       \
    X(fwd_decode, 1, 0, 1)                                                                        \
    /* decode split target: workgroups per CU over all (b, kv head) */                            \
    X(dec_wg_per_cu, 2, 1, 16)                                                                    \
    /* decode MFMA rows: 16 when the query rows fit 16 (C5: 105 vs 110 us with dec_hmaj = 1),     \
       else 32 */                                                                                 \
    X(dec_mr, 16, 16, 32)                                                                         \
    /* split combine: one workgroup per row when rows are few */                                  \
    X(comb_row, 1, 0, 1)                                                                          \
    /* decode: the last split of each (b, kv head) merges the partials (no separate combine       \
       launch; C5: 126.8 vs 105.5 us - the coherent partial stores and the 64-wave merge tail     \
       cost more than the 5 us combine launch they replace) */                                    \
    X(dec_fold, 0, 0, 1)                                                                          \
    /* decode over per-sequence cache lengths (2 <= b <= 64): split slots shared in proportion to \
       the key tiles (ragged caches) */                                                           \
    X(dec_bal, 1, 0, 1)                                                                           \
    /* backward grid: 1 = the key blocks of one (b, kv head) consecutive on one XCD (they then    \
       sweep the same Q / dO tiles together; C3: 3.03 vs 2.88 ms - their dQ atomics then collide) */ \
    X(bwd_order, 0, 0, 1)                                                                         \
    /* backward query-tile sweep: 1 = last tile first (C3 on the round-3 session-2 kernel: 2.496  \
       vs 2.513 ms, non-causal 4.410 vs 4.423; dK/dV equal up to fp32 summation order) */         \
    X(bwd_desc, 1, 0, 1)                                                                          \
    /* decode workgroup: 0 = 1 kv head x 4 splits, 1 = 4 kv heads x one split, 2 = 8 kv heads x   \
       one split (C5 fp8: 116 / 110 / 112 us) */                                                  \
    X(dec_hmaj, 1, 0, 2)

// Atomic: a launch on another thread reads each knob once, as a whole value.
struct Options {
#define XFA_KNOB_FIELD(name, def, lo, hi) std::atomic<int> name{def};
    XFA_KNOBS(XFA_KNOB_FIELD)
#undef XFA_KNOB_FIELD
};
Options& options();

// Records which forward kernel (and schedule) a launch used, for fmha_last_kernel(): the name,
// the persistent mode (0 = one workgroup per item, 1 boustrophedon, 2 XCD-grouped pairs,
// 3 dynamic queue), the per-XCD queues flag and the grid.  Thread-local, set by the launchers.
void note_launch(const char* kernel, int persistent, int xcdq, unsigned gx, unsigned gy, unsigned gz, int block);
// ... and which generated body the kernel ran where one kernel name covers several: a trailing
// " body=<name>" field of the same record (after note_launch)
void note_body(const char* body);

// Which mechanism applies the attention sink of a launch with p.sink: the
// launcher records it, the C ABI then runs the post-pass where it is kSinkPass and names the
// mechanism in fmha_last_kernel().  Thread-local, cleared by every forward entry.
enum SinkMech { kSinkNone = 0, kSinkEpilogue, kSinkCombine, kSinkPass };
void note_sink(SinkMech mech);

// The schedule of one forward launch, shared by every forward launcher: the params as the
// kernel gets them (n_mblocks, persistent, xcd_queues filled in) and the grid.  An item is one
// row block of `rows_per_item` query rows (seqlen_q * group of them) of one (b, kv head);
// `slots` workgroups stay resident once there are more items than slots (and fwd_persistent
// > 0), else one workgroup runs one item.  By the kernel's FwdQueue (fmha_fwd_sched.h, where
// the modes are described and fwd_walk walks them):
//   kQueueStatic: boustrophedon (1) or XCD-grouped pairs (2, fwd_order = 1 and slots % 8 == 0);
//   kQueueXcd:    the same, or with p.work_ctr the dynamic item queue (3), one queue per XCD
//                 where fwd_xcdq asks and the slots and (b, kv head) units fill 8 XCDs;
//   kQueueRagged: the 8-wave fp8 kernel's packed launches (it has no per-XCD queues): one
//                 dynamic queue as soon as there are more items than CUs, walked by
//                 min(items, slots) workgroups.
struct FwdPlan { FwdParams pp; dim3 grid; };
inline FwdPlan plan_fwd(const FwdParams& p, int rows_per_item, int slots, int splits, FwdQueue queue) {
    FwdPlan s{p, dim3()};
    const int n_mb = (p.seqlen_q * p.group + rows_per_item - 1) / rows_per_item;
    const int items = p.b * p.hk * n_mb;
    const unsigned gz = splits > 1 ? splits : 1;
    s.pp.n_mblocks = n_mb;
    s.pp.persistent = 0;
    s.pp.xcd_queues = 0;
    s.grid = dim3(p.b * p.hk, n_mb, gz);
    if (p.persist_per_cu <= 0) return s;
    if (queue == kQueueRagged) {
        if (items > p.num_cus) { s.pp.persistent = 3; s.grid = dim3(items < slots ? items : slots, 1, gz); }
    } else if (items > slots) {
        const bool dyn = queue == kQueueXcd && p.work_ctr;
        s.pp.persistent = dyn ? 3 : (p.order == 1 && slots % 8 == 0) ? 2 : 1;
        s.pp.xcd_queues = dyn && p.xcdq && slots % 8 == 0 && p.b * p.hk >= 8;
        s.grid = dim3(slots, 1, gz);
    }
    return s;
}

// Raises the dynamic-LDS limit of the kernels of one launcher, once per device.
template <auto... Kernels>
inline void allow_lds(int device, int bytes) {
    static std::atomic<unsigned long long> done{0};
    once_per_device(done, device, [&] {
        ((void)hipFuncSetAttribute((const void*)Kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), ...);
    });
}
// The tail of every planned launch: the record for fmha_last_kernel(), the launch, its status.
inline hipError_t launch_planned(const char* name, void (*kern)(const FwdParams), const FwdPlan& s,
                                 int block, size_t lds, hipStream_t st) {
    note_launch(name, s.pp.persistent, s.pp.xcd_queues, s.grid.x, s.grid.y, s.grid.z, block);
    hipLaunchKernelGGL(kern, s.grid, dim3(block), lds, st, s.pp);
    return hipGetLastError();
}

// Forward for head dim bucket HD (64 or 128) and dtype; launches the combine when
// p.num_splits > 1.  Returns the launch status.
hipError_t launch_fwd_hd64_bf16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_hd64_f16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_hd128_bf16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_hd128_f16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_hd256_bf16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_hd256_f16(const FwdParams& p, hipStream_t st);

// Backward (preprocess + main + convert) for head dim bucket HD.
hipError_t launch_bwd_hd64_bf16(const BwdParams& p, hipStream_t st);
hipError_t launch_bwd_hd64_f16(const BwdParams& p, hipStream_t st);
hipError_t launch_bwd_hd128_bf16(const BwdParams& p, hipStream_t st);
hipError_t launch_bwd_hd128_f16(const BwdParams& p, hipStream_t st);
hipError_t launch_bwd_hd256_bf16(const BwdParams& p, hipStream_t st);
hipError_t launch_bwd_hd256_f16(const BwdParams& p, hipStream_t st);

// fp8 (e4m3fn) Q/K/V forward, D = 128 (fmha_fwd_fp8.hip): bf16 or fp16 output.
hipError_t launch_fwd_fp8(const FwdParams& p, bool out_fp16, hipStream_t st);
// return_softmax with dropout: the dropped-out softmax [b, h, sq_r, sk_r] (fmha_sdmask_kernel.h)
hipError_t launch_sdmask_bf16(const FwdParams& p, void* s, int sq_r, int sk_r, hipStream_t st);
hipError_t launch_sdmask_f16(const FwdParams& p, void* s, int sq_r, int sk_r, hipStream_t st);

// KV-cache append (+ rotary) pass, fmha_append.hip
struct AppendParams {
    const void* q; void* q_out;
    void* kcache; void* vcache;
    const void* knew; const void* vnew;
    const int* block_table; int bt_stride; int page;
    const int* cache_seqlens; int* seqlens_out;
    const void* cos; const void* sin; int rdim; int interleaved; int q_per_token;
    int b, sq, h, hk, d, snew;
    int64_t q_batch, q_row, q_head;          // elements (q and q_out share the layout)
    int64_t kn_batch, kn_row, kn_head;       // elements (knew / vnew share the layout)
    int64_t page_stride, row_stride, head_stride;   // cache strides (elements)
    int cache_fp8;                           // 1: the caches hold OCP fp8 e4m3fn bytes, written as
    float k_inv, v_inv;                      //    e4m3(clamp(value x k_inv / v_inv, +-448))
};
hipError_t launch_append(const AppendParams& p, bool fp16, hipStream_t st);

// bf16 / fp16 -> fp8 e4m3fn quantisation with its descales (fmha_quant.hip)
struct QuantParams {
    const void* x;                    // [b, s, h, d] by element strides, or packed [total, h, d]
    void* x8;                         // contiguous e4m3fn bytes of the same logical shape
    float* descale;                   // [1] (gran 0) or [b, h / group]
    unsigned* amax;                   // scratch of the same count: max |x| as float bits
    const int* cu;                    // packed: cu_seqlens [b + 1] (then s = the longest sequence)
    int b, s, h, group, d, gran;
    int64_t x_batch, x_row, x_head;   // elements
};
hipError_t launch_quantize_fp8(const QuantParams& p, bool fp16, hipStream_t st);

// Causal ALiBi LSE convention (fmha_append.hip): the kernels bias a causal score by
// -slope |pos + diag - key| (its largest value 0 sits on the diagonal, which the in-loop
// reference max needs), the reference by +slope key (mask_hip.h:163-164); the two differ by the
// row constant slope (pos + diag), diag = sk - sq per sequence.  dst[row] = src[row] +
// sign * slope (pos + diag) for finite entries: sign +1 turns the kernels' LSE into the
// reference's (forward), -1 back (backward input).
struct LseAlibiParams {
    const float* src;
    float* dst;
    float sign;
    const float* alibi;
    int alibi_bstride;
    int b, h, seqlen_q, seqlen_k;
    const int* cu_seqlens_q;
    const int* cu_seqlens_k;
    const int* seqused_k;
    const int* leftpad_k;
    int64_t lse_batch, lse_head;
};
hipError_t launch_lse_alibi(const LseAlibiParams& p, hipStream_t st);

// Attention-sink post-pass (fmha_append.hip), for launches that end in a generated body or in
// the folded decode merge: in place, O[row] *= f and LSE[row] = merged over all (batch, row,
// head) with f and the merged LSE from sink_merge(LSE[row], sink[head]).  O by the call's own
// element strides, LSE [.., rows] by its strides; a packed (varlen) launch is batch 1 with
// rows = total_q.  Rows with f == 1 are not stored, rows without keys (LSE = +inf) are left alone.
struct SinkPassParams {
    void* o;
    float* lse;
    const float* sink;
    int64_t o_batch, o_row, o_head;
    int64_t lse_batch, lse_head;
    int b, h, rows, d;
};
hipError_t launch_sink_pass(const SinkPassParams& p, bool fp16, hipStream_t st);

// Gradient of the attention sink (fmha_bwd.hip): dsink[h] = - sum_(b, row) exp(sink[h] - LSE) D
// over LSE / D [b][h][rows] by element strides
struct SinkBwdParams {
    const float* lse;
    const float* dsum;
    const float* sink;
    float* dsink;
    int b, h, rows;
    int64_t batch_stride, head_stride;
};
hipError_t launch_bwd_sink(const SinkBwdParams& p, hipStream_t st);

// Merge of partial attention states (fmha_merge.hip): n parts (O_i, LSE_i) -> (O, LSE), the part
// pointers by value.  O by element strides (the parts share one set), LSE [.., rows] by its
// strides; a packed input is batch 1 with rows = total_q.  o / lse may be part 0's buffers.
constexpr int kMergeMaxParts = 16;    // FMHA_MERGE_MAX_PARTS of the header
struct MergeParams {
    const void* o_parts[kMergeMaxParts];
    const float* lse_parts[kMergeMaxParts];
    void* o;
    float* lse;                       // or null
    const float* sink;                // fp32 [h] or null
    int64_t po_batch, po_row, po_head;
    int64_t o_batch, o_row, o_head;
    int64_t pl_batch, pl_head;
    int64_t l_batch, l_head;
    int n, b, rows, h, d;
};
hipError_t launch_merge_states(const MergeParams& p, bool fp16, hipStream_t st);

// MLA decode over a paged latent cache (fmha_mla.hip): the decode kernel and, for
// p.num_splits > 1, the split combine at head size 512
hipError_t launch_mla_decode(const MlaParams& p, bool fp16, hipStream_t st);
// ... and over an fp8 latent cache (p.kv: rows of 656 bytes, fmha_mla_decode_fp8_kernel.h)
hipError_t launch_mla_decode_fp8(const MlaParams& p, bool fp16, hipStream_t st);
// ... and over index-selected tokens of either cache (p.indices, fmha_mla_decode_sparse_kernel.h
// and fmha_mla_decode_sparse_fp8_kernel.h)
hipError_t launch_mla_decode_sparse(const MlaParams& p, bool fp8, bool fp16, hipStream_t st);

// MLA prefill (fmha_fwd_mla.hip): the forward at head size 192 for Q K^T and 128 for V; one pass
// (p.num_splits = 1), none of the score features, p.d unused
hipError_t launch_fwd_mla_bf16(const FwdParams& p, hipStream_t st);
hipError_t launch_fwd_mla_f16(const FwdParams& p, hipStream_t st);
// ... and its backward (fmha_bwd_mla.hip): preprocess -> dK/dV -> dQ, no atomics and no workspace
// but p.dsum (fp32, laid out like the LSE); tokens: the query rows of the whole batch
hipError_t launch_bwd_mla_bf16(const BwdParams& p, int64_t tokens, hipStream_t st);
hipError_t launch_bwd_mla_f16(const BwdParams& p, int64_t tokens, hipStream_t st);

// Append to an fp8 latent cache (fmha_append.hip): token t's 512 latent features, quantised per
// 128-feature group, and its 64 rotary features, copied, into the 656-byte row slot[t] of the
// cache; row strides in elements.  A slot outside [0, slots) writes nothing.
struct MlaAppendParams {
    const void* latent;        // [tokens, 512]
    const void* k_pe;          // [tokens, 64]
    void* cache;               // [slots, 656] bytes
    const int64_t* slot;       // [tokens]
    int64_t latent_row, pe_row;
    int64_t slots;
    int tokens;
};
hipError_t launch_mla_append_fp8(const MlaAppendParams& p, bool fp16, hipStream_t st);

// D = 256 (bucket of 129..256): 4 waves x 32 rows, one wave per SIMD (512 registers:
// Q fragments and the O accumulator alone are 192), no LDS-DMA pipeline
inline int fwd_block_m(int d, int waves) { return d > 128 ? 128 : waves * 32; }
inline int fwd_num_m_blocks(int seqlen_q, int group, int d, int waves) {
    return (seqlen_q * group + fwd_block_m(d, waves) - 1) / fwd_block_m(d, waves);
}

}  // namespace xfa
