// fmha_fwd_kernel.h — fused QK^T -> online softmax -> PV forward for gfx950 (CDNA4).
//
// Replaces the reference's hot kernel `compute_attn_1rowblock_splitkv`
// (csrc/flash_attn/src/flash_fwd_kernel_hip.h:585-1283) and its combine
// `combine_attn_seqk_parallel` (:1322-1568).  Same math (online softmax with exp2 and the
// scale folded into one FMA, bottom-right aligned causal/local windows, ALiBi, softcap,
// varlen, paged K/V, split-KV + LSE combine), re-designed for CDNA4:
//
//  * one workgroup = NW waves; each wave owns 32 query rows -> BLOCK_M = 32*NW rows;
//    GQA groups are packed into the row dimension (row = pos*G + g), so the G query heads
//    sharing a K/V head share every K/V tile (the reference swaps only for Sq == 1,
//    export.cpp:526-532);
//  * S^T = K * Q^T with v_mfma_f32_32x32x16_{bf16,f16}: the accumulator holds 16 keys of ONE
//    query row per lane (row = lane & 31), so row max / row sum are lane-local plus one
//    v_permlane32_swap; the P accumulator is then, after a pairwise cvt, directly the B operand
//    of O^T += V^T * P^T (no LDS round trip for P) and the O^T accumulator keeps one query row
//    per lane, so the online-softmax rescale is lane-local too;
//  * K and V tiles (64 keys x HD) are register-staged into a double-buffered, XOR-swizzled LDS
//    image (one barrier per tile); K is read with ds_read_b128, V with the gfx950 transposing
//    ds_read_b64_tr_b16 — both conflict-free on the same image;
//  * masking runs only on the tiles that cross a window edge; tiles a wave cannot see are
//    skipped by that wave (wave-uniform branch); the heaviest causal row blocks launch first.
// This file's own: the item body's schedules (fwd_item: the register-staged and LDS-DMA masked
// loops, the 4-buffer pipeline), the score features, leftpad, split-KV, sink and dropout, the
// dropout key write-back and the split-KV combines.  The row geometry, the softmax state, the
// tile pieces, the asm V^T read ring, the DMA piece offsets and the epilogue under the schedules
// are fmha_fwd_tile.h's (shared with fwd_mla_item); the item schedules and the loop over a
// workgroup's items are fmha_fwd_sched.h's.
#pragma once

#include "fmha_common.h"
#include "fmha_fwd_sched.h"
#include "fmha_fwd_tile.h"

namespace xfa {

#ifndef XFA_SCHED_FENCE
#define XFA_SCHED_FENCE 1
#endif
constexpr bool SCHED_FENCE = XFA_SCHED_FENCE;


// One work item = (batch x kv-head, query row block, split).  SINK: the instantiation the _sink
// entries launch, whose epilogue merges the attention sink; the others compile to the code they
// had before sinks existed (a runtime branch in the shared epilogue measured + 0.75 % on the
// B2 S4096 H64/Hk8 D64 window (127, 0) forward, profiles/sink_ab.log).
template <int HD, typename T, int NW, bool MASK, bool FEAT, bool SINK = false>
__device__ __forceinline__ void fwd_item(const FwdParams& p, char* smem, const int bh,
                                         const int m_block, const int split) {
    using V8 = typename DT<T>::v8;
    constexpr int NT = NW * 64;
    constexpr int BM = NW * 32;
    constexpr int CPR = HD / 8;                 // 16-byte chunks per K/V row
    constexpr int NLD = kBlockN * CPR / NT;     // chunks per thread per tile
    constexpr int TILE = kBlockN * HD * 2;      // bytes of one K (or V) tile
    // LDS buffers (K and V tile each): D <= 128 runs the 4-buffer LDS-DMA pipeline; D = 256
    // (32 KiB tiles) only the double-buffered register-staged loop, 128 KiB of LDS
    constexpr int NBUF = fwd_nbuf(HD);
    constexpr bool PIPE = HD <= 128;
    constexpr int VREG = NBUF * TILE;           // LDS: K tiles of buffers 0..3, then V tiles
    constexpr int NS = HD / 16;                 // k-steps of the QK^T product
    constexpr int ND = HD / 32;                 // 32-wide d tiles of O^T
    static_assert(NLD >= 1 && (NT % CPR) == 0, "tile/thread geometry");
    // Pieces the FEAT instances keep a copy of.  These instances spill (92 - 224 bytes a lane),
    // and through fmha_fwd_tile.h's edge_mask + raise_max (D <= 128) or qk (D = 256) ten of them
    // spilled 4 - 16 bytes more than before the header existed, part of it inside the tile loops;
    // with the copies none does (profiles/fwd_tile_isa_diff.txt).  The other instances take the
    // shared pieces: with these copies their D = 128 4-wave builds spill up to 76 bytes more.
    constexpr bool OWN_MASK_MAX = FEAT && PIPE, OWN_QK = FEAT && !PIPE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hh = lane >> 5;

    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;

    int q_off = 0, sq = p.seqlen_q, k_off = 0, sk = p.seqlen_k;
    // varlen / seqused_k: scalar offsets only (not a FEAT specialisation)
    if (p.cu_seqlens_q) { q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off; }
    if (p.cu_seqlens_k) { k_off = p.cu_seqlens_k[bidx]; sk = p.cu_seqlens_k[bidx + 1] - k_off; }
    if (p.seqused_k) sk = p.seqused_k[bidx];
    // cache_leftpad (block_info.h leftpad_k): the sequence is cache rows [lp, sk)
    const int lp = p.leftpad_k ? p.leftpad_k[bidx] : 0;
    sk -= lp;
    const int row0 = m_block * BM;
    if (row0 >= sq * p.group) return;
    const RowGeom<MASK> g(p, sq, sk, p.group, hk_i, row0, BM, wave, lane & 31, kNoFloor);
    const int pos = g.pos, head = g.head, diag = g.diag;
    // Key-tile range of the workgroup, and of this split.
    int nb_lo = g.nb_lo, nb_hi = g.nb_hi;
    const bool is_split = p.num_splits > 1;
    if (is_split) {
        const int per = (nb_hi - nb_lo + p.num_splits - 1) / p.num_splits;
        const int s_lo = nb_lo + split * per;
        nb_hi = min(nb_hi, s_lo + per);
        nb_lo = min(s_lo, nb_hi);
    }

    float alibi_w = 0.f;
    if (FEAT && p.alibi) alibi_w = p.alibi[bidx * p.alibi_bstride + head] * p.alibi_mul;
    const float c = p.scale_log2;

    V8 qf[NS];
    q_frags(q_row<T>(p, bidx, q_off, sq, p.d, g.row_ok, pos, head, hh), qf, p.d);

    // ---- K/V tile loader (register staged: issue early, write to LDS late)
    const int lc = tid % CPR;
    const int lrow0 = tid / CPR;
    constexpr int LROW_STEP = NT / CPR;
    const bool lc_ok = lc * 8 < p.d;
    const bool paged = FEAT && p.block_table != nullptr;
    // fp8 (OCP e4m3fn) K/V: 1-byte elements, dequantised to T with the per-tensor scale while
    // staging (the LDS image and everything after it are unchanged)
    const bool kv8 = FEAT && p.kv_fp8;
    const int esz = kv8 ? 1 : 2;
    // dense / varlen: one SRD per K and V covering this sequence's rows of this kv head
    const char* kseq = reinterpret_cast<const char*>(p.k) +
                       ((int64_t)bidx * p.k_batch + (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head) * esz;
    const char* vseq = reinterpret_cast<const char*>(p.v) +
                       ((int64_t)bidx * p.v_batch + (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head) * esz;
    const uint32_t kbytes = (uint32_t)(((int64_t)(sk > 0 ? sk - 1 : 0) * p.k_row + p.d) * esz);
    const uint32_t vbytes = (uint32_t)(((int64_t)(sk > 0 ? sk - 1 : 0) * p.v_row + p.d) * esz);
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(kseq, kbytes);
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(vseq, vbytes);
    // paged: per-row page pointers (clamped, unconditional loads + data select)
    const char* kpool = reinterpret_cast<const char*>(p.k) + ((int64_t)hk_i * p.k_head + lc * 8) * esz;
    const char* vpool = reinterpret_cast<const char*>(p.v) + ((int64_t)hk_i * p.v_head + lc * 8) * esz;
    const int* btab = paged ? p.block_table + (int64_t)bidx * p.bt_stride : nullptr;

    u32x4 kr[NLD], vr[NLD];
    auto load_to = [&](int nb, u32x4 (&ko)[NLD], u32x4 (&vo)[NLD]) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = nb * kBlockN + lrow0 + i * LROW_STEP;
            const bool ok = lc_ok && n < sk;
            if (paged) {
                const int nc = (ok ? n : 0) + lp;
                const int pi = nc / p.page_size;
                const int pg = btab[pi];
                const int pr = nc - pi * p.page_size;
                const char* ka = kpool + ((int64_t)pg * p.k_batch + (int64_t)pr * p.k_row) * esz;
                const char* va = vpool + ((int64_t)pg * p.v_batch + (int64_t)pr * p.v_row) * esz;
                if (kv8) {
                    const uint2 kx = *reinterpret_cast<const uint2*>(ka);
                    const uint2 vx = *reinterpret_cast<const uint2*>(va);
                    ko[i] = ok ? fp8x8_to<T>(kx.x, kx.y, p.k_scale) : u32x4{0, 0, 0, 0};
                    vo[i] = ok ? fp8x8_to<T>(vx.x, vx.y, p.v_scale) : u32x4{0, 0, 0, 0};
                } else {
                    const u32x4 kx = *reinterpret_cast<const u32x4*>(ka);
                    const u32x4 vx = *reinterpret_cast<const u32x4*>(va);
                    ko[i] = ok ? kx : u32x4{0, 0, 0, 0};
                    vo[i] = ok ? vx : u32x4{0, 0, 0, 0};
                }
            } else if (kv8) {
                const u32x2 kx = buf_load8(krs, ok ? n * (int)p.k_row + lc * 8 : kOOB);
                const u32x2 vx = buf_load8(vrs, ok ? n * (int)p.v_row + lc * 8 : kOOB);
                ko[i] = fp8x8_to<T>(kx[0], kx[1], p.k_scale);
                vo[i] = fp8x8_to<T>(vx[0], vx[1], p.v_scale);
            } else {
                ko[i] = buf_load16(krs, ok ? n * (int)p.k_row * 2 + lc * 16 : kOOB);
                vo[i] = buf_load16(vrs, ok ? n * (int)p.v_row * 2 + lc * 16 : kOOB);
            }
        }
    };
    auto store_from = [&](int buf, const u32x4 (&ki)[NLD], const u32x4 (&vi)[NLD]) {
        char* ks = smem + buf * TILE;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int r = lrow0 + i * LROW_STEP;
            *reinterpret_cast<u32x4*>(ks + kv_off<HD>(r, lc)) = ki[i];
            *reinterpret_cast<u32x4*>(ks + VREG + kv_off<HD>(r, lc)) = vi[i];
        }
    };

    constexpr int RB = HD * 16;                 // bytes of one 8-row block of the kv_off image
    int kb[2], vb[2];                           // per-lane LDS read bases
    k_read_bases<HD>((int)(size_t)smem, lane, kb);
    v_read_bases<HD>((int)(size_t)smem + VREG, lane, vb);
    SoftmaxRow<ND> sm;

    // ---- the pieces of one 64-key tile (K / V in buffer `buf`)
    // V^T operand of O^T += V^T P^T for (kt, sp, dt) through the transposing LDS read
    auto rd_v = [&](const int buf, const int i) {
        const int kt = i / (2 * ND), sp = (i / ND) & 1, dt = i % ND;
        const int o = buf * TILE + (4 * kt + 2 * sp) * RB + 512 * dt;
        const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)(vb[0] + o));
        const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)(vb[1] + o));
        const s16x8 av = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        return __builtin_bit_cast(V8, av);
    };
    // score features of values [v0, v0 + n) (flattened st[kt][r], v = 16 kt + r), then the edge
    // mask where a window edge crosses the tile
    auto transform_part = [&](f32x16 (&st)[2], const int n0, const bool need_mask, const int v0,
                              const int n) {
        if constexpr (OWN_MASK_MAX) {         // (edge_mask, fused into the feature loop)
#pragma unroll
            for (int v = v0; v < v0 + n; ++v) {
                const int kt = v >> 4, r = v & 15;
                const int key = n0 + 4 * hh + key_of(v);
                if (p.softcap_pre > 0.f) st[kt][r] = fast_tanh(st[kt][r] * p.softcap_pre);
                if (p.alibi) st[kt][r] -= alibi_w * (float)abs(pos + diag - key);
                if (need_mask && (key >= g.my_lr || key < g.my_ll)) st[kt][r] = -INFINITY;
            }
            return;
        }
        if (FEAT) {
#pragma unroll
            for (int v = v0; v < v0 + n; ++v) {
                const int kt = v >> 4, r = v & 15;
                if (p.softcap_pre > 0.f) st[kt][r] = fast_tanh(st[kt][r] * p.softcap_pre);
                if (p.alibi) st[kt][r] -= alibi_w * (float)abs(pos + diag - (n0 + 4 * hh + key_of(v)));
            }
        }
        if (need_mask) edge_mask(st, n0, hh, g.my_lr, g.my_ll, v0, n);
    };
    // dropout on the P operand of PV (the row sums keep the undropped P, as the reference's
    // softmax does before apply_dropout, flash_fwd_kernel_hip.h): each run of 4 keys of this
    // lane's row draws one Philox block (fmha_common.h drop_block)
    auto drop_tile = [&](V8 (&pb)[4], const int n0) {
        if (!(FEAT && p.drop)) return;
        const int bhg = bidx * p.h + head;
        uint64_t dseed, doff;
        drop_key(p, dseed, doff);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 w = drop_block(dseed, doff, bhg, pos, n0 + 32 * kt + 8 * j + 4 * hh);
                const uint32_t word = (pos & 2) ? ((pos & 1) ? w[3] : w[2]) : ((pos & 1) ? w[1] : w[0]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (!drop_keep(word, i, p.keep_thr)) pb[2 * kt + (j >> 1)][(j & 1) * 4 + i] = (T)0.f;
            }
    };
    // O^T += V^T P^T (V^T reads one MFMA ahead)
    constexpr int NPV = 4 * ND;                 // PV MFMAs per tile
    auto pv = [&](const int vs, const V8 (&pb)[4]) {
        V8 a = rd_v(vs, 0);
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            V8 nx = a;
            if (i + 1 < NPV) nx = rd_v(vs, i + 1);
            sm.acc_o[i % ND] = DT<T>::mfma32(a, pb[i / ND], sm.acc_o[i % ND]);
            a = nx;
        }
    };
    // one tile of the per-wave masked loops
    auto masked_tile = [&](const int buf, const int n0) {
        f32x16 st[2];
        if constexpr (OWN_QK) {
            st[0] = f32x16{};
            st[1] = f32x16{};
            V8 a0 = rd_k<T, HD>(kb, buf * TILE, 0, 0), a1 = rd_k<T, HD>(kb, buf * TILE, 0, 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                V8 n0_ = a0, n1_ = a1;
                if (s + 1 < NS) { n0_ = rd_k<T, HD>(kb, buf * TILE, s + 1, 0); n1_ = rd_k<T, HD>(kb, buf * TILE, s + 1, 1); }
                st[0] = DT<T>::mfma32(a0, qf[s], st[0]);
                st[1] = DT<T>::mfma32(a1, qf[s], st[1]);
                a0 = n0_;
                a1 = n1_;
            }
        } else {
            qk<T, HD>(kb, buf * TILE, qf, st);
        }
        transform_part(st, n0, g.edge(n0), 0, 32);
        if constexpr (OWN_MASK_MAX) {         // (SoftmaxRow::raise_max)
            const float mx = row_max(st);
            const float m_new = fmaxf(sm.m_sc, mx * c);
            if (__any(m_new > sm.m_sc + p.max_slack)) {
                const float alpha = m_new == -INFINITY ? 1.f : fast_exp2(sm.m_sc - m_new);
                sm.l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sm.acc_o[dt][r] *= alpha;
                sm.m_sc = m_new;
            }
        } else {
            sm.raise_max(row_max(st), c, p.max_slack);
        }
        V8 pb[4];
        exp_tile<T>(sm, st, pb, c);
        drop_tile(pb, n0);
        pv(buf, pb);
    };

    // ---- tiles that need per-wave masking / skipping: one tile in flight, two LDS buffers
    auto masked_range = [&](const int lo, const int hi) {
        if (lo >= hi) return;
        load_to(lo, kr, vr);
        store_from(0, kr, vr);
        // Retire every outstanding load (Q fragments included) here: otherwise the loop-header
        // merge of the waitcnt scoreboard makes the first QK^T MFMA of EVERY iteration wait
        // vmcnt(0), i.e. drain the next tile's prefetch (vmcnt=0, expcnt=7, lgkmcnt=15).
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        int buf = 0;
        for (int nb = lo; nb < hi; ++nb) {
            const bool more = nb + 1 < hi;
            if (more) load_to(nb + 1, kr, vr);
            if (g.active(nb * kBlockN)) masked_tile(buf, nb * kBlockN);
            if (more) store_from(buf ^ 1, kr, vr);
            __syncthreads();
            buf ^= 1;
        }
    };

    // ---- tiles every row of the workgroup sees in full: two-stage software pipeline.
    // Step j issues QK^T of tile j+1 beside the softmax VALU of tile j, then PV of tile j beside
    // the row max of tile j+1 (T15): the MFMA pipe always has independent work while the VALU
    // finishes a tile.  K/V tiles stream straight into LDS (buffer_load ... lds, no staging
    // registers) three tiles ahead through NBUF = 4 rotating buffers: at step j buffer
    // (j+1)%4 holds K of j+1, j%4 holds V of j, and tiles j+2 (landing) and j+3 (issued now)
    // are in flight.  One raw s_barrier per tile, preceded by a counted vmcnt that retires
    // exactly tile j+2.  The LDS image is the same swizzled image the register-staged path
    // writes: lane l of a wave-instruction lands at +16 l, so it fetches the global chunk
    // (l % CPR) ^ swz(row) of its row.
    constexpr int IPW = TILE / 1024 / NW;          // DMA wave-instructions per wave per K (V) tile
    static_assert(IPW >= 1 && IPW * 1024 * NW == TILE, "DMA geometry");
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int dma_k[IPW], dma_v[IPW];                    // per-lane byte offsets within a tile
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        dma_k[i] = dma_piece_d<HD>(wave * IPW + i, lane, (int)p.k_row * 2, p.d);
        dma_v[i] = dma_piece_d<HD>(wave * IPW + i, lane, (int)p.v_row * 2, p.d);
    }
    typedef __attribute__((address_space(3))) void lds_void;
    auto dma_tile = [&](const int nb, const int buf) {
        // (soffset pinned to an SGPR: derived from a tile index the compiler kept in a VGPR,
        // each DMA piece became a waterfall loop)
        const int kso = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.k_row * 2);
        const int vso = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.v_row * 2);
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int piece = wave_u * IPW + i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                krs, (lds_void*)(smem + buf * TILE + piece * 1024), 16, dma_k[i], kso, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                vrs, (lds_void*)(smem + VREG + buf * TILE + piece * 1024), 16, dma_v[i], vso, 0, 0);
        }
    };
    constexpr int NDMA = 2 * IPW;                  // vmem instructions per tile per wave
    // D = 256 (no pipeline, NBUF = 2): the per-wave masked loop with K/V by LDS-DMA, tile
    // j+1 in flight while tile j computes (no staging registers: the 512-register budget is
    // taken by the Q fragments and the O accumulator)
    auto dma_range = [&](const int lo, const int hi) {
        if (lo >= hi) return;
        dma_tile(lo, 0);
        publish();
        int buf = 0;
        for (int nb = lo; nb < hi; ++nb) {
            if (nb + 1 < hi) dma_tile(nb + 1, buf ^ 1);
            if (g.active(nb * kBlockN)) masked_tile(buf, nb * kBlockN);
            publish();
            buf ^= 1;
        }
    };
    // Tiles [lo, hm) need no mask; tiles [hm, hi) (the causal diagonal / right window edge /
    // ragged end) are masked in registers on the way through the same pipeline (a wave whose
    // rows cannot see such a tile computes zeros for it instead of branching out of the
    // interleaved schedule).  Every row sees tile lo (f_lo lies past every row's left window
    // edge, and visible keys are contiguous), so only the right edge can cut a pipeline tile.
    //
    // Scores leave phase b already scaled and shifted, X = S c - m_sc, so phase a is exp + cvt
    // only; the VALU of a tile splits evenly between the two MFMA phases (per wave and tile:
    // a = 32 v_exp + 32 fp32 row-sum adds + 16 cvt beside 16 QK^T MFMAs, b = 32 fma + 16 max3
    // beside 16 PV MFMAs), each within the MFMA gaps.  The edge mask runs after phase b on the edge tiles only.
    const int lim_e = g.my_lr - 4 * hh;           // right edge of this lane's keys, minus its offset
    auto pipe_range = [&](const int lo, const int hm, const int hi) {
        const bool third = lo + 2 < hi;
        dma_tile(lo, 0);
        dma_tile(lo + 1, 1);
        if (third) dma_tile(lo + 2, 2);
        publish<NDMA>(third ? NDMA : 0);
        // scores ping-pong between sa and sb from step to step (st: this tile, sn: the next),
        // so the QK^T accumulators never need a register copy onto a loop-carried value
        f32x16 sa[2], sb[2];
        qk<T, HD>(kb, 0, qf, sa);
        transform_part(sa, lo * kBlockN, lo >= hm, 0, 32);
        sm.raise_max(row_max(sa), c, p.max_slack);
        scale_shift(sa, c, sm.exp_ref());
        const int nsteps = hi - lo - 1;
        auto step = [&](auto KB, auto VB, auto WB, const int j, f32x16 (&st)[2], f32x16 (&sn)[2]) {
            constexpr int ks = decltype(KB)::value, vs = decltype(VB)::value, wb = decltype(WB)::value;
            const bool issue = j + 3 < hi;
            if (issue) dma_tile(j + 3, wb);
            if (SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
            // phase a: S_{j+1} = K_{j+1} Q^T on the MFMA pipe, P_j = exp2(X_j) -> T on the VALU
            sn[0] = f32x16{};
            sn[1] = f32x16{};
            V8 pb[4];
            float rs = 0.f;                       // fp32 row sum of P_j
            constexpr int EV = 32 / (2 * NS);     // exp values per QK^T MFMA
            V8 a0 = rd_k<T, HD>(kb, ks * TILE, 0, 0), a1 = rd_k<T, HD>(kb, ks * TILE, 0, 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                V8 n0 = a0, n1 = a1;
                if (s + 1 < NS) { n0 = rd_k<T, HD>(kb, ks * TILE, s + 1, 0); n1 = rd_k<T, HD>(kb, ks * TILE, s + 1, 1); }
                sn[0] = DT<T>::mfma32(a0, qf[s], sn[0]);
                expx_part<T>(st, pb, rs, (2 * s) * EV, EV);
                sn[1] = DT<T>::mfma32(a1, qf[s], sn[1]);
                expx_part<T>(st, pb, rs, (2 * s + 1) * EV, EV);
                // pins the row-sum adds into this MFMA gap: unpinned, the compiler sinks them
                // below phase b (rs is only read there) into a VALU-only run of 32 adds
                // (+1.5-2 % C2, same-box A/B)
                asm volatile("" : "+v"(rs));
                a0 = n0;
                a1 = n1;
                if (SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
            }
            // phase b: O += V_j^T P_j on the MFMA pipe; on the VALU X_{j+1} = S_{j+1} c - m_sc
            // (transforms and edge mask first) and its row max, beside the asm V^T read ring
            constexpr int MV = 32 / NPV;          // score values per PV MFMA
            const float mr = sm.exp_ref();
            float mx = -INFINITY;
            pv_ring<T, HD, vs * TILE>(sm.acc_o, vb, pb, [&](auto I) {
                constexpr int i = decltype(I)::value;
                if (FEAT) transform_part(sn, (j + 1) * kBlockN, false, i * MV, MV);
#pragma unroll
                for (int v = i * MV; v < (i + 1) * MV; ++v)
                    sn[v >> 4][v & 15] = __builtin_fmaf(sn[v >> 4][v & 15], c, -mr);
                if constexpr (MV == 2) mx = fmaxf(fmaxf(mx, sn[(i * 2) >> 4][(i * 2) & 15]), sn[(i * 2 + 1) >> 4][(i * 2 + 1) & 15]);
                else {
#pragma unroll
                    for (int v = i * MV; v < (i + 1) * MV; ++v) mx = fmaxf(mx, sn[v >> 4][v & 15]);
                }
                if (SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
            });
            // an opaque use pins the max chain inside phase b (else it is sunk below the edge
            // branch, out of the MFMA gaps)
            asm volatile("" : "+v"(mx));
            sm.l_run += rs;
            // edge tile: mask, then the row max again
            if (j + 1 >= hm) mx = right_mask_max(sn, lim_e - (j + 1) * kBlockN);
            sm.rescale_x_halves(mx, sn, p.max_slack);
            publish<NDMA>(issue ? NDMA : 0);      // tile j+2 landed everywhere
        };
        typedef std::integral_constant<int, 0> I0;
        typedef std::integral_constant<int, 1> I1;
        typedef std::integral_constant<int, 2> I2;
        typedef std::integral_constant<int, 3> I3;
        // step r (tile j = lo + r) reads K of j+1 from buffer (r+1)%4 and V of j from r%4; a
        // wave runs the steps up to the last tile any of its rows sees (RowGeom::steps_w)
        const int nsteps_w = g.steps_w(nsteps, lo);
        int r = 0;
        while (r < nsteps_w) {
            step(I1{}, I0{}, I3{}, lo + r, sa, sb);
            if (++r >= nsteps_w) break;
            step(I2{}, I1{}, I0{}, lo + r, sb, sa);
            if (++r >= nsteps_w) break;
            step(I3{}, I2{}, I1{}, lo + r, sa, sb);
            if (++r >= nsteps_w) break;
            step(I0{}, I3{}, I2{}, lo + r, sb, sa);
            ++r;
        }
        // drain: the wave's last tile's softmax and PV.  V^T through the asm reads: a wave that
        // leaves early still has its DMA share of tile j+3 in flight, and the builtin
        // transposing read would make the compiler drain it (vmcnt(0)) first
        V8 pb[4];
        if (nsteps_w & 1) expx_tile<T>(sm, sb, pb);
        else expx_tile<T>(sm, sa, pb);
        switch (nsteps_w & 3) {
            case 0: pv_ring<T, HD, 0 * TILE>(sm.acc_o, vb, pb, [](auto) {}); break;
            case 1: pv_ring<T, HD, 1 * TILE>(sm.acc_o, vb, pb, [](auto) {}); break;
            case 2: pv_ring<T, HD, 2 * TILE>(sm.acc_o, vb, pb, [](auto) {}); break;
            default: pv_ring<T, HD, 3 * TILE>(sm.acc_o, vb, pb, [](auto) {}); break;
        }
        // the steps this wave skips: its DMA share and the barriers only
        for (; r < nsteps; ++r) {
            const int j = lo + r;
            const bool issue = j + 3 < hi;
            if (issue) dma_tile(j + 3, (r + 3) & 3);
            publish<NDMA>(issue ? NDMA : 0);
        }
        __syncthreads();
    };
    // Key tiles (RowGeom::pipe_split): [nb_lo, f_lo) run through the per-wave masked loop, the
    // rest through the pipeline, [f_hi, nb_hi) of them masked on the way.
    int f_lo = nb_hi, f_hi = nb_hi;
    if (PIPE && p.pipe && !paged && !kv8 && !(FEAT && p.drop)) {
        g.pipe_split(nb_lo, nb_hi, f_lo, f_hi);
        if (p.pipe == 2 && f_hi - f_lo < 2) f_lo = f_hi = nb_hi;
    }
    if (p.prio_hi && __builtin_amdgcn_readfirstlane(wave) >= NW / 2) __builtin_amdgcn_s_setprio(1);
    // (fwd_pipe=2: edge tiles through the per-wave masked loop instead - A/B knob)
    const int p_hi = (p.pipe == 2 && f_hi - f_lo >= 2) ? f_hi : nb_hi;
    if (!PIPE && !paged && !kv8) dma_range(nb_lo, f_lo);
    else masked_range(nb_lo, f_lo);
    if constexpr (PIPE) {
        if (f_lo < p_hi) pipe_range(f_lo, f_hi, p_hi);
    }
    masked_range(p_hi, nb_hi);

    // ---- epilogue: normalise, write O (or the split partial) and LSE
    const RowNorm n = sm.norm();
    const float inv = n.inv;
    if (!g.row_ok) return;
    if (is_split) {
        const int64_t rid = (((int64_t)split * p.b + bidx) * p.h + head) * p.seqlen_q + pos;
        float* oa = p.oaccum + rid * HD;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = 32 * dt + 8 * q + 4 * hh;
                f32x4 v = {sm.acc_o[dt][4 * q] * inv, sm.acc_o[dt][4 * q + 1] * inv,
                           sm.acc_o[dt][4 * q + 2] * inv, sm.acc_o[dt][4 * q + 3] * inv};
                *reinterpret_cast<f32x4*>(oa + d) = v;
            }
        if (hh == 0) p.lseaccum[rid] = n.empty ? -INFINITY : sm.lse(n);
        return;
    }
    if constexpr (SINK) {
        // attention sink, once per row, outside the key loop: `head` is the query head (GQA rows
        // are packed per kv head); the entries refuse dropout with a sink, so no rp_keep here
        float inv_o = inv, lse_o = INFINITY;
        if (!n.empty) {
            const SinkMerge sk_m = sink_merge(sm.lse(n), p.sink[head]);
            inv_o = inv * sk_m.f;
            lse_o = sk_m.lse;
        }
        store_row<T, ND>(p, bidx, q_off, pos, head, hh, sm.acc_o, inv_o, p.d, lse_o);
        return;
    }
    store_row<T, ND>(p, bidx, q_off, pos, head, hh, sm.acc_o, (FEAT && p.drop) ? inv * p.rp_keep : inv, p.d, sm.lse(n));
}

// Grid: one workgroup per item or persistent, as plan_fwd chose; fwd_walk (fmha_fwd_sched.h)
// runs this workgroup's items.
constexpr FwdQueue kFwdQueue = kQueueXcd;   // for plan_fwd and fwd_walk
template <int HD, typename T, int NW, bool MASK, bool FEAT>
__global__ void __launch_bounds__(NW * 64, fwd_waves_per_simd(HD)) fmha_fwd_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the key this launch used, for the backward (the reference writes params.rng_state the
    // same way, flash_fwd_kernel_hip.h); one lane of one workgroup
    if (FEAT && p.drop && p.rng_out && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 &&
        threadIdx.x == 0) {
        uint64_t dseed, doff;
        drop_key(p, dseed, doff);
        p.rng_out[0] = (int64_t)dseed;
        p.rng_out[1] = (int64_t)doff;
    }
    fwd_walk<kFwdQueue>(p, [&](int bh, int m_block) { fwd_item<HD, T, NW, MASK, FEAT>(p, smem, bh, m_block, blockIdx.z); });
}

// The same launch with an attention sink merged in the epilogue (one split, no dropout: the
// _sink entries refuse it); reported under fmha_fwd_kernel's name with " sink=epilogue".
template <int HD, typename T, int NW, bool MASK, bool FEAT>
__global__ void __launch_bounds__(NW * 64, fwd_waves_per_simd(HD)) fmha_fwd_sink_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fwd_walk<kFwdQueue>(p, [&](int bh, int m_block) { fwd_item<HD, T, NW, MASK, FEAT, true>(p, smem, bh, m_block, blockIdx.z); });
}

// Split-KV combine: lse = log sum_s exp(lse_s); O = sum_s exp(lse_s - lse) O_s
// (reference combine_attn_seqk_parallel, flash_fwd_kernel_hip.h:1322-1568; empty -> +inf).
// One wave per (b, h, pos) row.
template <int HD, typename T>
__global__ void __launch_bounds__(256) fmha_combine_kernel(const CombineParams cp) {
    // The split partials are independent loads: the LSE reduction runs with the splits across
    // the lanes, and the O sum keeps CU = 8 splits' rows in flight per wave (a serial loop over
    // splits exposes one load latency per split, which at 32 splits cost more than the bytes).
    const int lane = threadIdx.x & 63;
    const int64_t rid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t rows = (int64_t)cp.b * cp.h * cp.seqlen_q;
    if (rid >= rows) return;
    const int pos = (int)(rid % cp.seqlen_q);
    const int head = (int)((rid / cp.seqlen_q) % cp.h);
    const int bidx = (int)(rid / ((int64_t)cp.seqlen_q * cp.h));
    const int ns = cp.dec_ns ? cp.dec_ns[bidx] : cp.num_splits;
    float mx = -INFINITY;
    for (int s = lane; s < ns; s += 64) mx = fmaxf(mx, cp.lseaccum[s * rows + rid]);
    mx = wave_max_halves(mx);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.f;
    if (mx != -INFINITY)
        for (int s = lane; s < ns; s += 64) sum += __expf(cp.lseaccum[s * rows + rid] - mx);
    sum = wave_sum_halves(sum);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    const bool empty = (mx == -INFINITY) || sum == 0.f;
    float lse = empty ? INFINITY : __logf(sum) + mx;
    // attention sink: merged once after the splits; the partials are then weighted against the
    // merged LSE, which is also the one stored
    if (cp.sink && !empty) lse = sink_merge(lse, cp.sink[head]).lse;
    constexpr int PER = HD / 64;
    constexpr int CU = 8;
    typedef float __attribute__((ext_vector_type(PER))) fv;
    fv acc = {};
    if (!empty) {
        const float* oa = cp.oaccum + rid * HD + lane * PER;
        const int64_t sstride = rows * HD;
        int s = 0;
        for (; s + CU <= ns; s += CU) {
            fv x[CU];
            float w[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                x[u] = *reinterpret_cast<const fv*>(oa + (s + u) * sstride);
                w[u] = __expf(cp.lseaccum[(s + u) * rows + rid] - lse);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) acc += w[u] * x[u];
        }
        for (; s < ns; ++s)
            acc += __expf(cp.lseaccum[s * rows + rid] - lse) * *reinterpret_cast<const fv*>(oa + s * sstride);
    }
    T* orow = reinterpret_cast<T*>(cp.o) + (int64_t)bidx * cp.o_batch + (int64_t)pos * cp.o_row +
              (int64_t)head * cp.o_head;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int d = lane * PER + i;
        if (d < cp.d) orow[d] = (T)acc[i];
    }
    if (cp.lse && lane == 0)
        cp.lse[(int64_t)bidx * cp.lse_batch + (int64_t)head * cp.lse_head + pos] = lse;
}

// Split-KV combine, one workgroup per row (few rows: the decode shapes, where the per-wave kernel
// above leaves most CUs idle and waits one memory latency per batch of 8 splits).  Thread t owns
// float4 chunk t % (HD / 4) of the splits s = t / (HD / 4) (mod 256 / (HD / 4)): every partial
// row of the first 8 rounds is loaded before the LSE merge (wave 0, splits across lanes) has
// produced the weights, so the row costs about one memory latency; the 256 / (HD / 4) partial
// sums of a chunk meet in LDS.  HD in {64, 128, 256}, at most 128 splits.
template <int HD, typename T>
__global__ void __launch_bounds__(256) fmha_combine_row_kernel(const CombineParams cp) {
    constexpr int D4 = HD / 4;
    constexpr int G = 256 / D4;
    constexpr int NB = 8;
    static_assert(G * D4 == 256, "chunks per thread");
    __shared__ float wsh[128];
    __shared__ f32x4 red[G][D4];
    const int t = threadIdx.x;
    const int64_t rid = blockIdx.x;
    const int64_t rows = (int64_t)cp.b * cp.h * cp.seqlen_q;
    const int pos = (int)(rid % cp.seqlen_q);
    const int head = (int)((rid / cp.seqlen_q) % cp.h);
    const int bidx = (int)(rid / ((int64_t)cp.seqlen_q * cp.h));
    const int ns = cp.dec_ns ? cp.dec_ns[bidx] : cp.num_splits;
    const int c = t % D4, g = t / D4;
    const float* oa = cp.oaccum + rid * HD + 4 * c;
    const int64_t sstride = rows * HD;
    f32x4 x[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int sp = g + G * u;
        x[u] = sp < ns ? *reinterpret_cast<const f32x4*>(oa + sp * sstride) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (t < 64) {
        const float l0 = t < ns ? cp.lseaccum[t * rows + rid] : -INFINITY;
        const float l1 = t + 64 < ns ? cp.lseaccum[(t + 64) * rows + rid] : -INFINITY;
        float mx = wave_max_halves(fmaxf(l0, l1));
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        float sum = mx == -INFINITY ? 0.f : __expf(l0 - mx) + __expf(l1 - mx);
        sum = wave_sum_halves(sum);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        const bool empty = (mx == -INFINITY) || sum == 0.f;
        float lse = empty ? INFINITY : __logf(sum) + mx;
        if (cp.sink && !empty) lse = sink_merge(lse, cp.sink[head]).lse;   // (as fmha_combine_kernel)
        wsh[t] = empty ? 0.f : __expf(l0 - lse);
        wsh[t + 64] = empty ? 0.f : __expf(l1 - lse);
        if (cp.lse && t == 0) cp.lse[(int64_t)bidx * cp.lse_batch + (int64_t)head * cp.lse_head + pos] = lse;
    }
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int sp = g + G * u;
        if (sp < ns) acc += wsh[sp] * x[u];
    }
    for (int s0 = g + G * NB; s0 < ns; s0 += G * NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int sp = s0 + G * u;
            x[u] = sp < ns ? *reinterpret_cast<const f32x4*>(oa + sp * sstride) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int sp = s0 + G * u;
            if (sp < ns) acc += wsh[sp] * x[u];
        }
    }
    red[g][c] = acc;
    __syncthreads();
    if (t < D4) {
        f32x4 o = red[0][t];
#pragma unroll
        for (int i = 1; i < G; ++i) o += red[i][t];
        T* orow = reinterpret_cast<T*>(cp.o) + (int64_t)bidx * cp.o_batch + (int64_t)pos * cp.o_row +
                  (int64_t)head * cp.o_head;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * t + i < cp.d) orow[4 * t + i] = (T)o[i];
    }
}

}  // namespace xfa
