// fmha_fwd_mla_kernel.h — MLA prefill: the forward at head size 192 for Q K^T and 128 for V
// (the un-absorbed form of multi-head latent attention: 128 "nope" + 64 rotary features in q and
// k, a 128-wide v), for gfx950 (CDNA4).  DESIGN.md §3.11.
//
// fwd_item's pipelined (D <= 128) path (fmha_fwd_kernel.h) with two widths instead of one HD:
//   * S^T = K Q^T over HDK = 192 features (NS = 12 k-steps of v_mfma_f32_32x32x16), P straight
//     from the accumulator as the B operand of O^T += V^T P^T over HDV = 128 columns (ND = 4);
//   * the kv_off<192> image for a K tile (64 keys x 384 B = 24 KiB) and the kv_off<128> image for
//     a V tile (16 KiB), both filled by LDS-DMA: 24 + 16 one-KiB pieces a tile pair;
//   * deferred rescale, the two-stage software pipeline over the tiles every row sees and the
//     masked per-wave loop over the tiles that cross the left window edge, as there.
// No FEAT path: no ALiBi, softcap, dropout, paged or fp8 K/V, leftpad, split-KV or sink.
//
// The ring.  fwd_item keeps tile pairs in 4 rotating buffers; four 40 KiB pairs are all of the
// CU's 160 KiB and leave no room for the item queue's claim slots (fwd_claim).  Here K has 4
// buffers and V has 3 (96 + 48 = 144 KiB), and V is issued one tile behind K: step j (tile j's
// softmax and PV, tile j + 1's QK^T) issues K of tile j + 3 into K buffer (j + 3) % 4 (K of
// j - 1, last read in step j - 2) and V of tile j + 2 into V buffer (j + 2) % 3 (V of j - 1, last
// read in step j - 1; the barrier that ends step j - 1 lies between).  The barrier that ends
// step j still waits for everything but step j's own issue, which is then K of j + 2 and V of
// j + 1: what step j + 1 reads.  Buffer numbers are run-time values (two adds a step per
// operand), so the step is unrolled twice (the score ping-pong) and not 12 times.
// This file's own: the item body's schedule (fwd_mla_item: the two rings, which tile each step
// issues, reads and retires, the VALU share of each MFMA gap).  The row geometry, the softmax
// state, the tile pieces, the asm V^T read ring, the DMA piece offsets and the epilogue under it
// are fmha_fwd_tile.h's, shared with fwd_item; the loop over a workgroup's items is
// fmha_fwd_sched.h's.
#pragma once

#include "fmha_common.h"
#include "fmha_fwd_sched.h"
#include "fmha_fwd_tile.h"

namespace xfa {

constexpr int kMlaHdk = 192;                    // q / k head size
constexpr int kMlaHdv = 128;                    // v / o head size
constexpr int kMlaKBuf = 4, kMlaVBuf = 3;       // ring depths
constexpr int kMlaKTile = kBlockN * kMlaHdk * 2;
constexpr int kMlaVTile = kBlockN * kMlaHdv * 2;
constexpr int kMlaSmem = kMlaKBuf * kMlaKTile + kMlaVBuf * kMlaVTile;
constexpr bool kMlaSchedFence = true;             // pins each MFMA gap's VALU share (fwd_item's SCHED_FENCE)

// One work item = (batch x kv head, query row block).
template <typename T, int NW, bool MASK>
__device__ __forceinline__ void fwd_mla_item(const FwdParams& p, char* smem, const int bh,
                                             const int m_block) {
    using V8 = typename DT<T>::v8;
    constexpr int HDK = kMlaHdk, HDV = kMlaHdv;
    constexpr int BM = NW * 32;
    constexpr int KT = kMlaKTile, VT = kMlaVTile;
    constexpr int VREG = kMlaKBuf * KT;         // LDS: the K buffers, then the V buffers
    constexpr int NS = HDK / 16;                // k-steps of the QK^T product
    constexpr int ND = HDV / 32;                // 32-wide d tiles of O^T

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hh = lane >> 5;

    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;

    int q_off = 0, sq = p.seqlen_q, k_off = 0, sk = p.seqlen_k;
    if (p.cu_seqlens_q) { q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off; }
    if (p.cu_seqlens_k) { k_off = p.cu_seqlens_k[bidx]; sk = p.cu_seqlens_k[bidx + 1] - k_off; }
    if (p.seqused_k) sk = p.seqused_k[bidx];
    sk = max(sk, 0);
    const int row0 = m_block * BM;
    if (row0 >= sq * p.group) return;
    // (this item's lim_r is clamped at 0)
    const RowGeom<MASK> g(p, sq, sk, p.group, hk_i, row0, BM, wave, lane & 31, 0);
    const float c = p.scale_log2;

    V8 qf[NS];
    q_frags(q_row<T>(p, bidx, q_off, sq, HDK, g.row_ok, g.pos, g.head, hh), qf);

    // ---- K / V of this sequence and kv head: one descriptor each, sized to the sequence
    const char* kseq = reinterpret_cast<const char*>(p.k) +
                       ((int64_t)bidx * p.k_batch + (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head) * 2;
    const char* vseq = reinterpret_cast<const char*>(p.v) +
                       ((int64_t)bidx * p.v_batch + (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head) * 2;
    const uint32_t kbytes = sk > 0 ? (uint32_t)(((int64_t)(sk - 1) * p.k_row + HDK) * 2) : 0u;
    const uint32_t vbytes = sk > 0 ? (uint32_t)(((int64_t)(sk - 1) * p.v_row + HDV) * 2) : 0u;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(kseq, kbytes);
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(vseq, vbytes);

    // per-lane LDS read bases of the kv_off<192> K and kv_off<128> V images
    int kb[2], vb[2];
    k_read_bases<HDK>((int)(size_t)smem, lane, kb);
    v_read_bases<HDV>((int)(size_t)smem + VREG, lane, vb);
    SoftmaxRow<ND> sm;

    // O^T += V^T P^T of the tile in the V buffer at byte offset vbo (run-time: added into the
    // two base registers)
    auto pv_asm = [&](const int vbo, const V8 (&pb)[4], auto&& beside) {
        const int vbj[2] = {vb[0] + vbo, vb[1] + vbo};
        pv_ring<T, HDV, 0>(sm.acc_o, vbj, pb, beside);
    };

    // ---- LDS-DMA: a K tile is 24 one-KiB pieces (three an 8-row block of the kv_off<192>
    // image), a V tile 16 (two an 8-row block)
    constexpr int IPK = KT / 1024 / NW, IPV = VT / 1024 / NW;   // wave-instructions per wave per tile
    static_assert(IPK * 1024 * NW == KT && IPV * 1024 * NW == VT, "DMA geometry");
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int dma_k[IPK], dma_v[IPV];                    // per-lane byte offsets within a tile
#pragma unroll
    for (int i = 0; i < IPK; ++i) dma_k[i] = dma_piece<HDK>(wave * IPK + i, lane, (int)p.k_row * 2);
#pragma unroll
    for (int i = 0; i < IPV; ++i) dma_v[i] = dma_piece<HDV>(wave * IPV + i, lane, (int)p.v_row * 2);
    typedef __attribute__((address_space(3))) void lds_void;
    // (soffset pinned to an SGPR; rows past the sequence's end are past the descriptor: zeros)
    auto dma_k_tile = [&](const int nb, const int kbo) {
        const int so = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.k_row * 2);
#pragma unroll
        for (int i = 0; i < IPK; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                krs, (lds_void*)(smem + kbo + (wave_u * IPK + i) * 1024), 16, dma_k[i], so, 0, 0);
    };
    auto dma_v_tile = [&](const int nb, const int vbo) {
        const int so = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.v_row * 2);
#pragma unroll
        for (int i = 0; i < IPV; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                vrs, (lds_void*)(smem + VREG + vbo + (wave_u * IPV + i) * 1024), 16, dma_v[i], so, 0, 0);
    };
    // what a barrier may leave in flight: a step's own issue, its V alone, or nothing
    auto publish_left = [&](const int left) { publish<IPK + IPV, IPV>(left); };

    // ---- tiles that need per-wave masking / skipping (the left window edge, or a range too
    // short for the pipeline): one tile pair in flight, K / V buffers 0 and 1
    auto masked_range = [&](const int lo, const int hi) {
        if (lo >= hi) return;
        dma_k_tile(lo, 0);
        dma_v_tile(lo, 0);
        publish();
        int buf = 0;
        for (int nb = lo; nb < hi; ++nb) {
            if (nb + 1 < hi) {
                dma_k_tile(nb + 1, (buf ^ 1) * KT);
                dma_v_tile(nb + 1, (buf ^ 1) * VT);
            }
            const int n0 = nb * kBlockN;
            if (g.active(n0)) {
                f32x16 st[2];
                qk<T, HDK>(kb, buf * KT, qf, st);
                if (g.edge(n0)) edge_mask(st, n0, hh, g.my_lr, g.my_ll);
                sm.raise_max(row_max(st), c, p.max_slack);
                V8 pb[4];
                exp_tile<T>(sm, st, pb, c);
                pv_asm(buf * VT, pb, [](auto) {});
            }
            publish();
            buf ^= 1;
        }
    };

    // ---- tiles every row of the workgroup sees from their left end: two-stage software
    // pipeline (fwd_item's pipe_range).  Tiles [lo, hm) need no mask; tiles [hm, hi) (the causal
    // diagonal / right window edge / ragged end) are masked in registers on the way through.
    const int lim_e = g.my_lr - 4 * hh;          // right edge of this lane's keys, minus its offset
    auto pipe_range = [&](const int lo, const int hm, const int hi) {
        const bool third = lo + 2 < hi;
        dma_k_tile(lo, 0);
        dma_v_tile(lo, 0);
        dma_k_tile(lo + 1, KT);
        if (third) dma_k_tile(lo + 2, 2 * KT);
        dma_v_tile(lo + 1, VT);
        publish_left(third ? IPK + IPV : 0);
        f32x16 sa[2], sb[2];
        qk<T, HDK>(kb, 0, qf, sa);
        if (lo >= hm) edge_mask(sa, lo * kBlockN, hh, g.my_lr, g.my_ll);
        sm.raise_max(row_max(sa), c, p.max_slack);
        scale_shift(sa, c, sm.exp_ref());
        const int nsteps = hi - lo - 1;
        // step r (tile j = lo + r): issues K of j + 3 and V of j + 2; returns what it left in flight
        auto issue = [&](const int r) {
            const int j = lo + r;
            int left = 0;
            if (j + 3 < hi) { dma_k_tile(j + 3, ((r + 3) & 3) * KT); left += IPK; }
            if (j + 2 < hi) { dma_v_tile(j + 2, ((r + 2) % 3) * VT); left += IPV; }
            return left;
        };
        auto step = [&](const int r, f32x16 (&st)[2], f32x16 (&sn)[2]) {
            const int j = lo + r;
            const int left = issue(r);
            const int kbo = __builtin_amdgcn_readfirstlane(((r + 1) & 3) * KT);
            const int vbo = __builtin_amdgcn_readfirstlane((r % 3) * VT);
            if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            // phase a: S_{j+1} = K_{j+1} Q^T on the MFMA pipe, P_j = exp2(X_j) -> T on the VALU
            sn[0] = f32x16{};
            sn[1] = f32x16{};
            V8 pb[4];
            float rs = 0.f;                       // fp32 row sum of P_j
            // 32 values over 2 NS = 24 MFMAs, in pairs: the first 16 MFMAs take one pair each
            V8 a0 = rd_k<T, HDK>(kb, kbo, 0, 0), a1 = rd_k<T, HDK>(kb, kbo, 0, 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                V8 n0 = a0, n1 = a1;
                if (s + 1 < NS) { n0 = rd_k<T, HDK>(kb, kbo, s + 1, 0); n1 = rd_k<T, HDK>(kb, kbo, s + 1, 1); }
                sn[0] = DT<T>::mfma32(a0, qf[s], sn[0]);
                if (2 * s < 16) expx_part<T>(st, pb, rs, 4 * s, 2);
                sn[1] = DT<T>::mfma32(a1, qf[s], sn[1]);
                if (2 * s + 1 < 16) expx_part<T>(st, pb, rs, 4 * s + 2, 2);
                // pins the row-sum adds into this MFMA gap: unpinned, the compiler sinks them
                // below phase b (rs is only read there) into a VALU-only run of 32 adds
                // (measured on fwd_item's step: +1.5-2 % C2, same-box A/B)
                asm volatile("" : "+v"(rs));
                a0 = n0;
                a1 = n1;
                if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            }
            // phase b: O += V_j^T P_j on the MFMA pipe; on the VALU X_{j+1} = S_{j+1} c - m_sc
            // and its row max
            constexpr int MV = 32 / (4 * ND);     // score values per PV MFMA
            const float mr = sm.exp_ref();
            float mx = -INFINITY;
            pv_asm(vbo, pb, [&](auto I) {
                constexpr int i = decltype(I)::value;
#pragma unroll
                for (int v = i * MV; v < (i + 1) * MV; ++v) {
                    sn[v >> 4][v & 15] = __builtin_fmaf(sn[v >> 4][v & 15], c, -mr);
                    mx = fmaxf(mx, sn[v >> 4][v & 15]);
                }
                if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            });
            // an opaque use pins the max chain inside phase b (else it is sunk below the edge
            // branch, out of the MFMA gaps)
            asm volatile("" : "+v"(mx));
            sm.l_run += rs;
            // edge tile: mask, then the row max again
            if (j + 1 >= hm) mx = right_mask_max(sn, lim_e - (j + 1) * kBlockN);
            sm.rescale_x_halves(mx, sn, p.max_slack);
            publish_left(left);                   // K of j + 2 and V of j + 1 landed everywhere
        };
        // a wave runs the steps up to the last tile any of its rows sees (RowGeom::steps_w)
        const int nsteps_w = g.steps_w(nsteps, lo);
        int r = 0;
        while (r < nsteps_w) {
            step(r, sa, sb);
            if (++r >= nsteps_w) break;
            step(r, sb, sa);
            ++r;
        }
        // drain: the wave's last tile's softmax and PV
        V8 pb[4];
        if (nsteps_w & 1) expx_tile<T>(sm, sb, pb);
        else expx_tile<T>(sm, sa, pb);
        pv_asm(__builtin_amdgcn_readfirstlane((nsteps_w % 3) * VT), pb, [](auto) {});
        // the steps this wave skips: its DMA share and the barriers only
        for (; r < nsteps; ++r) publish_left(issue(r));
        __syncthreads();
    };
    // Key tiles (RowGeom::pipe_split): [nb_lo, f_lo) run through the per-wave masked loop, the
    // rest through the pipeline, [f_hi, nb_hi) of them masked.
    // (fwd_pipe = 2, fwd_item's A/B setting for its edge tiles, runs the pipeline here as 1 does)
    int f_lo = g.nb_hi, f_hi = g.nb_hi;
    if (p.pipe) g.pipe_split(g.nb_lo, g.nb_hi, f_lo, f_hi);
    if (p.prio_hi && __builtin_amdgcn_readfirstlane(wave) >= NW / 2) __builtin_amdgcn_s_setprio(1);
    masked_range(g.nb_lo, f_lo);
    if (f_lo < g.nb_hi) pipe_range(f_lo, f_hi, g.nb_hi);

    // ---- epilogue: normalise, write O and LSE
    const RowNorm n = sm.norm();
    if (!g.row_ok) return;
    store_row<T, ND>(p, bidx, q_off, g.pos, g.head, hh, sm.acc_o, n.inv, HDV, sm.lse(n));
}

constexpr FwdQueue kFwdMlaQueue = kQueueXcd;   // for plan_fwd and fwd_walk
template <typename T, int NW, bool MASK>
__global__ void __launch_bounds__(NW * 64, NW / 4) fmha_fwd_mla_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fwd_walk<kFwdMlaQueue>(p, [&](int bh, int m_block) { fwd_mla_item<T, NW, MASK>(p, smem, bh, m_block); });
}

}  // namespace xfa
