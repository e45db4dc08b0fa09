// fmha_fwdpp_kernel.h — 8-wave "ping-pong" forward for D = 128 (two waves per SIMD, 32 query
// rows per wave).
//
// Replaces the reference's `compute_attn_1rowblock_splitkv` (flash_fwd_kernel_hip.h:585-1283)
// for the shapes the 4-wave kernel (fmha_fwd4_kernel.h) runs — dense and varlen, D = 128, bf16 /
// fp16, causal / right window / none, one split — with the same math and item (256 query rows
// of one (batch x kv head)), re-structured for two waves per SIMD:
//
//  * wave w owns rows 32w .. 32w + 31 of the item; waves w and w + 4 share a SIMD;
//  * a wave alternates an MFMA phase (PV of tile j, QK^T of tile j+1) and a VALU phase (softmax
//    of tile j+1, its share of the LDS-DMA of tile j+3), each closed by a barrier, and waves 4-7
//    run one phase behind waves 0-3: on every SIMD one wave issues MFMAs while the other issues
//    VALU / DMA (tools/gen_fwdpp.py generates the item body, fmha_fwdpp_body.h);
//  * no row max in the loop (P against tile 0's max, a rare redo past 2^fwd_slack), as the
//    4-wave kernel.
// This file's own: the left-window extras of the 32x32x16 body (T0, l_w, f_w), the LDS images
// and DMA offsets, the 16x16x32 body's operands, the paged descriptors and the score-feature
// scalars.  The item geometry is fmha_fwd_geom.h's, the item schedules fmha_fwd_sched.h's.
#pragma once

#include "fmha_fwd_geom.h"
#include "fmha_fwd_sched.h"
#ifdef XFA_FWDPP_BODY
#include XFA_FWDPP_BODY         // an A/B variant of the generated body (tools/fwdpp_variants.sh)
#else
#include "fmha_fwdpp_body.h"
#endif
#ifdef XFA_FWDPP16_BODY
#include XFA_FWDPP16_BODY
#else
#include "fmha_fwdpp16_body.h"  // the same schedule on v_mfma_f32_16x16x32 (tools/gen_fwdpp16.py)
#endif

namespace xfa {

constexpr int kFwdppRows = 256;            // query rows per workgroup (8 waves x 32)
constexpr FwdQueue kFwdppQueue = kQueueXcd; // for plan_fwd and fwd_walk

#ifdef XFA_FWDPP_STAMPS
// Diagnostic build only (tools/fwdpp_variants.sh "name=--stamps", tools/pp_stamps.py): each wave
// sums the s_memtime cycles of every phase class (gen_fwdpp.ST_*) over its items in lanes 0-7 of
// one register; the kernel adds them into this array at its end (read by fmha_fwdpp_stamps).
static __device__ unsigned g_fwdpp_stamps[8 * 8];
#define XFA_PP_ACC_PARAM , unsigned& acc
#define XFA_PP_ACC_ARG , acc
#else
#define XFA_PP_ACC_PARAM
#define XFA_PP_ACC_ARG
#endif
constexpr int kFwdppTile = 128 * 64 * 2;   // bytes of one K (or V) tile at D = 128
constexpr int kFwdppVReg = kFwdppRing * kFwdppTile;      // the V ring follows the K ring
constexpr int kFwdppSmem = 2 * kFwdppRing * kFwdppTile;  // (kFwdppRing: the generated body's)

// The 16x16x32 body's image: kv_off with the chunk XORed by ppx16(row bits 2-3) = 0, 2, 3, 1
// instead of the bits themselves.  Its K row reads (16 lanes of a ds_read_b128 bank group cover
// rows {0-3, 12-15} at one chunk and rows {4-11} at the next) and its V^T reads (rows 4 g + q of
// lane group g) then land on distinct banks: 4 / 2 cycles instead of 8 / 4 (tools/fwdpp_banks.py;
// PMC r06: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.5 with the plain image)
__device__ __forceinline__ constexpr int ppx16(int x) { return (0x78 >> (2 * x)) & 3; }

// One (batch x kv head, 256-row query block) item.  M16: the body on the 16x16x32 MFMA shape
// (a lane holds rows l16 and 16 + l16 of its wave's 32; per-lane operands below).
template <bool BF16, bool M16, bool PG>
__device__ __forceinline__ void fwdpp_item(const FwdParams& p, char* smem, const int bh, const int m_block XFA_PP_ACC_PARAM) {
    constexpr int HD = 128;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));       // item-local: not hoisted out of the persistent loop
    const int lane = tid & 63;
    const int lr = lane & 31;
    const int hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;
    // varlen / seqused_k: this sequence's rows of the packed tensors
    const SeqRange sr = seq_range<true>(p, bidx);
    const int q_off = sr.q_off, sq = sr.sq, k_off = sr.k_off, sk = sr.sk;
    const int G = p.group;
    const int rows_total = sq * G;
    const int row0 = m_block * kFwdppRows;
    if (row0 >= rows_total) return;    // workgroup-uniform
    const int diag = sk - sq;
    const KeyLimit lim_r{sk, diag, p.wr};
    // left window (wl >= 0, the 32x32 body only): keys [lim_l(pos), lim_r(pos))
    auto lim_l = [&](int pos) { return p.wl >= 0 ? max(0, pos + diag - p.wl) : 0; };

    // key tiles of the workgroup: [T0, T0 + ntl) — T0 > 0 when the item's first row's window
    // starts past key 0; the body counts tiles from T0 (K / V bases, limits shifted by 64 T0)
    const int ntl_abs = key_tiles(lim_r, (min(row0 + kFwdppRows, rows_total) - 1) / G);
    const int T0 = (M16 || ntl_abs <= 0) ? 0 : min(lim_l(row0 / G) / kBlockN, ntl_abs - 1);
    const int ntl = ntl_abs - T0;

    // this wave: rows wrow0 .. wrow0 + 31; last tile t_w; tiles >= e_w need the right edge mask,
    // tiles < l_w the left one; before tile f_w no row of the wave sees a key
    const int wrow0 = row0 + 32 * wave;
    int t_w, e_w, l_w = 0, f_w = 0;
    if (wave_tiles<32>(lim_r, wrow0, rows_total, G, ntl_abs, t_w, e_w)) {
        t_w = max(t_w - T0, -1);
        e_w -= T0;
        l_w = (lim_l((min(wrow0 + 32, rows_total) - 1) / G) + kBlockN - 1) / kBlockN - T0;
        f_w = lim_l(wrow0 / G) / kBlockN - T0;
    }
    t_w = __builtin_amdgcn_readfirstlane(t_w);
    e_w = __builtin_amdgcn_readfirstlane(e_w);
    l_w = __builtin_amdgcn_readfirstlane(l_w);
    f_w = __builtin_amdgcn_readfirstlane(f_w);

    // this lane's row; its key limits count from tile 0 of the body (absolute tile T0)
    const LaneRow lrow = lane_row<2>(p, lim_r, wrow0 + lr, rows_total, hk_i, 16 * hh, 16 * hh, hh);
    const bool ok = lrow.ok;
    const int pos = lrow.pos, head = lrow.head, qoff = lrow.qoff, ooff = lrow.ooff, loff = lrow.loff;
    const int lim = lrow.lim - kBlockN * T0;
    const int liml = (ok ? lim_l(pos) : 0) - 4 * hh - kBlockN * T0;
    const int wid = max(lim - liml, 0);

    if (ntl <= 0) {
        store_empty_row(p, bidx, q_off, lrow, hh);
        return;
    }

    // SRDs: Q / O / LSE of this sequence; K / V of this sequence and kv head, their range ending
    // at the workgroup's last key tile (the ring's DMA past it reads zeros and moves no bytes)
    const RowSrds srd = row_srds<2>(p, bidx, q_off, sq);
    const i32x4 qsrd = srd.q, osrd = srd.o, lsrd = srd.lse;
    const int k_row = (int)p.k_row;
    const int64_t k0 = (int64_t)k_off + (int64_t)kBlockN * T0;   // the item's first key row
    const char* kseq = reinterpret_cast<const char*>(p.k) +
                       ((int64_t)bidx * p.k_batch + k0 * p.k_row + (int64_t)hk_i * p.k_head) * 2;
    const char* vseq = reinterpret_cast<const char*>(p.v) +
                       ((int64_t)bidx * p.v_batch + k0 * p.v_row + (int64_t)hk_i * p.v_head) * 2;
    const int nk = min(sk, ntl_abs * kBlockN) - kBlockN * T0;
    const int kvbytes = __builtin_amdgcn_readfirstlane((int)(((nk - 1) * k_row + HD) * 2));
    const int kblo = ptr_lo(kseq), kbhi = ptr_hi(kseq), vblo = ptr_lo(vseq), vbhi = ptr_hi(vseq);

    // LDS-DMA: wave w loads 8-row block w of every K / V tile, pieces i = chunks 8i .. 8i+7 of
    // the kv_off image (lane l lands at +16 l); K and V share the offsets (k_row == v_row)
    // (M16: the chunk XOR by row bits 2-3 goes through ppx16, so the 16x16x32 body's K row and
    // V^T reads are conflict-free too; see ppx16)
    // (paged: the descriptor base points at the wave's 8 rows, so the row offset is lr / 4)
    const int r = 8 * wave + lr / 4;
    const int cch = 4 * hh + ((lane & 3) ^ (M16 ? ppx16((r >> 2) & 3) : ((r >> 2) & 3)));
    const int dma0 = (PG ? lr / 4 : r) * k_row * 2 + cch * 16;
    // LDS read bases (kv_off image, slot 0; the ring slots are immediate offsets)
    const int sbase = (int)(size_t)smem;
    int kb[2], vb[2];
    {
        const int q4 = (lane & 15) >> 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kb[u] = sbase + kv_off<HD>(lr, 2 * u + hh);
            const int rr = 8 * u + 4 * hh + q4;
            const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
            vb[u] = sbase + kFwdppVReg + kv_off<HD>(rr, col >> 3) + 8 * ((col >> 2) & 1);
        }
    }
    const int kstep = __builtin_amdgcn_readfirstlane(kBlockN * k_row * 2);
    const int kdst = __builtin_amdgcn_readfirstlane(sbase + wave * 2048);
    const int grp = __builtin_amdgcn_readfirstlane(wave >> 2);
    const float thr = __builtin_amdgcn_exp2f(p.max_slack);
    if constexpr (M16) {
        static_assert(kFwdpp16Ring == kFwdppRing, "both bodies address the same LDS ring");
        // row tile rt of this lane: row wrow0 + 16 rt + l16, 4 keys per 16-key block from 4 g
        const int g = lane >> 4, l16 = lane & 15;
        // (Q chunk 4 s + g, O columns 16 dt + 4 g)
        LaneRow rt[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
            rt[t] = lane_row<2>(p, lim_r, wrow0 + 16 * t + l16, rows_total, hk_i, 16 * g, 8 * g, g);
        // K row reads: key 16 kt + l16, chunk 4 s + g; V^T reads: lane 4 q + p of group g, key
        // 4 g + q (+ 32 ks + 16 h), d 16 dt + 4 p, base per dt parity e (kv_off image)
        const int kb0 = sbase + 2048 * ((lane >> 3) & 1) + 64 * (lane & 7) + 16 * (g ^ ppx16((lane >> 2) & 3));
        const int q4 = (lane & 15) >> 2, p4 = lane & 3;
        int vb16[2];
#pragma unroll
        for (int e = 0; e < 2; ++e)
            vb16[e] = sbase + kFwdppVReg + 2048 * (g >> 1) + 64 * (4 * (g & 1) + q4) +
                      16 * ((2 * e + (p4 >> 1)) ^ ppx16(g)) + 8 * (p4 & 1);
#ifdef XFA_FWDPP16_STAMPS
#define XFA_PP16_ACC_ARG , acc
#else
#define XFA_PP16_ACC_ARG
#endif
        if constexpr (BF16)
            fwdpp16_item_bf16(kblo, kbhi, vblo, vbhi, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                              p.scale_log2, thr, kb0, vb16[0], vb16[1], dma0, dma0 + 128, rt[0].lim, rt[1].lim, rt[0].qoff,
                              rt[1].qoff, rt[0].ooff, rt[1].ooff, rt[0].loff, rt[1].loff XFA_PP16_ACC_ARG);
        else
            fwdpp16_item_f16(kblo, kbhi, vblo, vbhi, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                             p.scale_log2, thr, kb0, vb16[0], vb16[1], dma0, dma0 + 128, rt[0].lim, rt[1].lim, rt[0].qoff,
                             rt[1].qoff, rt[0].ooff, rt[1].ooff, rt[0].loff, rt[1].loff XFA_PP16_ACC_ARG);
#undef XFA_PP16_ACC_ARG
        return;
    }
    // score features (gen_fwdpp.feature_block): bit 0 softcap, bit 1 ALiBi (the lane's row slope
    // in raw-score units and its distance pos + diag - 4 hh to the lane's key offset 0)
    // bit 2: causal ALiBi (wr = 0, every visible key <= pos + diag) in the linear frame +w key
    // (gen_fwdpp._alibi_linear_ops: one v_fmac per score instead of the |.| form's two)
    const bool lin = p.alibi && p.wr == 0;
    const int feat = __builtin_amdgcn_readfirstlane((p.softcap_pre > 0.f ? 1 : 0) | (p.alibi ? (lin ? 4 : 2) : 0));
    const float scp2 = p.softcap_pre * (2.f * kLog2e);
    const float alw = (p.alibi && ok) ? p.alibi[bidx * p.alibi_bstride + head] * p.alibi_mul : 0.f;
    // |.| form: the distance base pos + diag - 4 hh - 64 T0; linear form: c w (64 T0 + 4 hh), the
    // tile-invariant part of the frame shift c w key0
    const float ald = lin ? p.scale_log2 * alw * (float)(kBlockN * T0 + 4 * hh)
                          : (float)(pos + diag - 4 * hh - kBlockN * T0);
    const float alw2 = p.scale_log2 * alw;                       // c w
    const float adiag = p.scale_log2 * alw * (float)(pos + diag);   // the |.| form's row offset
    // the row's best ALiBi bias: -w times the distance from pos + diag to its nearest visible key
    // (keys [lim_l, lim_r)); tile 0's reference max is lifted by it
    const int hi_k = ok ? lim_r(pos) : 0, lo_k = ok ? lim_l(pos) : 0;
    const int near = min(max(pos + diag, lo_k), max(hi_k - 1, lo_k));
    const float alm = hi_k > lo_k ? (lin ? alw * (float)near : -alw * (float)abs(pos + diag - near)) : 0.f;
    if constexpr (PG) {
#ifndef XFA_FWDPP_STAMPS
        // paged K/V (gen_fwdpp.py PAGED): per tile, each wave's 8 rows sit in one page (page size
        // a power of two >= 8, fwd4_eligible); the body loads the page id from this sequence's
        // block-table row and builds the wave's descriptors from the pools' bases (kblo.. here:
        // pool + this kv head's offset), the page stride and the row bytes
        const int* btab = p.block_table + (int64_t)bidx * p.bt_stride;
        const char* kpool = reinterpret_cast<const char*>(p.k) + (int64_t)hk_i * p.k_head * 2;
        const char* vpool = reinterpret_cast<const char*>(p.v) + (int64_t)hk_i * p.v_head * 2;
        const int pkl = ptr_lo(kpool), pkh = ptr_hi(kpool), pvl = ptr_lo(vpool), pvh = ptr_hi(vpool);
        const int pstr = __builtin_amdgcn_readfirstlane((int)(p.k_batch * 2));
        const int rowb = __builtin_amdgcn_readfirstlane(k_row * 2);
        const int lgp = __builtin_amdgcn_readfirstlane(31 - __builtin_clz(p.page_size));
        const int pmask = __builtin_amdgcn_readfirstlane(p.page_size - 1);
        const int skv = __builtin_amdgcn_readfirstlane(sk);
        const int skey0 = __builtin_amdgcn_readfirstlane(kBlockN * T0 + 8 * wave);
        if constexpr (BF16)
            fwdpp_pg_item_bf16(pkl, pkh, pvl, pvh, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                               p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma0, dma0 + 128, lim, qoff, ooff,
                               loff, feat, scp2, alw, ald, alm, l_w, liml, wid, f_w, alw2, adiag, btab, pstr, rowb,
                               lgp, pmask, skv, skey0);
        else
            fwdpp_pg_item_f16(pkl, pkh, pvl, pvh, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                              p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma0, dma0 + 128, lim, qoff, ooff,
                              loff, feat, scp2, alw, ald, alm, l_w, liml, wid, f_w, alw2, adiag, btab, pstr, rowb,
                              lgp, pmask, skv, skey0);
#endif
        return;
    }
    if constexpr (BF16)
        fwdpp_item_bf16(kblo, kbhi, vblo, vbhi, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                        p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma0, dma0 + 128, lim, qoff, ooff, loff,
                        feat, scp2, alw, ald, alm, l_w, liml, wid, f_w, alw2, adiag XFA_PP_ACC_ARG);
    else
        fwdpp_item_f16(kblo, kbhi, vblo, vbhi, kvbytes, qsrd, osrd, lsrd, kstep, kdst, ntl, t_w, e_w, grp,
                       p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma0, dma0 + 128, lim, qoff, ooff, loff,
                       feat, scp2, alw, ald, alm, l_w, liml, wid, f_w, alw2, adiag XFA_PP_ACC_ARG);
}

// Persistent grid (one workgroup per CU) over the items (fwd_walk, fmha_fwd_sched.h).
template <bool BF16, bool M16 = false, bool PG = false>
__global__ void __launch_bounds__(512, 1) fmha_fwdpp_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef XFA_FWDPP_STAMPS
    unsigned acc = 0;
#endif
    fwd_walk<kFwdppQueue>(p, [&](int bh, int m_block) { fwdpp_item<BF16, M16, PG>(p, smem, bh, m_block XFA_PP_ACC_ARG); });
#ifdef XFA_FWDPP_STAMPS
    if ((threadIdx.x & 63) < 8) atomicAdd(&g_fwdpp_stamps[(threadIdx.x >> 6) * 8 + (threadIdx.x & 63)], acc);
#endif
}

}  // namespace xfa
