// fmha_fwd4_kernel.h — 4-wave forward for D = 128 (one wave per SIMD, 64 query rows per wave).
//
// Replaces the reference's `compute_attn_1rowblock_splitkv` (flash_fwd_kernel_hip.h:585-1283)
// for the shapes the BASELINE configurations run (dense and varlen, D = 128, bf16 / fp16,
// causal / right window / none, one split): same math as fmha_fwd_kernel.h, re-structured so one
// wave owns 64 query rows (two 32-row MFMA blocks) and the whole 512-register file:
//
//  * every K fragment and every V^T fragment read from LDS feeds two MFMAs (the two row blocks),
//    half the LDS reads per MFMA of the 8-wave kernel;
//  * the key-tile loop is a three-stage pipeline — step j runs QK^T of tile j+2, the softmax of
//    tile j+1 and PV of tile j on one instruction stream — with every instruction placed in an
//    MFMA gap by tools/gen_fwd4.py;
//  * no row max in the loop: P = exp2(S c - m) against the first tile's true row max; a tile
//    whose partial row sums pass 2^fwd_slack re-runs its softmax against the true running max
//    after rescaling O and l (rare; same result up to rounding);
//  * K / V tiles arrive by LDS-DMA into 4-slot K and V rings: step j issues K_{j+4} and V_{j+2}
//    and publishes K_{j+3}, V_{j+1} at its mid-point barrier (one barrier per tile).
//
// The item's whole pipeline is one generated asm statement with a fixed register map
// (fmha_fwd4_body.h).  This file's own: the read bases of the LDS images and the DMA offsets
// of the 4-slot rings.  The item geometry is fmha_fwd_geom.h's, the item schedules
// fmha_fwd_sched.h's.
#pragma once

#include "fmha_fwd_geom.h"
#include "fmha_fwd_sched.h"
#ifdef XFA_FWD4_BODY
#include XFA_FWD4_BODY          // an A/B variant of the generated body (tools/fwd4_variants.sh)
#else
#include "fmha_fwd4_body.h"
#endif

namespace xfa {

constexpr int kFwd4Rows = 256;            // query rows per workgroup (4 waves x 64)
constexpr int kFwd4Tile = 128 * 64 * 2;   // bytes of one K (or V) tile at D = 128
constexpr int kFwd4VReg = 4 * kFwd4Tile;  // V ring after the 4 K slots
constexpr int kFwd4Smem = 8 * kFwd4Tile;  // 128 KiB

constexpr FwdQueue kFwd4Queue = kQueueXcd;   // for plan_fwd and fwd_walk

// One (batch x kv head, 256-row query block) item.
template <bool BF16>
__device__ __forceinline__ void fwd4_item(const FwdParams& p, char* smem, const int bh, const int m_block) {
    constexpr int HD = 128;
    // item-local copies made opaque: otherwise hipcc hoists lane- and parameter-derived values
    // out of the persistent item loop and keeps them live across the asm body
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
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
    const int row0 = m_block * kFwd4Rows;
    if (row0 >= rows_total) return;    // workgroup-uniform
    const KeyLimit lim_r{sk, sk - sq, p.wr};

    // key tiles of the workgroup: [0, ntl)
    const int ntl = key_tiles(lim_r, (min(row0 + kFwd4Rows, rows_total) - 1) / G);
    // this wave: rows wrow0 .. wrow0 + 63; last tile t_w; tiles >= e_w need the edge mask
    const int wrow0 = row0 + 64 * wave;
    int t_w, e_w;
    wave_tiles<64>(lim_r, wrow0, rows_total, G, ntl, t_w, e_w);
    t_w = __builtin_amdgcn_readfirstlane(t_w);
    e_w = __builtin_amdgcn_readfirstlane(e_w);

    // per lane: the rows of the two 32-row blocks
    LaneRow r[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        r[rb] = lane_row<2>(p, lim_r, wrow0 + 32 * rb + lr, rows_total, hk_i, 16 * hh, 16 * hh, hh);

    if (ntl <= 0) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) store_empty_row(p, bidx, q_off, r[rb], hh);
        return;
    }

    // SRDs: Q / O / LSE of this sequence; K / V of this sequence and kv head, their range ending
    // at the workgroup's last key tile (the ring's DMA past it reads zeros and moves no bytes)
    const RowSrds srd = row_srds<2>(p, bidx, q_off, sq);
    const int k_row = (int)p.k_row;
    const char* kseq = reinterpret_cast<const char*>(p.k) +
                       ((int64_t)bidx * p.k_batch + (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head) * 2;
    const char* vseq = reinterpret_cast<const char*>(p.v) +
                       ((int64_t)bidx * p.v_batch + (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head) * 2;
    const int nk = min(sk, ntl * kBlockN);
    const uint32_t kvbytes = (uint32_t)(((nk - 1) * k_row + HD) * 2);

    // per-lane DMA offsets: piece g = wave*4 + i is 8 rows x 8 chunks of the kv_off image (lane
    // l lands at g KiB + 16 l); pieces 2h and 2h+1 differ by 8 chunks (128 bytes); K and V share
    // them (k_row == v_row, checked on the host)
    int dma[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int g = wave * 4 + 2 * h;
        const int dr = 8 * (g / 2) + (lane & 31) / 4;
        const int cch = 4 * (lane >> 5) + ((lane & 3) ^ ((dr >> 2) & 3));
        dma[h] = dr * k_row * 2 + cch * 16;
    }
    // LDS read bases (kv_off image, slot 0; the ring slots are immediate offsets)
    const int sbase = (int)(size_t)smem;
    int kb[2], vb[2];
    {
        const int q4 = (lane & 15) >> 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kb[u] = sbase + kv_off<HD>(lr, 2 * u + hh);
            const int vr = 8 * u + 4 * hh + q4;
            const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
            vb[u] = sbase + kFwd4VReg + kv_off<HD>(vr, col >> 3) + 8 * ((col >> 2) & 1);
        }
    }
    const int kstep = __builtin_amdgcn_readfirstlane(kBlockN * k_row * 2);
    (void)kvbytes;
    const int kdst = __builtin_amdgcn_readfirstlane(sbase + wave * 4096);
    const float thr = __builtin_amdgcn_exp2f(p.max_slack);
    if constexpr (BF16)
        fwd4_item_bf16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), (int)kvbytes, srd.q, srd.o, srd.lse, kstep, kdst,
                       ntl, t_w, e_w, p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma[0], dma[0] + 128, dma[1],
                       dma[1] + 128, r[0].lim, r[1].lim, r[0].qoff, r[1].qoff, r[0].ooff, r[1].ooff, r[0].loff, r[1].loff);
    else
        fwd4_item_f16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), (int)kvbytes, srd.q, srd.o, srd.lse, kstep, kdst,
                      ntl, t_w, e_w, p.scale_log2, thr, kb[0], kb[1], vb[0], vb[1], dma[0], dma[0] + 128, dma[1],
                      dma[1] + 128, r[0].lim, r[1].lim, r[0].qoff, r[1].qoff, r[0].ooff, r[1].ooff, r[0].loff, r[1].loff);
}

// Persistent grid (one workgroup per CU) over the items (fwd_walk, fmha_fwd_sched.h).
template <bool BF16>
__global__ void __launch_bounds__(256, 1) fmha_fwd4_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fwd_walk<kFwd4Queue>(p, [&](int bh, int m_block) { fwd4_item<BF16>(p, smem, bh, m_block); });
}

}  // namespace xfa
