// fmha_fwd_geom.h — the item geometry the four asm-body shells share (fwd4_item, fwdpp_item,
// fwd8w_item, fwd8pp_item): buffer descriptors as the generated bodies take them, the key-tile
// bounds of a workgroup and a wave, a lane's row offsets, and the output of an item no row of
// which sees a key.  What differs per kernel stays in its own file: the LDS images and DMA
// offsets, the 16x16x32 operands, the paged descriptors, the score-feature scalars.
#pragma once

#include "fmha_common.h"

namespace xfa {

typedef __attribute__((ext_vector_type(4))) int i32x4;

// A raw buffer descriptor in four SGPRs (the bodies' s_load-free operands): 48-bit base, byte
// extent, the gfx950 data format word.
__device__ __forceinline__ i32x4 make_srd(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32) & 0xFFFF);
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}
// The two base words of such a descriptor alone (the bodies step the K / V bases per tile).
__device__ __forceinline__ int ptr_lo(const void* ptr) {
    return __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)ptr);
}
__device__ __forceinline__ int ptr_hi(const void* ptr) {
    return __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)ptr >> 32) & 0xFFFF);
}

// Q / O / LSE descriptors of sequence (bidx, q_off, sq): every head's rows of this sequence and
// nothing of the next one (a kOOB lane offset is out of range of all three).  QB: bytes per Q
// element (2, or 1 for fp8); O is 16-bit, D = 128.
struct RowSrds { i32x4 q, o, lse; };
template <int QB>
__device__ __forceinline__ RowSrds row_srds(const FwdParams& p, const int bidx, const int q_off, const int sq) {
    constexpr int HD = 128;
    const char* qseq = reinterpret_cast<const char*>(p.q) + ((int64_t)bidx * p.q_batch + (int64_t)q_off * p.q_row) * QB;
    char* oseq = reinterpret_cast<char*>(p.o) + ((int64_t)bidx * p.o_batch + (int64_t)q_off * p.o_row) * 2;
    const uint32_t qbytes = (uint32_t)(((int64_t)(sq - 1) * p.q_row + (int64_t)(p.h - 1) * p.q_head + HD) * QB);
    const uint32_t obytes = (uint32_t)(((int64_t)(sq - 1) * p.o_row + (int64_t)(p.h - 1) * p.o_head + HD) * 2);
    // LSE rows of this sequence: [h][lse_head] floats
    const float* lseq = p.lse ? p.lse + (int64_t)bidx * p.lse_batch + q_off : p.lse;
    const int64_t lbytes = p.lse ? ((int64_t)(p.h - 1) * p.lse_head + sq) * 4 : 0;
    return RowSrds{make_srd(qseq, qbytes), make_srd(oseq, obytes), make_srd(lseq, (uint32_t)min(lbytes, (int64_t)kOOB - 1))};
}

// Right key limit (exclusive) of query position pos: the window's edge or the end of the keys.
struct KeyLimit {
    int sk, diag, wr;
    __device__ __forceinline__ int operator()(const int pos) const { return wr >= 0 ? min(sk, pos + diag + wr + 1) : sk; }
};

// Key tiles [0, n) of a workgroup whose last row is query position pos_hi (0: no visible key).
__device__ __forceinline__ int key_tiles(const KeyLimit& lim_r, const int pos_hi) {
    const int n_hi = lim_r.sk > 0 ? lim_r(pos_hi) : 0;
    return n_hi > 0 ? (n_hi + kBlockN - 1) / kBlockN : 0;
}

// The wave that owns rows [wrow0, wrow0 + WROWS) of the item (WROWS 32 or 64): its last key
// tile t_w (-1: none) and the first tile e_w that needs the right edge mask, both wave-uniform.
// False (and t_w = -1, e_w past every tile) where the wave has no row or the item no tile.
template <int WROWS>
__device__ __forceinline__ bool wave_tiles(const KeyLimit& lim_r, const int wrow0, const int rows_total, const int G,
                                           const int ntl, int& t_w, int& e_w) {
    t_w = -1;
    e_w = 1 << 30;
    if (!(wrow0 < rows_total && ntl > 0)) return false;
    const int wp_lo = wrow0 / G, wp_hi = (min(wrow0 + WROWS, rows_total) - 1) / G;
    const int lr_hi = lim_r(wp_hi), lr_lo = lim_r(wp_lo);
    t_w = lr_hi > 0 ? min(ntl, (lr_hi + kBlockN - 1) / kBlockN) - 1 : -1;
    e_w = lr_lo > 0 ? lr_lo / kBlockN : 0;
    return true;
}

// One lane's query row `row` of the item: byte offsets into the sequence's Q / O / LSE
// descriptors (kOOB past the item's rows) and the key limit of tile 0 for the lane's keys.
// The lane holds Q bytes from qlane and O bytes from olane of the row; its keys start at 4 kq
// within each block, and only the lanes with kq = 0 store the LSE.  (32x32 MFMA: lane half hh
// -> qlane 16 hh QB, olane 16 hh, kq hh; 16x16: lane group g -> 16 g, 8 g, g.)
struct LaneRow { bool ok; int pos, head, qoff, ooff, loff, lim; };
template <int QB>
__device__ __forceinline__ LaneRow lane_row(const FwdParams& p, const KeyLimit& lim_r, const int row,
                                            const int rows_total, const int hk_i, const int qlane,
                                            const int olane, const int kq) {
    const int G = p.group;
    LaneRow r;
    r.ok = row < rows_total;
    r.pos = r.ok ? row / G : 0;
    r.head = hk_i * G + (r.ok ? row - r.pos * G : 0);
    r.qoff = r.ok ? (r.pos * (int)p.q_row + r.head * (int)p.q_head) * QB + qlane : kOOB;
    r.ooff = r.ok ? (r.pos * (int)p.o_row + r.head * (int)p.o_head) * 2 + olane : kOOB;
    r.loff = (r.ok && kq == 0) ? (int)(r.head * p.lse_head + r.pos) * 4 : kOOB;
    r.lim = (r.ok ? lim_r(r.pos) : lim_r.sk) - 4 * kq;     // rows past the item: no limit
    return r;
}

// An item no row of which sees a key: O = 0, LSE = +inf (the reference's empty-row output) for
// the lane's row (32x32 layout: lane half hh writes the 16-byte chunks 2 c + hh of the row).
__device__ __forceinline__ void store_empty_row(const FwdParams& p, const int bidx, const int q_off,
                                                const LaneRow& r, const int hh) {
    if (r.ooff == kOOB) return;
    char* oseq = reinterpret_cast<char*>(p.o) + ((int64_t)bidx * p.o_batch + (int64_t)q_off * p.o_row) * 2;
#pragma unroll
    for (int c = 0; c < 8; ++c) *reinterpret_cast<u32x4*>(oseq + r.ooff + 32 * c) = u32x4{0, 0, 0, 0};
    if (p.lse && hh == 0) p.lse[(int64_t)bidx * p.lse_batch + q_off + r.loff / 4] = INFINITY;
}

}  // namespace xfa
