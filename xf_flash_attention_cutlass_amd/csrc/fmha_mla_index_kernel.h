// fmha_mla_index_kernel.h — the MLA indexer's logits (fmha_mla_index_logits), gfx950 (CDNA4):
// DeepSeek-V3.2's "lightning indexer" over a paged fp8 index-key cache,
//
//   logit[r, s] = descale[s] * sum_h w[r, h] * relu( sum_d q8[r, h, d] * k8[s, d] )
//
// for every query row r = (batch, position) and every key s the row may see, -inf for the keys it
// may not (the contract is in include/paged_attn.h).  One pass over 132 bytes a
// key; HBM-bound, so the design is about keeping loads in flight, not about the MFMA rate.
//
//  * Product: S[heads x keys] on v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales (mfma_fp8):
//    A = 32 heads of q x 64 features, B = 32 keys x 64 features, heads / 32 x 2 MFMAs a 32-key tile
//    and position.  Lane l supplies A row l % 32 (a head) and B column l % 32 (a key), 32 bytes
//    each; the reduction index may be permuted as long as both operands agree, so lane half
//    h = l / 32 takes bytes [64 h, 64 h + 64) of its row, the first 32 for the first MFMA: a lane's
//    four 16-byte loads are one contiguous 64-byte run and the wave's loads of one tile cover its 32
//    128-byte lines exactly once.  The accumulator gives lane l key l % 32 and the 16 heads
//    8 (r / 4) + 4 h + r % 4 of the head block.
//  * q stays in registers for the whole key walk (heads / 32 x 16 VGPRs a position), and so do
//    the weights, laid out as the 16 accumulator rows the lane owns per head block.  Up to two
//    positions are resident; a longer seqlen_q is walked in groups of two per key tile, re-reading
//    q and the weights (cache hits) and the tile's registers, never the keys from HBM.
//  * Keys go from global memory straight to the B operand: no LDS, no barrier.  Each lane resolves
//    its own key's page (block_table[(s0 + l % 32) / page]), so a tile may straddle pages.  The
//    loads run kIdxAhead tiles ahead (one: measured against two and three) and
//    the block-table entry one tile further, so that the wait for a table entry never waits for a
//    key tile issued after it.  A lane without a key (past
//    the sequence, or behind a table entry outside [0, num_blocks)) reads row 0 of block 0 and its
//    result is replaced by -inf: no table value becomes an address.
//  * Epilogue in registers: relu, fma with the lane's weights, one add across the lane halves, the
//    descale, the visibility select, one 128-byte store of 32 consecutive logits by lanes 0..31.
//  * Work: item = (batch, chunk of kMlaIndexChunk keys); 4 waves, wave w the chunk's tiles
//    [8 w, 8 w + 8); grid = batch x ceil(max_seqlen_k / chunk) from the host's max_seqlen_k alone.
//    Every logit has one writer: no scratch, no combine.
#pragma once

#include "fmha_common.h"
#include "fmha_fwd_fp8_kernel.h"
#include "fmha_launch.h"

namespace xfa {

constexpr int kIdxTile = 32;                 // keys of one MFMA tile
constexpr int kIdxWaves = 4;
constexpr int kIdxTilesPerWave = kMlaIndexChunk / kIdxTile / kIdxWaves;
#ifndef XFA_MLA_INDEX_AHEAD                  // (an A/B build may set another: tools/mla_index_ab.py)
#define XFA_MLA_INDEX_AHEAD 1                // (measured: DESIGN.md §3.13 - 1 beat 2 and 3)
#endif
constexpr int kIdxAhead = XFA_MLA_INDEX_AHEAD;   // key tiles in flight beyond the one being consumed
static_assert(kMlaIndexChunk % (kIdxTile * kIdxWaves) == 0, "a chunk is whole tiles for every wave");

// One lane's share of a key tile: its quarter row as the two B operands, its key's descale, and
// whether the key exists (in the sequence, behind a valid table entry).
struct IdxKeys {
    i32x8 k[2];
    float descale;
    int ok;
};

// Block of lane's key of the tile at s0.  Unconditional, so that no branch stands between the loads:
// a key past n - 1 asks for the last key's entry, an empty sequence for entry 0 (the table has one:
// max_seqlen_k >= 1 in every launch)
__device__ __forceinline__ int idx_block(const MlaIndexParams& p, const int* table, int n, int s0, int lane) {
    const int s = max(0, min(s0 + (lane & 31), n - 1));
    return table[s / p.page];
}

__device__ __forceinline__ IdxKeys idx_load(const MlaIndexParams& p, int blk, int n, int s0, int lane) {
    const int s = s0 + (lane & 31);
    const bool ok = s < n && (unsigned)blk < (unsigned)p.num_blocks;
    const int row = ok ? s % p.page : 0;
    const uint8_t* block = reinterpret_cast<const uint8_t*>(p.cache) + (ok ? (int64_t)blk * p.page * 132 : 0);
    const u32x4* src = reinterpret_cast<const u32x4*>(block + row * 128 + 64 * (lane >> 5));
    IdxKeys t;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const u32x4 lo = src[2 * j], hi = src[2 * j + 1];
        t.k[j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    }
    t.descale = *reinterpret_cast<const float*>(block + (int64_t)p.page * 128 + 4 * row);
    t.ok = ok;
    return t;
}

// q and the weights of the positions [pos0, pos0 + NP) of batch bi, as the lane needs them
template <int HB, int NP>
struct IdxQuery {
    i32x8 q[NP][HB][2];
    float w[NP][HB][16];
};

template <int HB, int NP>
__device__ __forceinline__ void idx_load_query(const MlaIndexParams& p, int bi, int pos0, int lane, IdxQuery<HB, NP>& x) {
    const int m = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool live = pos0 + i < p.seqlen_q;           // (uniform)
        const int pos = live ? pos0 + i : pos0;
        const uint8_t* qr = reinterpret_cast<const uint8_t*>(p.q8) + (int64_t)bi * p.q_batch + (int64_t)pos * p.q_row;
        const float* wr = p.weights + ((int64_t)bi * p.seqlen_q + pos) * p.heads;
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            const u32x4* src = reinterpret_cast<const u32x4*>(qr + (int64_t)(32 * hb + m) * p.q_head + 64 * h);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 lo = src[2 * j], hi = src[2 * j + 1];
                x.q[i][hb][j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) x.w[i][hb][r] = wr[32 * hb + 8 * (r >> 2) + 4 * h + (r & 3)];
        }
    }
}

// The logits of one key tile for the positions of x, stored
template <int HB, int NP>
__device__ __forceinline__ void idx_tile(const MlaIndexParams& p, const IdxQuery<HB, NP>& x, const IdxKeys& t,
                                         int bi, int pos0, int n, int s0, int lane) {
    const int s = s0 + (lane & 31);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pos = pos0 + i;
        if (pos >= p.seqlen_q) break;                      // (uniform)
        float sum = 0.f;
        if (s0 < n) {                                      // (uniform: a tile past the sequence is all -inf)
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                f32x16 acc = {0};
                acc = mfma_fp8(x.q[i][hb][0], t.k[0], acc);
                acc = mfma_fp8(x.q[i][hb][1], t.k[1], acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) sum = fmaf(x.w[i][hb][r], fmaxf(acc[r], 0.f), sum);
            }
            sum = wave_sum_halves(sum) * t.descale;
        }
        const int vis = max(0, min(n - p.seqlen_q + pos + 1, n));
        const float out = (t.ok && s < vis) ? sum : -INFINITY;
        if (lane < 32 && s < p.max_seqlen_k)
            p.logits[((int64_t)bi * p.seqlen_q + pos) * p.logits_row + s] = out;
    }
}

// NP positions resident; MANY: seqlen_q > NP, walked in groups of NP per key tile
template <int HEADS, int NP, bool MANY>
__global__ void __launch_bounds__(kIdxWaves * 64) fmha_mla_index_logits_kernel(const MlaIndexParams p) {
    constexpr int HB = HEADS / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = (p.max_seqlen_k + kMlaIndexChunk - 1) / kMlaIndexChunk;
    const int bi = blockIdx.x / chunks, chunk = blockIdx.x - bi * chunks;
    const int n = max(0, min(p.context_lens[bi], p.max_seqlen_k));
    const int* table = p.block_table + (int64_t)bi * p.bt_stride;
    const int s_lo = chunk * kMlaIndexChunk + wave * (kIdxTilesPerWave * kIdxTile);
    if (s_lo >= p.max_seqlen_k) return;

    IdxQuery<HB, NP> x;
    if (!MANY && s_lo < n) idx_load_query<HB, NP>(p, bi, 0, lane, x);

    // tile i's keys are asked for at step i - kIdxAhead, its table entry one step earlier; a tile
    // at or past n asks for nothing new (every lane reads the last table entry and block 0, row 0)
    IdxKeys keys[kIdxAhead + 1];
    int blk = 0;
    auto block_of = [&](int i) { return idx_block(p, table, n, s_lo + i * kIdxTile, lane); };
#pragma unroll
    for (int i = 0; i < kIdxAhead; ++i) {
        blk = block_of(i);
        keys[i] = idx_load(p, blk, n, s_lo + i * kIdxTile, lane);
    }
    blk = block_of(kIdxAhead);
#pragma unroll
    for (int i = 0; i < kIdxTilesPerWave; ++i) {
        const int s0 = s_lo + i * kIdxTile;
        if (s0 >= p.max_seqlen_k) break;
        if (i + kIdxAhead < kIdxTilesPerWave) {
            const int next = block_of(i + kIdxAhead + 1);
            keys[(i + kIdxAhead) % (kIdxAhead + 1)] = idx_load(p, blk, n, s0 + kIdxAhead * kIdxTile, lane);
            blk = next;
        }
        const IdxKeys& t = keys[i % (kIdxAhead + 1)];
        if constexpr (MANY) {
            for (int pos0 = 0; pos0 < p.seqlen_q; pos0 += NP) {
                if (s0 < n) idx_load_query<HB, NP>(p, bi, pos0, lane, x);
                idx_tile<HB, NP>(p, x, t, bi, pos0, n, s0, lane);
            }
        } else {
            idx_tile<HB, NP>(p, x, t, bi, 0, n, s0, lane);
        }
    }
}

}  // namespace xfa
