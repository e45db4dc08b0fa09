// fmha_mla_index_ragged_kernel.h — the MLA indexer's logits for prefill (fmha_mla_index_logits_ragged),
// gfx950 (CDNA4): DeepGEMM's fp8_mqa_logits over a packed, non-paged key array,
//
//   logit[r, s] = k_scale[s] * sum_h w[r, h] * relu( sum_d q8[r, h, d] * k8[s, d] )   ks[r] <= s < ke[r]
//
// and -inf for every other s < N (the contract is in include/paged_attn.h).
// The opposite regime of fmha_mla_index_kernel.h: a key is reused by thousands of rows, so the
// kernel is bound by the fp8 MFMA rate and the relu / fma epilogue, and the design is about keeping
// q and the weights resident and skipping what no row may see.
//
//  * Product and operand mapping: those of fmha_mla_index_kernel.h (A = 32 heads x 64 features, B =
//    32 keys x 64 features, lane half l / 32 owns bytes [64 h, 64 h + 64) of its row, accumulator
//    row r of lane l is head 8 (r / 4) + 4 h + r % 4 of the head block): the arithmetic and its error
//    bound carry over.
//  * Item = 16 query rows x a chunk of kMlaRaggedChunk keys.  WAVES x NP = 16: wave w owns rows
//    [NP w, NP w + NP) and keeps their q (heads / 32 x 16 registers a row) and accumulator-row
//    weights (as many) resident for the whole chunk - IdxQuery<HB, NP>.  8 waves x 2 rows, two waves
//    a SIMD, is what is launched: measured 17-27 % faster than 4 waves x 4 rows at one wave a SIMD
//    (XFA_MLA_RAGGED_ROWS=4 builds that one).
//  * Keys enter the CU once per workgroup: a stage is 128 keys (four 4 KiB tiles) and their
//    scales, fetched with coalesced 16-byte loads (8 lanes a key row) into registers while the
//    stage before it is being multiplied, then written to one of two LDS slots; one barrier a
//    stage.  Image: byte (row, 16-byte chunk c) at row * 128 + 16 (c ^ (row / 2 % 8)) - the fp8
//    forward's K image (k8_off): the B operand reads (ds_read_b128, lane = key l % 32, chunks 4 h ..
//    4 h + 3) and the writes are free of bank conflicts (tools/mla_index_ragged_banks.py).
//  * Range skipping: lo = clamp(ks), hi = clamp(ke) per row; the workgroup takes the union
//    [min lo, max hi) of its rows, cut to the chunk and widened to stages.  Stages outside it issue
//    no loads and no MFMAs: all threads fill them with -inf, with 16-byte stores where the buffer's
//    alignment allows.  Inside, a wave whose rows all miss a tile stores -inf without MFMAs; else
//    the per-row select happens in registers (a select, not a multiply: NaN keys or scales outside
//    a row's range never reach it).
//  * Epilogue in registers, as idx_tile: relu, fma with the weights (one chain per head block), one
//    add across the lane halves, the scale, the select, one 128-byte store by lanes 0..31 per row
//    and tile.  Row i + 1's MFMAs are issued before row i's epilogue (independent accumulators).
//  * Grid = ceil(M / 16) x ceil(N / chunk), row blocks fastest: neighbours share a key chunk (L2).
//    Every logit has one writer: no scratch, no combine.
#pragma once

#include <type_traits>

#include "fmha_mla_index_kernel.h"

namespace xfa {

#ifndef XFA_MLA_RAGGED_ROWS                  // (an A/B build may set 4: tools/mla_index_ragged_ab.py)
#define XFA_MLA_RAGGED_ROWS 2                // (measured: DESIGN.md §3.13.2 - 2 beat 4)
#endif
constexpr int kRagRowsPerWave = XFA_MLA_RAGGED_ROWS;
constexpr int kRagStage = 128;               // keys of one LDS slot
constexpr int kRagStageTiles = kRagStage / kIdxTile;
static_assert(kMlaRaggedRows % kRagRowsPerWave == 0 && kMlaRaggedChunk % kRagStage == 0, "whole waves, whole stages");

// The 16 rows' ranges, clamped; rows past M are empty
__device__ __forceinline__ void rag_range(const MlaIndexRaggedParams& p, int r, int& lo, int& hi) {
    lo = hi = 0;
    if (r < p.m) {
        lo = max(0, min(p.ks[r], p.n));
        hi = max(0, min(p.ke[r], p.n));
    }
}

// -inf into columns [a, b) of the item's rows, by all threads; a % 4 == 0
template <int THREADS>
__device__ __forceinline__ void rag_fill(const MlaIndexRaggedParams& p, int r0, int a, int b, int tid) {
    if (a >= b) return;
    const bool vec = !((reinterpret_cast<uintptr_t>(p.logits) & 15) | (p.logits_row & 3));   // (uniform)
    const int b4 = vec ? a + ((b - a) & ~3) : a;
    for (int i = 0; i < kMlaRaggedRows && r0 + i < p.m; ++i) {
        float* row = p.logits + (int64_t)(r0 + i) * p.logits_row;
        for (int c = a + 4 * tid; c < b4; c += 4 * THREADS)
            *reinterpret_cast<f32x4*>(row + c) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int c = b4 + tid; c < b; c += THREADS) row[c] = -INFINITY;
    }
}

template <int HB, int NP>
__device__ __forceinline__ void rag_load_query(const MlaIndexRaggedParams& p, int row0, int lane, IdxQuery<HB, NP>& x) {
    const int m = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int r = min(row0 + i, p.m - 1);              // (uniform; a row past M is never stored)
        const uint8_t* qr = reinterpret_cast<const uint8_t*>(p.q8) + (int64_t)r * p.q_row;
        const float* wr = p.weights + (int64_t)r * (32 * HB);
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            const u32x4* src = reinterpret_cast<const u32x4*>(qr + (int64_t)(32 * hb + m) * p.q_head + 64 * h);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 lo = src[2 * j], hi = src[2 * j + 1];
                x.q[i][hb][j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            }
#pragma unroll
            for (int r16 = 0; r16 < 16; ++r16) x.w[i][hb][r16] = wr[32 * hb + 8 * (r16 >> 2) + 4 * h + (r16 & 3)];
        }
    }
}

template <int HEADS, int NP>
__global__ void __launch_bounds__(64 * (kMlaRaggedRows / NP)) fmha_mla_index_ragged_kernel(const MlaIndexRaggedParams p) {
    constexpr int HB = HEADS / 32, WAVES = kMlaRaggedRows / NP, THREADS = 64 * WAVES;
    constexpr int LOADS = kRagStage * 8 / THREADS;         // 16-byte pieces of a stage a thread moves
    static_assert(LOADS >= 1 && THREADS >= kRagStage, "a stage is whole loads; its scales one load of some threads");
    __shared__ __attribute__((aligned(16))) uint8_t lds_k[2][kRagStage * 128];
    __shared__ float lds_s[2][kRagStage];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x / p.row_blocks, rb = blockIdx.x - chunk * p.row_blocks;
    const int r0 = rb * kMlaRaggedRows;
    const int c0 = chunk * kMlaRaggedChunk, c1 = min(c0 + kMlaRaggedChunk, p.n);

    // the union of the rows' ranges, cut to the chunk and widened to stages: [st_lo, st_hi)
    int u_lo = p.n, u_hi = 0;
    for (int i = 0; i < kMlaRaggedRows; ++i) {
        int a, b;
        rag_range(p, r0 + i, a, b);
        if (a < b) u_lo = min(u_lo, a), u_hi = max(u_hi, b);
    }
    u_lo = max(u_lo, c0), u_hi = min(u_hi, c1);
    if (u_lo >= u_hi) {                                    // no row sees a key of this chunk
        rag_fill<THREADS>(p, r0, c0, c1, tid);
        return;
    }
    const int st_lo = (u_lo - c0) / kRagStage, st_hi = (u_hi - c0 + kRagStage - 1) / kRagStage;

    // stage st: 16-byte piece j * THREADS + tid = (key row, chunk) of the stage; a key past N - 1
    // reads the last key (it is in no row's range)
    u32x4 kreg[LOADS];
    float sreg = 0.f;
    auto fetch = [&](int st) {
        const int s0 = c0 + st * kRagStage;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const int piece = j * THREADS + tid;
            const int s = min(s0 + (piece >> 3), p.n - 1);
            kreg[j] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(p.k8) + (int64_t)s * p.k_row + 16 * (piece & 7));
        }
        if (tid < kRagStage) sreg = p.k_scale[min(s0 + tid, p.n - 1)];
    };
    auto publish = [&](int buf) {
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const int piece = j * THREADS + tid, row = piece >> 3;
            *reinterpret_cast<u32x4*>(&lds_k[buf][k8_off(row, piece & 7)]) = kreg[j];
        }
        if (tid < kRagStage) lds_s[buf][tid] = sreg;
    };
    fetch(st_lo);

    int lo[NP], hi[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) rag_range(p, r0 + wave * NP + i, lo[i], hi[i]);
    IdxQuery<HB, NP> x;
    rag_load_query<HB, NP>(p, r0 + wave * NP, lane, x);

    rag_fill<THREADS>(p, r0, c0, c0 + st_lo * kRagStage, tid);
    rag_fill<THREADS>(p, r0, min(c0 + st_hi * kRagStage, c1), c1, tid);

    const int m = lane & 31, h = lane >> 5;
    for (int st = st_lo; st < st_hi; ++st) {
        const int buf = (st - st_lo) & 1;
        publish(buf);
        __syncthreads();                                   // (the slot's readers of two stages ago passed the last one)
        if (st + 1 < st_hi) fetch(st + 1);
#pragma unroll
        for (int tt = 0; tt < kRagStageTiles; ++tt) {
            const int s0 = c0 + st * kRagStage + tt * kIdxTile;
            if (s0 >= c1) break;
            const int s = s0 + m;
            bool any = false;
#pragma unroll
            for (int i = 0; i < NP; ++i) any |= max(lo[i], s0) < min(hi[i], s0 + kIdxTile);
            if (!any) {                                    // (uniform) no row of this wave sees the tile
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int r = r0 + wave * NP + i;
                    if (r < p.m && lane < 32 && s < p.n) p.logits[(int64_t)r * p.logits_row + s] = -INFINITY;
                }
                continue;
            }
            const int row = tt * kIdxTile + m;
            i32x8 kb[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 a = *reinterpret_cast<const u32x4*>(&lds_k[buf][k8_off(row, 4 * h + 2 * j)]);
                const u32x4 b = *reinterpret_cast<const u32x4*>(&lds_k[buf][k8_off(row, 4 * h + 2 * j + 1)]);
                kb[j] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
            }
            const float scale = lds_s[buf][row];
            f32x16 acc[2][HB];
            auto product = [&](auto I) {
                constexpr int i = decltype(I)::value;
#pragma unroll
                for (int hb = 0; hb < HB; ++hb) {
                    f32x16 z = {0};
                    z = mfma_fp8(x.q[i][hb][0], kb[0], z);
                    acc[i & 1][hb] = mfma_fp8(x.q[i][hb][1], kb[1], z);
                }
            };
            auto row_out = [&](auto I) {
                constexpr int i = decltype(I)::value;
                if constexpr (i + 1 < NP) product(std::integral_constant<int, i + 1>{});
                float sum = 0.f;
#pragma unroll
                for (int hb = 0; hb < HB; ++hb) {
                    float part = 0.f;
#pragma unroll
                    for (int r16 = 0; r16 < 16; ++r16) part = fmaf(x.w[i][hb][r16], fmaxf(acc[i & 1][hb][r16], 0.f), part);
                    sum += part;
                }
                sum = wave_sum_halves(sum) * scale;
                const float out = (s >= lo[i] && s < hi[i]) ? sum : -INFINITY;
                const int r = r0 + wave * NP + i;
                if (r < p.m && lane < 32 && s < p.n) p.logits[(int64_t)r * p.logits_row + s] = out;
            };
            product(std::integral_constant<int, 0>{});
            row_out(std::integral_constant<int, 0>{});
            if constexpr (NP > 1) row_out(std::integral_constant<int, 1>{});
            if constexpr (NP > 2) row_out(std::integral_constant<int, 2>{});
            if constexpr (NP > 3) row_out(std::integral_constant<int, 3>{});
        }
    }
}

}  // namespace xfa
