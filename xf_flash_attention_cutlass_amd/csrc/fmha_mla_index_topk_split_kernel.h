// fmha_mla_index_topk_split_kernel.h — the MLA indexer's selection with a row split over several
// workgroups (fmha_mla_index_topk_split), gfx950 (CDNA4); DESIGN.md §3.13.4, the contract is in
// include/paged_attn.h.  The select itself - key, order, ties, what is never read, rank, store -
// is fmha_mla_index_select.h's; here are two work splits over it:
//
//  * fmha_mla_index_topk_part_kernel, grid rows x S: workgroup (row, c) selects over the chunk of
//    visible columns [c L, min((c + 1) L, vis)) and writes its selection to scratch in ascending
//    position: the keys at keys[row][c][0 .. count), their columns at cols[row][c][0 .. count),
//    count at counts[row][c].  L <= kMlaTopkStage: a chunk is read from global memory once,
//    transformed, and kept in LDS as keys for every later sweep.
//  * fmha_mla_index_topk_merge_kernel, grid rows: the row's S topk candidate keys, in list order
//    (chunk, then place), staged in LDS; a place at or beyond its chunk's count is key 0 and is not
//    read.  The same select over the list; a selected place's column comes from scratch and goes
//    through the block table as in fmha_mla_index_topk_kernel.h.
//
// Exact because an element with fewer than topk elements ahead of it in the row's order (key
// descending, position ascending) has fewer than topk ahead of it in its chunk: every globally
// selected element is in its chunk's selection; the list is in ascending position, so the select
// over it breaks ties and orders its output as the select over the row does.  Every scratch and
// output word has one writer; there are no atomics on global memory.
//
//  * Threshold, both kernels: passes of 8 bits over 8 LDS histograms (one per wave pair), as the
//    one-workgroup kernel's, always over LDS after the first sweep.
#pragma once

#include "fmha_launch.h"
#include "fmha_mla_index_select.h"

namespace xfa {

constexpr int kTopkSplitWaves = 16;
constexpr int kTopkSplitThreads = kTopkSplitWaves * 64;
constexpr int kTopkSplitHists = 8;                  // LDS histograms: one per wave pair
// LDS words: histograms, the summed bins, the per-wave counts (> T, == T), the scan's verdict
constexpr int kTopkSplitTotW = kTopkSplitHists * 256, kTopkSplitCntW = kTopkSplitTotW + 256;
constexpr int kTopkSplitCtlW = kTopkSplitCntW + 2 * kTopkSplitWaves, kTopkSplitKeysW = kTopkSplitCtlW + 32;
static_assert(kTopkSplitKeysW % 4 == 0, "the staged keys are read 16 bytes at a time");
// ... then the staged keys: virtual columns, so up to 3 more than the keys, whole vectors
constexpr int topk_split_lds_bytes(int keys) { return 4 * (kTopkSplitKeysW + (keys > 0 ? (keys + 3 + 3) / 4 * 4 : 0)); }
static_assert(topk_split_lds_bytes(kMlaTopkStage) <= 147456, "a staged chunk or list and the histograms fit the LDS");

// The threshold of the keys r walks, more than topk of them.  FETCH: the first pass reads them from
// global memory and stages them in LDS (else they are staged already); every later pass reads LDS.
template <bool FETCH>
__device__ __forceinline__ TopkCut topk_split_threshold(const TopkRow& r, unsigned* lds, int topk, int tid) {
    unsigned* const tot = lds + kTopkSplitTotW;
    unsigned* const ctl = lds + kTopkSplitCtlW;
    unsigned* const skeys = lds + kTopkSplitKeysW;
    const int lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < kTopkSplitHists * 256; t += kTopkSplitThreads) lds[t] = 0u;
    __syncthreads();
    unsigned* const h = lds + (wave >> 1) * 256;
    unsigned prefix = 0u, need = (unsigned)topk, state = 0u;
    int shift = 24;
    for (; shift >= 0 && state == 0u; shift -= 8) {
        if (FETCH && shift == 24)
            topk_sweep(r, false, skeys, [&](int64_t v0, const unsigned k[4]) {
                if (v0 < r.lr) *reinterpret_cast<u32x4*>(skeys + v0) = u32x4{k[0], k[1], k[2], k[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j) topk_hist<2>(h, k[j], 0u, 24, 8, lane);
            });
        else
            topk_sweep(r, true, skeys, [&](int64_t, const unsigned k[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) topk_hist<2>(h, k[j], prefix, shift, 8, lane);
            });
        __syncthreads();
        if (tid < 256) {
            unsigned s = 0u;
#pragma unroll
            for (int g = 0; g < kTopkSplitHists; ++g) { s += lds[g * 256 + tid]; lds[g * 256 + tid] = 0u; }
            tot[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {                                                   // lane l: bins 4 l .. 4 l + 3
            const u32x4 x = *reinterpret_cast<const u32x4*>(tot + 4 * lane);
            const unsigned c[4] = {x[0], x[1], x[2], x[3]}, mine = c[0] + c[1] + c[2] + c[3];
            topk_verdict(ctl, c, topk_suffix(mine, lane) - mine, 4 * lane, prefix, 8, need);
        }
        __syncthreads();
        if (ctl[2] != 2u) { prefix = ctl[0]; need = ctl[1]; }
        state = ctl[2];
    }
    return topk_cut(state, prefix, need, shift + 8);
}

// Keys > T and == T before this wave, and the entries of the whole walk (one barrier)
__device__ __forceinline__ TopkRuns topk_split_runs(const TopkRow& r, bool staged, unsigned* lds, TopkCut cut, int topk,
                                                    int wave, int lane) {
    int cg = 0, ce = 0;
    topk_sweep(r, staged, lds + kTopkSplitKeysW, [&](int64_t, const unsigned k[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { cg += k[j] > cut.T; ce += k[j] == cut.T; }
    });
    topk_wave_counts<kTopkSplitWaves>(lds + kTopkSplitCntW, cg, ce, wave, lane);
    __syncthreads();
    return topk_wave_scan<kTopkSplitWaves>(lds + kTopkSplitCntW, wave, cut.need_eq, topk);
}

__global__ void __launch_bounds__(kTopkSplitThreads) fmha_mla_index_topk_part_kernel(const MlaIndexTopkSplitParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* const lds = reinterpret_cast<unsigned*>(smem);
    unsigned* const skeys = lds + kTopkSplitKeysW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x / p.splits, c = blockIdx.x - row * p.splits;
    const int bi = row / p.seqlen_q, pos = row - bi * p.seqlen_q;
    const int n = max(0, min(p.context_lens[bi], p.max_seqlen_k));
    const int vis = max(0, min(n - p.seqlen_q + pos + 1, n));
    const int lo = min(c * p.chunk, vis);                                  // (splits * chunk < 2^20)
    const int topk = p.topk;
    const TopkRow r = topk_row<kTopkSplitWaves>(p.logits + (int64_t)row * p.logits_row + lo, min(p.chunk, vis - lo), wave, lane);
    const int64_t at = ((int64_t)row * p.splits + c) * topk;
    int* const cols = p.cols + at;
    int* const keys = reinterpret_cast<int*>(p.keys + at);

    const bool staged = r.vis > topk;                                      // (uniform, like all below)
    const TopkCut cut = staged ? topk_split_threshold<true>(r, lds, topk, tid) : TopkCut{0u, 0};
    TopkRuns run = topk_split_runs(r, staged, lds, cut, topk, wave, lane);

    // ---- the ordered emit: a pair is two stores at the same rank
    topk_sweep(r, staged, skeys, [&](int64_t v0, const unsigned k[4]) {
        const TopkRank q = topk_rank(k, cut.T, cut.need_eq);
        topk_store(cols, v0, q, run.gt_run, run.eq_run, cut.need_eq, topk,
                   [&](int64_t c0, int j) { return lo + (int)(c0 - r.a) + j; });
        topk_store(keys, v0, q, run.gt_run, run.eq_run, cut.need_eq, topk, [&](int64_t, int j) { return (int)k[j]; });
        run.gt_run += q.tg; run.eq_run += q.te;
    });
    if (tid == 0) p.counts[(int64_t)row * p.splits + c] = run.count;
}

__global__ void __launch_bounds__(kTopkSplitThreads) fmha_mla_index_topk_merge_kernel(const MlaIndexTopkSplitParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* const lds = reinterpret_cast<unsigned*>(smem);
    unsigned* const skeys = lds + kTopkSplitKeysW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, bi = row / p.seqlen_q;
    const int* table = p.block_table + (int64_t)bi * p.bt_stride;
    int* out = p.indices + (int64_t)row * p.indices_row;
    const int topk = p.topk, list = p.splits * topk;                       // (<= kMlaTopkStage)
    const int64_t at = (int64_t)row * list;
    const int* const cols = p.cols + at;

    // ---- the list: what the chunks wrote, key 0 behind it
    int have = 0;
    for (int c = 0; c < p.splits; ++c) {
        const int count = max(0, min(p.counts[(int64_t)row * p.splits + c], topk));
        for (int j = tid; j < topk; j += kTopkSplitThreads) skeys[c * topk + j] = j < count ? p.keys[at + c * topk + j] : 0u;
        have += count;
    }
    if (tid < ((4 - list) & 3)) skeys[list + tid] = 0u;                    // (the last vector's rest)
    __syncthreads();
    const TopkRow r = topk_row<kTopkSplitWaves>(reinterpret_cast<const float*>(skeys), list, wave, lane);   // (a = 0)

    const TopkCut cut = have > topk ? topk_split_threshold<false>(r, lds, topk, tid) : TopkCut{0u, 0};
    TopkRuns run = topk_split_runs(r, true, lds, cut, topk, wave, lane);

    // ---- the ordered emit: place -> column -> slot
    topk_sweep(r, true, skeys, [&](int64_t v0, const unsigned k[4]) {
        const TopkRank q = topk_rank(k, cut.T, cut.need_eq);
        int cur = -2, blk = -1;
        topk_store(out, v0, q, run.gt_run, run.eq_run, cut.need_eq, topk, [&](int64_t c0, int j) {
            const int col = cols[c0 + j];
            const int pg = col / p.page, off = col - pg * p.page;
            if (pg != cur) { cur = pg; blk = table[pg]; }
            const int64_t slot = (int64_t)blk * p.page + off;
            return ((unsigned)blk < (unsigned)p.num_blocks && slot <= 0x7fffffffLL) ? (int)slot : -1;
        });
        run.gt_run += q.tg; run.eq_run += q.te;
    });
    topk_tail<kTopkSplitThreads>(out, run.count, topk, tid);
}

}  // namespace xfa
