// fmha_mla_index_topk_kernel.h — the MLA indexer's selection (fmha_mla_index_topk), gfx950 (CDNA4):
// for every row of fmha_mla_index_logits' result the topk largest visible logits, as physical
// cache slots in ascending key position, -1 behind them (the contract is in
// include/paged_attn.h).  The select itself - key, order, ties, what is never read, one writer per
// output word - is fmha_mla_index_select.h's; here are the work split and the pass structure for
// tens of long rows:
//
//  * Work: one workgroup of 16 waves per row, the row's candidates its visible columns [0, vis).
//  * Threshold T: passes of 8 bits (4 at most), the shift a run-time value of one loop.  A pass
//    counts into one of 8 LDS histograms (one per wave pair), two leader rounds before the LDS add.
//    256 threads sum the 8 histograms (and clear them), wave 0 gives the verdict over the 256 bins.
//    8-bit digits and not 11 + 11 + 10: 8 private histograms are 8 KB, not 64 KB, beside a staged
//    row of 128 KB; the fourth pass reads LDS.
//  * The row between passes: a row of at most kMlaTopkStage visible keys is transformed once, in
//    pass 0, and kept in LDS as keys (128 KB); a longer row is read again from global memory (L2)
//    in every pass, four 16-byte loads in flight per lane.
//  * vis <= topk (every step of a short context) skips the passes: T = 0 selects what is selectable.
//  * Emit: one count sweep (keys > T and keys == T per wave), the scan over waves, then the
//    ordered sweep.  The entry is block_table[column / page] * page + column % page in 64 bits, one
//    division per lane and step and one table read per page run; a table entry outside
//    [0, num_blocks) or a slot beyond int32 gives -1 in place.
#pragma once

#include "fmha_launch.h"
#include "fmha_mla_index_select.h"

namespace xfa {

constexpr int kTopkWaves = 16;
constexpr int kTopkThreads = kTopkWaves * 64;
constexpr int kTopkHists = 8;                       // LDS histograms: one per wave pair
// LDS words: histograms, the summed bins, the per-wave counts (> T, == T), the scan's verdict
constexpr int kTopkHistW = 0, kTopkTotW = kTopkHists * 256, kTopkCntW = kTopkTotW + 256;
constexpr int kTopkCtlW = kTopkCntW + 2 * kTopkWaves, kTopkKeysW = kTopkCtlW + 32;
static_assert(kTopkKeysW % 4 == 0, "the staged keys are read 16 bytes at a time");
// ... then the staged keys: virtual columns, so up to 3 more than the visible keys, whole vectors
constexpr int topk_lds_bytes(int keys) { return 4 * (kTopkKeysW + (keys > 0 ? (keys + 3 + 3) / 4 * 4 : 0)); }
static_assert(topk_lds_bytes(kMlaTopkStage) <= 147456, "the staged row and the histograms fit the LDS");

__global__ void __launch_bounds__(kTopkThreads) fmha_mla_index_topk_kernel(const MlaIndexTopkParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* const lds = reinterpret_cast<unsigned*>(smem);
    unsigned* const hist = lds + kTopkHistW;
    unsigned* const tot = lds + kTopkTotW;
    unsigned* const wcnt = lds + kTopkCntW;
    unsigned* const ctl = lds + kTopkCtlW;
    unsigned* const skeys = lds + kTopkKeysW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, bi = row / p.seqlen_q, pos = row - bi * p.seqlen_q;
    const int n = max(0, min(p.context_lens[bi], p.max_seqlen_k));
    const int* table = p.block_table + (int64_t)bi * p.bt_stride;
    int* out = p.indices + (int64_t)row * p.indices_row;
    const int topk = p.topk;
    const TopkRow r = topk_row<kTopkWaves>(p.logits + (int64_t)row * p.logits_row, max(0, min(n - p.seqlen_q + pos + 1, n)),
                                           wave, lane);

    // ---- the threshold
    TopkCut cut{0u, 0};
    bool staged = false;
    if (r.vis > topk) {                                                    // (uniform, like all below)
        staged = r.vis <= kMlaTopkStage;
        for (int t = tid; t < kTopkHists * 256; t += kTopkThreads) hist[t] = 0u;
        __syncthreads();
        unsigned* const h = hist + (wave >> 1) * 256;
        unsigned prefix = 0u, need = (unsigned)topk, state = 0u;
        int shift = 24;
        for (; shift >= 0 && state == 0u; shift -= 8) {
            if (shift == 24)
                topk_sweep(r, false, skeys, [&](int64_t v0, const unsigned k[4]) {
                    if (staged && v0 < r.lr) *reinterpret_cast<u32x4*>(skeys + v0) = u32x4{k[0], k[1], k[2], k[3]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) topk_hist<2>(h, k[j], 0u, 24, 8, lane);
                });
            else
                topk_sweep(r, staged, skeys, [&](int64_t, const unsigned k[4]) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) topk_hist<2>(h, k[j], prefix, shift, 8, lane);
                });
            __syncthreads();
            if (tid < 256) {
                unsigned s = 0u;
#pragma unroll
                for (int g = 0; g < kTopkHists; ++g) { s += hist[g * 256 + tid]; hist[g * 256 + tid] = 0u; }
                tot[tid] = s;
            }
            __syncthreads();
            if (wave == 0) {                                               // lane l: bins 4 l .. 4 l + 3
                const u32x4 x = *reinterpret_cast<const u32x4*>(tot + 4 * lane);
                const unsigned c[4] = {x[0], x[1], x[2], x[3]}, mine = c[0] + c[1] + c[2] + c[3];
                topk_verdict(ctl, c, topk_suffix(mine, lane) - mine, 4 * lane, prefix, 8, need);
            }
            __syncthreads();
            if (ctl[2] != 2u) { prefix = ctl[0]; need = ctl[1]; }
            state = ctl[2];
        }
        cut = topk_cut(state, prefix, need, shift + 8);
    }
    const unsigned T = cut.T;
    const int need_eq = cut.need_eq;

    // ---- per-wave counts of keys > T and keys == T, and the scan over waves
    int cg = 0, ce = 0;
    topk_sweep(r, staged, skeys, [&](int64_t, const unsigned k[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { cg += k[j] > T; ce += k[j] == T; }
    });
    topk_wave_counts<kTopkWaves>(wcnt, cg, ce, wave, lane);
    __syncthreads();
    TopkRuns run = topk_wave_scan<kTopkWaves>(wcnt, wave, need_eq, topk);

    // ---- the ordered emit
    topk_sweep(r, staged, skeys, [&](int64_t v0, const unsigned k[4]) {
        const TopkRank q = topk_rank(k, T, need_eq);
        if (q.hit()) {                                    // (a lane with nothing to store does not divide)
            const int c0 = (int)(v0 - r.a);               // (>= -3; a lane with a hit has c0 < vis)
            const int pg0 = c0 >= 0 ? c0 / p.page : -1, off0 = c0 - pg0 * p.page;
            int cur = -2, blk = -1;
            topk_store(out, c0, q, run.gt_run, run.eq_run, need_eq, topk, [&](int64_t, int j) {
                const bool next = off0 + j >= p.page;     // (a page is 16 columns or more: one boundary a step)
                const int pg = pg0 + next, off = off0 + j - (next ? p.page : 0);
                if (pg != cur) { cur = pg; blk = table[pg]; }
                const int64_t slot = (int64_t)blk * p.page + off;
                return ((unsigned)blk < (unsigned)p.num_blocks && slot <= 0x7fffffffLL) ? (int)slot : -1;
            });
        }
        run.gt_run += q.tg; run.eq_run += q.te;
    });
    topk_tail<kTopkThreads>(out, run.count, topk, tid);
}

}  // namespace xfa
