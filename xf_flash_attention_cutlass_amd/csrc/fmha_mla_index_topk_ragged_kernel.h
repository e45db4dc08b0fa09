// fmha_mla_index_topk_ragged_kernel.h — the MLA indexer's selection for prefill rows
// (fmha_mla_index_topk_ragged), gfx950 (CDNA4): for every row of fmha_mla_index_logits_ragged's
// result the topk largest logits of its own column range [lo, hi), as cache slots (or columns) in
// ascending column order, -1 behind them (the contract is in
// include/paged_attn.h).  The select itself - key, order, ties, what is never read, one writer per
// output word - is fmha_mla_index_select.h's, the text fmha_mla_index_topk_kernel runs; here are
// the work split and the pass structure for thousands of rows of every length:
//
//  * Work: one workgroup of 4 waves per row, the row's candidates its columns [lo, hi), blockIdx 0
//    the LAST row (in a causal chunk the longest rows start first).  At most 25 KB of LDS: a
//    histogram of 2048 bins, a list of 2048 (key, column) pairs and 64 control words, sized by the
//    launch (no histogram and no list where no row can be longer than topk) - four workgroups and
//    more share a CU, and a barrier joins 4 waves.
//  * hi - lo <= topk: no threshold.  One sweep in workgroup-wide steps of 1024 columns; per step a
//    ballot count per wave, one barrier (the counts are double-buffered), the ordered store.
//  * Threshold otherwise: three unrolled passes of 11 + 11 + 10 bits, one leader round before the
//    LDS add, every thread the verdict over its own bins of the one histogram.  Pass 0 (sign,
//    exponent, 2 mantissa bits: index logits sit in a few exponents, so 8 bits would leave the whole
//    row in one bin) counts from global memory.  If the bin the threshold falls in holds at most
//    kMlaTopkRaggedStage keys, a second sweep writes them to LDS as (key, virtual column) and counts,
//    per wave, the keys of higher bins; passes 1 and 2 and the per-wave counts of keys > T and == T
//    then run over that list alone, and global memory is read once more, by the emit: three reads
//    of the row in all.  A larger bin (equal values, values that share 11 bits) keeps to global
//    memory: passes 1 and 2 re-read the row (L2) under the prefix, then a count sweep, then the emit.
//    The list is filled through an LDS counter in no fixed order; it is only ever counted, so the
//    result does not depend on that order.
//  * Emit: the entry is slots[column] when that lies in [0, 2^31), else -1 in place - or the column.
#pragma once

#include "fmha_launch.h"
#include "fmha_mla_index_select.h"

namespace xfa {

#ifndef XFA_RAGTOPK_BITS0                   // (A/B builds: tools/mla_index_topk_ragged_ab.py)
#define XFA_RAGTOPK_BITS0 11
#endif
#ifndef XFA_RAGTOPK_COMPACT
#define XFA_RAGTOPK_COMPACT 1
#endif
#ifndef XFA_RAGTOPK_REVERSE
#define XFA_RAGTOPK_REVERSE 1
#endif
constexpr int kRagTopkWaves = kMlaTopkRaggedThreads / 64;
constexpr int kRagTopkB0 = XFA_RAGTOPK_BITS0, kRagTopkB1 = (32 - kRagTopkB0 + 1) / 2, kRagTopkB2 = 32 - kRagTopkB0 - kRagTopkB1;
constexpr int kRagTopkBins = 1 << (kRagTopkB0 > kRagTopkB1 ? kRagTopkB0 : kRagTopkB1);
// LDS words: control (verdict 0..3, list length 4), the scan's wave totals, the per-wave counts,
// the histogram, then the list's keys and its columns (`cap` each)
constexpr int kRagTopkTotW = 8, kRagTopkCntW = 24, kRagTopkHistW = 64;
static_assert(kRagTopkWaves <= 16 && kRagTopkTotW + kRagTopkWaves <= kRagTopkCntW && kRagTopkCntW + 2 * kRagTopkWaves <= kRagTopkHistW,
              "the control words hold a count per wave");
constexpr int ragtopk_cap(int keys, int topk) {
    return XFA_RAGTOPK_COMPACT && keys > topk ? (keys < kMlaTopkRaggedStage ? keys : kMlaTopkRaggedStage) : 0;
}
constexpr int ragtopk_lds_bytes(int keys, int topk) {
    return 4 * (kRagTopkHistW + (keys > topk ? kRagTopkBins + 2 * ragtopk_cap(keys, topk) : 0));
}
static_assert(4 * ragtopk_lds_bytes(0x7fffffff, 1) <= 163840 || kRagTopkWaves != 4, "four workgroups share a CU's LDS");

// One pass' histogram of digit [SHIFT, SHIFT + BITS), from the list (keys lkey[0, n)) or from
// global memory
template <int SHIFT, int BITS>
__device__ __forceinline__ void ragtopk_pass(const TopkRow& r, bool list, const unsigned* lkey, int n, unsigned* hist,
                                             unsigned prefix, int tid, int lane) {
    if (list) {
        for (int i0 = 0; i0 < n; i0 += kMlaTopkRaggedThreads)
            topk_hist<1>(hist, i0 + tid < n ? lkey[i0 + tid] : 0u, prefix, SHIFT, BITS, lane);
    } else {
        topk_sweep(r, false, lkey, [&](int64_t, const unsigned k[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) topk_hist<1>(hist, k[j], prefix, SHIFT, BITS, lane);
        });
    }
}

// The verdict of a pass of 2^BITS bins into ctl: thread t owns bins PT t .. PT t + PT - 1 (and clears
// them), a suffix scan over lanes and waves gives the count above them
template <int BITS>
__device__ __forceinline__ void ragtopk_scan(unsigned* hist, unsigned* wtot, unsigned* ctl, unsigned prefix, unsigned need,
                                             int tid, int lane, int wave) {
    constexpr int PT = (1 << BITS) / kMlaTopkRaggedThreads;
    static_assert(PT >= 1 && PT * kMlaTopkRaggedThreads == (1 << BITS), "every thread owns whole bins");
    __syncthreads();
    unsigned c[PT], mine = 0u;
#pragma unroll
    for (int j = 0; j < PT; ++j) { c[j] = hist[PT * tid + j]; hist[PT * tid + j] = 0u; mine += c[j]; }
    unsigned sfx = topk_suffix(mine, lane);
    if (lane == 0) wtot[wave] = sfx;
    __syncthreads();
#pragma unroll
    for (int w = 1; w < kRagTopkWaves; ++w)
        if (w > wave) sfx += wtot[w];
    topk_verdict(ctl, c, sfx - mine, PT * tid, prefix, BITS, need);
    __syncthreads();
}

__global__ void __launch_bounds__(kMlaTopkRaggedThreads) fmha_mla_index_topk_ragged_kernel(const MlaIndexTopkRaggedParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* const ctl = reinterpret_cast<unsigned*>(smem);
    unsigned* const wtot = ctl + kRagTopkTotW;
    unsigned* const wcnt = ctl + kRagTopkCntW;
    unsigned* const hist = ctl + kRagTopkHistW;
    unsigned* const lkey = hist + kRagTopkBins;
    unsigned* const lcol = lkey + p.cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = XFA_RAGTOPK_REVERSE ? p.rows - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int klo = max(0, min(p.ks[row], p.keys)), khi = max(0, min(p.ke[row], p.keys));
    int* out = p.indices + (int64_t)row * p.indices_row;
    const int topk = p.topk;
    const TopkRow r = topk_row<kRagTopkWaves>(p.logits + (int64_t)row * p.logits_row + klo, max(0, khi - klo), wave, lane);
    // the entry of key j of a vector whose key 0 is row column c0 (a selected key has c0 + j in [lo, hi))
    const auto entry = [&](int64_t c0, int j) {
        if (!p.slots) return (int)(c0 + j);
        const int64_t s = p.slots[c0 + j];
        return (uint64_t)s <= 0x7fffffffull ? (int)s : -1;
    };

    // ---- at most topk candidates: everything selectable, in one sweep of workgroup-wide steps
    if (r.vis <= topk) {                                                   // (uniform, like all below)
        int run = 0, par = 0;
        for (int64_t b0 = 0; b0 < r.lr; b0 += 4 * kMlaTopkRaggedThreads, par ^= kRagTopkWaves) {
            const int64_t v0 = b0 + 4 * tid;
            unsigned k[4] = {0u, 0u, 0u, 0u};
            if (v0 < r.lr) topk_load(r, v0, k);
            const TopkRank q = topk_rank(k, 0u, 0);
            if (lane == 0) wcnt[par + wave] = (unsigned)q.tg;
            __syncthreads();
            int before = run;
#pragma unroll
            for (int w = 0; w < kRagTopkWaves; ++w) {
                const int c = (int)wcnt[par + w];
                if (w < wave) before += c;
                run += c;
            }
            topk_store(out, klo + v0 - r.a, q, before, 0, 0, topk, entry);
        }
        topk_tail<kMlaTopkRaggedThreads>(out, run, topk, tid);
        return;
    }

    // ---- the threshold
    for (int t = tid; t < kRagTopkBins; t += kMlaTopkRaggedThreads) hist[t] = 0u;
    if (tid == 0) ctl[4] = 0u;
    unsigned prefix = 0u, need = (unsigned)topk, state;
    int shift = 32 - kRagTopkB0, n_list = 0, above_w = 0;
    bool list = false;
    __syncthreads();
    ragtopk_pass<32 - kRagTopkB0, kRagTopkB0>(r, false, lkey, 0, hist, 0u, tid, lane);
    ragtopk_scan<kRagTopkB0>(hist, wtot, ctl, 0u, need, tid, lane, wave);
    state = ctl[2];
    if (state != 2u) { prefix = ctl[0]; need = ctl[1]; }
    if (state == 0u) {
        list = XFA_RAGTOPK_COMPACT && ctl[3] <= (unsigned)kMlaTopkRaggedStage && ctl[3] <= (unsigned)p.cap;
        if (list) {              // the threshold bin's keys into LDS; the keys of higher bins, counted
            n_list = (int)ctl[3];
            topk_sweep(r, false, lkey, [&](int64_t v0, const unsigned k[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned d = k[j] >> (32 - kRagTopkB0);
                    above_w += d > prefix;
                    const bool in = k[j] != 0u && d == prefix;
                    const uint64_t m = __ballot(in);
                    if (m != 0) {                                          // (uniform)
                        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
                        unsigned base = 0u;
                        if (lane == lead) base = atomicAdd(&ctl[4], (unsigned)__popcll(m));
                        const unsigned at = (unsigned)__builtin_amdgcn_readlane((int)base, lead) + (unsigned)topk_below(m);
                        if (in && at < (unsigned)p.cap) { lkey[at] = k[j]; lcol[at] = (unsigned)(v0 + j); }
                    }
                }
            });
            __syncthreads();
        }
        ragtopk_pass<kRagTopkB2, kRagTopkB1>(r, list, lkey, n_list, hist, prefix, tid, lane);
        ragtopk_scan<kRagTopkB1>(hist, wtot, ctl, prefix, need, tid, lane, wave);
        state = ctl[2]; prefix = ctl[0]; need = ctl[1]; shift = kRagTopkB2;
        if (state == 0u) {
            ragtopk_pass<0, kRagTopkB2>(r, list, lkey, n_list, hist, prefix, tid, lane);
            ragtopk_scan<kRagTopkB2>(hist, wtot, ctl, prefix, need, tid, lane, wave);
            state = ctl[2]; prefix = ctl[0]; need = ctl[1]; shift = 0;
        }
    }
    const TopkCut cut = topk_cut(state, prefix, need, shift);
    const unsigned T = cut.T;
    const int need_eq = cut.need_eq;

    // ---- per-wave counts of keys > T and keys == T, and the scan over waves
    if (list) {                  // the keys of higher bins, then the list's, each to its column's wave
        topk_wave_counts<kRagTopkWaves>(wcnt, above_w, 0, wave, lane);
        __syncthreads();
        for (int i = tid; i < n_list; i += kMlaTopkRaggedThreads) {
            const unsigned k = lkey[i];
            const int w = min((int)(lcol[i] / (unsigned)r.seg), kRagTopkWaves - 1);    // (seg < 2^30)
            if (k > T) atomicAdd(&wcnt[w], 1u);
            else if (k == T && need_eq > 0) atomicAdd(&wcnt[kRagTopkWaves + w], 1u);
        }
    } else {
        int cg = 0, ce = 0;
        topk_sweep(r, false, lkey, [&](int64_t, const unsigned k[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { cg += k[j] > T; ce += k[j] == T; }
        });
        topk_wave_counts<kRagTopkWaves>(wcnt, cg, ce, wave, lane);
    }
    __syncthreads();
    TopkRuns run = topk_wave_scan<kRagTopkWaves>(wcnt, wave, need_eq, topk);

    // ---- the ordered emit
    topk_sweep(r, false, lkey, [&](int64_t v0, const unsigned k[4]) {
        const TopkRank q = topk_rank(k, T, need_eq);
        topk_store(out, klo + v0 - r.a, q, run.gt_run, run.eq_run, need_eq, topk, entry);
        run.gt_run += q.tg; run.eq_run += q.te;
    });
    topk_tail<kMlaTopkRaggedThreads>(out, run.count, topk, tid);
}

}  // namespace xfa
