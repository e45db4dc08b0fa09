// fmha_mla_index_topk_ragged_kernel.h — the MLA indexer's selection for prefill rows
// (fmha_mla_index_topk_ragged), gfx950 (CDNA4): for every row of fmha_mla_index_logits_ragged's
// result the topk largest logits of its own column range [lo, hi), as cache slots (or columns) in
// ascending column order, -1 behind them (the contract is in
// include/paged_attn.h).  The same exact radix select as fmha_mla_index_topk_kernel - its key, its
// order, its ties, its output order; the helpers come from its header - with a work split for
// thousands of rows of every length instead of tens of long ones:
//
//  * Work: one workgroup of 4 waves per row, blockIdx 0 the LAST row (in a causal chunk the longest
//    rows start first).  At most 25 KB of LDS: a histogram of 2048 bins, a list of 2048 (key,
//    column) pairs and 64 control words, sized by the launch (no histogram and no list where no row
//    can be longer than topk) - four workgroups and more share a CU, and a barrier joins 4 waves.
//  * The row is walked as in the decode kernel: virtual columns v = (column - lo) + a, where a in
//    [0, 3] is what the row's first candidate (row base + lo) lies behind a 16-byte boundary; wave w
//    owns [w seg, (w + 1) seg), four 16-byte loads in flight per lane, element by element at the
//    two ragged ends: nothing outside [lo, hi) is read.  Position order is (wave, step, lane, j).
//  * hi - lo <= topk: no threshold.  One sweep in workgroup-wide steps of 1024 columns; per step a
//    ballot count per wave, one barrier (the counts are double-buffered), the ordered store.
//  * Threshold otherwise: three most-significant-digit passes of 11 + 11 + 10 bits.  Pass 0 (sign,
//    exponent, 2 mantissa bits: index logits sit in a few exponents, so 8 bits would leave the whole
//    row in one bin) counts from global memory.  If the bin the threshold falls in holds at most
//    kMlaTopkRaggedStage keys, a second sweep writes them to LDS as (key, virtual column) and counts,
//    per wave, the keys of higher bins; passes 1 and 2 and the per-wave counts of keys > T and == T
//    then run over that list alone, and global memory is read once more, by the emit: three reads
//    of the row in all.  A larger bin (equal values, values that share 11 bits) keeps to global
//    memory: passes 1 and 2 re-read the row (L2) under the prefix, then a count sweep, then the emit.
//    The list is filled through an LDS counter in no fixed order; it is only ever counted, so the
//    result does not depend on that order.  A bin taken whole ends the passes early, fewer
//    selectable keys than topk ends them in pass 0 (then T = 0 selects what is selectable).
//  * Emit: as in the decode kernel (ballots, the running counts of the wave, the scan over waves);
//    the entry is slots[column] when that lies in [0, 2^31), else -1 in place - or the column.
#pragma once

#define XFA_TOPK_HELPERS_ONLY
#include "fmha_mla_index_topk_kernel.h"

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

// Digit [SHIFT, SHIFT + BITS) of a selectable key that matches `prefix` above it, into h.  The
// lanes that share the first active lane's digit are counted by ballot and added once.
template <int SHIFT, int BITS>
__device__ __forceinline__ void ragtopk_hist(unsigned* h, unsigned k, unsigned prefix, int lane) {
    const unsigned d = (k >> SHIFT) & ((1u << BITS) - 1u);
    bool act = k != 0u;
    if constexpr (SHIFT + BITS < 32) act = act && (k >> ((SHIFT + BITS) & 31)) == prefix;
    const uint64_t m = __ballot(act);
    if (m != 0) {                                                          // (uniform)
        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
        const bool same = act && d == (unsigned)__builtin_amdgcn_readlane((int)d, lead);
        const uint64_t sm = __ballot(same);
        if (lane == lead) atomicAdd(&h[d], (unsigned)__popcll(sm));
        act = act && !same;
    }
    if (act) atomicAdd(&h[d], 1u);
}

// One pass' histogram, from the list (keys lkey[0, n)) or from global memory
template <int SHIFT, int BITS>
__device__ __forceinline__ void ragtopk_pass(const TopkRow& r, bool list, const unsigned* lkey, int n, unsigned* hist,
                                             unsigned prefix, int tid, int lane) {
    if (list) {
        for (int i0 = 0; i0 < n; i0 += kMlaTopkRaggedThreads)
            ragtopk_hist<SHIFT, BITS>(hist, i0 + tid < n ? lkey[i0 + tid] : 0u, prefix, lane);
    } else {
        topk_sweep(r, false, lkey, [&](int64_t, const unsigned k[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ragtopk_hist<SHIFT, BITS>(hist, k[j], prefix, lane);
        });
    }
}

// The verdict of a pass of 2^BITS bins: thread t owns bins PT t .. PT t + PT - 1 (and clears them),
// a suffix scan over lanes and waves gives the count above them.  ctl[0] the prefix with the digit
// under which the count crosses `need`, ctl[1] what is still needed of that bin, ctl[2] 1 where
// the bin is taken whole and 2 where all bins together hold fewer than `need`, ctl[3] the bin's count.
template <int BITS>
__device__ __forceinline__ void ragtopk_scan(unsigned* hist, unsigned* wtot, unsigned* ctl, unsigned prefix, unsigned need,
                                             int tid, int lane, int wave) {
    constexpr int PT = (1 << BITS) / kMlaTopkRaggedThreads;
    static_assert(PT >= 1 && PT * kMlaTopkRaggedThreads == (1 << BITS), "every thread owns whole bins");
    __syncthreads();
    unsigned c[PT], mine = 0u;
#pragma unroll
    for (int j = 0; j < PT; ++j) { c[j] = hist[PT * tid + j]; hist[PT * tid + j] = 0u; mine += c[j]; }
    unsigned sfx = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_down((int)sfx, o);
        if (lane + o < 64) sfx += t;
    }
    if (lane == 0) wtot[wave] = sfx;
    __syncthreads();
#pragma unroll
    for (int w = 1; w < kRagTopkWaves; ++w)
        if (w > wave) sfx += wtot[w];
    if (tid == 0 && sfx < need) ctl[2] = 2u;                               // fewer selectable keys than topk
    unsigned above = sfx - mine;
#pragma unroll
    for (int j = PT - 1; j >= 0; --j) {
        if (above < need && above + c[j] >= need) {                        // (one thread, one j)
            ctl[0] = (prefix << BITS) | (unsigned)(PT * tid + j);
            ctl[1] = need - above;
            ctl[2] = c[j] == need - above ? 1u : 0u;
            ctl[3] = c[j];
        }
        above += c[j];
    }
    __syncthreads();
}

// Where a lane's four keys go: bit j of gm / em: key j is > T / == T; gb, eb: such keys of the lower
// lanes of this step; tg, te: of the whole wave's step
struct RagTopkRank {
    unsigned gm, em;
    int gb, eb, tg, te;
};
__device__ __forceinline__ RagTopkRank ragtopk_rank(const unsigned k[4], unsigned T, int need_eq) {
    RagTopkRank q{0u, 0u, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool g = k[j] > T, e = need_eq > 0 && k[j] == T;
        const uint64_t bg = __ballot(g), be = __ballot(e);
        q.gm |= (unsigned)g << j; q.em |= (unsigned)e << j;
        q.gb += topk_below(bg); q.eb += topk_below(be);
        q.tg += __popcll(bg); q.te += __popcll(be);
    }
    return q;
}
// ... and their stores: c0 the column of key 0 (a lane with a hit has c0 + j in [lo, hi)); gbase,
// ebase the keys > T and == T before this wave's step
__device__ __forceinline__ void ragtopk_store(const int64_t* slots, int* out, int64_t c0, const RagTopkRank& q, int gbase,
                                              int ebase, int need_eq, int topk) {
    if (!(q.gm | q.em)) return;
    int gb = gbase + q.gb, eb = ebase + q.eb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = (q.gm >> j) & 1, e = (q.em >> j) & 1;
        if (g || (e && eb < need_eq)) {
            const int at = gb + min(eb, need_eq);
            int entry = (int)(c0 + j);
            if (slots) {
                const int64_t s = slots[c0 + j];
                entry = (uint64_t)s <= 0x7fffffffull ? (int)s : -1;
            }
            if ((unsigned)at < (unsigned)topk) out[at] = entry;
        }
        gb += g; eb += e;
    }
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

    TopkRow r;
    const unsigned* src = reinterpret_cast<const unsigned*>(p.logits + (int64_t)row * p.logits_row + klo);
    r.a = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    r.al = src - r.a;
    r.vis = max(0, khi - klo);
    const int64_t cols = (int64_t)r.a + r.vis;
    r.lr = r.vis > 0 ? (cols + 3) & ~(int64_t)3 : 0;
    const int64_t seg = ((cols + kRagTopkWaves - 1) / kRagTopkWaves + kTopkStep - 1) & ~(int64_t)(kTopkStep - 1);
    const int64_t left = r.lr - wave * seg;
    r.steps = (int)max((int64_t)0, min((left + kTopkStep - 1) / kTopkStep, seg / kTopkStep));
    r.lo = wave * seg + lane * 4;

    // ---- at most topk candidates: everything selectable, in one sweep of workgroup-wide steps
    if (r.vis <= topk) {                                                   // (uniform, like all below)
        int run = 0, par = 0;
        for (int64_t b0 = 0; b0 < r.lr; b0 += 4 * kMlaTopkRaggedThreads, par ^= kRagTopkWaves) {
            const int64_t v0 = b0 + 4 * tid;
            unsigned k[4] = {0u, 0u, 0u, 0u};
            if (v0 < r.lr) topk_load(r, v0, k);
            const RagTopkRank q = ragtopk_rank(k, 0u, 0);
            if (lane == 0) wcnt[par + wave] = (unsigned)q.tg;
            __syncthreads();
            int before = run;
#pragma unroll
            for (int w = 0; w < kRagTopkWaves; ++w) {
                const int c = (int)wcnt[par + w];
                if (w < wave) before += c;
                run += c;
            }
            ragtopk_store(p.slots, out, klo + v0 - r.a, q, before, 0, 0, topk);
        }
        for (int t = run + tid; t < topk; t += kMlaTopkRaggedThreads) out[t] = -1;
        return;
    }

    // ---- the threshold: keys > T are selected, and the first need_eq keys == T
    for (int t = tid; t < kRagTopkBins; t += kMlaTopkRaggedThreads) hist[t] = 0u;
    if (tid == 0) ctl[4] = 0u;
    unsigned prefix = 0u, need = (unsigned)topk, state, T = 0u;
    int need_eq = 0, shift = 32 - kRagTopkB0, n_list = 0, above_w = 0;
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
    if (state == 0u) { T = prefix; need_eq = (int)need; }                  // all 32 bits found
    else if (state == 1u) T = max(1u, prefix << shift) - 1u;               // everything >= the prefix

    // ---- per-wave counts of keys > T and keys == T, and the scan over waves
    if (list) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) above_w += __shfl_xor(above_w, o);
        if (lane == 0) { wcnt[wave] = (unsigned)above_w; wcnt[kRagTopkWaves + wave] = 0u; }
        __syncthreads();
        for (int i = tid; i < n_list; i += kMlaTopkRaggedThreads) {
            const unsigned k = lkey[i];
            const int w = min((int)(lcol[i] / (unsigned)seg), kRagTopkWaves - 1);      // (seg < 2^30)
            if (k > T) atomicAdd(&wcnt[w], 1u);
            else if (k == T && need_eq > 0) atomicAdd(&wcnt[kRagTopkWaves + w], 1u);
        }
    } else {
        int cg = 0, ce = 0;
        topk_sweep(r, false, lkey, [&](int64_t, const unsigned k[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { cg += k[j] > T; ce += k[j] == T; }
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cg += __shfl_xor(cg, o); ce += __shfl_xor(ce, o); }
        if (lane == 0) { wcnt[wave] = (unsigned)cg; wcnt[kRagTopkWaves + wave] = (unsigned)ce; }
    }
    __syncthreads();
    int gt_run = 0, eq_run = 0, gt_all = 0, eq_all = 0;
#pragma unroll
    for (int w = 0; w < kRagTopkWaves; ++w) {
        const int g = (int)wcnt[w], e = (int)wcnt[kRagTopkWaves + w];
        if (w < wave) { gt_run += g; eq_run += e; }
        gt_all += g; eq_all += e;
    }
    const int count = min(topk, gt_all + min(eq_all, need_eq));

    // ---- the ordered emit
    topk_sweep(r, false, lkey, [&](int64_t v0, const unsigned k[4]) {
        const RagTopkRank q = ragtopk_rank(k, T, need_eq);
        ragtopk_store(p.slots, out, klo + v0 - r.a, q, gt_run, eq_run, need_eq, topk);
        gt_run += q.tg; eq_run += q.te;
    });
    for (int t = count + tid; t < topk; t += kMlaTopkRaggedThreads) out[t] = -1;
}

}  // namespace xfa
