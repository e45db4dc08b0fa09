// fmha_mla_index_select.h — the exact radix select under the selection kernels of the MLA indexer
// (fmha_mla_index_topk_kernel.h, fmha_mla_index_topk_ragged_kernel.h and the two kernels of
// fmha_mla_index_topk_split_kernel.h), gfx950 (CDNA4); DESIGN.md §3.13.1.  The kernels differ in
// what they walk, how they split it over waves and workgroups, and in their pass structure;
// what a row's result is, is stated here once, and every piece of it has one text:
//
//  * Key: the logit's bits made order-preserving (negative: all bits flipped, else the sign bit
//    set) after -0 became +0; NaN and -inf become key 0, which no finite value, subnormal or +inf
//    maps to and which is never counted nor selected.  Integer work only: nothing is flushed.
//  * Order: a row is walked in "virtual" columns v = (column - first candidate) + a, where a in
//    [0, 3] is what the first candidate lies behind a 16-byte boundary, so that every lane's four
//    columns are one aligned 16-byte load whatever the row's offset is.  Wave w owns the contiguous
//    virtual columns [w seg, (w + 1) seg), seg a multiple of 256; in one step lane l holds columns
//    256 step + 4 l .. + 3 of the segment.  Position order is therefore (wave, step, lane, j).
//  * Never read: anything outside the row's candidates.  A vector that straddles either end is
//    loaded element by element.
//  * Threshold: most-significant-digit radix passes.  A pass counts one digit of the selectable keys
//    that match the digits found so far; its verdict is the digit under which the count from the
//    top crosses what is still needed.  A bin taken whole ends the passes (everything >= the prefix
//    is selected, no ties to break); fewer selectable keys than topk ends them in the first pass
//    (T = 0 then selects what is selectable).  Digit widths and where the counts live are the
//    kernel's.
//  * Ties: keys > T are selected, and of the keys == T the first need_eq in position order.
//  * Output: a selected key goes to (# greater before it) + min(# equal before it, need_eq), so the
//    entries stand in ascending position; -1 from the count to topk.  Every output word has one
//    writer (every scratch word of the split kernels too) and there are no atomics on global
//    memory: the result is a function of the inputs alone.
#pragma once

#include "fmha_common.h"

namespace xfa {

constexpr int kTopkStep = 256;                      // virtual columns of one wave step (64 lanes x 4)

__device__ __forceinline__ unsigned topk_key(unsigned u) {
    if (u == 0x80000000u) u = 0u;                                          // -0 is +0
    const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u & 0x7fffffffu) > 0x7f800000u || u == 0xff800000u) ? 0u : k;   // NaN, -inf: unselectable
}

struct TopkRow {
    const unsigned* al;        // the row's first candidate, moved back to a 16-byte boundary
    int a;                     // ... by this many columns
    int vis;                   // candidates
    int64_t lr;                // virtual columns, rounded up to whole vectors
    int64_t seg;               // virtual columns of one wave's segment
    int64_t lo;                // this lane's first virtual column
    int steps;                 // this wave's steps
};

// The walk of a row of `vis` (>= 0) candidates from `first` by WAVES waves, for this wave and lane
template <int WAVES>
__device__ __forceinline__ TopkRow topk_row(const float* first, int vis, int wave, int lane) {
    TopkRow r;
    const unsigned* src = reinterpret_cast<const unsigned*>(first);
    r.a = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    r.al = src - r.a;
    r.vis = vis;
    const int64_t cols = (int64_t)r.a + r.vis;
    r.lr = r.vis > 0 ? (cols + 3) & ~(int64_t)3 : 0;
    r.seg = ((cols + WAVES - 1) / WAVES + kTopkStep - 1) & ~(int64_t)(kTopkStep - 1);
    const int64_t left = r.lr - wave * r.seg;
    r.steps = (int)max((int64_t)0, min((left + kTopkStep - 1) / kTopkStep, r.seg / kTopkStep));
    r.lo = wave * r.seg + lane * 4;
    return r;
}

// The keys of virtual columns v0 .. v0 + 3 from global memory; columns outside [0, vis) are key 0
__device__ __forceinline__ void topk_load(const TopkRow& r, int64_t v0, unsigned k[4]) {
    const int64_t c0 = v0 - r.a;
    if (c0 >= 0 && c0 + 4 <= r.vis) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(r.al + v0);
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = topk_key(x[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (c0 + j >= 0 && c0 + j < r.vis) ? topk_key(r.al[v0 + j]) : 0u;
    }
}

// f(v0, keys) for every step of the wave, in order; four steps' loads are issued before the first
// is used.  staged: the keys come from LDS (skeys, by virtual column).
template <typename F>
__device__ __forceinline__ void topk_sweep(const TopkRow& r, bool staged, const unsigned* skeys, F&& f) {
    for (int s0 = 0; s0 < r.steps; s0 += 4) {
        unsigned k[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t v0 = r.lo + (int64_t)(s0 + u) * kTopkStep;
            if (s0 + u < r.steps && v0 < r.lr) {
                if (staged) {
                    const u32x4 x = *reinterpret_cast<const u32x4*>(skeys + v0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) k[u][j] = x[j];
                } else {
                    topk_load(r, v0, k[u]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) k[u][j] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s0 + u < r.steps) f(r.lo + (int64_t)(s0 + u) * kTopkStep, k[u]);       // (uniform)
    }
}

// Lanes below this one whose bit is set
__device__ __forceinline__ int topk_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Digit [shift, shift + bits) of a selectable key that matches `prefix` above it, into histogram h.
// Index logits sit in a few exponents and 64 same-address LDS adds serialise: PEELS times over, the
// lanes that share the digit of the first active lane are counted by ballot and added once.
template <int PEELS>
__device__ __forceinline__ void topk_hist(unsigned* h, unsigned k, unsigned prefix, int shift, int bits, int lane) {
    const unsigned d = (k >> shift) & ((1u << bits) - 1u);
    bool act = k != 0u && (shift + bits == 32 || (k >> ((shift + bits) & 31)) == prefix);
#pragma unroll
    for (int peel = 0; peel < PEELS; ++peel) {
        const uint64_t m = __ballot(act);
        if (m == 0) break;                                                 // (uniform)
        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
        const bool same = act && d == (unsigned)__builtin_amdgcn_readlane((int)d, lead);
        const uint64_t sm = __ballot(same);
        if (lane == lead) atomicAdd(&h[d], (unsigned)__popcll(sm));
        act = act && !same;
    }
    if (act) atomicAdd(&h[d], 1u);
}

// x of this lane and of all higher lanes of the wave
__device__ __forceinline__ unsigned topk_suffix(unsigned x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_down((int)x, o);
        if (lane + o < 64) x += t;
    }
    return x;
}

// The verdict of a pass of 2^bits bins, by the thread that owns the bins first .. first + PT - 1 with
// counts c and `above` keys in the bins over them (no barrier in here).  ctl[0] the prefix with the
// digit under which the count crosses `need`, ctl[1] what is still needed of that bin, ctl[2] 1 where
// the bin is taken whole and 2 where all bins together hold fewer than `need`, ctl[3] the bin's count.
template <int PT>
__device__ __forceinline__ void topk_verdict(unsigned* ctl, const unsigned (&c)[PT], unsigned above, int first,
                                             unsigned prefix, int bits, unsigned need) {
    unsigned all = above;
#pragma unroll
    for (int j = 0; j < PT; ++j) all += c[j];
    if (first == 0 && all < need) ctl[2] = 2u;                             // fewer selectable keys than topk
#pragma unroll
    for (int j = PT - 1; j >= 0; --j) {
        if (above < need && above + c[j] >= need) {                        // (one thread, one j)
            ctl[0] = (prefix << bits) | (unsigned)(first + j);
            ctl[1] = need - above;
            ctl[2] = c[j] == need - above ? 1u : 0u;
            ctl[3] = c[j];
        }
        above += c[j];
    }
}

// What the passes found, as the threshold: keys > T are selected, and the first need_eq keys == T.
// state: the last verdict's ctl[2]; shift: the bits below `prefix`.
struct TopkCut {
    unsigned T;
    int need_eq;
};
__device__ __forceinline__ TopkCut topk_cut(unsigned state, unsigned prefix, unsigned need, int shift) {
    if (state == 0u) return {prefix, (int)need};                           // all 32 bits found
    if (state == 1u) return {max(1u, prefix << shift) - 1u, 0};            // everything >= the prefix
    return {0u, 0};                                                        // everything selectable
}

// A wave's keys > T (cg) and == T (ce), summed over its lanes (each lane's own counts go in), into
// wcnt[wave] and wcnt[WAVES + wave] ...
template <int WAVES>
__device__ __forceinline__ void topk_wave_counts(unsigned* wcnt, int cg, int ce, int wave, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cg += __shfl_xor(cg, o); ce += __shfl_xor(ce, o); }
    if (lane == 0) { wcnt[wave] = (unsigned)cg; wcnt[WAVES + wave] = (unsigned)ce; }
}
// ... and, a barrier later, the scan over waves: the keys > T and == T before this wave, and how
// many entries the row gets
struct TopkRuns {
    int gt_run, eq_run, count;
};
template <int WAVES>
__device__ __forceinline__ TopkRuns topk_wave_scan(const unsigned* wcnt, int wave, int need_eq, int topk) {
    int gt_run = 0, eq_run = 0, gt_all = 0, eq_all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int g = (int)wcnt[w], e = (int)wcnt[WAVES + w];
        if (w < wave) { gt_run += g; eq_run += e; }
        gt_all += g; eq_all += e;
    }
    return {gt_run, eq_run, min(topk, gt_all + min(eq_all, need_eq))};
}

// Where a lane's four keys go: g[j] / e[j]: key j is > T / == T; gb, eb: such keys of the lower
// lanes of this step; tg, te: of the whole wave's step.  (The flags are bools, lane masks in SGPRs:
// packed into bit masks they cost the 16-wave kernel VGPRs and a wave of occupancy.)
struct TopkRank {
    bool g[4], e[4];
    int gb, eb, tg, te;
    __device__ __forceinline__ bool hit() const { return g[0] | g[1] | g[2] | g[3] | e[0] | e[1] | e[2] | e[3]; }
};
__device__ __forceinline__ TopkRank topk_rank(const unsigned k[4], unsigned T, int need_eq) {
    TopkRank q{{}, {}, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q.g[j] = k[j] > T;
        q.e[j] = need_eq > 0 && k[j] == T;
        const uint64_t bg = __ballot(q.g[j]), be = __ballot(q.e[j]);
        q.gb += topk_below(bg); q.eb += topk_below(be);
        q.tg += __popcll(bg); q.te += __popcll(be);
    }
    return q;
}
// ... and their stores: gbase, ebase the keys > T and == T before this wave's step; entry(c0, j)
// what is written for key j, c0 the column of key 0 (called for selected keys only, j ascending)
template <typename E>
__device__ __forceinline__ void topk_store(int* out, int64_t c0, const TopkRank& q, int gbase, int ebase, int need_eq,
                                           int topk, E&& entry) {
    if (!q.hit()) return;
    int gb = gbase + q.gb, eb = ebase + q.eb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (q.g[j] || (q.e[j] && eb < need_eq)) {
            const int at = gb + min(eb, need_eq);
            const int x = entry(c0, j);
            if ((unsigned)at < (unsigned)topk) out[at] = x;
        }
        gb += q.g[j]; eb += q.e[j];
    }
}

// -1 from the count to topk
template <int THREADS>
__device__ __forceinline__ void topk_tail(int* out, int count, int topk, int tid) {
    for (int t = count + tid; t < topk; t += THREADS) out[t] = -1;
}

}  // namespace xfa
