// fmha_mla_index_topk_kernel.h — the MLA indexer's selection (fmha_mla_index_topk), gfx950 (CDNA4):
// for every row of fmha_mla_index_logits' result the topk largest visible logits, as physical
// cache slots in ascending key position, -1 behind them (the contract is in
// include/paged_attn.h).  An exact radix select, not a sort; no atomics on global memory, no
// scratch, every output word has one writer, so the result is a function of the inputs alone.
//
//  * Work: one workgroup of 16 waves per row.  The row is walked in "virtual" columns v = column +
//    a, where a in [0, 3] is what the row's first logit lies behind a 16-byte boundary, so that
//    every lane's four columns are one aligned 16-byte load whatever the row stride is.  Wave w
//    owns the contiguous virtual columns [w seg, (w + 1) seg), seg a multiple of 256; in one step
//    lane l holds columns 256 step + 4 l .. + 3 of the segment.  Position order is therefore (wave,
//    step, lane, j): the ordered emit needs a count per wave, a scan over 16 counts and ballots.
//    A vector that straddles column 0 or `vis` is loaded element by element: nothing outside
//    [0, vis) is read.
//  * Key: the logit's bits made order-preserving (negative: all bits flipped, else the sign bit
//    set) after -0 became +0; NaN and -inf become key 0, which no finite value, subnormal or +inf
//    maps to and which is never counted nor selected.  Integer work only: nothing is flushed.
//  * Threshold T: most-significant-digit radix passes of 8 bits (4 at most).  A pass counts the
//    current digit of the keys that match the digits found so far into one of 8 LDS histograms
//    (one per wave pair); before the LDS add the lanes that share the digit of the first active
//    lane are counted by ballot and added once, twice over, since index logits sit in a few
//    exponents and 64 same-address adds serialise.  256 threads sum the 8 histograms (and clear
//    them), wave 0 scans the 256 bins from the top and finds the digit under which the count
//    crosses what is still needed.  A bin taken whole ends the passes early (everything >= the
//    prefix is selected, no ties to break); fewer selectable keys than topk ends them in pass 0.
//    8-bit digits and not 11 + 11 + 10: 8 private histograms are 8 KB, not 64 KB, beside a staged
//    row of 128 KB; the fourth pass reads LDS.
//  * The row between passes: a row of at most kMlaTopkStage visible keys is transformed once, in
//    pass 0, and kept in LDS as keys (128 KB); a longer row is read again from global memory (L2)
//    in every pass, four 16-byte loads in flight per lane.
//  * vis <= topk (every step of a short context) skips the passes: T = 0 selects what is selectable.
//  * Emit: one count sweep (keys > T and keys == T per wave), the scan over waves, then the
//    ordered sweep: a key > T goes to (# greater before it) + min(# equal before it, need_eq), a
//    key == T likewise while fewer than need_eq equals precede it - the lowest positions win the
//    ties.  The slot is block_table[column / page] * page + column % page in 64 bits, one division
//    per lane and step and one table read per page run; a table entry outside [0, num_blocks) or a
//    slot beyond int32 gives -1 in place.  Then -1 from the count to topk.
#pragma once

#include "fmha_common.h"
#include "fmha_launch.h"

namespace xfa {

constexpr int kTopkWaves = 16;
constexpr int kTopkThreads = kTopkWaves * 64;
constexpr int kTopkStep = 256;                      // virtual columns of one wave step (64 lanes x 4)
constexpr int kTopkHists = 8;                       // LDS histograms: one per wave pair
// LDS words: histograms, the summed bins, the per-wave counts (> T, == T), the scan's verdict
constexpr int kTopkHistW = 0, kTopkTotW = kTopkHists * 256, kTopkCntW = kTopkTotW + 256;
constexpr int kTopkCtlW = kTopkCntW + 2 * kTopkWaves, kTopkKeysW = kTopkCtlW + 32;
static_assert(kTopkKeysW % 4 == 0, "the staged keys are read 16 bytes at a time");
// ... then the staged keys: virtual columns, so up to 3 more than the visible keys, whole vectors
constexpr int topk_lds_bytes(int keys) { return 4 * (kTopkKeysW + (keys > 0 ? (keys + 3 + 3) / 4 * 4 : 0)); }
static_assert(topk_lds_bytes(kMlaTopkStage) <= 147456, "the staged row and the histograms fit the LDS");

__device__ __forceinline__ unsigned topk_key(unsigned u) {
    if (u == 0x80000000u) u = 0u;                                          // -0 is +0
    const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u & 0x7fffffffu) > 0x7f800000u || u == 0xff800000u) ? 0u : k;   // NaN, -inf: unselectable
}

struct TopkRow {
    const unsigned* al;        // the row's first logit, moved back to a 16-byte boundary
    int a;                     // ... by this many columns
    int vis;                   // visible columns
    int64_t lr;                // virtual columns, rounded up to whole vectors
    int64_t lo;                // this lane's first virtual column
    int steps;                 // this wave's steps
};

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

// Digit `shift` of the selectable keys that match `prefix` above it, into histogram h
__device__ __forceinline__ void topk_hist(unsigned* h, const unsigned k[4], unsigned prefix, int shift, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned d = (k[j] >> shift) & 255u;
        bool act = k[j] != 0u && (shift == 24 || (k[j] >> ((shift + 8) & 31)) == prefix);
#pragma unroll
        for (int peel = 0; peel < 2; ++peel) {
            const uint64_t m = __ballot(act);
            if (m == 0) break;                                             // (uniform)
            const int lead = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
            const bool same = act && d == (unsigned)__builtin_amdgcn_readlane((int)d, lead);
            const uint64_t sm = __ballot(same);
            if (lane == lead) atomicAdd(&h[d], (unsigned)__popcll(sm));
            act = act && !same;
        }
        if (act) atomicAdd(&h[d], 1u);
    }
}

#ifndef XFA_TOPK_HELPERS_ONLY        // (fmha_mla_index_topk_ragged_kernel.h takes the helpers above only)
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

    TopkRow r;
    const unsigned* src = reinterpret_cast<const unsigned*>(p.logits + (int64_t)row * p.logits_row);
    r.a = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    r.al = src - r.a;
    r.vis = max(0, min(n - p.seqlen_q + pos + 1, n));
    const int64_t cols = (int64_t)r.a + r.vis;
    r.lr = r.vis > 0 ? (cols + 3) & ~(int64_t)3 : 0;
    const int64_t seg = ((cols + kTopkWaves - 1) / kTopkWaves + kTopkStep - 1) & ~(int64_t)(kTopkStep - 1);
    const int64_t left = r.lr - wave * seg;
    r.steps = (int)max((int64_t)0, min((left + kTopkStep - 1) / kTopkStep, seg / kTopkStep));
    r.lo = wave * seg + lane * 4;

    // ---- the threshold: keys > T are selected, and the first need_eq keys == T
    unsigned T = 0u;
    int need_eq = 0;
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
                    topk_hist(h, k, 0u, 24, lane);
                });
            else
                topk_sweep(r, staged, skeys, [&](int64_t, const unsigned k[4]) { topk_hist(h, k, prefix, shift, lane); });
            __syncthreads();
            if (tid < 256) {
                unsigned s = 0u;
#pragma unroll
                for (int g = 0; g < kTopkHists; ++g) { s += hist[g * 256 + tid]; hist[g * 256 + tid] = 0u; }
                tot[tid] = s;
            }
            __syncthreads();
            if (wave == 0) {             // lane l: bins 4 l .. 4 l + 3; the count above each bin, from the top
                const u32x4 c = *reinterpret_cast<const u32x4*>(tot + 4 * lane);
                const unsigned mine = c[0] + c[1] + c[2] + c[3];
                unsigned sfx = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned t = (unsigned)__shfl_down((int)sfx, o);
                    if (lane + o < 64) sfx += t;
                }
                if (lane == 0 && sfx < need) ctl[2] = 2u;                  // fewer selectable keys than topk
                unsigned above = sfx - mine;
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    if (above < need && above + c[j] >= need) {            // (one lane, one j)
                        ctl[0] = (prefix << 8) | (unsigned)(4 * lane + j);
                        ctl[1] = need - above;
                        ctl[2] = c[j] == need - above ? 1u : 0u;           // the bin is taken whole
                    }
                    above += c[j];
                }
            }
            __syncthreads();
            if (ctl[2] != 2u) { prefix = ctl[0]; need = ctl[1]; }
            state = ctl[2];
        }
        if (state == 0u) { T = prefix; need_eq = (int)need; }              // all 32 bits found
        else if (state == 1u) T = max(1u, prefix << (shift + 8)) - 1u;     // everything >= the prefix
    }

    // ---- per-wave counts of keys > T and keys == T, and the scan over waves
    int cg = 0, ce = 0;
    topk_sweep(r, staged, skeys, [&](int64_t, const unsigned k[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { cg += k[j] > T; ce += k[j] == T; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cg += __shfl_xor(cg, o); ce += __shfl_xor(ce, o); }
    if (lane == 0) { wcnt[wave] = (unsigned)cg; wcnt[kTopkWaves + wave] = (unsigned)ce; }
    __syncthreads();
    int gt_run = 0, eq_run = 0, gt_all = 0, eq_all = 0;
#pragma unroll
    for (int w = 0; w < kTopkWaves; ++w) {
        const int g = (int)wcnt[w], e = (int)wcnt[kTopkWaves + w];
        if (w < wave) { gt_run += g; eq_run += e; }
        gt_all += g; eq_all += e;
    }
    const int count = min(topk, gt_all + min(eq_all, need_eq));

    // ---- the ordered emit
    topk_sweep(r, staged, skeys, [&](int64_t v0, const unsigned k[4]) {
        bool g[4], e[4];
        int gb = gt_run, eb = eq_run, tg = 0, te = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[j] = k[j] > T;
            e[j] = need_eq > 0 && k[j] == T;
            const uint64_t bg = __ballot(g[j]), be = __ballot(e[j]);
            gb += topk_below(bg); eb += topk_below(be);
            tg += __popcll(bg); te += __popcll(be);
        }
        gt_run += tg; eq_run += te;
        if (!(g[0] | g[1] | g[2] | g[3] | e[0] | e[1] | e[2] | e[3])) return;
        const int c0 = (int)(v0 - r.a);                   // (>= -3; a lane with a hit has c0 < vis)
        int pg = c0 >= 0 ? c0 / p.page : -1, off = c0 - pg * p.page, cur = -2, blk = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (off >= p.page) { off -= p.page; ++pg; }
            if (g[j] || (e[j] && eb < need_eq)) {
                if (pg != cur) { cur = pg; blk = table[pg]; }
                const int64_t slot = (int64_t)blk * p.page + off;
                const int at = gb + min(eb, need_eq);
                if (at < topk) out[at] = ((unsigned)blk < (unsigned)p.num_blocks && slot <= 0x7fffffffLL) ? (int)slot : -1;
            }
            gb += g[j]; eb += e[j]; ++off;
        }
    });
    for (int t = count + tid; t < topk; t += kTopkThreads) out[t] = -1;
}
#endif

}  // namespace xfa
