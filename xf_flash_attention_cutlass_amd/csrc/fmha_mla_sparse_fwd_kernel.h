// fmha_mla_sparse_fwd_kernel.h — sparse MLA attention over M new tokens (fmha_mla_sparse_fwd;
// DeepSeek-V3.2's prefill, FlashMLA's flash_mla_sparse_fwd), gfx950 (CDNA4).
//
// For query (pos, head), K is the rows of kv [s_kv, 1, 576] at the valid entries of
// indices[pos, 0 .. topk), in that order, duplicates as often as they occur; an entry is valid iff
// 0 <= entry < s_kv.  S = scale q K^T, O = softmax(S) K[:, :512], LSE = logsumexp(S),
// max_logits = max(S).  The products, the softmax and the image layout are
// fmha_mla_decode_sparse_kernel's (fmha_mla_decode_sparse_kernel.h), tile for tile in ascending
// order, so O and LSE equal that kernel's at num_splits = 1 bit for bit.  What differs is who
// gathers:
//
//  * A WORKGROUP is one query position and four consecutive 16-head tiles; wave w owns head tile
//    4 group + w.  Grid = s_q * ceil(ceil(heads / 16) / 4), the groups of a position neighbours in
//    launch order.  No key split, no scratch, no combine.
//  * ONE image of a 32-key tile serves the four waves (§3.10's layout: 1152-byte pitch, mla_off).
//    Wave w gathers rows 8 w .. 8 w + 7 of it: 9 global_load_dwordx4 (36 registers), chunk
//    f = 64 j + lane of that 8-row group, row f / 72 - the decode kernel's map, the two slots of an
//    instruction read out of the slot register with v_readlane_b32.  A selected row is pulled
//    through L2 and written to LDS once per 64 heads, not once per 16.
//  * TWO images (73,728 B), one barrier per tile.  While the four waves compute tile t out of
//    image t & 1, the loads of tile t + 1 fly; after its products a wave writes its 8 rows into
//    image (t + 1) & 1, refills its ring with tile t + 2 and meets the others at the barrier: every
//    wave has then finished reading image t & 1 (free for tile t + 2) and image (t + 1) & 1 is
//    complete.  The barrier waits for the LDS counter only, so the ring's loads stay in flight
//    across it.
//  * Every wave fetches the tile's 32 entries itself (one coalesced load, one tile further ahead
//    than the rows it feeds): it needs the slots of its own 8 rows and the whole invalid mask for
//    the -inf scores.  An invalid lane takes row 0 (the host requires s_kv >= 1), so no load leaves
//    [kv, kv + s_kv * row stride) whatever the indices hold; such a row goes into the image as
//    zeros and scores -inf, both behind the wave-uniform "mask not zero".
//  * A wave whose head tile does not exist (heads 16, 40, ...) loads no Q, does no products and
//    stores nothing; it gathers its rows and meets every barrier.  Lanes past `heads` of a partial
//    tile compute the last head again and store nothing.
#pragma once

#include "fmha_mla_decode_sparse_kernel.h"

namespace xfa {

constexpr int kMlaFwdImages = 2;
constexpr int kMlaFwdSmem = kMlaFwdImages * kMlaImage;

// the workgroup barrier of the tile loop: LDS traffic retired, vector loads left in flight
__device__ __forceinline__ void mla_fwd_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_sparse_fwd_kernel(const MlaSparseFwdParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NLW = 9;              // load instructions of a wave's 8 rows
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;           // query row (MFMA column) of this lane
    const int hh = lane >> 4;           // key sub-block of this lane
    // workgroup -> (position, group of four head tiles); wave -> head tile
    const int H = p.h;
    const int htiles = (H + 15) >> 4;
    const int pos = blockIdx.x / p.groups;
    const int group = blockIdx.x - pos * p.groups;
    const int htile = 4 * group + wave;
    const bool live = htile < htiles;   // wave-uniform
    const bool row_ok = htile * 16 + lr < H;
    const int head = min(htile * 16 + lr, H - 1);
    const float c = p.scale_log2;
    const int topk = p.topk;
    const uint32_t nrows = (uint32_t)min(p.s_kv, (int64_t)0x80000000LL);
    const int t_end = (topk + kMlaKeys - 1) / kMlaKeys;

    // The entries of index tile t: lane l gets entry 32 t + l % 32, the load clamped to the row.
    // mla_sparse_fetch without its select: what the load brought is first touched in slots_of, a
    // tile later, so the fetch does not make the ring's loads, issued just before it, drain.
    const int* ind = p.indices + (int64_t)pos * p.ind_row;
    auto fetch = [&](const int t) __attribute__((always_inline)) {
        return ind[min(t * kMlaKeys + (lane & 31), topk - 1)];
    };
    int idx_n = fetch(0);

    // ---- Q fragments (B operand of S^T): lane holds Q[row][32 s + 8 hh .. +7]
    V8 qf[NS];
    if (live) {
        const T* qrow = reinterpret_cast<const T*>(p.q) + (int64_t)pos * p.q_row + (int64_t)head * p.q_head + 8 * hh;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            qf[s] = *reinterpret_cast<const V8*>(qrow + 32 * s);
    } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = V8{};
    }

    // ---- this wave's rows of a tile: 8 wave .. + 7.  Instruction j loads chunk f = 64 j + lane of
    // the group: row f / 72, one of two rows known at compile time.
    const char* pool = reinterpret_cast<const char*>(p.kv);
    const int64_t pitch = p.kv_row * (int64_t)sizeof(T);
    const int row0 = 8 * wave;
    // entries of tile t -> (rows, invalid mask): a place at or past topk is invalid, an invalid lane
    // takes row 0
    auto slots_of = [&](const int idx, const int t, uint32_t& inv) __attribute__((always_inline)) {
        const bool ok = (uint32_t)idx < nrows && t * kMlaKeys + (lane & 31) < topk;
        inv = (uint32_t)__builtin_amdgcn_ballot_w64(!ok);
        return ok ? idx : 0;
    };
    u32x4 raw[NLW];
    auto issue = [&](const int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NLW; ++j) {
            constexpr int kRowB = kMlaCPR;
            const int ra = (64 * j) / kRowB, rb = (64 * j + 63) / kRowB;      // rows of lanes 0 and 63
            const int sa = __builtin_amdgcn_readlane(slot, row0 + ra);
            const int sb = __builtin_amdgcn_readlane(slot, row0 + rb);
            const int thr = kRowB * rb - 64 * j;                              // first lane of row rb
            const int mine = (ra != rb && lane >= thr) ? sb : sa;
            const int chunk = 64 * j + lane - kRowB * ((ra != rb && lane >= thr) ? rb : ra);
            const u32x4* src = reinterpret_cast<const u32x4*>(pool + (int64_t)mine * pitch + 16 * chunk);
            raw[j] = mla_sparse_load(src);
        }
    };
    // the ring goes into image `dst` (rows of invalid entries as zeros: they hold row 0's bytes,
    // whatever they are, and enter O^T += V^T P^T as 0 * V, which a NaN or Inf survives)
    int woff[NLW];
#pragma unroll
    for (int j = 0; j < NLW; ++j) {
        const int f = 64 * j + lane;
        woff[j] = mla_off(f / kMlaCPR, f % kMlaCPR) + row0 * kMlaPitch;
    }
    auto stash = [&](char* dst, const uint32_t inv) __attribute__((always_inline)) {
        if (inv) {
#pragma unroll
            for (int j = 0; j < NLW; ++j) {
                const int row = row0 + (64 * j + lane) / kMlaCPR;
                const u32x4 v = ((inv >> row) & 1u) ? u32x4{0u, 0u, 0u, 0u} : raw[j];
                *reinterpret_cast<u32x4*>(dst + woff[j]) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NLW; ++j) *reinterpret_cast<u32x4*>(dst + woff[j]) = raw[j];
        }
    };

    // K operand of k-step s and V^T operand of d tile dt: as fmha_mla_decode_kernel
    const int kb2 = (lr >> 2) & 1;
    const int kbase = lr * kMlaPitch + 16 * (hh ^ (lr & 2));
    const int koff_e = kbase + 64 * kb2, koff_o = kbase - 64 * kb2;
    const int q4 = (lane & 15) >> 2;
    const int vrow = 4 * hh + q4;
    int voff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        voff[u] = vrow * kMlaPitch + 32 * (u ^ ((vrow >> 1) & 3)) + 16 * ((lane >> 1) & 1) + 8 * (lane & 1);

    f32x4 acc_o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc_o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // ---- prologue: tile 0 into image 0, tile 1 into the ring.  inv_c: the invalid mask of the
    // tile about to be computed, inv_n: of the tile in the ring, idx_n: entries of the tile after it
    uint32_t inv_c = 0, inv_n = 0;
    {
        const int slot = slots_of(idx_n, 0, inv_c);
        issue(slot);
        idx_n = fetch(min(1, t_end - 1));
    }
    stash(smem, __builtin_amdgcn_readfirstlane(inv_c));
    if (t_end > 1) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        const int slot = slots_of(idx_n, 1, inv_n);
        issue(slot);
        idx_n = fetch(min(2, t_end - 1));
        __builtin_amdgcn_sched_barrier(0);
    }
    mla_fwd_barrier();

    // the products of one tile out of `img`: fmha_mla_decode_sparse_kernel's, statement for statement
    auto products = [&](const char* img, const uint32_t inv) __attribute__((always_inline)) {
        // S^T = K Q^T: two 16-key blocks, the row reads in groups of 6 k-steps
        f32x4 st[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            st[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s0 = 0; s0 < NS; s0 += 6) {
                V8 kf[6];
#pragma unroll
                for (int s = s0; s < s0 + 6; ++s)
                    kf[s - s0] = *reinterpret_cast<const V8*>(img + ((s & 1) ? koff_o : koff_e) + 64 * s + h * 16 * kMlaPitch);
#pragma unroll
                for (int s = s0; s < s0 + 6; ++s) st[h] = dec_mfma16<T>(kf[s - s0], qf[s], st[h]);
            }
        }
        // element (kb, i) is entry 16 kb + 4 hh + i of the tile
        if (inv) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((inv >> (16 * kb + 4 * hh + i)) & 1u) st[kb][i] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, st[kb][i]);
        mx = quad_max16(mx);
        const float m_new = fmaxf(m_run, mx);
        const float mref = (m_new == -INFINITY) ? 0.f : m_new * c;
        if (__any(m_new > m_run)) {
            const float alpha = fast_exp2(m_run * c - mref);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc_o[dt][i] *= alpha;
            m_run = m_new;
        }
        V8 pb;
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = fast_exp2(fmaf(st[kb][i], c, -mref));
                rs += e;
                pb[4 * kb + i] = (T)e;
            }
        l_run += rs;
        // O^T += V^T P^T over the first 512 columns of the same image, 4 d tiles a group
#pragma unroll
        for (int d0 = 0; d0 < ND; d0 += 4) {
            s16x4 t0[4], t1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const char* a = img + voff[u] + 128 * (d0 >> 2);
                t0[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
                t1[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 16 * kMlaPitch));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const s16x8 av = {t0[u][0], t0[u][1], t0[u][2], t0[u][3], t1[u][0], t1[u][1], t1[u][2], t1[u][3]};
                acc_o[d0 + u] = dec_mfma16<T>(__builtin_bit_cast(V8, av), pb, acc_o[d0 + u]);
            }
        }
    };

    // ---- the tiles, ascending
    for (int t = 0; t < t_end; ++t) {
        char* img = smem + (t & 1) * kMlaImage;
        if (live) products(img, __builtin_amdgcn_readfirstlane(inv_c));
        if (t + 1 < t_end) {
            // tile t + 1: ring -> the other image (nobody reads it: every wave passed the last
            // barrier after its products of tile t - 1), then the ring takes tile t + 2
            stash(smem + ((t + 1) & 1) * kMlaImage, __builtin_amdgcn_readfirstlane(inv_n));
            inv_c = inv_n;
            if (t + 2 < t_end) {
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                const int slot = slots_of(idx_n, t + 2, inv_n);
                issue(slot);
                idx_n = fetch(min(t + 3, t_end - 1));
                __builtin_amdgcn_sched_barrier(0);
            }
            mla_fwd_barrier();
        }
    }

    // ---- epilogue: normalised O, LSE and the largest scaled score; a row without a valid entry
    // gives O = 0, LSE = +inf, max_logits = -inf
    if (!live) return;
    const float l_full = quad_sum16(l_run);
    const bool empty = (l_full == 0.f) || (l_full != l_full);
    const float inv = empty ? 0.f : 1.f / l_full;
    if (!row_ok) return;
    // (the fma spelt out: the decode kernel's m_run * c + log2 l contracts to one, and here the
    // product m_run * c, which max_logits shares, would otherwise be rounded on its own)
    const float lsev = empty ? -INFINITY : fmaf(m_run, c, __log2f(l_full)) * kLn2;
    typedef __attribute__((ext_vector_type(4))) T T4;
    T* orow = reinterpret_cast<T*>(p.o) + (int64_t)pos * p.o_row + (int64_t)head * p.o_head;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
        *reinterpret_cast<T4*>(orow + 16 * dt + 4 * hh) =
            T4{(T)(acc_o[dt][0] * inv), (T)(acc_o[dt][1] * inv), (T)(acc_o[dt][2] * inv), (T)(acc_o[dt][3] * inv)};
    if (hh == 0) {
        const int64_t rid = (int64_t)pos * H + head;
        if (p.lse) p.lse[rid] = empty ? INFINITY : lsev;
        if (p.max_logits) p.max_logits[rid] = empty ? -INFINITY : m_run * c * kLn2;
    }
}

}  // namespace xfa
