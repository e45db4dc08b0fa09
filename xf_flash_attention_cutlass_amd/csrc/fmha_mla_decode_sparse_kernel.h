// fmha_mla_decode_sparse_kernel.h — fmha_mla_decode_kernel (fmha_mla_decode_kernel.h) over
// index-selected tokens (fmha_mla_decode_sparse; DeepSeek-V3.2's sparse attention, FlashMLA's
// `indices`), gfx950 (CDNA4).
//
// For query (batch, pos, head), K is the cache rows at the valid entries of
// indices[batch, pos, 0 .. topk), in that order, duplicates as often as they occur; an entry is a
// physical slot, block * page_size + row, and is valid iff 0 <= entry < num_slots.  No block
// table, no cache_seqlens, no mask.  Everything after the image is the dense kernel: the mapping
// of a wave to an item with a private image and no barrier, the 32-key tile, mla_off, the image
// write offsets, both product loops, the softmax, the epilogue and the combine.  A kernel of its
// own, so that the dense kernel's instructions stay what they were.  What differs:
//
//  * Row tiles.  Every position has its own indices, so a 16-row tile is 16 heads of ONE
//    position: row_tiles = seqlen_q * ceil(heads / 16), row tile = pos * htiles + htile; lanes
//    past `heads` compute the last head again and store nothing.  A split is an equal range of
//    the ceil(topk / 32) index tiles.
//  * The slots of a tile.  A tile's 32 entries are consecutive int32: ONE coalesced load, lane l
//    entry l % 32, issued one tile ahead (after the previous tile's row loads, so it has landed
//    when those rows are in the image).  Positions at or past topk count as invalid (the load is
//    clamped to the row's last entry).  One unsigned compare validates (a negative entry is
//    >= 2^31 >= num_slots), one ballot gives the tile's 32-bit invalid mask in an SGPR pair, and
//    an invalid lane takes slot 0 (the host requires num_blocks >= 1): an invalid entry is never
//    turned into an address, and no load leaves the cache whatever the indices hold.
//  * The gather.  Per load instruction the lane-to-row map is the dense kernel's: chunk f =
//    64 j + lane of an 8-row group, row f / 72 - two rows per instruction, known at compile
//    time.  The two slots come out of the slot register with v_readlane_b32, the lane picks its
//    own under a compile-time lane mask, and the address is kv + slot * 1152 + 16 (f % 72) in 64
//    bits (global_load_dwordx4; caches past 4 GiB work), WITHOUT the dense kernels' non-temporal
//    hint (XFA_MLA_SPARSE_NT: measured slower here).
//  * Invalid entries can sit anywhere in a tile.  Such a row goes into the image as zeros (the
//    load brought slot 0, whatever it holds, and 0 * NaN must not reach O^T += V^T P^T) and its
//    score is -inf, both behind the wave-uniform "this tile's invalid mask is not zero": a fully
//    valid tile pays nothing.  A tile without a valid entry leaves m_run and l_run as they were
//    (every e is exp2(-inf) = 0 and the image is zeros); a split without one writes O = 0,
//    LSE = -inf.
#pragma once

#include "fmha_mla_decode_kernel.h"

// the cache-row loads' policy: 0 plain loads, 1 the non-temporal hint (the dense kernels' choice).
// Measured (tools/mla_ab.py --sparse --ab-lib, profiles/mla_decode_sparse_nt_ab.log): plain loads
// are faster in every cell, by up to a third where 8 head tiles share their rows through L2.
#ifndef XFA_MLA_SPARSE_NT
#define XFA_MLA_SPARSE_NT 0
#endif

namespace xfa {

template <typename V>
__device__ __forceinline__ V mla_sparse_load(const V* src) {
    if constexpr (XFA_MLA_SPARSE_NT) return __builtin_nontemporal_load(src);
    else return *src;
}

// The slots of index tile t of one (batch, pos): lane l gets entry 32 t + l % 32 (the load
// clamped to the row), an entry at or past topk becomes -1
__device__ __forceinline__ int mla_sparse_fetch(const int* ind, const int t, const int topk, const int lane) {
    const int e = t * kMlaKeys + (lane & 31);
    const int v = ind[min(e, topk - 1)];
    return e < topk ? v : -1;
}

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_decode_sparse_kernel(const MlaParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NLD = kMlaNLD;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;           // query row (MFMA column) of this lane
    const int hh = lane >> 4;           // key sub-block of this lane
    // wave -> item -> (batch, split, row tile = (pos, head tile))
    const int nt = p.row_tiles, ns = p.num_splits;
    const int item = blockIdx.x * kMlaWaves + wave;
    if (item >= p.b * ns * nt) return;
    const int bs = item / nt;
    const int rtile = item - bs * nt;
    const int bidx = bs / ns;
    const int split = bs - bidx * ns;
    char* img = smem + wave * kMlaImage;

    const int sq = p.seqlen_q, H = p.h;
    const int htiles = (H + 15) >> 4;
    const int pos = rtile / htiles;
    const int htile = rtile - pos * htiles;
    // a lane past the last head of a partial head tile computes the last head again and stores
    // nothing: an MFMA column depends on its own query row alone
    const bool row_ok = htile * 16 + lr < H;
    const int head = min(htile * 16 + lr, H - 1);
    const float c = p.scale_log2;
    const int topk = p.topk;
    const uint32_t nslots = (uint32_t)min(p.num_slots, (int64_t)0x80000000LL);

    // index tiles of this split: [0, ceil(topk / 32)) in num_splits equal ranges
    const int t_end = (topk + kMlaKeys - 1) / kMlaKeys;
    const int per = (t_end + ns - 1) / ns;
    const int t_lo = min(t_end, split * per);
    const int t_hi = min(t_end, t_lo + per);

    const int* ind = p.indices + (int64_t)bidx * p.ind_batch + (int64_t)pos * p.ind_row;
    int idx_n = t_lo < t_hi ? mla_sparse_fetch(ind, t_lo, topk, lane) : -1;

    // ---- Q fragments (B operand of S^T): lane holds Q[row][32 s + 8 hh .. +7]
    V8 qf[NS];
    {
        const T* qrow = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch +
                        (int64_t)pos * p.q_row + (int64_t)head * p.q_head + 8 * hh;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            qf[s] = *reinterpret_cast<const V8*>(qrow + 32 * s);
    }

    // ---- cache loads.  Row r of the tile is the cache row at slot[r]; instruction i of half
    // tile h loads chunk f = 64 (i % 9) + lane of the 8-row group 2 h + i / 9 (the dense kernel's
    // map): row f / 72, one of two rows known at compile time.
    // (the kernel argument itself: the compiler knows it for a global address and emits global,
    // not flat, loads)
    const char* pool = reinterpret_cast<const char*>(p.kv);
    // entries -> (slots, invalid mask): an invalid lane takes slot 0
    auto slots_of = [&](const int idx, uint32_t& inv) __attribute__((always_inline)) {
        const bool ok = (uint32_t)idx < nslots;
        inv = (uint32_t)__builtin_amdgcn_ballot_w64(!ok);
        return ok ? idx : 0;
    };
    // the raw ring: one tile, 2 x 18 register quads (144 registers)
    u32x4 raw[2][NLD];
    auto issue = [&](const int h, const int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            constexpr int kRowB = kMlaCPR;
            const int j = i % 9, row0 = 16 * h + 8 * (i / 9);
            const int ra = (64 * j) / kRowB, rb = (64 * j + 63) / kRowB;      // rows of lanes 0 and 63
            const int sa = __builtin_amdgcn_readlane(slot, row0 + ra);
            const int sb = __builtin_amdgcn_readlane(slot, row0 + rb);
            const int thr = kRowB * rb - 64 * j;                              // first lane of row rb
            const int mine = (ra != rb && lane >= thr) ? sb : sa;
            const int chunk = 64 * j + lane - kRowB * ((ra != rb && lane >= thr) ? rb : ra);
            const u32x4* src = reinterpret_cast<const u32x4*>(pool + (int64_t)mine * kMlaPitch + 16 * chunk);
            raw[h][i] = mla_sparse_load(src);
        }
    };

    // ---- image offsets.  Writes: chunk f = 64 j + lane of an 8-row group (9 instructions).
    int woff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int f = 64 * j + lane;
        woff[j] = mla_off(f / kMlaCPR, f % kMlaCPR);
    }
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

    // invalid mask of the tile in the ring, entries of the tile after it
    uint32_t inv_c = 0;
    if (t_lo < t_hi) {
        const int slot = slots_of(idx_n, inv_c);
        issue(0, slot);
        issue(1, slot);
        idx_n = mla_sparse_fetch(ind, min(t_lo + 1, t_hi - 1), topk, lane);
    }
    // retire the Q loads (issued before the ring) explicitly, as fmha_mla_decode_kernel does
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * NLD + 1));

    // One tile: the ring goes into the image and is refilled at once with the next tile, whose
    // loads fly across this tile's products.  LAST: the last tile of a split, which refills
    // nothing.
    auto tile = [&](auto LAST, const int t) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST)::value;
        const uint32_t inv = __builtin_amdgcn_readfirstlane(inv_c);
        if (inv) {
            // rows of invalid entries hold slot 0's bytes, whatever they are: they enter
            // O^T += V^T P^T as 0 * V, which a NaN or Inf survives, so they go in as zeros
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int row = 16 * h + 8 * (i / 9) + (64 * (i % 9) + lane) / kMlaCPR;
                    const u32x4 v = ((inv >> row) & 1u) ? u32x4{0u, 0u, 0u, 0u} : raw[h][i];
                    *reinterpret_cast<u32x4*>(img + woff[i % 9] + (16 * h + 8 * (i / 9)) * kMlaPitch) = v;
                }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < NLD; ++i)
                    *reinterpret_cast<u32x4*>(img + woff[i % 9] + (16 * h + 8 * (i / 9)) * kMlaPitch) = raw[h][i];
        }
        if constexpr (!last) {
            // pin the LDS writes before the refill and the refill before the products, as
            // fmha_mla_decode_kernel does
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const int slot = slots_of(idx_n, inv_c);
            issue(0, slot);
            issue(1, slot);
            idx_n = mla_sparse_fetch(ind, min(t + 2, t_hi - 1), topk, lane);
            __builtin_amdgcn_sched_barrier(0);
        }
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

    for (int t = t_lo; t + 1 < t_hi; ++t) tile(std::false_type{}, t);
    if (t_lo < t_hi) tile(std::true_type{}, t_hi - 1);

    // ---- epilogue: as fmha_mla_decode_kernel
    const float l_full = quad_sum16(l_run);
    const bool empty = (l_full == 0.f) || (l_full != l_full);
    const float inv = empty ? 0.f : 1.f / l_full;
    if (!row_ok) return;
    const float lsev = empty ? -INFINITY : (m_run * c + __log2f(l_full)) * kLn2;
    if (ns > 1) {
        const int64_t rid = (((int64_t)split * p.b + bidx) * H + head) * sq + pos;
        float* oa = p.oaccum + rid * kMlaDV;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
            *reinterpret_cast<f32x4*>(oa + 16 * dt + 4 * hh) =
                f32x4{acc_o[dt][0] * inv, acc_o[dt][1] * inv, acc_o[dt][2] * inv, acc_o[dt][3] * inv};
        if (hh == 0) p.lseaccum[rid] = lsev;
    } else {
        typedef __attribute__((ext_vector_type(4))) T T4;
        T* orow = reinterpret_cast<T*>(p.o) + (int64_t)bidx * p.o_batch + (int64_t)pos * p.o_row +
                  (int64_t)head * p.o_head;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
            *reinterpret_cast<T4*>(orow + 16 * dt + 4 * hh) =
                T4{(T)(acc_o[dt][0] * inv), (T)(acc_o[dt][1] * inv), (T)(acc_o[dt][2] * inv), (T)(acc_o[dt][3] * inv)};
        if (p.lse && hh == 0)
            p.lse[((int64_t)bidx * H + head) * sq + pos] = empty ? INFINITY : lsev;
    }
}

}  // namespace xfa
