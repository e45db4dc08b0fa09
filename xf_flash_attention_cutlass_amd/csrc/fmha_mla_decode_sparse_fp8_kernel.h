// fmha_mla_decode_sparse_fp8_kernel.h — fmha_mla_decode_fp8_kernel (fmha_mla_decode_fp8_kernel.h)
// over index-selected tokens (fmha_mla_decode_sparse_fp8), gfx950 (CDNA4): the sparse decode of
// fmha_mla_decode_sparse_kernel.h over the 656-byte rows of the fp8 latent cache.
//
// The mapping (a 16-row tile is 16 heads of one position), the index tiles, their one coalesced
// load a tile ahead, the validation (one unsigned compare, one ballot, slot 0 for an invalid lane)
// and the invalid-row handling are the 16-bit sparse kernel's; the loads by kind, the descale
// through ds_bpermute_b32, the conversion, the image writes and everything after the image are
// the dense fp8 kernel's.  A kernel of its own.  Per load instruction the lane-to-row map is
// the dense fp8 kernel's, only the source address changes (kv + slot * 656 + the lane's constant,
// 64 bits, plain global loads - XFA_MLA_SPARSE_NT):
//      latent load i     row 2 i + lane / 32: two rows, their slots by v_readlane_b32, the lane's
//                        own under lane >= 32
//      rotary load j     row 8 j + lane / 8: eight rows, the lane's slot by ds_bpermute_b32
//      descale load      row lane % 16, the lane's slot by ds_bpermute_b32
// A row of an invalid entry is zeroed AFTER the conversion (slot 0 may dequantise to NaN) and its
// score is -inf, both behind the wave-uniform test of the tile's invalid mask.
#pragma once

#include "fmha_mla_decode_fp8_kernel.h"
#include "fmha_mla_decode_sparse_kernel.h"

namespace xfa {

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_decode_sparse_fp8_kernel(const MlaParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NL = kMlaNL8, NR = kMlaNR8;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;           // query row (MFMA column) of this lane
    const int hh = lane >> 4;           // key sub-block of this lane
    // wave -> item -> (batch, split, row tile = (pos, head tile)), as fmha_mla_decode_sparse_kernel
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
    const bool row_ok = htile * 16 + lr < H;
    const int head = min(htile * 16 + lr, H - 1);
    const float c = p.scale_log2;
    const int topk = p.topk;
    const uint32_t nslots = (uint32_t)min(p.num_slots, (int64_t)0x80000000LL);

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

    // ---- cache loads: row r of the tile is the cache row at slot[r]
    // (the kernel argument itself: the compiler knows it for a global address and emits global,
    // not flat, loads)
    const char* pool = reinterpret_cast<const char*>(p.kv);
    auto slots_of = [&](const int idx, uint32_t& inv) __attribute__((always_inline)) {
        const bool ok = (uint32_t)idx < nslots;
        inv = (uint32_t)__builtin_amdgcn_ballot_w64(!ok);
        return ok ? idx : 0;
    };
    // the raw ring: one tile, 2 x (8 latent quads + 2 rotary quads + the descale dword)
    u32x4 lat[2][NL], rot[2][NR];
    unsigned dsr[2];
    const int c32 = lane & 31, r2 = lane >> 5, r8 = lane >> 3;
    const int lat_v = 16 * c32;
    const int rot_v = 528 + 16 * (lane & 7);
    const int dsr_v = 512 + 4 * (lane >> 4);
    auto row_at = [&](const int slot, const int off) __attribute__((always_inline)) {
        return pool + (int64_t)slot * kMlaRow8 + off;
    };
    auto issue = [&](const int h, const int slot) __attribute__((always_inline)) {
        // (the descales first: loads retire in order, and the first conversion needs them)
        const int sd = __builtin_amdgcn_ds_bpermute(4 * (16 * h + (lane & 15)), slot);
        dsr[h] = mla_sparse_load(reinterpret_cast<const unsigned*>(row_at(sd, dsr_v)));
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int sa = __builtin_amdgcn_readlane(slot, 16 * h + 2 * i);
            const int sb = __builtin_amdgcn_readlane(slot, 16 * h + 2 * i + 1);
            lat[h][i] = mla_sparse_load(reinterpret_cast<const u32x4*>(row_at(r2 ? sb : sa, lat_v)));
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int sr = __builtin_amdgcn_ds_bpermute(4 * (16 * h + 8 * j + r8), slot);
            rot[h][j] = mla_sparse_load(reinterpret_cast<const u32x4*>(row_at(sr, rot_v)));
        }
    };

    // ---- image offsets of the writes, as fmha_mla_decode_fp8_kernel
    const int odd = (lane >> 2) & 1;                        // the odd chunk goes first
    int wl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wl[u] = r2 * kMlaPitch + 16 * ((2 * c32 + odd) ^ (2 * u));
    const int wr = r8 * kMlaPitch + 16 * ((64 + (lane & 7)) ^ (r8 & 6));
    const int src = 4 * (16 * (c32 >> 3) + r2);
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

    uint32_t inv_c = 0;
    if (t_lo < t_hi) {
        const int slot = slots_of(idx_n, inv_c);
        issue(0, slot);
        issue(1, slot);
        idx_n = mla_sparse_fetch(ind, min(t_lo + 1, t_hi - 1), topk, lane);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * (NL + NR + 1) + 1));

    // The ring into the image.  ZERO: the rows whose bit is set in inv are written as zeros (after
    // the conversion: a NaN descale times anything must not reach 0 * V).
    auto fill = [&](auto ZERO, const uint32_t inv) __attribute__((always_inline)) {
        constexpr bool zero = decltype(ZERO)::value;
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const u32x4 v = lat[h][i];
                const float ds = __uint_as_float(__builtin_amdgcn_ds_bpermute(src + 8 * i, (int)dsr[h]));
                u32x4 a = mla8_dequant<T>(odd ? v[2] : v[0], odd ? v[3] : v[1], ds);
                u32x4 b = mla8_dequant<T>(odd ? v[0] : v[2], odd ? v[1] : v[3], ds);
                if (zero && ((inv >> (16 * h + 2 * i + r2)) & 1u)) a = b = z;
                char* dst = img + (16 * h + 2 * i) * kMlaPitch;
                *reinterpret_cast<u32x4*>(dst + wl[i & 3]) = a;
                *reinterpret_cast<u32x4*>(dst + (wl[i & 3] ^ 16)) = b;
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const bool keep = !zero || !((inv >> (16 * h + 8 * j + r8)) & 1u);
                *reinterpret_cast<u32x4*>(img + (16 * h + 8 * j) * kMlaPitch + wr) = keep ? rot[h][j] : z;
            }
        }
    };

    // One tile: the ring goes into the image and is refilled at once with the next tile, whose
    // loads fly across this tile's products.  LAST: the last tile of a split, which refills
    // nothing.
    auto tile = [&](auto LAST, const int t) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST)::value;
        const uint32_t inv = __builtin_amdgcn_readfirstlane(inv_c);
        if (inv) fill(std::true_type{}, inv);
        else fill(std::false_type{}, 0u);
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
