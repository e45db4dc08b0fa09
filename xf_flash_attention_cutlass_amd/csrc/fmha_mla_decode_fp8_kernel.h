// fmha_mla_decode_fp8_kernel.h — fmha_mla_decode_kernel (fmha_mla_decode_kernel.h) over an fp8
// paged latent cache (fmha_mla_decode_fp8; the layout FlashMLA serves DeepSeek with, vLLM's
// fp8_ds_mla), gfx950 (CDNA4).
//
// A cache row is 656 bytes: 512 e4m3fn latent features, four fp32 descales (descale j for
// features 128 j .. +127) and the 64 rotary features in q's 16-bit type.  The operand the kernel
// attends over is T(float(e4m3) * descale) for the latent features - one fp32 product rounded
// once to q's type T - and the stored values for the rotary ones.  With that row as K and its
// first 512 features as V everything is the 16-bit kernel: the mapping (a wave is an item, its
// image is private, no barrier), the 32-key tiles, the 36,864-byte image under mla_off, both
// product loops, the softmax, the edge and last-tile handling, the epilogue and the combine.  A
// kernel of its own, so that the 16-bit kernel's instructions stay what they were; the two share
// mla_off and the constants.  What differs is how a tile gets from HBM into the image:
//
//  * Loads by kind, not by address.  A 16-row half tile is one run of 10,496 bytes inside one
//    page (41 chunks of 16 bytes a row), read by 11 load instructions in which every lane is live
//    and all lanes of an instruction hold the same kind of chunk:
//      8 latent loads    load i, lane l: row 2 i + l / 32, latent chunk c = l % 32 (16 e4m3 bytes)
//                        -> 16 values of T = image chunks 2 c and 2 c + 1 (adjacent under mla_off:
//                        its XOR leaves bit 0 of the chunk alone)
//      2 rotary loads    load j, lane l: row 8 j + l / 8, rotary chunk l % 8 (8 values of T),
//                        copied to image chunk 64 + l % 8
//      1 descale load    lane l gets ONE dword, descale l / 16 of row l % 16
//    Per-lane offsets inside the half tile are loop constants (one register a kind), the load's
//    number is an immediate; every byte of the run is read once, in pieces of 512 (latent), 128
//    (rotary) and 16 bytes (descales) of the same cache lines.  The descriptor, the non-temporal
//    policy and the scalar page fetch one tile ahead are the 16-bit kernel's.  The raw ring of a
//    tile is 2 x (10 quads + 1 dword) = 82 registers (144 in the 16-bit kernel).
//  * A latent lane takes its descale - row, group c / 8 - from lane 16 (c / 8) + row of the
//    descale dword with ds_bpermute_b32, which moves registers through the LDS crossbar and
//    touches no LDS memory: no staging area, no ordering between a store and a read to keep.
//    Then v_cvt_pk_f32_fp8, v_pk_mul_f32 by the descale, one rounding to T, two ds_write_b128.
//    No lane mask anywhere: no lane holds descales or nothing among lanes that convert.
//  * Image offsets: row & 6, the XOR of mla_off, is 2 (i % 4) for every lane of latent load i
//    (l / 32 only sets bit 0 of the row) and (l / 8) & 6 for the rotary loads: 4 offset registers
//    for the latent writes, 1 for the rotary ones, the rest immediates.
//  * The two 16-byte writes of a latent lane: the 8 consecutive lanes of a ds_write_b128 group
//    hold 8 consecutive c of one row, 32 bytes apart, so the first and the fifth would meet in a
//    bank if all wrote their even chunk first.  Lanes with bit 2 of the lane set write the odd
//    chunk first (the halves of the raw quad are swapped before the conversion: 4 selects under
//    one mask): 4 even and 4 odd chunks of 8 consecutive pairs cover the 32 banks once, under
//    the XOR too.  The 8 lanes of a rotary group write one row's 128 contiguous bytes.  All 18
//    writes of a half tile are conflict-free (tools/mla_banks.py).
//  * The last tile of a sequence zeroes rows >= sk AFTER the conversion: what lies there may
//    dequantise to NaN (a NaN descale), and enters O^T += V^T P^T as 0 * V.
//  * LDS: the four images, 147,456 bytes, one workgroup per CU as before.
#pragma once

#include "fmha_mla_decode_kernel.h"

namespace xfa {

constexpr int kMlaRow8 = 656;                               // bytes per cache row
constexpr int kMlaNL8 = 8;                                  // latent loads per 16-row half tile
constexpr int kMlaNR8 = 2;                                  // rotary loads per half tile

// 8 e4m3 bytes x descale -> 8 values of T: one fp32 product (v_pk_mul_f32), rounded once
template <typename T>
__device__ __forceinline__ u32x4 mla8_dequant(const unsigned lo, const unsigned hi, const float ds) {
    typedef __attribute__((ext_vector_type(2))) float f2;
    typedef __attribute__((ext_vector_type(2))) T T2;
    const f2 s2 = {ds, ds};
    const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false) * s2, b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true) * s2;
    const f2 c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false) * s2, d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true) * s2;
    const T2 ta = {(T)a[0], (T)a[1]}, tb = {(T)b[0], (T)b[1]}, tc = {(T)c[0], (T)c[1]}, td = {(T)d[0], (T)d[1]};
    return u32x4{__builtin_bit_cast(unsigned, ta), __builtin_bit_cast(unsigned, tb),
                 __builtin_bit_cast(unsigned, tc), __builtin_bit_cast(unsigned, td)};
}

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_decode_fp8_kernel(const MlaParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NL = kMlaNL8, NR = kMlaNR8;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;           // query row (MFMA column) of this lane
    const int hh = lane >> 4;           // key sub-block of this lane
    // wave -> item -> (batch, split, row tile), as fmha_mla_decode_kernel
    const int nt = p.row_tiles, ns = p.num_splits;
    const int item = blockIdx.x * kMlaWaves + wave;
    if (item >= p.b * ns * nt) return;
    const int bs = item / nt;
    const int rtile = item - bs * nt;
    const int bidx = bs / ns;
    const int split = bs - bidx * ns;
    char* img = smem + wave * kMlaImage;

    const int sq = p.seqlen_q, H = p.h;
    const int sk = max(0, min(__builtin_amdgcn_readfirstlane(p.cache_seqlens[bidx]), p.max_seqlen_k));
    const int rows = sq * H;
    const int diag = sk - sq;
    const int r = rtile * 16 + lr;
    const bool row_ok = r < rows;
    const int pos = min(r, rows - 1) / H;
    const int head = min(r, rows - 1) - pos * H;
    const int my_lim = p.causal ? min(sk, max(0, pos + diag + 1)) : sk;
    const float c = p.scale_log2;

    const int t_end = (sk + kMlaKeys - 1) / kMlaKeys;
    const int per = (t_end + ns - 1) / ns;
    const int t_lo = min(t_end, split * per);
    const int t_hi = min(t_end, t_lo + per);

    // ---- Q fragments (B operand of S^T): lane holds Q[row][32 s + 8 hh .. +7]
    V8 qf[NS];
    {
        const T* qrow = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch +
                        (int64_t)pos * p.q_row + (int64_t)head * p.q_head + 8 * hh;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            qf[s] = *reinterpret_cast<const V8*>(qrow + 32 * s);
    }

    // ---- cache loads: half tile u = 2 t + h is rows 16 u .. +15 of the sequence, one page
    // (wave-uniform descriptor over exactly that page), one contiguous run.  A half tile past the
    // sequence's last page re-reads the start of the last page: its keys are >= sk.
    typedef __attribute__((address_space(4))) const int cint;
    cint* btab = (cint*)(p.block_table + (int64_t)bidx * p.bt_stride);
    const int last_pg = sk > 0 ? (sk - 1) / p.page_size : 0;
    const uint32_t page_bytes = (uint32_t)p.page_size * kMlaRow8;
    const char* pool = uniform_ptr(reinterpret_cast<const char*>(p.kv));
    auto fetch_page = [&](const int u, int (&pg)[2]) __attribute__((always_inline)) {
        const int row0 = 16 * u;
        const int pi = __builtin_amdgcn_readfirstlane(row0 / p.page_size);
        const bool past = pi > last_pg;
        pg[0] = btab[past ? last_pg : pi];
        pg[1] = past ? 0 : row0 - pi * p.page_size;
    };
    // the raw ring: one tile, 2 x (8 latent quads + 2 rotary quads + the descale dword)
    u32x4 lat[2][NL], rot[2][NR];
    unsigned dsr[2];
    const int c32 = lane & 31, r2 = lane >> 5, r8 = lane >> 3;
    const int lat_v = r2 * kMlaRow8 + 16 * c32;
    const int rot_v = r8 * kMlaRow8 + 528 + 16 * (lane & 7);
    const int dsr_v = (lane & 15) * kMlaRow8 + 512 + 4 * (lane >> 4);
    auto issue = [&](const int h, const int (&pg)[2]) __attribute__((always_inline)) {
        const int page = __builtin_amdgcn_readfirstlane(pg[0]);
        const int x = __builtin_amdgcn_readfirstlane(pg[1]);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(uniform_ptr(pool + (int64_t)page * page_bytes), page_bytes);
        // (the descales first: loads retire in order, and the first conversion needs them)
        dsr[h] = __builtin_amdgcn_raw_buffer_load_b32(rs, dsr_v, x * kMlaRow8, XFA_DEC_CPOL);
#pragma unroll
        for (int i = 0; i < NL; ++i)
            lat[h][i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lat_v, (x + 2 * i) * kMlaRow8, XFA_DEC_CPOL);
#pragma unroll
        for (int j = 0; j < NR; ++j)
            rot[h][j] = __builtin_amdgcn_raw_buffer_load_b128(rs, rot_v, (x + 8 * j) * kMlaRow8, XFA_DEC_CPOL);
    };

    // ---- image offsets of the writes.  Latent load i: row 2 i + r2, whose row & 6 is 2 (i % 4);
    // wl[u]: the lane's first write for i % 4 == u (the second is 16 bytes to the other side),
    // from row 2 i of the half tile.  Rotary load j: row 8 j + r8, row & 6 = r8 & 6; wr from row
    // 8 j.  src: 4 x the lane of the descale dword that holds this lane's descale, for row r2.
    const int odd = (lane >> 2) & 1;                        // the odd chunk goes first
    int wl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wl[u] = r2 * kMlaPitch + 16 * ((2 * c32 + odd) ^ (2 * u));
    const int wr = r8 * kMlaPitch + 16 * ((64 + (lane & 7)) ^ (r8 & 6));
    const int src = 4 * (16 * (c32 >> 3) + r2);
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

    int pg_a[2] = {0, 0}, pg_b[2] = {0, 0};
    if (t_lo < t_hi) {
        fetch_page(2 * t_lo, pg_a);
        fetch_page(2 * t_lo + 1, pg_b);
        issue(0, pg_a);
        issue(1, pg_b);
        fetch_page(2 * min(t_lo + 1, t_hi - 1), pg_a);
        fetch_page(2 * min(t_lo + 1, t_hi - 1) + 1, pg_b);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * (NL + NR + 1)));

    // The ring into the image.  ZERO: rows >= nval of the tile are written as zeros (after the
    // conversion: a NaN descale times anything must not reach 0 * V).
    auto fill = [&](auto ZERO, const int nval) __attribute__((always_inline)) {
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
                if (zero && 16 * h + 2 * i + r2 >= nval) a = b = z;
                char* dst = img + (16 * h + 2 * i) * kMlaPitch;
                *reinterpret_cast<u32x4*>(dst + wl[i & 3]) = a;
                *reinterpret_cast<u32x4*>(dst + (wl[i & 3] ^ 16)) = b;
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const bool keep = !zero || 16 * h + 8 * j + r8 < nval;
                *reinterpret_cast<u32x4*>(img + (16 * h + 8 * j) * kMlaPitch + wr) = keep ? rot[h][j] : z;
            }
        }
    };

    // One tile: the ring goes into the image and is refilled at once with the next tile, whose
    // loads fly across this tile's products.  LAST: the last tile of a split, which refills
    // nothing and alone can hold the sequence's end.
    auto tile = [&](auto LAST, const int t) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST)::value;
        const int keyb = t * kMlaKeys;
        bool plain = true;
        if constexpr (last) {
            if (keyb + kMlaKeys > sk) {
                plain = false;
                fill(std::true_type{}, sk - keyb);
            }
        }
        if (plain) fill(std::false_type{}, kMlaKeys);
        if constexpr (!last) {
            // pin the LDS writes before the refill and the refill before the products, as
            // fmha_mla_decode_kernel does
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            issue(0, pg_a);
            issue(1, pg_b);
            __builtin_amdgcn_sched_barrier(0);
            fetch_page(2 * min(t + 2, t_hi - 1), pg_a);
            fetch_page(2 * min(t + 2, t_hi - 1) + 1, pg_b);
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
        const bool edge = keyb + kMlaKeys > my_lim;
        if (__builtin_amdgcn_ballot_w64(edge)) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (keyb + 16 * kb + 4 * hh + i >= my_lim) st[kb][i] = -INFINITY;
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
