// fmha_mla_sparse_fwd_fp8_kernel.h — fmha_mla_sparse_fwd_kernel (fmha_mla_sparse_fwd_kernel.h) over
// the 656-byte rows of the fp8 latent cache (fmha_mla_sparse_fwd_fp8), gfx950 (CDNA4): DeepSeek-V3.2's
// sparse prefill straight out of the cache it is served with, no 16-bit copy of the selected rows.
//
// For query (pos, head), K is the dequantised rows of kv [s_kv, 1, 656 bytes] at the valid entries
// of indices[pos, 0 .. topk): feature i < 512 is T(float(e4m3[i]) * descale[i / 128]), one fp32
// product rounded once to q's type T, the 64 rotary features as stored.  From
// fmha_mla_sparse_fwd_kernel, unchanged: a workgroup is one position and four 16-head tiles, wave w
// owns head tile 4 group + w and rows 8 w .. 8 w + 7 of every 32-key tile, two images (73,728 B), one
// barrier a tile that waits for the LDS counter only, the index fetch one tile further ahead, dead
// waves that gather and meet every barrier, the products and the epilogue.  From
// fmha_mla_decode_sparse_fp8_kernel: loads by kind, the descale through ds_bpermute_b32,
// mla8_dequant, rows of invalid entries zeroed AFTER the conversion.  The image is byte for byte
// what that kernel builds for the same tile, so O and LSE equal its at num_splits = 1 bit for bit.
// A kernel of its own, so that the 16-bit kernel's instructions stay what they are.  What is new:
//
//  * A wave's share of the shared image is 8 rows x 41 chunks of 16 bytes, read by 6 load
//    instructions in which every lane is live (the 16-bit kernel: 9; a decode wave, which gathers
//    all 32 rows for its 16 heads alone: 22):
//      4 latent loads    load i, lane l: row 8 w + 2 i + l / 32, latent chunk c = l % 32; the two
//                        slots of an instruction by v_readlane_b32, the lane's own under l >= 32
//      1 rotary load     lane l: row 8 w + l / 8, rotary chunk l % 8, the slot by ds_bpermute_b32
//      1 descale load    lane l gets ONE dword, descale (l / 8) % 4 of row 8 w + l % 8 (lanes 32-63
//                        repeat lanes 0-31), the slot by ds_bpermute_b32
//    The raw ring of a tile is 4 x 4 + 4 + 1 = 21 registers (36 in the 16-bit kernel, 82 in a
//    decode wave).  A selected row is pulled through L2 and converted once per 64 heads.
//  * A latent lane of load i - row 2 i + l / 32 of the eight, group c / 8 - takes its descale from
//    lane 8 (c / 8) + 2 i + l / 32 of the descale dword: ds_bpermute_b32 at 4 (8 (c / 8) + l / 32)
//    plus the immediate 8 i, one register for the four loads.
//  * Image offsets: 8 w is a multiple of 8, so row & 6 is 2 i for latent load i and (l / 8) & 6
//    for the rotary load - the decode kernel's wl[] / wr plus 8 w * 1152; the odd-chunk-first swap
//    keeps every ds_write_b128 group conflict-free as there (tools/mla_banks.py).
//  * The kv row stride is a parameter in BYTES (>= 656, a multiple of 16): a padded cache works.
//  * No load leaves [kv, kv + s_kv * row stride): an invalid lane takes row 0 (the host requires
//    s_kv >= 1).  What row 0 dequantises to (possibly NaN) is replaced by zeros after the
//    conversion and scores -inf, both behind the wave-uniform test of the tile's invalid mask.
#pragma once

#include "fmha_mla_decode_fp8_kernel.h"
#include "fmha_mla_sparse_fwd_kernel.h"

namespace xfa {

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_sparse_fwd_fp8_kernel(const MlaSparseFwdParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NL = 4;               // latent loads of a wave's 8 rows
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

    // The entries of index tile t: lane l gets entry 32 t + l % 32, the load clamped to the row; what
    // it brought is first touched in slots_of, a tile later (as fmha_mla_sparse_fwd_kernel)
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

    // ---- this wave's rows of a tile: 8 wave .. + 7, row r of them the cache row at slot[8 wave + r]
    const char* pool = reinterpret_cast<const char*>(p.kv);
    const int64_t pitch = p.kv_row;     // bytes
    const int row0 = 8 * wave;
    // entries of tile t -> (rows, invalid mask): a place at or past topk is invalid, an invalid lane
    // takes row 0
    auto slots_of = [&](const int idx, const int t, uint32_t& inv) __attribute__((always_inline)) {
        const bool ok = (uint32_t)idx < nrows && t * kMlaKeys + (lane & 31) < topk;
        inv = (uint32_t)__builtin_amdgcn_ballot_w64(!ok);
        return ok ? idx : 0;
    };
    // the raw ring: 4 latent quads, the rotary quad, the descale dword
    u32x4 lat[NL], rot;
    unsigned dsr;
    const int c32 = lane & 31, r2 = lane >> 5, r8 = lane >> 3;
    const int lat_v = 16 * c32;
    const int rot_v = 528 + 16 * (lane & 7);
    const int dsr_v = 512 + 4 * (r8 & 3);
    auto row_at = [&](const int slot, const int off) __attribute__((always_inline)) {
        return pool + (int64_t)slot * pitch + off;
    };
    auto issue = [&](const int slot) __attribute__((always_inline)) {
        // (the descales first: loads retire in order, and the first conversion needs them)
        const int sd = __builtin_amdgcn_ds_bpermute(4 * (row0 + (lane & 7)), slot);
        dsr = mla_sparse_load(reinterpret_cast<const unsigned*>(row_at(sd, dsr_v)));
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int sa = __builtin_amdgcn_readlane(slot, row0 + 2 * i);
            const int sb = __builtin_amdgcn_readlane(slot, row0 + 2 * i + 1);
            lat[i] = mla_sparse_load(reinterpret_cast<const u32x4*>(row_at(r2 ? sb : sa, lat_v)));
        }
        const int sr = __builtin_amdgcn_ds_bpermute(4 * (row0 + r8), slot);
        rot = mla_sparse_load(reinterpret_cast<const u32x4*>(row_at(sr, rot_v)));
    };

    // ---- image offsets of the writes: fmha_mla_decode_fp8_kernel's, from row 8 wave.  Latent load
    // i: row row0 + 2 i + r2, whose row & 6 is 2 i; wl[i] from row row0 + 2 i (the second write is
    // 16 bytes to the other side).  Rotary load: row row0 + r8, row & 6 = r8 & 6.  src: 4 x the lane
    // of the descale dword that holds this lane's descale for load 0.
    const int odd = (lane >> 2) & 1;                        // the odd chunk goes first
    int wl[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) wl[u] = (row0 + r2) * kMlaPitch + 16 * ((2 * c32 + odd) ^ (2 * u));
    const int wr = (row0 + r8) * kMlaPitch + 16 * ((64 + (lane & 7)) ^ (r8 & 6));
    const int src = 4 * (8 * (c32 >> 3) + r2);
    // The ring, converted, into image `dst`.  ZERO: the rows whose bit is set in inv are written as
    // zeros (after the conversion: a NaN descale times anything must not reach 0 * V).
    auto fill = [&](auto ZERO, char* dst, const uint32_t inv) __attribute__((always_inline)) {
        constexpr bool zero = decltype(ZERO)::value;
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const u32x4 v = lat[i];
            const float ds = __uint_as_float(__builtin_amdgcn_ds_bpermute(src + 8 * i, (int)dsr));
            u32x4 a = mla8_dequant<T>(odd ? v[2] : v[0], odd ? v[3] : v[1], ds);
            u32x4 b = mla8_dequant<T>(odd ? v[0] : v[2], odd ? v[1] : v[3], ds);
            if (zero && ((inv >> (row0 + 2 * i + r2)) & 1u)) a = b = z;
            char* d = dst + 2 * i * kMlaPitch;
            *reinterpret_cast<u32x4*>(d + wl[i]) = a;
            *reinterpret_cast<u32x4*>(d + (wl[i] ^ 16)) = b;
        }
        const bool keep = !zero || !((inv >> (row0 + r8)) & 1u);
        *reinterpret_cast<u32x4*>(dst + wr) = keep ? rot : z;
    };
    auto stash = [&](char* dst, const uint32_t inv) __attribute__((always_inline)) {
        if (inv) fill(std::true_type{}, dst, inv);
        else fill(std::false_type{}, dst, 0u);
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

    // the products of one tile out of `img`: fmha_mla_sparse_fwd_kernel's, statement for statement
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

    // ---- epilogue: as fmha_mla_sparse_fwd_kernel
    if (!live) return;
    const float l_full = quad_sum16(l_run);
    const bool empty = (l_full == 0.f) || (l_full != l_full);
    const float inv = empty ? 0.f : 1.f / l_full;
    if (!row_ok) return;
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
