// fmha_bwd_mla_kernel.h — MLA prefill backward: the gradient of the attention with head size 192
// for Q K^T and 128 for V (fmha_fwd_mla_kernel.h), for gfx950 (CDNA4).  DESIGN.md §3.12.
//
// No atomics: every output element has one writer and one summation order, so there is no fp32
// dQ accumulator, no zeroing pass, no convert pass and no deterministic mode.
//   * fmha_bwd_mla_pre_kernel: D[row] = sum over the 128 columns of dO * O (fp32, laid out like
//     the LSE).  Zeroes nothing.
//   * fmha_bwd_mla_dkdv_kernel: fmha_bwd_kernel's KV-stationary mapping without its dQ phase.  One
//     workgroup = 128 keys of one (batch, kv head), 4 waves x 32 keys, one wave a SIMD; dK^T
//     (6 tiles) and dV^T (4 tiles) of a wave's keys stay in accumulators while the workgroup sweeps
//     the G heads of the group x 32-row query tiles.  A wave's K and V rows are only ever its own
//     B operands and stay in registers (48 + 32); LDS holds the double-buffered Q (32 x 192) and
//     dO (32 x 128) tiles in the kv_off images (row reads for S and dP, transposing reads for
//     Q^T and dO^T) and a per-wave LSE / D slot.
//   * fmha_bwd_mla_dq_kernel: Q-stationary, fwd_mla_item's orientation with the LSE known.  One
//     workgroup = 128 query rows of one (batch, head), 4 waves x 32 rows; Q (12 fragments) and dO
//     (8 fragments) stay in registers as B operands, LSE and D are two scalars a lane.  64-key
//     tiles of K [64][192] and V [64][128] stream through two LDS stages; S^T = K Q^T,
//     dP^T = V dO^T, dS^T = P (dP^T - D) -> T is straight from the accumulator the B operand of
//     dQ^T += K^T dS^T, K^T by transposing reads of the same K tile.
// Tiles reach LDS through registers (16-byte buffer loads a tile ahead, ds_write_b128 after the
// tile's products), so every wait is the compiler's own.  Loads go through buffer descriptors
// sized to each sequence: rows past a sequence's end and keys past sk arrive as zeros.
#pragma once

#include "fmha_common.h"

namespace xfa {

constexpr int kBwdMlaHdk = 192;                 // q / k / dq / dk head size
constexpr int kBwdMlaHdv = 128;                 // v / o / dO / dv head size
constexpr int kBwdMlaWaves = 4;
constexpr int kBwdMlaBlockN = 128;              // keys per dK/dV workgroup
constexpr int kBwdMlaBlockQ = 32;               // query rows per tile of its sweep
constexpr int kBwdMlaBlockM = 128;              // query rows per dQ workgroup
constexpr int kBwdMlaQTile = kBwdMlaBlockQ * kBwdMlaHdk * 2;
constexpr int kBwdMlaDoTile = kBwdMlaBlockQ * kBwdMlaHdv * 2;
// dK/dV: 2 x (Q tile, dO tile), then one 64-float LSE / D slot a wave
constexpr int kBwdMlaDkdvSmem = 2 * (kBwdMlaQTile + kBwdMlaDoTile) + kBwdMlaWaves * 256;
constexpr int kBwdMlaKTile = kBlockN * kBwdMlaHdk * 2;
constexpr int kBwdMlaVTile = kBlockN * kBwdMlaHdv * 2;
constexpr int kBwdMlaDqSmem = 2 * (kBwdMlaKTile + kBwdMlaVTile);   // 2 x (K tile, V tile) = 80 KiB

// ---------------------------------------------------------------- preprocess ---------------
// D[row] = sum_d dO * O over the 128 value columns (fp32)
template <typename T>
__global__ void __launch_bounds__(256) fmha_bwd_mla_pre_kernel(const BwdParams p, int total_rows) {
    constexpr int TPR = kBwdMlaHdv / 8;         // threads per (token, head) row
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int r = t / TPR;
    const int c = t % TPR;
    if (r >= total_rows) return;
    const int head = r % p.h;
    const int tok = r / p.h;                    // dense: b*sq + pos ; packed: global token
    int bidx, pos;
    if (p.cu_seqlens_q) { bidx = 0; pos = tok; }
    else { bidx = tok / p.seqlen_q; pos = tok - bidx * p.seqlen_q; }
    const int d0 = c * 8;
    const T* o = reinterpret_cast<const T*>(p.o) + (int64_t)bidx * p.o_batch + (int64_t)pos * p.o_row +
                 (int64_t)head * p.o_head + d0;
    const T* g = reinterpret_cast<const T*>(p.dout) + (int64_t)bidx * p.do_batch +
                 (int64_t)pos * p.do_row + (int64_t)head * p.do_head + d0;
    typedef __attribute__((ext_vector_type(8))) T T8;
    const T8 ov = *reinterpret_cast<const T8*>(o);
    const T8 gv = *reinterpret_cast<const T8*>(g);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf((float)ov[j], (float)gv[j], acc);
#pragma unroll
    for (int m = TPR / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (c == 0) p.dsum[(int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + pos] = acc;
}

// One transposed A operand (32 rows of the head dim x 16 rows of the tile) from a kv_off image:
// two ds_read_b64_tr_b16, the lane's two 4-row blocks 8 rows apart
template <typename V8>
__device__ __forceinline__ V8 bwd_mla_tr_read(const int a0, const int a1) {
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)a0);
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)a1);
    const s16x8 av = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    return __builtin_bit_cast(V8, av);
}

// ---------------------------------------------------------------- dK / dV ------------------
// grid (key blocks, batch x kv heads): key block 0, which every causal row sees, first
template <typename T, bool MASK, bool PACKED>
__global__ void __launch_bounds__(kBwdMlaWaves * 64, 1) fmha_bwd_mla_dkdv_kernel(const BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using V8 = typename DT<T>::v8;
    constexpr int HDK = kBwdMlaHdk, HDV = kBwdMlaHdv;
    constexpr int NT = kBwdMlaWaves * 64;
    constexpr int BN = kBwdMlaBlockN, BQ = kBwdMlaBlockQ;
    constexpr int NSK = HDK / 16, NSV = HDV / 16;     // k-steps of S = Q K^T and dP = dO V^T
    constexpr int NDK = HDK / 32, NDV = HDV / 32;     // 32-wide d tiles of dK^T and dV^T
    constexpr int CK = HDK / 8, CV = HDV / 8;         // 16-byte chunks a row
    constexpr int QLD = BQ * CK / NT, GLD = BQ * CV / NT;   // Q / dO chunks a thread a tile
    static_assert(QLD * NT == BQ * CK && GLD * NT == BQ * CV, "Q / dO tile geometry");
    constexpr int RBK = HDK * 16, RBV = HDV * 16;     // bytes of one 8-row block of each image
    constexpr int STAGE = kBwdMlaQTile + kBwdMlaDoTile;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int hh = lane >> 5;

    const int bh = blockIdx.y;
    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;
    const int n0 = (int)blockIdx.x * BN;

    int q_off = 0, sq = p.seqlen_q, k_off = 0, sk = p.seqlen_k;
    if constexpr (PACKED) {
        q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off;
        k_off = p.cu_seqlens_k[bidx]; sk = p.cu_seqlens_k[bidx + 1] - k_off;
    }
    if (n0 >= sk) return;
    const int diag = sk - sq;

    // query positions that can see any key of [n0, n0 + BN)
    int p_lo = 0, p_hi = sq;
    if (MASK && p.wr >= 0) p_lo = max(0, n0 - diag - p.wr);
    if (MASK && p.wl >= 0) p_hi = min(sq, n0 + BN - 1 - diag + p.wl + 1);
    const int t_lo = p_lo / BQ;
    const int ntiles = p_hi > p_lo ? (p_hi + BQ - 1) / BQ - t_lo : 0;
    const int G = p.group;
    const int n_iter = ntiles * G;

    // ---- this wave's K and V rows: the B operands of S = Q K^T and dP = dO V^T (key on the
    // lane, d chunk 2s + hh), in registers for the whole sweep
    const int my_key = n0 + wave * 32 + lr;
    V8 kfrag[NSK], vfrag[NSV];
    {
        const T* kb = reinterpret_cast<const T*>(p.k) + (int64_t)bidx * p.k_batch +
                      (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head;
        const T* vb = reinterpret_cast<const T*>(p.v) + (int64_t)bidx * p.v_batch +
                      (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head;
        const __amdgpu_buffer_rsrc_t krs = make_rsrc(kb, (uint32_t)(((int64_t)(sk - 1) * p.k_row + HDK) * 2));
        const __amdgpu_buffer_rsrc_t vrs = make_rsrc(vb, (uint32_t)(((int64_t)(sk - 1) * p.v_row + HDV) * 2));
        const bool ok = my_key < sk;
        const int ko = ok ? (int)((uint32_t)my_key * (uint32_t)p.k_row * 2u) + 16 * hh : kOOB;
        const int vo = ok ? (int)((uint32_t)my_key * (uint32_t)p.v_row * 2u) + 16 * hh : kOOB;
#pragma unroll
        for (int s = 0; s < NSK; ++s) kfrag[s] = __builtin_bit_cast(V8, buf_load16(krs, ok ? ko + 32 * s : kOOB));
#pragma unroll
        for (int s = 0; s < NSV; ++s) vfrag[s] = __builtin_bit_cast(V8, buf_load16(vrs, ok ? vo + 32 * s : kOOB));
    }

    // ---- Q / dO tile loader: QLD + GLD 16-byte chunks a thread, through registers
    u32x4 qreg[QLD], greg[GLD];
    float lse_raw = 0.f, d_raw = 0.f;             // lane's row (lr) of the tile: its LSE and D
    bool lsd_ok = false;
    // lanes 0-31 hold the LSE (pre-multiplied by log2e; +inf past the sequence's end), 32-63 D
    auto lsd_value = [&]() { return hh ? (lsd_ok ? d_raw : 0.f) : (lsd_ok ? lse_raw * kLog2e : INFINITY); };
    auto tile_of = [&](const int it, int& head, int& q0) {
        const int g = it / ntiles;
        head = hk_i * G + g;
        q0 = (t_lo + (it - g * ntiles)) * BQ;
    };
    auto load_q = [&](const int it) {
        int head, q0;
        tile_of(it, head, q0);
        {
            const int pos = q0 + lr;
            const bool ok = pos < sq;
            const int64_t lrow = (int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + q_off;
            const int off = (ok ? pos : 0) * 4;
            lse_raw = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(p.lse + lrow, (uint32_t)(sq * 4)), off, 0, 0));
            d_raw = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(p.dsum + lrow, (uint32_t)(sq * 4)), off, 0, 0));
            lsd_ok = ok;
        }
        // this head's rows [q0, sq): rows past the end read as zeros
        const T* qb = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch +
                      (int64_t)(q_off + q0) * p.q_row + (int64_t)head * p.q_head;
        const T* gb = reinterpret_cast<const T*>(p.dout) + (int64_t)bidx * p.do_batch +
                      (int64_t)(q_off + q0) * p.do_row + (int64_t)head * p.do_head;
        const int nrows = sq - q0;                // > 0: the tile starts below p_hi <= sq
        const __amdgpu_buffer_rsrc_t qrs = make_rsrc(qb, (uint32_t)(((int64_t)(nrows - 1) * p.q_row + HDK) * 2));
        const __amdgpu_buffer_rsrc_t grs = make_rsrc(gb, (uint32_t)(((int64_t)(nrows - 1) * p.do_row + HDV) * 2));
#pragma unroll
        for (int i = 0; i < QLD; ++i) {
            const int idx = tid + i * NT, r = idx / CK, c = idx - r * CK;
            qreg[i] = buf_load16(qrs, r < nrows ? r * (int)p.q_row * 2 + c * 16 : kOOB);
        }
#pragma unroll
        for (int i = 0; i < GLD; ++i) {
            const int idx = tid + i * NT, r = idx / CV, c = idx - r * CV;
            greg[i] = buf_load16(grs, r < nrows ? r * (int)p.do_row * 2 + c * 16 : kOOB);
        }
    };
    auto store_q = [&](const int stage) {
        char* q_lds = smem + stage * STAGE;
        char* g_lds = q_lds + kBwdMlaQTile;
#pragma unroll
        for (int i = 0; i < QLD; ++i) {
            const int idx = tid + i * NT, r = idx / CK, c = idx - r * CK;
            *reinterpret_cast<u32x4*>(q_lds + kv_off<HDK>(r, c)) = qreg[i];
        }
#pragma unroll
        for (int i = 0; i < GLD; ++i) {
            const int idx = tid + i * NT, r = idx / CV, c = idx - r * CV;
            *reinterpret_cast<u32x4*>(g_lds + kv_off<HDV>(r, c)) = greg[i];
        }
    };

    // per-lane LDS addresses within a stage (kv_off images): the row read of k-step s is
    // qa[s & 1] + 512 (s >> 1), the transposing read (sp, dt, part) qt[part] + 2 RB sp + 512 dt
    const int sbase = (int)(size_t)smem;
    const int q4 = (lane & 15) >> 2;
    int qa[2], ga[2], qt[2], gt[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        qa[u] = sbase + kv_off<HDK>(lr, 2 * u + hh);
        ga[u] = sbase + kBwdMlaQTile + kv_off<HDV>(lr, 2 * u + hh);
        const int r = 8 * u + 4 * hh + q4;
        const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        qt[u] = sbase + kv_off<HDK>(r, col >> 3) + 8 * ((col >> 2) & 1);
        gt[u] = sbase + kBwdMlaQTile + kv_off<HDV>(r, col >> 3) + 8 * ((col >> 2) & 1);
    }
    typedef __attribute__((address_space(3))) V8 lds_v8;

    f32x16 dk[NDK], dv[NDV];
#pragma unroll
    for (int dt = 0; dt < NDK; ++dt) dk[dt] = f32x16{};
#pragma unroll
    for (int dt = 0; dt < NDV; ++dt) dv[dt] = f32x16{};

    const float c = p.scale_log2;
    float lsd_cur = 0.f;
    float* const lsd_slot = reinterpret_cast<float*>(smem + 2 * STAGE + wave * 256);
    if (n_iter > 0) {
        load_q(0);
        store_q(0);
        lsd_cur = lsd_value();
    }
    __syncthreads();

    for (int it = 0; it < n_iter; ++it) {
        int head, q0;
        tile_of(it, head, q0);
        const int so = (it & 1) * STAGE;
        // this tile's LSE / D -> this wave's slot, read back below as broadcast float4s
        lsd_slot[lane] = lsd_cur;
        if (it + 1 < n_iter) load_q(it + 1);

        // ---- S = Q K^T and dP = dO V^T (key on the lane, query rows in registers)
        f32x16 s_acc = f32x16{}, dp_acc = f32x16{};
#pragma unroll
        for (int s = 0; s < NSK; ++s) {
            const V8 a = *(const lds_v8*)(size_t)(qa[s & 1] + so + 512 * (s >> 1));
            s_acc = DT<T>::mfma32(a, kfrag[s], s_acc);
            if (s < NSV) {
                const V8 g = *(const lds_v8*)(size_t)(ga[s & 1] + so + 512 * (s >> 1));
                dp_acc = DT<T>::mfma32(g, vfrag[s], dp_acc);
            }
        }
        // ---- P = exp2(S c - LSE log2e), dS = P (dP - D)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            // rows 8gq + 4hh + i of this tile: slot[row] holds its LSE, slot[32 + row] its D
            const f32x4 l = *reinterpret_cast<const f32x4*>(lsd_slot + 8 * gq + 4 * hh);
            const f32x4 dd = *reinterpret_cast<const f32x4*>(lsd_slot + 32 + 8 * gq + 4 * hh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * gq + i;
                const float pr = fast_exp2(fmaf(s_acc[r], c, -l[i]));
                s_acc[r] = pr;
                dp_acc[r] = pr * (dp_acc[r] - dd[i]);
            }
        }
        // the window mask only where this wave's 32 keys x the 32 rows cross an edge, as one
        // wave-uniform block: P and dS of invisible scores -> 0
        if constexpr (MASK) {
            const int kw0 = n0 + wave * 32, kw1 = kw0 + 31;
            bool need_mask = false;
            if (p.wr >= 0) need_mask = need_mask || kw1 >= q0 + diag + p.wr + 1;
            if (p.wl >= 0) need_mask = need_mask || kw0 < q0 + BQ - 1 + diag - p.wl;
            if (need_mask) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pos = q0 + 8 * (r >> 2) + 4 * hh + (r & 3);
                    const int hi = p.wr >= 0 ? min(sk, pos + diag + p.wr + 1) : sk;
                    const int lo = p.wl >= 0 ? max(0, pos + diag - p.wl) : 0;
                    const bool vis = (unsigned)(my_key - lo) < (unsigned)max(hi - lo, 0);
                    s_acc[r] = vis ? s_acc[r] : 0.f;
                    dp_acc[r] = vis ? dp_acc[r] : 0.f;
                }
            }
        }
        // ---- dV^T += dO^T P ; dK^T += Q^T dS  (P / dS, rounded to T, are the B operands)
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            V8 pb, sb;
#pragma unroll
            for (int j = 0; j < 8; ++j) { pb[j] = (T)s_acc[8 * sp + j]; sb[j] = (T)dp_acc[8 * sp + j]; }
#pragma unroll
            for (int dt = 0; dt < NDV; ++dt) {
                const V8 a = bwd_mla_tr_read<V8>(gt[0] + so + 2 * RBV * sp + 512 * dt, gt[1] + so + 2 * RBV * sp + 512 * dt);
                dv[dt] = DT<T>::mfma32(a, pb, dv[dt]);
            }
#pragma unroll
            for (int dt = 0; dt < NDK; ++dt) {
                const V8 a = bwd_mla_tr_read<V8>(qt[0] + so + 2 * RBK * sp + 512 * dt, qt[1] + so + 2 * RBK * sp + 512 * dt);
                dk[dt] = DT<T>::mfma32(a, sb, dk[dt]);
            }
        }
        // the next tile -> the other stage (last read in iteration it - 1, a barrier ago)
        if (it + 1 < n_iter) {
            store_q((it + 1) & 1);
            lsd_cur = lsd_value();
        }
        __syncthreads();
    }

    // ---- epilogue: dK = scale (dK^T)^T, dV = (dV^T)^T; keys no row sees get their zeros
    if (my_key >= sk) return;
    typedef __attribute__((ext_vector_type(4))) T T4;
    T* dkr = reinterpret_cast<T*>(p.dk) + (int64_t)bidx * p.dk_batch + (int64_t)(k_off + my_key) * p.dk_row +
             (int64_t)hk_i * p.dk_head;
    T* dvr = reinterpret_cast<T*>(p.dv) + (int64_t)bidx * p.dv_batch + (int64_t)(k_off + my_key) * p.dv_row +
             (int64_t)hk_i * p.dv_head;
#pragma unroll
    for (int dt = 0; dt < NDK; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const T4 kv = {(T)(dk[dt][4 * gq] * p.scale), (T)(dk[dt][4 * gq + 1] * p.scale),
                           (T)(dk[dt][4 * gq + 2] * p.scale), (T)(dk[dt][4 * gq + 3] * p.scale)};
            *reinterpret_cast<T4*>(dkr + 32 * dt + 8 * gq + 4 * hh) = kv;
        }
#pragma unroll
    for (int dt = 0; dt < NDV; ++dt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const T4 vv = {(T)dv[dt][4 * gq], (T)dv[dt][4 * gq + 1], (T)dv[dt][4 * gq + 2], (T)dv[dt][4 * gq + 3]};
            *reinterpret_cast<T4*>(dvr + 32 * dt + 8 * gq + 4 * hh) = vv;
        }
}

// ---------------------------------------------------------------- dQ -----------------------
// grid (row blocks, batch x heads): the last row block, which sees the most causal keys, first
template <typename T, bool MASK, bool PACKED>
__global__ void __launch_bounds__(kBwdMlaWaves * 64, 1) fmha_bwd_mla_dq_kernel(const BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using V8 = typename DT<T>::v8;
    constexpr int HDK = kBwdMlaHdk, HDV = kBwdMlaHdv;
    constexpr int NT = kBwdMlaWaves * 64;
    constexpr int BM = kBwdMlaBlockM;
    constexpr int KT = kBwdMlaKTile, VT = kBwdMlaVTile, STAGE = KT + VT;
    constexpr int NSK = HDK / 16, NSV = HDV / 16;
    constexpr int ND = HDK / 32;                      // 32-wide d tiles of dQ^T
    constexpr int CK = HDK / 8, CV = HDV / 8;
    constexpr int KLD = kBlockN * CK / NT, VLD = kBlockN * CV / NT;   // chunks a thread a tile
    static_assert(KLD * NT == kBlockN * CK && VLD * NT == kBlockN * CV, "K / V tile geometry");
    constexpr int RBK = HDK * 16, RBV = HDV * 16;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31;
    const int hh = lane >> 5;

    const int bh = blockIdx.y;
    const int bidx = bh / p.h;
    const int head = bh - bidx * p.h;
    const int hk_i = head / p.group;
    const int m_block = (int)gridDim.x - 1 - (int)blockIdx.x;

    int q_off = 0, sq = p.seqlen_q, k_off = 0, sk = p.seqlen_k;
    if constexpr (PACKED) {
        q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off;
        k_off = p.cu_seqlens_k[bidx]; sk = p.cu_seqlens_k[bidx + 1] - k_off;
    }
    sk = max(sk, 0);
    const int row0 = m_block * BM;
    if (row0 >= sq) return;

    const int diag = sk - sq;
    // Window limits for query position `pos`: keys [lim_l, lim_r)
    auto lim_r = [&](int pos) { return (MASK && p.wr >= 0) ? max(0, min(sk, pos + diag + p.wr + 1)) : sk; };
    auto lim_l = [&](int pos) { return (MASK && p.wl >= 0) ? max(0, pos + diag - p.wl) : 0; };
    // Key-tile range of the whole workgroup
    const int pos_hi = min(row0 + BM, sq) - 1;
    const int n_lo = lim_l(row0);
    const int n_hi = lim_r(pos_hi);
    const int nb_lo = n_lo / kBlockN;
    const int nb_hi = n_hi > n_lo ? (n_hi + kBlockN - 1) / kBlockN : nb_lo;

    // This lane's query row
    const int wrow0 = row0 + wave * 32;
    const int row = wrow0 + lr;
    const bool row_ok = row < sq;
    const int pos = row_ok ? row : 0;
    const bool wave_ok = wrow0 < sq;
    const int wp_hi = min(wrow0 + 32, sq) - 1;
    const int w_lr_min = lim_r(wrow0), w_lr_max = lim_r(wp_hi);
    const int w_ll_min = lim_l(wrow0), w_ll_max = lim_l(wp_hi);
    const int my_lr = lim_r(pos), my_ll = lim_l(pos);
    const float c = p.scale_log2;

    // ---- Q and dO fragments (B operands of S^T = K Q^T and dP^T = V dO^T): lane holds
    // Q[row][16s + 8hh .. +7]; the row's LSE (x log2e; +inf past the end) and D
    V8 qf[NSK], gf[NSV];
    float lse2 = INFINITY, dsum = 0.f;
    {
        const T* qseq = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch + (int64_t)q_off * p.q_row;
        const T* gseq = reinterpret_cast<const T*>(p.dout) + (int64_t)bidx * p.do_batch + (int64_t)q_off * p.do_row;
        const uint32_t qbytes = (uint32_t)(((int64_t)(sq - 1) * p.q_row + (int64_t)(p.h - 1) * p.q_head + HDK) * 2);
        const uint32_t gbytes = (uint32_t)(((int64_t)(sq - 1) * p.do_row + (int64_t)(p.h - 1) * p.do_head + HDV) * 2);
        const __amdgpu_buffer_rsrc_t qr = make_rsrc(qseq, qbytes);
        const __amdgpu_buffer_rsrc_t gr = make_rsrc(gseq, gbytes);
        const int qo = (int)(((int64_t)pos * p.q_row + (int64_t)head * p.q_head) * 2) + 16 * hh;
        const int go = (int)(((int64_t)pos * p.do_row + (int64_t)head * p.do_head) * 2) + 16 * hh;
#pragma unroll
        for (int s = 0; s < NSK; ++s) qf[s] = __builtin_bit_cast(V8, buf_load16(qr, row_ok ? qo + 32 * s : kOOB));
#pragma unroll
        for (int s = 0; s < NSV; ++s) gf[s] = __builtin_bit_cast(V8, buf_load16(gr, row_ok ? go + 32 * s : kOOB));
        if (row_ok) {
            const int64_t li = (int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + q_off + pos;
            lse2 = p.lse[li] * kLog2e;
            dsum = p.dsum[li];
        }
    }

    // ---- K / V of this sequence and kv head: one descriptor each, sized to the sequence
    const char* kseq = reinterpret_cast<const char*>(p.k) +
                       ((int64_t)bidx * p.k_batch + (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head) * 2;
    const char* vseq = reinterpret_cast<const char*>(p.v) +
                       ((int64_t)bidx * p.v_batch + (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head) * 2;
    const uint32_t kbytes = sk > 0 ? (uint32_t)(((int64_t)(sk - 1) * p.k_row + HDK) * 2) : 0u;
    const uint32_t vbytes = sk > 0 ? (uint32_t)(((int64_t)(sk - 1) * p.v_row + HDV) * 2) : 0u;
    const __amdgpu_buffer_rsrc_t krs = make_rsrc(kseq, kbytes);
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(vseq, vbytes);

    // ---- K / V tile loader: KLD + VLD 16-byte chunks a thread, through registers; keys past sk
    // lie past the descriptors (the row pitch is at least a head) and arrive as zeros
    u32x4 kreg[KLD], vreg[VLD];
    auto load_kv = [&](const int nb) {
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            const int idx = tid + i * NT, r = idx / CK, cc = idx - r * CK;
            const int key = nb * kBlockN + r;
            kreg[i] = buf_load16(krs, key < sk ? (int)((uint32_t)key * (uint32_t)p.k_row * 2u) + cc * 16 : kOOB);
        }
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int idx = tid + i * NT, r = idx / CV, cc = idx - r * CV;
            const int key = nb * kBlockN + r;
            vreg[i] = buf_load16(vrs, key < sk ? (int)((uint32_t)key * (uint32_t)p.v_row * 2u) + cc * 16 : kOOB);
        }
    };
    auto store_kv = [&](const int stage) {
        char* k_lds = smem + stage * STAGE;
        char* v_lds = k_lds + KT;
#pragma unroll
        for (int i = 0; i < KLD; ++i) {
            const int idx = tid + i * NT, r = idx / CK, cc = idx - r * CK;
            *reinterpret_cast<u32x4*>(k_lds + kv_off<HDK>(r, cc)) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int idx = tid + i * NT, r = idx / CV, cc = idx - r * CV;
            *reinterpret_cast<u32x4*>(v_lds + kv_off<HDV>(r, cc)) = vreg[i];
        }
    };

    // Per-lane LDS read addresses within a stage (kv_off images, as fwd_mla_item): the K row read
    // of k-step s, 32-key half kt is ka[s & 1] + 4 RBK kt + 512 (s >> 1); the K^T transposing read
    // (kt, sp, dt, part) is kt_[part] + RBK (4 kt + 2 sp) + 512 dt
    const int sbase = (int)(size_t)smem;
    const int q4 = (lane & 15) >> 2;
    int ka[2], va[2], kt_[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ka[u] = sbase + kv_off<HDK>(lr, 2 * u + hh);
        va[u] = sbase + KT + kv_off<HDV>(lr, 2 * u + hh);
        const int r = 8 * u + 4 * hh + q4;
        const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        kt_[u] = sbase + kv_off<HDK>(r, col >> 3) + 8 * ((col >> 2) & 1);
    }
    typedef __attribute__((address_space(3))) V8 lds_v8;

    f32x16 acc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc[dt] = f32x16{};

    if (nb_lo < nb_hi) {
        load_kv(nb_lo);
        store_kv(0);
    }
    __syncthreads();
    for (int nb = nb_lo; nb < nb_hi; ++nb) {
        const int so = ((nb - nb_lo) & 1) * STAGE;
        if (nb + 1 < nb_hi) load_kv(nb + 1);
        const int n0 = nb * kBlockN;
        // a wave skips the tiles none of its rows sees (they would add exact zeros)
        const bool active = wave_ok && n0 < w_lr_max && n0 + kBlockN > w_ll_min;
        if (active) {
            // ---- S^T = K Q^T and dP^T = V dO^T (query on the lane, keys in registers)
            f32x16 st[2] = {f32x16{}, f32x16{}}, dp[2] = {f32x16{}, f32x16{}};
#pragma unroll
            for (int s = 0; s < NSK; ++s)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const V8 a = *(const lds_v8*)(size_t)(ka[s & 1] + so + 4 * RBK * kt + 512 * (s >> 1));
                    st[kt] = DT<T>::mfma32(a, qf[s], st[kt]);
                }
#pragma unroll
            for (int s = 0; s < NSV; ++s)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    const V8 a = *(const lds_v8*)(size_t)(va[s & 1] + so + 4 * RBV * kt + 512 * (s >> 1));
                    dp[kt] = DT<T>::mfma32(a, gf[s], dp[kt]);
                }
            // ---- P = exp2(S c - LSE log2e); edge tiles masked in registers
#pragma unroll
            for (int v = 0; v < 32; ++v) st[v >> 4][v & 15] = fast_exp2(fmaf(st[v >> 4][v & 15], c, -lse2));
            if (n0 + kBlockN > w_lr_min || n0 < w_ll_max) {
#pragma unroll
                for (int v = 0; v < 32; ++v) {
                    const int kt = v >> 4, r = v & 15;
                    const int key = n0 + 4 * hh + 32 * kt + (r & 3) + 8 * (r >> 2);
                    if (key >= my_lr || key < my_ll) st[kt][r] = 0.f;
                }
            }
            // ---- dS^T = P (dP^T - D) -> T: the B operands of dQ^T += K^T dS^T
            V8 sb[4];
#pragma unroll
            for (int v = 0; v < 32; ++v) {
                const int kt = v >> 4, r = v & 15;
                sb[2 * kt + (r >> 3)][r & 7] = (T)(st[kt][r] * (dp[kt][r] - dsum));
            }
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int sp = 0; sp < 2; ++sp)
#pragma unroll
                    for (int dt = 0; dt < ND; ++dt) {
                        const int o = so + RBK * (4 * kt + 2 * sp) + 512 * dt;
                        const V8 a = bwd_mla_tr_read<V8>(kt_[0] + o, kt_[1] + o);
                        acc[dt] = DT<T>::mfma32(a, sb[2 * kt + sp], acc[dt]);
                    }
        }
        // the next tile -> the other stage (last read in the iteration before, a barrier ago)
        if (nb + 1 < nb_hi) store_kv(((nb + 1 - nb_lo) & 1));
        __syncthreads();
    }

    // ---- epilogue: dQ = scale acc -> T; rows without a visible key keep their exact zeros
    if (!row_ok) return;
    T* dqrow = reinterpret_cast<T*>(p.dq) + (int64_t)bidx * p.dq_batch + (int64_t)(q_off + pos) * p.dq_row +
               (int64_t)head * p.dq_head;
    store_o_row16<T, ND>(dqrow, acc, p.scale, HDK, hh);
}

}  // namespace xfa
