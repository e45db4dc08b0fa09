// fmha_fwd_mla_kernel.h — MLA prefill: the forward at head size 192 for Q K^T and 128 for V
// (the un-absorbed form of multi-head latent attention: 128 "nope" + 64 rotary features in q and
// k, a 128-wide v), for gfx950 (CDNA4).  DESIGN.md §3.11.
//
// fwd_item's pipelined (D <= 128) path (fmha_fwd_kernel.h) with two widths instead of one HD:
//   * S^T = K Q^T over HDK = 192 features (NS = 12 k-steps of v_mfma_f32_32x32x16), P straight
//     from the accumulator as the B operand of O^T += V^T P^T over HDV = 128 columns (ND = 4);
//   * the kv_off<192> image for a K tile (64 keys x 384 B = 24 KiB) and the kv_off<128> image for
//     a V tile (16 KiB), both filled by LDS-DMA: 24 + 16 one-KiB pieces a tile pair;
//   * deferred rescale, the two-stage software pipeline over the tiles every row sees and the
//     masked per-wave loop over the tiles that cross the left window edge, as there.
// No FEAT path: no ALiBi, softcap, dropout, paged or fp8 K/V, leftpad, split-KV or sink.
//
// The ring.  fwd_item keeps tile pairs in 4 rotating buffers; four 40 KiB pairs are all of the
// CU's 160 KiB and leave no room for the item queue's claim slots (fwd_claim).  Here K has 4
// buffers and V has 3 (96 + 48 = 144 KiB), and V is issued one tile behind K: step j (tile j's
// softmax and PV, tile j + 1's QK^T) issues K of tile j + 3 into K buffer (j + 3) % 4 (K of
// j - 1, last read in step j - 2) and V of tile j + 2 into V buffer (j + 2) % 3 (V of j - 1, last
// read in step j - 1; the barrier that ends step j - 1 lies between).  The barrier that ends
// step j still waits for everything but step j's own issue, which is then K of j + 2 and V of
// j + 1: what step j + 1 reads.  Buffer numbers are run-time values (two adds a step per
// operand), so the step is unrolled twice (the score ping-pong) and not 12 times.
#pragma once

#include "fmha_common.h"
#include "fmha_fwd_sched.h"

#include <type_traits>

namespace xfa {

constexpr int kMlaHdk = 192;                    // q / k head size
constexpr int kMlaHdv = 128;                    // v / o head size
constexpr int kMlaKBuf = 4, kMlaVBuf = 3;       // ring depths
constexpr int kMlaKTile = kBlockN * kMlaHdk * 2;
constexpr int kMlaVTile = kBlockN * kMlaHdv * 2;
constexpr int kMlaSmem = kMlaKBuf * kMlaKTile + kMlaVBuf * kMlaVTile;
constexpr bool kMlaSchedFence = true;             // pins each MFMA gap's VALU share (fwd_item's SCHED_FENCE)

// One work item = (batch x kv head, query row block).
template <typename T, int NW, bool MASK>
__device__ __forceinline__ void fwd_mla_item(const FwdParams& p, char* smem, const int bh,
                                             const int m_block) {
    using V8 = typename DT<T>::v8;
    constexpr int HDK = kMlaHdk, HDV = kMlaHdv;
    constexpr int BM = NW * 32;
    constexpr int KT = kMlaKTile, VT = kMlaVTile;
    constexpr int VREG = kMlaKBuf * KT;         // LDS: the K buffers, then the V buffers
    constexpr int NS = HDK / 16;                // k-steps of the QK^T product
    constexpr int ND = HDV / 32;                // 32-wide d tiles of O^T
    constexpr int RBK = HDK * 16, RBV = HDV * 16;   // bytes of one 8-row block of each image

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 31;
    const int hh = lane >> 5;

    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;

    int q_off = 0, sq = p.seqlen_q, k_off = 0, sk = p.seqlen_k;
    if (p.cu_seqlens_q) { q_off = p.cu_seqlens_q[bidx]; sq = p.cu_seqlens_q[bidx + 1] - q_off; }
    if (p.cu_seqlens_k) { k_off = p.cu_seqlens_k[bidx]; sk = p.cu_seqlens_k[bidx + 1] - k_off; }
    if (p.seqused_k) sk = p.seqused_k[bidx];
    sk = max(sk, 0);
    const int G = p.group;
    const int rows_total = sq * G;
    const int row0 = m_block * BM;
    if (row0 >= rows_total) return;

    const int diag = sk - sq;
    // Window limits for query position `pos`: keys [lim_l, lim_r).
    auto lim_r = [&](int pos) { return (MASK && p.wr >= 0) ? max(0, min(sk, pos + diag + p.wr + 1)) : sk; };
    auto lim_l = [&](int pos) { return (MASK && p.wl >= 0) ? max(0, pos + diag - p.wl) : 0; };

    // Key-tile range of the whole workgroup.
    const int pos_lo = row0 / G;
    const int pos_hi = (min(row0 + BM, rows_total) - 1) / G;
    const int n_lo = lim_l(pos_lo);
    const int n_hi = lim_r(pos_hi);
    const int nb_lo = n_lo / kBlockN;
    const int nb_hi = n_hi > n_lo ? (n_hi + kBlockN - 1) / kBlockN : nb_lo;

    // This lane's query row.
    const int wrow0 = row0 + wave * 32;
    const int row = wrow0 + lr;
    const bool row_ok = row < rows_total;
    const int pos = row_ok ? row / G : 0;
    const int head = hk_i * G + (row_ok ? row - pos * G : 0);
    const bool wave_ok = wrow0 < rows_total;
    const int wp_lo = wrow0 / G;
    const int wp_hi = (min(wrow0 + 32, rows_total) - 1) / G;
    const int w_lr_min = lim_r(wp_lo), w_lr_max = lim_r(wp_hi);
    const int w_ll_min = lim_l(wp_lo), w_ll_max = lim_l(wp_hi);
    const int my_lr = lim_r(pos), my_ll = lim_l(pos);
    const float c = p.scale_log2;

    // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[row][16s + 8hh .. +7]
    V8 qf[NS];
    {
        const T* qseq = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch + (int64_t)q_off * p.q_row;
        const uint32_t qbytes = (uint32_t)(((int64_t)(sq - 1) * p.q_row + (int64_t)(p.h - 1) * p.q_head + HDK) * 2);
        const __amdgpu_buffer_rsrc_t qr = make_rsrc(qseq, qbytes);
        // (the asm keeps per-column offsets from being hoisted out of the persistent item loop)
        int hh_q = hh;
        asm volatile("" : "+v"(hh_q));
        const int qrow_off = row_ok ? (int)(((int64_t)pos * p.q_row + (int64_t)head * p.q_head) * 2) + 16 * hh_q : kOOB;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = __builtin_bit_cast(V8, buf_load16(qr, qrow_off + 32 * s));
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

    // Per-lane LDS read addresses (kv_off images, as fwd_item): the K row read of k-step s,
    // 32-key half kt is kb[s & 1] + RBK*4*kt + 512*(s >> 1); the V^T transposed read
    // (kt, sp, dt, part) is vb[part] + RBV*(4 kt + 2 sp) + 512 dt.
    const int q4 = (lane & 15) >> 2;
    int kb[2], vb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        kb[u] = (int)(size_t)smem + kv_off<HDK>(lr, 2 * u + hh);
        const int r = 8 * u + 4 * hh + q4;
        const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        vb[u] = (int)(size_t)smem + VREG + kv_off<HDV>(r, col >> 3) + 8 * ((col >> 2) & 1);
    }
    typedef __attribute__((address_space(3))) V8 lds_v8;
    f32x16 acc_o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc_o[dt] = f32x16{};
    // running row max in scaled (log2) units: P = exp2(S c - m_sc); -inf until the row's first
    // visible key
    float m_sc = -INFINITY;
    float l_run = 0.f;

    // ---- the pieces of one 64-key tile (kbo / vbo: byte offset of the K / V buffer)
    auto rd_k = [&](const int kbo, const int s, const int kt) {
        return *(const lds_v8*)(size_t)(kb[s & 1] + kbo + kt * 4 * RBK + 512 * (s >> 1));
    };
    auto mask_tile = [&](f32x16 (&st)[2], const int n0) {
#pragma unroll
        for (int v = 0; v < 32; ++v) {
            const int kt = v >> 4, r = v & 15;
            const int key = n0 + 4 * hh + 32 * kt + (r & 3) + 8 * (r >> 2);
            if (key >= my_lr || key < my_ll) st[kt][r] = -INFINITY;
        }
    };
    // Deferred rescale (fwd_item): the running max only moves once some row's true max exceeds
    // it by more than max_slack (log2 units).
    auto rescale_o = [&](const float alpha) {
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha;
    };
    auto raise_max = [&](const float mx) {
        const float m_new = fmaxf(m_sc, mx * c);
        if (__any(m_new > m_sc + p.max_slack)) {
            rescale_o(m_new == -INFINITY ? 1.f : fast_exp2(m_sc - m_new));
            m_sc = m_new;
        }
    };
    typedef __attribute__((ext_vector_type(2))) float f2;
    typedef typename DT<T>::v2 T2;
    auto exp_ref = [&]() { return (m_sc == -INFINITY) ? 0.f : m_sc; };
    // P = exp2(S c - m_sc) -> T; the row sum accumulates the fp32 P values
    auto exp_tile = [&](const f32x16 (&st)[2], V8 (&pb)[4]) {
        const float mr = exp_ref();
        const f2 c2 = {c, c}, m2 = {mr, mr};
        float rs[2] = {0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 32; v += 2) {
            const int kt = v >> 4, r = v & 15;
            f2 x = {st[kt][r], st[kt][r + 1]};
            x = __builtin_elementwise_fma(x, c2, -m2);
            const float e0 = fast_exp2(x[0]), e1 = fast_exp2(x[1]);
            rs[0] += e0;
            rs[1] += e1;
            const T2 e = {(T)e0, (T)e1};
            pb[2 * kt + (r >> 3)][r & 7] = e[0];
            pb[2 * kt + (r >> 3)][(r & 7) + 1] = e[1];
        }
        l_run += rs[0] + rs[1];
    };
    // S^T = K Q^T (LDS reads one k-step ahead of the MFMAs)
    auto qk = [&](const int kbo, f32x16 (&st)[2]) {
        st[0] = f32x16{};
        st[1] = f32x16{};
        V8 a0 = rd_k(kbo, 0, 0), a1 = rd_k(kbo, 0, 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            V8 n0 = a0, n1 = a1;
            if (s + 1 < NS) { n0 = rd_k(kbo, s + 1, 0); n1 = rd_k(kbo, s + 1, 1); }
            st[0] = DT<T>::mfma32(a0, qf[s], st[0]);
            st[1] = DT<T>::mfma32(a1, qf[s], st[1]);
            a0 = n0;
            a1 = n1;
        }
    };
    constexpr int NPV = 4 * ND;                 // PV MFMAs per tile
    auto row_max = [&](const f32x16 (&st)[2]) {
        float mx = st[0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[0][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[1][r]);
        return wave_max_halves(mx);
    };
    // The pipeline's scores are X = S c - m_sc already: P = exp2(X) -> T for values [v0, v0 + n)
    auto expx_part = [&](const f32x16 (&st)[2], V8 (&pb)[4], float& rs, const int v0, const int n) {
#pragma unroll
        for (int v = v0; v < v0 + n; v += 2) {
            const int kt = v >> 4, r = v & 15;
            const float e0 = fast_exp2(st[kt][r]), e1 = fast_exp2(st[kt][r + 1]);
            rs += e0;
            rs += e1;
            const T2 e = {(T)e0, (T)e1};
            pb[2 * kt + (r >> 3)][r & 7] = e[0];
            pb[2 * kt + (r >> 3)][(r & 7) + 1] = e[1];
        }
    };
    // Deferred rescale on pipeline scores: mx = this row's max of X = S c - m_sc over the new
    // tile.  Rows still at m_sc = -inf had X computed against 0 (exp_ref) and take m_sc = mx.
    auto rescale_x = [&](const float mx, f32x16 (&sx)[2]) {
        const bool fresh = m_sc == -INFINITY;
        if (__any(mx > p.max_slack || (fresh && mx != -INFINITY))) {
            // a volatile asm cannot be speculated: keeps the rare rescale a real branch
            asm volatile("; rescale_x");
            const float delta = fresh ? (mx == -INFINITY ? 0.f : mx) : fmaxf(mx, 0.f);
            rescale_o(fresh ? 1.f : fast_exp2(-delta));
#pragma unroll
            for (int v = 0; v < 32; ++v) sx[v >> 4][v & 15] -= delta;
            m_sc = fresh ? (mx == -INFINITY ? -INFINITY : mx) : m_sc + delta;
        }
    };

    // V^T operand through inline-asm transposing reads (the compiler's waitcnt pass treats the
    // ds_read_tr builtin as aliasing every in-flight LDS-DMA and would drain the DMA queue before
    // it); covered by explicit lgkmcnt waits.  Base registers vbj = vb + the V buffer's offset,
    // OFF (the operand within the tile) an immediate.
    auto rd_v_asm = [&](const int (&vbj)[2], auto OFF) {
        constexpr int off = decltype(OFF)::value;
        s16x4 t0, t1;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t0) : "v"(vbj[0]), "i"(off));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t1) : "v"(vbj[1]), "i"(off));
        const s16x8 av = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        return __builtin_bit_cast(V8, av);
    };
    auto lgkm_wait = [&](auto N) {
        constexpr int n = decltype(N)::value;
        __builtin_amdgcn_s_waitcnt(0xC07F | (n << 8));
        // the MFMA consuming the asm-read registers must not be scheduled above the wait
        __builtin_amdgcn_sched_barrier(0);
    };
    auto voffs = [&](auto I) {                     // immediate offset of PV operand I in a V tile
        constexpr int i = decltype(I)::value;
        return std::integral_constant<int, (4 * (i / (2 * ND)) + 2 * ((i / ND) & 1)) * RBV + 512 * (i % ND)>{};
    };
    // O^T += V^T P^T of one tile, V^T read two MFMAs ahead; `beside(I)` runs after MFMA I
    auto pv_asm = [&](const int vbo, const V8 (&pb)[4], auto&& beside) {
        const int vbj[2] = {vb[0] + vbo, vb[1] + vbo};
        V8 ring[3];
        ring[0] = rd_v_asm(vbj, voffs(std::integral_constant<int, 0>{}));
        ring[1] = rd_v_asm(vbj, voffs(std::integral_constant<int, 1>{}));
        static_for<NPV>([&](auto I) {
            constexpr int i = decltype(I)::value;
            if constexpr (i + 2 < NPV) {
                ring[(i + 2) % 3] = rd_v_asm(vbj, voffs(std::integral_constant<int, i + 2>{}));
                lgkm_wait(std::integral_constant<int, 4>{});
            } else if constexpr (i + 1 < NPV) {
                lgkm_wait(std::integral_constant<int, 2>{});
            } else {
                lgkm_wait(std::integral_constant<int, 0>{});
            }
            acc_o[i % ND] = DT<T>::mfma32(ring[i % 3], pb[i / ND], acc_o[i % ND]);
            beside(I);
        });
    };

    // ---- LDS-DMA: a K tile is 24 one-KiB pieces (8 rows x 8 chunks of the kv_off<192> image,
    // three pieces an 8-row block), a V tile 16 (two an 8-row block); lane l of a
    // wave-instruction lands at +16 l, so it fetches chunk 8 (g % PPB) + 4 (l >> 5) +
    // ((l & 3) ^ swz(row)) of row 8 (g / PPB) + (l & 31) / 4.
    constexpr int IPK = KT / 1024 / NW, IPV = VT / 1024 / NW;   // wave-instructions per wave per tile
    static_assert(IPK * 1024 * NW == KT && IPV * 1024 * NW == VT, "DMA geometry");
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int dma_k[IPK], dma_v[IPV];                    // per-lane byte offsets within a tile
#pragma unroll
    for (int i = 0; i < IPK; ++i) {
        constexpr int PPB = HDK / 64;
        const int g = wave * IPK + i;
        const int r = 8 * (g / PPB) + (lane & 31) / 4;
        const int cch = 8 * (g % PPB) + 4 * (lane >> 5) + ((lane & 3) ^ ((r >> 2) & 3));
        dma_k[i] = r * (int)p.k_row * 2 + cch * 16;
    }
#pragma unroll
    for (int i = 0; i < IPV; ++i) {
        constexpr int PPB = HDV / 64;
        const int g = wave * IPV + i;
        const int r = 8 * (g / PPB) + (lane & 31) / 4;
        const int cch = 8 * (g % PPB) + 4 * (lane >> 5) + ((lane & 3) ^ ((r >> 2) & 3));
        dma_v[i] = r * (int)p.v_row * 2 + cch * 16;
    }
    typedef __attribute__((address_space(3))) void lds_void;
    // (soffset pinned to an SGPR; rows past the sequence's end are past the descriptor: zeros)
    auto dma_k_tile = [&](const int nb, const int kbo) {
        const int so = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.k_row * 2);
#pragma unroll
        for (int i = 0; i < IPK; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                krs, (lds_void*)(smem + kbo + (wave_u * IPK + i) * 1024), 16, dma_k[i], so, 0, 0);
    };
    auto dma_v_tile = [&](const int nb, const int vbo) {
        const int so = __builtin_amdgcn_readfirstlane(nb * kBlockN * (int)p.v_row * 2);
#pragma unroll
        for (int i = 0; i < IPV; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                vrs, (lds_void*)(smem + VREG + vbo + (wave_u * IPV + i) * 1024), 16, dma_v[i], so, 0, 0);
    };
    // counted vmcnt (the DMA writes are invisible to the compiler's waitcnt tracking: `left`
    // vmem instructions may stay in flight) + a barrier that the compiler may not move memory
    // operations across
    auto publish = [&](const int left) {
        if (left == IPK + IPV) __builtin_amdgcn_s_waitcnt(waitcnt_vm(IPK + IPV));
        else if (left == IPV) __builtin_amdgcn_s_waitcnt(waitcnt_vm(IPV));
        else __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // ---- tiles that need per-wave masking / skipping (the left window edge, or a range too
    // short for the pipeline): one tile pair in flight, K / V buffers 0 and 1
    auto masked_range = [&](const int lo, const int hi) {
        if (lo >= hi) return;
        dma_k_tile(lo, 0);
        dma_v_tile(lo, 0);
        publish(0);
        int buf = 0;
        for (int nb = lo; nb < hi; ++nb) {
            if (nb + 1 < hi) {
                dma_k_tile(nb + 1, (buf ^ 1) * KT);
                dma_v_tile(nb + 1, (buf ^ 1) * VT);
            }
            const int n0 = nb * kBlockN;
            const bool active = wave_ok && n0 < w_lr_max && n0 + kBlockN > w_ll_min;
            if (active) {
                f32x16 st[2];
                qk(buf * KT, st);
                if ((n0 + kBlockN > w_lr_min) || (n0 < w_ll_max)) mask_tile(st, n0);
                raise_max(row_max(st));
                V8 pb[4];
                exp_tile(st, pb);
                pv_asm(buf * VT, pb, [](auto) {});
            }
            publish(0);
            buf ^= 1;
        }
    };

    // ---- tiles every row of the workgroup sees from their left end: two-stage software
    // pipeline (fwd_item's pipe_range).  Tiles [lo, hm) need no mask; tiles [hm, hi) (the causal
    // diagonal / right window edge / ragged end) are masked in registers on the way through.
    const int lim_e = my_lr - 4 * hh;            // right edge of this lane's keys, minus its offset
    auto pipe_range = [&](const int lo, const int hm, const int hi) {
        const bool third = lo + 2 < hi;
        dma_k_tile(lo, 0);
        dma_v_tile(lo, 0);
        dma_k_tile(lo + 1, KT);
        if (third) dma_k_tile(lo + 2, 2 * KT);
        dma_v_tile(lo + 1, VT);
        publish(third ? IPK + IPV : 0);
        f32x16 sa[2], sb[2];
        qk(0, sa);
        if (lo >= hm) mask_tile(sa, lo * kBlockN);
        raise_max(row_max(sa));
        {
            const float mr = exp_ref();
#pragma unroll
            for (int v = 0; v < 32; ++v) sa[v >> 4][v & 15] = __builtin_fmaf(sa[v >> 4][v & 15], c, -mr);
        }
        const int nsteps = hi - lo - 1;
        // step r (tile j = lo + r): issues K of j + 3 and V of j + 2; returns what it left in flight
        auto issue = [&](const int r) {
            const int j = lo + r;
            int left = 0;
            if (j + 3 < hi) { dma_k_tile(j + 3, ((r + 3) & 3) * KT); left += IPK; }
            if (j + 2 < hi) { dma_v_tile(j + 2, ((r + 2) % 3) * VT); left += IPV; }
            return left;
        };
        auto step = [&](const int r, f32x16 (&st)[2], f32x16 (&sn)[2]) {
            const int j = lo + r;
            const int left = issue(r);
            const int kbo = __builtin_amdgcn_readfirstlane(((r + 1) & 3) * KT);
            const int vbo = __builtin_amdgcn_readfirstlane((r % 3) * VT);
            if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            // phase a: S_{j+1} = K_{j+1} Q^T on the MFMA pipe, P_j = exp2(X_j) -> T on the VALU
            sn[0] = f32x16{};
            sn[1] = f32x16{};
            V8 pb[4];
            float rs = 0.f;                       // fp32 row sum of P_j
            // 32 values over 2 NS = 24 MFMAs, in pairs: the first 16 MFMAs take one pair each
            V8 a0 = rd_k(kbo, 0, 0), a1 = rd_k(kbo, 0, 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                V8 n0 = a0, n1 = a1;
                if (s + 1 < NS) { n0 = rd_k(kbo, s + 1, 0); n1 = rd_k(kbo, s + 1, 1); }
                sn[0] = DT<T>::mfma32(a0, qf[s], sn[0]);
                if (2 * s < 16) expx_part(st, pb, rs, 4 * s, 2);
                sn[1] = DT<T>::mfma32(a1, qf[s], sn[1]);
                if (2 * s + 1 < 16) expx_part(st, pb, rs, 4 * s + 2, 2);
                // pins the row-sum adds into this MFMA gap
                asm volatile("" : "+v"(rs));
                a0 = n0;
                a1 = n1;
                if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            }
            // phase b: O += V_j^T P_j on the MFMA pipe; on the VALU X_{j+1} = S_{j+1} c - m_sc
            // and its row max
            constexpr int MV = 32 / NPV;          // score values per PV MFMA
            const float mr = exp_ref();
            float mx = -INFINITY;
            pv_asm(vbo, pb, [&](auto I) {
                constexpr int i = decltype(I)::value;
#pragma unroll
                for (int v = i * MV; v < (i + 1) * MV; ++v) {
                    sn[v >> 4][v & 15] = __builtin_fmaf(sn[v >> 4][v & 15], c, -mr);
                    mx = fmaxf(mx, sn[v >> 4][v & 15]);
                }
                if (kMlaSchedFence) __builtin_amdgcn_sched_barrier(0);
            });
            // an opaque use pins the max chain inside phase b
            asm volatile("" : "+v"(mx));
            l_run += rs;
            if (j + 1 >= hm) {                    // edge tile: mask, then the row max again
                const int lim_t = lim_e - (j + 1) * kBlockN;
                float mm = -INFINITY;
#pragma unroll
                for (int v = 0; v < 32; ++v) {
                    const int off = 32 * (v >> 4) + ((v & 15) & 3) + 8 * ((v & 15) >> 2);
                    if (off >= lim_t) sn[v >> 4][v & 15] = -INFINITY;
                    mm = fmaxf(mm, sn[v >> 4][v & 15]);
                }
                mx = mm;
            }
            // the decision needs no row max: some lane's half-row max passes the slack iff some
            // row's does, so the halves are combined only on the (rare) rescale path
            if (__any(mx > p.max_slack || (m_sc == -INFINITY && mx != -INFINITY)))
                rescale_x(wave_max_halves(mx), sn);
            publish(left);                        // K of j + 2 and V of j + 1 landed everywhere
        };
        // Causal diagonal / right window edge: a wave stops after the last tile any of its rows
        // sees, drains it, then only issues its DMA share and joins the barriers for the rest of
        // the workgroup's steps (the skipped tiles would add exact zeros).
        const int t_w = __builtin_amdgcn_readfirstlane((w_lr_max + kBlockN - 1) / kBlockN - 1);
        const int nsteps_w = __builtin_amdgcn_readfirstlane(wave_ok ? max(0, min(nsteps, t_w - lo)) : nsteps);
        int r = 0;
        while (r < nsteps_w) {
            step(r, sa, sb);
            if (++r >= nsteps_w) break;
            step(r, sb, sa);
            ++r;
        }
        // drain: the wave's last tile's softmax and PV
        V8 pb[4];
        {
            float rs = 0.f;
            if (nsteps_w & 1) expx_part(sb, pb, rs, 0, 32);
            else expx_part(sa, pb, rs, 0, 32);
            l_run += rs;
        }
        pv_asm(__builtin_amdgcn_readfirstlane((nsteps_w % 3) * VT), pb, [](auto) {});
        // the steps this wave skips: its DMA share and the barriers only
        for (; r < nsteps; ++r) publish(issue(r));
        __syncthreads();
    };
    // Key tiles: [nb_lo, f_lo) cross the left window edge (per-wave masked loop); the rest run
    // through the pipeline, [f_hi, nb_hi) of them masked (the right window edge / the end of
    // the keys).  Every row sees tile f_lo, and visible keys are contiguous.
    // (fwd_pipe = 2, fwd_item's A/B setting for its edge tiles, runs the pipeline here as 1 does)
    int f_lo = nb_hi, f_hi = nb_hi;
    if (p.pipe) {
        const int ll_max = lim_l(pos_hi), lr_min = lim_r(pos_lo);
        f_lo = max(nb_lo, (ll_max + kBlockN - 1) / kBlockN);
        f_hi = max(f_lo, min(nb_hi, lr_min / kBlockN));
        if (nb_hi - f_lo < 2) f_lo = f_hi = nb_hi;
    }
    if (p.prio_hi && __builtin_amdgcn_readfirstlane(wave) >= NW / 2) __builtin_amdgcn_s_setprio(1);
    masked_range(nb_lo, f_lo);
    if (f_lo < nb_hi) pipe_range(f_lo, f_hi, nb_hi);

    // ---- epilogue: normalise, write O and LSE
    const float l_full = wave_sum_halves(l_run);
    const bool empty = (l_full == 0.f) || (l_full != l_full);
    const float inv = empty ? 1.f : 1.f / l_full;
    if (!row_ok) return;
    T* orow = reinterpret_cast<T*>(p.o) + (int64_t)bidx * p.o_batch +
              (int64_t)(q_off + pos) * p.o_row + (int64_t)head * p.o_head;
    store_o_row16<T, ND>(orow, acc_o, inv, HDV, hh);
    if (p.lse && hh == 0) {
        p.lse[(int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + q_off + pos] =
            empty ? INFINITY : (m_sc + __log2f(l_full)) * kLn2;
    }
}

constexpr FwdQueue kFwdMlaQueue = kQueueXcd;   // for plan_fwd and fwd_walk
template <typename T, int NW, bool MASK>
__global__ void __launch_bounds__(NW * 64, NW / 4) fmha_fwd_mla_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fwd_walk<kFwdMlaQueue>(p, [&](int bh, int m_block) { fwd_mla_item<T, NW, MASK>(p, smem, bh, m_block); });
}

}  // namespace xfa
