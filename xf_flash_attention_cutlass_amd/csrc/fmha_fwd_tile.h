// fmha_fwd_tile.h — what the compiler-scheduled forward items share under their pipelines:
// fwd_item (fmha_fwd_kernel.h) and fwd_mla_item (fmha_fwd_mla_kernel.h) all of it, fwd8_item
// (fmha_fwd_fp8_kernel.h) the row geometry and the O / LSE store.  Here: the key-tile bounds of
// a workgroup, a wave and a lane's row; the per-row softmax state with the deferred rescale; the
// pieces of one 64-key tile in the 32x32x16 layout (Q fragments, K row reads of a kv_off image,
// S^T = K Q^T, edge masks, row max, exp); the asm transposing V^T read ring of the PV product;
// the LDS-DMA piece offsets and the counted publish; the epilogue.  What differs per kernel
// stays in its own file: the buffer rings and their schedules (which tile is issued, read and
// retired when, SCHED_FENCE / kMlaSchedFence), the score features, leftpad, split-KV, sink,
// dropout, and the fp8 operands and softmax.
#pragma once

#include "fmha_common.h"

#include <climits>
#include <type_traits>

namespace xfa {

// ---- 1. Row geometry.  Rows are packed (row = pos * G + g); a workgroup owns rows [row0, row0
// + BM), a wave 32 of them, lane l and l ^ 32 the row wrow0 + (l & 31).
// floor_r: the least value lim_r returns: 0 in fwd_mla_item, kNoFloor (which folds away) in the
// callers that do not clamp.
constexpr int kNoFloor = INT_MIN;
template <bool MASK>
struct RowGeom {
    int sk, diag, wl, wr, floor_r;
    int pos_lo, pos_hi;                          // first and last query position of the workgroup
    int nb_lo, nb_hi;                            // key-tile range of the whole workgroup
    bool row_ok, wave_ok;
    int pos, head;                               // this lane's query row
    int w_lr_min, w_lr_max, w_ll_min, w_ll_max;  // the limits over the wave's rows
    int my_lr, my_ll;                            // this lane's keys: [my_ll, my_lr)

    // Window limits for query position `pos`: keys [lim_l, lim_r).
    __device__ __forceinline__ int lim_r(const int pos) const {
        return (MASK && wr >= 0) ? max(floor_r, min(sk, pos + diag + wr + 1)) : sk;
    }
    __device__ __forceinline__ int lim_l(const int pos) const { return (MASK && wl >= 0) ? max(0, pos + diag - wl) : 0; }

    // (the caller has returned already where row0 >= sq * G)
    __device__ __forceinline__ RowGeom(const FwdParams& p, const int sq, const int sk_, const int G, const int hk_i,
                                       const int row0, const int BM, const int wave, const int lr, const int floor_r_)
        : sk(sk_), diag(sk_ - sq), wl(p.wl), wr(p.wr), floor_r(floor_r_) {
        const int rows_total = sq * G;
        pos_lo = row0 / G;
        pos_hi = (min(row0 + BM, rows_total) - 1) / G;
        const int n_lo = lim_l(pos_lo);
        const int n_hi = lim_r(pos_hi);
        nb_lo = n_lo / kBlockN;
        nb_hi = n_hi > n_lo ? (n_hi + kBlockN - 1) / kBlockN : nb_lo;
        const int wrow0 = row0 + wave * 32;
        const int row = wrow0 + lr;
        row_ok = row < rows_total;
        pos = row_ok ? row / G : 0;
        head = hk_i * G + (row_ok ? row - pos * G : 0);
        wave_ok = wrow0 < rows_total;
        const int wp_lo = wrow0 / G;
        const int wp_hi = (min(wrow0 + 32, rows_total) - 1) / G;
        w_lr_min = lim_r(wp_lo), w_lr_max = lim_r(wp_hi);
        w_ll_min = lim_l(wp_lo), w_ll_max = lim_l(wp_hi);
        my_lr = lim_r(pos), my_ll = lim_l(pos);
    }
    // the tile at key n0: does any row of the wave see it; does a window edge cross it
    __device__ __forceinline__ bool active(const int n0) const { return wave_ok && n0 < w_lr_max && n0 + kBlockN > w_ll_min; }
    __device__ __forceinline__ bool edge(const int n0) const { return (n0 + kBlockN > w_lr_min) || (n0 < w_ll_max); }
    // Key tiles of [lo, hi) (the workgroup's, or a split's share): [lo, f_lo) cross the left
    // window edge (a per-wave masked loop); [f_lo, f_hi) every row of the workgroup sees in
    // full; [f_hi, hi) cross the right window edge / the end of the keys.  The last two ranges
    // can run through a pipeline (every row sees tile f_lo, and visible keys are contiguous);
    // one shorter than two tiles is not worth its prologue.
    __device__ __forceinline__ void pipe_split(const int lo, const int hi, int& f_lo, int& f_hi) const {
        const int ll_max = lim_l(pos_hi), lr_min = lim_r(pos_lo);
        f_lo = max(lo, (ll_max + kBlockN - 1) / kBlockN);
        f_hi = max(f_lo, min(hi, lr_min / kBlockN));
        if (hi - f_lo < 2) f_lo = f_hi = hi;
    }
    // Causal diagonal / right window edge: a wave stops after the last tile t_w any of its rows
    // sees (visible keys are contiguous): of a pipeline's `nsteps` steps from tile lo it runs
    // steps_w, drains, then only issues its DMA share and joins the barriers for the rest of
    // the workgroup's steps (the same barrier count).  The skipped tiles would add exact zeros,
    // so results are bit-identical, and the wave's SIMD partner gets the whole issue port
    // meanwhile.
    __device__ __forceinline__ int steps_w(const int nsteps, const int lo) const {
        const int t_w = __builtin_amdgcn_readfirstlane((w_lr_max + kBlockN - 1) / kBlockN - 1);
        return __builtin_amdgcn_readfirstlane(wave_ok ? max(0, min(nsteps, t_w - lo)) : nsteps);
    }
};

// ---- 2. Per-row softmax state (one query row per lane; lanes l and l ^ 32 each hold half of
// the row's keys and of O's columns) and its moves.
struct RowNorm { float l_full; bool empty; float inv; };
template <int ND>
struct SoftmaxRow {
    f32x16 acc_o[ND];
    // running row max in scaled (log2) units: P = exp2(S c - m_sc); -inf until the row's first
    // visible key
    float m_sc = -INFINITY;
    float l_run = 0.f;
    __device__ __forceinline__ SoftmaxRow() {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) acc_o[dt] = f32x16{};
    }
    // Deferred rescale: the running max m_sc (the exp reference) only moves once some row's
    // true max exceeds it by more than `slack` (log2 units), so P = exp2(S c - m_sc) stays
    // below 2^slack; O, l and the LSE are all relative to the same m_sc, so the result is
    // unchanged up to rounding (the relative rounding of P in T does not depend on the scale).
    __device__ __forceinline__ void rescale_o(const float alpha) {
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha;
    }
    __device__ __forceinline__ void raise_max(const float mx, const float c, const float slack) {
        const float m_new = fmaxf(m_sc, mx * c);
        if (__any(m_new > m_sc + slack)) {
            rescale_o(m_new == -INFINITY ? 1.f : fast_exp2(m_sc - m_new));
            m_sc = m_new;
        }
    }
    __device__ __forceinline__ float exp_ref() const { return (m_sc == -INFINITY) ? 0.f : m_sc; }
    // Deferred rescale on pipeline scores: mx = this row's max of X = S c - m_sc over the new
    // tile.  Rows still at m_sc = -inf had X computed against 0 (exp_ref) and take m_sc = mx.
    __device__ __forceinline__ void rescale_x(const float mx, f32x16 (&sx)[2], const float slack) {
        const bool fresh = m_sc == -INFINITY;
        if (__any(mx > slack || (fresh && mx != -INFINITY))) {
            // a volatile asm cannot be speculated: keeps the rare rescale a real branch
            // (if-converted it costs 64 VALU on every tile)
            asm volatile("; rescale_x");
            const float delta = fresh ? (mx == -INFINITY ? 0.f : mx) : fmaxf(mx, 0.f);
            rescale_o(fresh ? 1.f : fast_exp2(-delta));
#pragma unroll
            for (int v = 0; v < 32; ++v) sx[v >> 4][v & 15] -= delta;
            m_sc = fresh ? (mx == -INFINITY ? -INFINITY : mx) : m_sc + delta;
        }
    }
    // ... from a lane's half-row max mxh.  The decision needs no row max: some lane's half-row
    // max passes the slack iff some row's does, so the halves are combined only on the (rare)
    // rescale path
    __device__ __forceinline__ void rescale_x_halves(const float mxh, f32x16 (&sx)[2], const float slack) {
        if (__any(mxh > slack || (m_sc == -INFINITY && mxh != -INFINITY))) rescale_x(wave_max_halves(mxh), sx, slack);
    }
    // ---- 6. Epilogue: the row sum, the empty-row rule (no visible key, or NaN) and 1 / l;
    // the LSE in natural units (+inf for an empty row, the reference's output)
    __device__ __forceinline__ RowNorm norm() const {
        const float l_full = wave_sum_halves(l_run);
        const bool empty = (l_full == 0.f) || (l_full != l_full);
        return RowNorm{l_full, empty, empty ? 1.f : 1.f / l_full};
    }
    __device__ __forceinline__ float lse(const RowNorm& n) const { return n.empty ? INFINITY : (m_sc + __log2f(n.l_full)) * kLn2; }
};
// O row (columns < d) scaled by inv, and the row's LSE, of query (bidx, q_off + pos, head)
template <typename T, int ND>
__device__ __forceinline__ void store_row(const FwdParams& p, const int bidx, const int q_off, const int pos, const int head,
                                          const int hh, const f32x16 (&acc_o)[ND], const float inv, const int d, const float lse) {
    T* orow = reinterpret_cast<T*>(p.o) + (int64_t)bidx * p.o_batch + (int64_t)(q_off + pos) * p.o_row + (int64_t)head * p.o_head;
    store_o_row16<T, ND>(orow, acc_o, inv, d, hh);
    if (p.lse && hh == 0) p.lse[(int64_t)bidx * p.lse_batch + (int64_t)head * p.lse_head + q_off + pos] = lse;
}

// ---- 3. Tile pieces.  A 64-key score tile is st[2] (32-key halves kt), flattened v = 16 kt + r;
// the lane with half hh holds the keys 4 hh + key_of(v) of its row.
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ constexpr int key_of(const int v) { return 32 * (v >> 4) + (v & 3) + 8 * ((v & 15) >> 2); }

// Q fragments (B operand of S^T = K Q^T): lane holds Q[row][16s + 8hh .. +7].  The descriptor
// covers this sequence's rows (d features each); a lane past them reads zeros.
struct QRow { __amdgpu_buffer_rsrc_t rsrc; int off, hh_q; };
template <typename T>
__device__ __forceinline__ QRow q_row(const FwdParams& p, const int bidx, const int q_off, const int sq, const int d,
                                      const bool row_ok, const int pos, const int head, const int hh) {
    const T* qseq = reinterpret_cast<const T*>(p.q) + (int64_t)bidx * p.q_batch + (int64_t)q_off * p.q_row;
    const uint32_t qbytes = (uint32_t)(((int64_t)(sq - 1) * p.q_row + (int64_t)(p.h - 1) * p.q_head + d) * 2);
    // column part as an immediate offset; the asm keeps per-column offsets from being
    // hoisted out of the persistent item loop (and spilled)
    int hh_q = hh;
    asm volatile("" : "+v"(hh_q));
    return QRow{make_rsrc(qseq, qbytes), row_ok ? (int)(((int64_t)pos * p.q_row + (int64_t)head * p.q_head) * 2) + 16 * hh_q : kOOB, hh_q};
}
template <typename V8, int NS>
__device__ __forceinline__ void q_frags(const QRow& q, V8 (&qf)[NS]) {          // d = 16 NS
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = __builtin_bit_cast(V8, buf_load16(q.rsrc, q.off + 32 * s));
}
template <typename V8, int NS>
__device__ __forceinline__ void q_frags(const QRow& q, V8 (&qf)[NS], const int d) {   // d <= 16 NS: zeros past d
    const bool full_d = d == 16 * NS;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int off = (full_d || 16 * s + 8 * q.hh_q < d) ? q.off : kOOB;
        qf[s] = __builtin_bit_cast(V8, buf_load16(q.rsrc, off + 32 * s));
    }
}

// Per-lane LDS read addresses (kv_off<HD> image at LDS address `base`): the K row read of
// k-step s, 32-key half kt is kb[s & 1] + RB*4*kt + 512*(s >> 1) (RB = 16 HD, the bytes of an
// 8-row block); the V^T transposed read (kt, sp, dt, part) is vb[part] + RB*(4 kt + 2 sp) +
// 512 dt.  Everything but the two base registers of each operand is an immediate offset of
// the ds_read (plus, in fwd_mla_item, the buffer's run-time offset).
template <int HD>
__device__ __forceinline__ void k_read_bases(const int base, const int lane, int (&kb)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) kb[u] = base + kv_off<HD>(lane & 31, 2 * u + (lane >> 5));
}
template <int HD>
__device__ __forceinline__ void v_read_bases(const int base, const int lane, int (&vb)[2]) {
    const int q4 = (lane & 15) >> 2;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = 8 * u + 4 * (lane >> 5) + q4;
        const int col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        vb[u] = base + kv_off<HD>(r, col >> 3) + 8 * ((col >> 2) & 1);
    }
}
// K operand of S^T = K Q^T for k-step s, 32-key half `kt`, read row-wise from the kv_off<HD>
// image at byte offset `bo` past the read bases
template <typename T, int HD>
__device__ __forceinline__ typename DT<T>::v8 rd_k(const int (&kb)[2], const int bo, const int s, const int kt) {
    typedef __attribute__((address_space(3))) typename DT<T>::v8 lds_v8;
    return *(const lds_v8*)(size_t)(kb[s & 1] + bo + kt * 4 * (HD * 16) + 512 * (s >> 1));
}
// S^T = K Q^T (LDS reads one k-step ahead of the MFMAs)
template <typename T, int HD>
__device__ __forceinline__ void qk(const int (&kb)[2], const int bo, const typename DT<T>::v8 (&qf)[HD / 16], f32x16 (&st)[2]) {
    typedef typename DT<T>::v8 V8;
    constexpr int NS = HD / 16;
    st[0] = f32x16{};
    st[1] = f32x16{};
    V8 a0 = rd_k<T, HD>(kb, bo, 0, 0), a1 = rd_k<T, HD>(kb, bo, 0, 1);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        V8 n0 = a0, n1 = a1;
        if (s + 1 < NS) { n0 = rd_k<T, HD>(kb, bo, s + 1, 0); n1 = rd_k<T, HD>(kb, bo, s + 1, 1); }
        st[0] = DT<T>::mfma32(a0, qf[s], st[0]);
        st[1] = DT<T>::mfma32(a1, qf[s], st[1]);
        a0 = n0;
        a1 = n1;
    }
}
// The edge mask of values [v0, v0 + n) of the tile at key n0: -inf outside the lane's keys
// [my_ll, my_lr).  (fwd_item's transform_part runs its score features before it.)
__device__ __forceinline__ void edge_mask(f32x16 (&st)[2], const int n0, const int hh, const int my_lr, const int my_ll,
                                          const int v0 = 0, const int n = 32) {
#pragma unroll
    for (int v = v0; v < v0 + n; ++v) {
        const int key = n0 + 4 * hh + key_of(v);
        if (key >= my_lr || key < my_ll) st[v >> 4][v & 15] = -INFINITY;
    }
}
// The right-edge mask inside a pipeline (no left edge there): values at key offsets >= lim_t =
// my_lr - 4 hh - n0, then the lane's half-row max again
__device__ __forceinline__ float right_mask_max(f32x16 (&sn)[2], const int lim_t) {
    float mm = -INFINITY;
#pragma unroll
    for (int v = 0; v < 32; ++v) {
        if (key_of(v) >= lim_t) sn[v >> 4][v & 15] = -INFINITY;
        mm = fmaxf(mm, sn[v >> 4][v & 15]);
    }
    return mm;
}
__device__ __forceinline__ float row_max(const f32x16 (&st)[2]) {
    float mx = st[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[1][r]);
    return wave_max_halves(mx);
}
// X = S c - mr of the whole tile (a pipeline's first tile; the later ones beside their PV)
__device__ __forceinline__ void scale_shift(f32x16 (&st)[2], const float c, const float mr) {
#pragma unroll
    for (int v = 0; v < 32; ++v) st[v >> 4][v & 15] = __builtin_fmaf(st[v >> 4][v & 15], c, -mr);
}
// P = exp2(S c - mr) -> T (the B operand of the PV product) for values [v0, v0 + n);
// the row sum accumulates the fp32 P values, as the reference's softmax does
// (softmax_hip.h:129-189), so the LSE is the fp32 log-sum-exp of the scores.  (Summing the
// rounded bf16 pairs with v_dot2c instead costs ~14 cycles a pair beside the MFMAs and moves
// the LSE by up to the bf16 unit roundoff, 2^-9; the fp32 adds fit the register budget only
// with the two-base kv_off image.)
template <typename T>
__device__ __forceinline__ void exp_part(const f32x16 (&st)[2], typename DT<T>::v8 (&pb)[4], const float c, const float mr,
                                         float (&rs)[2], const int v0, const int n) {
    typedef typename DT<T>::v2 T2;
    const f32x2 c2 = {c, c}, m2 = {mr, mr};
#pragma unroll
    for (int v = v0; v < v0 + n; v += 2) {
        const int kt = v >> 4, r = v & 15;
        f32x2 x = {st[kt][r], st[kt][r + 1]};
        x = __builtin_elementwise_fma(x, c2, -m2);
        const float e0 = fast_exp2(x[0]), e1 = fast_exp2(x[1]);
        rs[0] += e0;
        rs[1] += e1;
        const T2 e = {(T)e0, (T)e1};
        pb[2 * kt + (r >> 3)][r & 7] = e[0];
        pb[2 * kt + (r >> 3)][(r & 7) + 1] = e[1];
    }
}
template <typename T, int ND>
__device__ __forceinline__ void exp_tile(SoftmaxRow<ND>& sm, const f32x16 (&st)[2], typename DT<T>::v8 (&pb)[4], const float c) {
    float rs[2] = {0.f, 0.f};
    exp_part<T>(st, pb, c, sm.exp_ref(), rs, 0, 32);
    sm.l_run += rs[0] + rs[1];
}
// The pipeline's scores are X = S c - m_sc already: P = exp2(X) -> T for values [v0, v0 + n)
template <typename T>
__device__ __forceinline__ void expx_part(const f32x16 (&st)[2], typename DT<T>::v8 (&pb)[4], float& rs, const int v0, const int n) {
    typedef typename DT<T>::v2 T2;
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
}
template <typename T, int ND>
__device__ __forceinline__ void expx_tile(SoftmaxRow<ND>& sm, const f32x16 (&st)[2], typename DT<T>::v8 (&pb)[4]) {
    float rs = 0.f;
    expx_part<T>(st, pb, rs, 0, 32);
    sm.l_run += rs;
}

// ---- 4. The V^T operand through inline-asm transposing reads: the compiler's waitcnt pass
// treats the ds_read_tr builtin as aliasing every in-flight LDS-DMA and would drain the DMA
// queue (vmcnt(0)) before it; the asm reads are covered by explicit lgkmcnt waits instead.
// vb: the two base registers (v_read_bases, plus a run-time buffer offset where the caller has
// one); byte offset OFF (buffer + row block) is an immediate.
template <typename T, int OFF>
__device__ __forceinline__ typename DT<T>::v8 rd_v_asm(const int (&vb)[2]) {
    s16x4 t0, t1;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t0) : "v"(vb[0]), "i"(OFF));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t1) : "v"(vb[1]), "i"(OFF));
    const s16x8 av = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    return __builtin_bit_cast(typename DT<T>::v8, av);
}
template <int N>
__device__ __forceinline__ void lgkm_wait() {
    __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
    // the MFMA consuming the asm-read registers must not be scheduled above the wait
    __builtin_amdgcn_sched_barrier(0);
}
// O^T += V^T P^T of one tile of the kv_off<HD> image: NPV = HD / 8 MFMAs, V^T read two MFMAs
// ahead through a three-deep ring (two ds_reads an operand: lgkmcnt 4 while two operands are
// behind the one needed, 2 and 0 as the ring drains).  BASE: the tile's immediate byte offset
// past vb.  `beside(I)` runs after MFMA I (I an integral_constant).
template <int HD, int BASE>
constexpr int pv_off(const int i) {             // immediate offset of PV operand i
    return BASE + (4 * (i / (2 * (HD / 32))) + 2 * ((i / (HD / 32)) & 1)) * (HD * 16) + 512 * (i % (HD / 32));
}
template <typename T, int HD, int BASE, typename F>
__device__ __forceinline__ void pv_ring(f32x16 (&acc_o)[HD / 32], const int (&vb)[2], const typename DT<T>::v8 (&pb)[4], F&& beside) {
    constexpr int ND = HD / 32, NPV = 4 * ND;
    typename DT<T>::v8 ring[3];
    ring[0] = rd_v_asm<T, pv_off<HD, BASE>(0)>(vb);
    ring[1] = rd_v_asm<T, pv_off<HD, BASE>(1)>(vb);
    static_for<NPV>([&](auto I) {
        constexpr int i = decltype(I)::value;
        if constexpr (i + 2 < NPV) {
            ring[(i + 2) % 3] = rd_v_asm<T, pv_off<HD, BASE>(i + 2)>(vb);
            lgkm_wait<4>();
        } else if constexpr (i + 1 < NPV) {
            lgkm_wait<2>();
        } else {
            lgkm_wait<0>();
        }
        acc_o[i % ND] = DT<T>::mfma32(ring[i % 3], pb[i / ND], acc_o[i % ND]);
        beside(I);
    });
}

// ---- 5. LDS-DMA.  A tile of the kv_off<HD> image is one-KiB pieces (8 rows x 8 chunks, HD / 64
// an 8-row block); lane l of a wave-instruction lands at +16 l, so for piece g it fetches chunk
// 8 (g % PPB) + 4 (l >> 5) + ((l & 3) ^ swz(row)) of row 8 (g / PPB) + (l & 31) / 4.  The
// per-lane byte offset of that chunk within a tile whose rows are row_bytes apart; with d, kOOB
// (zeros) for a chunk past the d features a row has.
template <int HD>
__device__ __forceinline__ int dma_piece(const int g, const int lane, const int row_bytes, int& cch) {
    constexpr int PPB = HD / 64;
    const int r = 8 * (g / PPB) + (lane & 31) / 4;
    cch = 8 * (g % PPB) + 4 * (lane >> 5) + ((lane & 3) ^ ((r >> 2) & 3));
    return r * row_bytes + cch * 16;
}
template <int HD>
__device__ __forceinline__ int dma_piece(const int g, const int lane, const int row_bytes) {
    int cch;
    return dma_piece<HD>(g, lane, row_bytes, cch);
}
template <int HD>
__device__ __forceinline__ int dma_piece_d(const int g, const int lane, const int row_bytes, const int d) {
    int cch;
    const int off = dma_piece<HD>(g, lane, row_bytes, cch);
    return cch * 8 < d ? off : kOOB;
}
// counted vmcnt (the DMA writes are invisible to the compiler's waitcnt tracking: `left` vmem
// instructions may stay in flight) + a barrier that the compiler may not move memory
// operations across
template <int... LEFTS>
__device__ __forceinline__ void publish(const int left = 0) {
    // (s_waitcnt takes an immediate: LEFTS are the counts the caller may pass besides 0)
    if (!((left == LEFTS ? (__builtin_amdgcn_s_waitcnt(waitcnt_vm(LEFTS)), true) : false) || ...))
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace xfa
