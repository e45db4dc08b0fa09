// fmha_mla_decode_kernel.h — split-KV decode for multi-head latent attention (MLA, the
// "absorbed" form of DeepSeek-V2/V3/R1 and Kimi) over a paged latent cache, gfx950 (CDNA4).
//
// Every query head attends over ONE shared 576-wide latent row per token (512 compressed-KV
// features + 64 rotary features); the value is the first 512 features of the same row:
//
//   S = scale q K^T (576 features),  O = softmax(S) K[:, :512],  LSE = logsumexp(S)
//
// Modelled on fmha_decode_kernel.h (its MR = 16 form): every wave is its own work item, with a
// wave-private LDS image and no barrier; S^T = K Q^T and O^T += V^T P^T on
// v_mfma_f32_16x16x32_{bf16,f16}; lane l holds query row l % 16 and, of each 16-key block, keys
// 4 (l / 16) .. +3.  What differs:
//
//  * ONE image serves K and V.  A 32-key tile is 32 rows of 1152 B (36,864 B); it is read as
//    the A operand of S^T (ds_read_b128 of rows, 18 k-steps x 2 key blocks) and, over its first
//    512 columns, transposed as the A operand of O^T (ds_read_b64_tr_b16, 32 d-tiles x 2).  The
//    cache row is loaded once.
//  * Rows of a batch are r = pos * num_heads + head; a wave owns the 16-row tile r / 16 of one
//    (batch, key split).  Items are numbered ((batch * splits) + split) * row_tiles + row_tile
//    and wave w of workgroup g runs item 4 g + w: with several row tiles (num_heads 128: 8) the
//    tiles of one (batch, split) sit in one workgroup or in the next one in launch order, so the
//    cache bytes come from HBM once and from L2 for the other tiles; with a single row tile
//    (16 heads) the four waves are four key splits.
//  * The rows of one page are contiguous (one kv head), and a 16-row half tile never straddles
//    a page (pages are multiples of 16 rows), so a half tile is ONE run of 18,432 bytes: 18
//    load instructions of 1 KiB, lane l at + 16 l, through a wave-uniform page descriptor and
//    scalar offset, with the non-temporal hint.  Chunk f = 64 i + l of the run is row f / 72,
//    16-byte chunk f % 72: the pattern repeats every 9 instructions (8 rows), so 9 write
//    offsets serve a tile.
//  * The image's swizzle (mla_off): byte (row, chunk) at row * 1152 + 16 (chunk ^ (row & 6)).
//    The 1152-byte pitch is 4.5 bank rows, so odd rows already sit half a bank row on; the XOR
//    with row & 6 (period 8 rows, inside the aligned 8-chunk blocks of a row: 72 = 9 x 8)
//    spreads the even (odd) rows.  Conflict-free for the row reads, the transposed reads and
//    the writes; every instruction of the loop is bank-checked in tools/mla_banks.py.  The XOR
//    leaves the k-step / d-tile index as an immediate: 2 address registers for the row reads
//    (even / odd k-steps), 4 for the transposed reads (d-tile & 3).
//  * One wave per SIMD (launch bounds 256 x 1): the O^T accumulators are 128 registers per lane,
//    the Q fragments 72, the raw ring of one tile 144 — the 512-entry unified file, not the 256
//    of two waves per SIMD.  Four images are 147,456 B of the CU's 160 KiB.  The translation unit
//    is built with VGPR-form MFMAs (build.py): with the accumulators in the accumulator half of
//    the file, the rescale (a VALU multiply) made the compiler copy all 128 of them across every
//    tile, and the kernel spilled.
//  * No slot balancing and no folded combine: the sequence's visible tiles are cut into
//    num_splits equal ranges; an empty range writes O = 0, LSE = -inf.  num_splits == 1 writes
//    O and LSE directly (no scratch, no combine); else fmha_combine_kernel<512, T> merges.
#pragma once

#include "fmha_decode_kernel.h"

namespace xfa {

constexpr int kMlaD = 576;                         // latent row: K width
constexpr int kMlaDV = 512;                        // V = its first 512 features
constexpr int kMlaKeys = 32;                       // keys per tile
constexpr int kMlaWaves = 4;                       // waves (= items) per workgroup
constexpr int kMlaPitch = kMlaD * 2;               // bytes per row
constexpr int kMlaCPR = kMlaPitch / 16;            // 16-byte chunks per row (72)
constexpr int kMlaImage = kMlaKeys * kMlaPitch;    // one wave's image
constexpr int kMlaNLD = 16 * kMlaPitch / 1024;     // load instructions per 16-row half tile (18)
constexpr int kMlaSmem = kMlaWaves * kMlaImage;

__device__ __forceinline__ int mla_off(int row, int chunk) {
    return row * kMlaPitch + ((chunk ^ (row & 6)) << 4);
}

template <typename T>
__global__ void __launch_bounds__(kMlaWaves * 64, 1) fmha_mla_decode_kernel(const MlaParams p) {
    using V8 = typename DT<T>::v8;
    constexpr int NS = kMlaD / 32;      // k-steps of S^T = K Q^T (18)
    constexpr int ND = kMlaDV / 16;     // 16-wide d tiles of O^T (32)
    constexpr int NLD = kMlaNLD;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;           // query row (MFMA column) of this lane
    const int hh = lane >> 4;           // key sub-block of this lane
    // wave -> item -> (batch, split, row tile)
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
    // this lane's query row; a tile may straddle query positions, so the causal limit is per lane
    // (a lane past the last row of a partial tile computes the last row again and stores
    // nothing: an MFMA column depends on its own query row alone)
    const int r = rtile * 16 + lr;
    const bool row_ok = r < rows;
    const int pos = min(r, rows - 1) / H;
    const int head = min(r, rows - 1) - pos * H;
    const int my_lim = p.causal ? min(sk, max(0, pos + diag + 1)) : sk;
    const float c = p.scale_log2;

    // key tiles of this split: the sequence's visible tiles [0, ceil(sk / 32)) (the last
    // position sees every key, causal or not) in num_splits equal ranges
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

    // ---- cache loads.  Half tile u = 2 t + h is rows 16 u .. +15 of the sequence: one page
    // (wave-uniform descriptor over exactly that page), one contiguous run.  A half tile past the
    // sequence's last page re-reads the start of the last page (never a table entry the sequence
    // does not own): its keys are >= sk, masked and zeroed below.
    typedef __attribute__((address_space(4))) const int cint;
    cint* btab = (cint*)(p.block_table + (int64_t)bidx * p.bt_stride);
    const int last_pg = sk > 0 ? (sk - 1) / p.page_size : 0;
    const uint32_t page_bytes = (uint32_t)p.page_size * kMlaPitch;
    const char* pool = uniform_ptr(reinterpret_cast<const char*>(p.kv));
    // (page id, first row inside the page) of a half tile, fetched ahead of its loads: scalar
    // loads never make the vector-load ring drain
    auto fetch_page = [&](const int u, int (&pg)[2]) __attribute__((always_inline)) {
        const int row0 = 16 * u;
        const int pi = __builtin_amdgcn_readfirstlane(row0 / p.page_size);
        const bool past = pi > last_pg;
        pg[0] = btab[past ? last_pg : pi];
        pg[1] = past ? 0 : row0 - pi * p.page_size;
    };
    // the raw ring: one tile, 2 x 18 register quads (144 registers)
    u32x4 raw[2][NLD];
    auto issue = [&](const int h, const int (&pg)[2]) __attribute__((always_inline)) {
        const int page = __builtin_amdgcn_readfirstlane(pg[0]);
        const int x = __builtin_amdgcn_readfirstlane(pg[1]);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(uniform_ptr(pool + (int64_t)page * page_bytes), page_bytes);
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            raw[h][i] = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * lane, x * kMlaPitch + 1024 * i, XFA_DEC_CPOL);
    };

    // ---- image offsets.  Writes: chunk f = 64 j + lane of an 8-row group (9 instructions).
    int woff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int f = 64 * j + lane;
        woff[j] = mla_off(f / kMlaCPR, f % kMlaCPR);
    }
    // K operand of k-step s: row lr, chunk 4 s + hh -> 16 ((4 s + hh) ^ (lr & 6)) =
    // 64 (s ^ b) + 16 (hh ^ (lr & 2)), b = bit 2 of lr: even k-steps + 64 b, odd ones - 64 b
    const int kb2 = (lr >> 2) & 1;
    const int kbase = lr * kMlaPitch + 16 * (hh ^ (lr & 2));
    const int koff_e = kbase + 64 * kb2, koff_o = kbase - 64 * kb2;
    // V^T operand of d tile dt: row 4 hh + q4 (+ 16 part), chunk 2 dt + h1, + 8 h0 bytes ->
    // chunk ^ (row & 6) = 8 (dt >> 2) + 2 ((dt & 3) ^ a) + h1, a = bits 1-2 of the row
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

    // pages of the two halves of the next tile
    int pg_a[2] = {0, 0}, pg_b[2] = {0, 0};
    if (t_lo < t_hi) {
        fetch_page(2 * t_lo, pg_a);
        fetch_page(2 * t_lo + 1, pg_b);
        issue(0, pg_a);
        issue(1, pg_b);
        fetch_page(2 * min(t_lo + 1, t_hi - 1), pg_a);
        fetch_page(2 * min(t_lo + 1, t_hi - 1) + 1, pg_b);
    }
    // retire the Q loads (issued before the ring) explicitly, as fmha_decode_kernel does
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * NLD));

    // One tile: the ring goes into the image and is refilled at once with the next tile, whose
    // loads fly across this tile's products.  LAST: the last tile of a split, which refills
    // nothing and alone can hold the sequence's end.
    auto tile = [&](auto LAST, const int t) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST)::value;
        const int keyb = t * kMlaKeys;
        bool plain = true;
        if constexpr (last) {
            // The tile that holds the sequence's end: the loads brought cache rows >= sk, whatever
            // they hold.  Their scores are replaced below, but they enter O^T += V^T P^T as
            // 0 * V, which a NaN or Inf survives: those rows go into the image as zeros.
            if (keyb + kMlaKeys > sk) {
                plain = false;
                const int nval = sk - keyb;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < NLD; ++i) {
                        const int row = 16 * h + 8 * (i / 9) + (64 * (i % 9) + lane) / kMlaCPR;
                        const u32x4 v = row < nval ? raw[h][i] : u32x4{0u, 0u, 0u, 0u};
                        *reinterpret_cast<u32x4*>(img + woff[i % 9] + (16 * h + 8 * (i / 9)) * kMlaPitch) = v;
                    }
            }
        }
        if (plain) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < NLD; ++i)
                    *reinterpret_cast<u32x4*>(img + woff[i % 9] + (16 * h + 8 * (i / 9)) * kMlaPitch) = raw[h][i];
        }
        if constexpr (!last) {
            // pin the LDS writes before the refill (a hoisted refill renames the ring's registers
            // and the loop then copies them back, draining the ring every tile), and the refill
            // before the products (the loads are to fly across all of them)
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
        // element (kb, i) is key keyb + 16 kb + 4 hh + i; the window edge behind a wave-uniform branch
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
        // P -> T: the B operand of the PV product, k index 8 hh + i = key i < 4 ? 4 hh + i :
        // 16 + 4 hh + (i - 4), the permutation the two transposed reads apply to V^T
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

    // ---- epilogue: normalised O and LSE; a row (or range) without a visible key is empty
    const float l_full = quad_sum16(l_run);
    const bool empty = (l_full == 0.f) || (l_full != l_full);
    const float inv = empty ? 0.f : 1.f / l_full;
    if (!row_ok) return;
    const float lsev = empty ? -INFINITY : (m_run * c + __log2f(l_full)) * kLn2;
    if (ns > 1) {
        // split partial (fp32), merged by fmha_combine_kernel<512, T>
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
