// fmha_fwd8w_kernel.h — 4-wave fp8 (e4m3fn) forward, D = 128 (one wave per SIMD, 64 query rows
// per wave): the structure of fmha_fwd4_kernel.h (bf16) on the block-scaled fp8 MFMA.
//
// Same semantics as fmha_fwd_fp8_kernel.h (north_star's fp8 GEMMs; the bf16 forward of the
// reference, flash_fwd_kernel_hip.h:1023-1200, on the dequantised inputs with P rounded to e4m3
// for PV).  Runs the fp8 launches with no left window (fp8_w4 knob); the item's whole
// pipeline is one generated asm statement (fmha_fwd8_body.h, tools/gen_fwd8.py).  This file's
// own: the fp8 LDS images (shared with fmha_fwd8pp_kernel.h), their read bases and DMA offsets,
// and the descales.  The item geometry is fmha_fwd_geom.h's, the item schedules
// fmha_fwd_sched.h's.
#pragma once

#include "fmha_fwd_geom.h"
#include "fmha_fwd_sched.h"
#ifdef XFA_FWD8_BODY                     // A/B builds of a generated variant (tools/fwd8_variant.py)
#include XFA_FWD8_BODY
#else
#include "fmha_fwd8_body.h"
#endif

namespace xfa {

#ifdef XFA_FWD8_STAMPS
// Diagnostic build only (gen_fwd8.py --stamps, read by tools/fwd8_stamps.py): each wave sums
// the s_memtime cycles per phase class in lanes 0..7 of one register; the kernel adds them into
// this array at its end (read by fmha_fwd8_stamps).
static __device__ unsigned long long g_fwd8_stamps[4 * 8];   // (64-bit: 256 workgroups x launches)
#define XFA_F8_ACC_PARAM , unsigned& acc
#define XFA_F8_ACC_ARG , acc
#else
#define XFA_F8_ACC_PARAM
#define XFA_F8_ACC_ARG
#endif

constexpr int kFwd8wRows = 256;            // query rows per workgroup (4 waves x 64)
constexpr int kFwd8wTile = 64 * 128;       // bytes of one fp8 K (or V) tile
constexpr int kFwd8wVReg = 4 * kFwd8wTile; // V ring after the 4 K slots
constexpr int kFwd8wSmem = 8 * kFwd8wTile; // 64 KiB
constexpr FwdQueue kFwd8wQueue = kQueueXcd; // for plan_fwd and fwd_walk

// fp8 LDS images (fmha_fwd_fp8_kernel.h): XOR of the 16-byte chunk by the row
__device__ __forceinline__ int k8w_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ ((row >> 1) & 7)); }
// V: the transposed reads take rows 4h + {0..3, 8..11} (+ 16 kb) per lane half h (the P
// k permutation, tools/gen_fwd8.py): the chunk XOR uses row bits 1 and 3 so the 8 rows of
// one read half land on 4 different chunk pairs per row parity (conflict-free)
__device__ __forceinline__ int v8w_swz(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }
__device__ __forceinline__ int v8w_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ v8w_swz(row)); }

// One (batch x kv head, 256-row query block) item.
template <bool F16, bool VARLEN, bool DSC>
__device__ __forceinline__ void fwd8w_item(const FwdParams& p, char* smem, const int bh, const int m_block XFA_F8_ACC_PARAM) {
    constexpr int HD = 128;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));        // item-local: not hoisted out of the persistent loop
    const int lane = tid & 63;
    const int lr = lane & 31;
    const int hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int bidx = bh / p.hk;
    const int hk_i = bh - bidx * p.hk;
    // this item's descales first: device descales are loaded under the rest of the prologue
    const Fp8Scales ds = fp8_scales<DSC>(p, bidx, hk_i);
    // varlen / seqused_k: this sequence's rows of the packed tensors (dense: q_off = k_off = 0)
    const SeqRange sr = seq_range<VARLEN>(p, bidx);
    const int q_off = sr.q_off, sq = sr.sq, k_off = sr.k_off, sk = sr.sk;
    const int G = p.group;
    const int rows_total = sq * G;
    const int row0 = m_block * kFwd8wRows;
    if (row0 >= rows_total) return;          // workgroup-uniform (also sq <= 0)
    const KeyLimit lim_r{sk, sk - sq, p.wr};

    const int ntl = key_tiles(lim_r, (min(row0 + kFwd8wRows, rows_total) - 1) / G);
    const int wrow0 = row0 + 64 * wave;
    int t_w, e_w;
    wave_tiles<64>(lim_r, wrow0, rows_total, G, ntl, t_w, e_w);
    t_w = __builtin_amdgcn_readfirstlane(t_w);
    e_w = __builtin_amdgcn_readfirstlane(e_w);

    // per lane: the rows of the two 32-row blocks (Q in fp8 bytes)
    LaneRow r[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
        r[rb] = lane_row<1>(p, lim_r, wrow0 + 32 * rb + lr, rows_total, hk_i, 32 * hh, 16 * hh, hh);

    if (ntl <= 0) {    // (also a sequence without keys)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) store_empty_row(p, bidx, q_off, r[rb], hh);
        return;
    }

    // bases and extents of this sequence's own rows: a lane past them reads zeros and stores
    // nothing (never the next sequence's rows)
    const RowSrds srd = row_srds<1>(p, bidx, q_off, sq);
    const int k_row = (int)p.k_row, v_row = (int)p.v_row;
    const char* kseq = reinterpret_cast<const char*>(p.k) + (int64_t)bidx * p.k_batch + (int64_t)k_off * p.k_row + (int64_t)hk_i * p.k_head;
    const char* vseq = reinterpret_cast<const char*>(p.v) + (int64_t)bidx * p.v_batch + (int64_t)k_off * p.v_row + (int64_t)hk_i * p.v_head;
    const int nk = min(sk, ntl * kBlockN);
    const uint32_t kvbytes = (uint32_t)((nk - 1) * k_row + HD);

    // LDS-DMA pieces g = 2 wave + i: 8 rows x 8 chunks, lane l lands at g KiB + 16 l, fetched
    // from the source chunk the image's XOR places there (K and V images differ)
    int dk[2], dv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int g = wave * 2 + i;
        const int dr = 8 * g + (lane >> 3);
        dk[i] = dr * k_row + 16 * ((lane & 7) ^ ((dr >> 1) & 7));
        dv[i] = dr * v_row + 16 * ((lane & 7) ^ v8w_swz(dr));
    }
    const int sbase = (int)(size_t)smem;
    int ka[4], va[4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) ka[2 * s + u] = sbase + k8w_off(lr, 4 * s + 2 * hh + u);
    {
        const int i = lane & 15, q = i >> 1, pb8 = i & 1, g = (lane >> 4) & 1;
        const int vr = 4 * hh + (q & 3) + 8 * (q >> 2);   // read kb adds 16 kb rows
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) va[dt] = sbase + kFwd8wVReg + v8w_off(vr, 2 * dt + g) + 8 * pb8;
    }
    const int kstep = __builtin_amdgcn_readfirstlane(kBlockN * k_row);
    const int kdst = __builtin_amdgcn_readfirstlane(sbase + wave * 2048);
    const float c = p.scale_log2 * ds.q * ds.k;
    const float thr = __builtin_amdgcn_exp2f(fminf(p.max_slack, 8.f));   // P <= 256 < 448
    if constexpr (F16)
        fwd8_item_f16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), (int)kvbytes, srd.q, srd.o, srd.lse, kstep,
                      kdst, ntl, t_w, e_w, c, thr, ds.v, ka[0], ka[1], ka[2], ka[3], va[0], va[1], va[2], va[3], dk[0],
                      dk[1], dv[0], dv[1], r[0].lim, r[1].lim, r[0].qoff, r[1].qoff, r[0].ooff, r[1].ooff, r[0].loff,
                      r[1].loff XFA_F8_ACC_ARG);
    else
        fwd8_item_bf16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), (int)kvbytes, srd.q, srd.o, srd.lse, kstep,
                       kdst, ntl, t_w, e_w, c, thr, ds.v, ka[0], ka[1], ka[2], ka[3], va[0], va[1], va[2], va[3], dk[0],
                       dk[1], dv[0], dv[1], r[0].lim, r[1].lim, r[0].qoff, r[1].qoff, r[0].ooff, r[1].ooff, r[0].loff,
                       r[1].loff XFA_F8_ACC_ARG);
}

// Persistent grid (one workgroup per CU) over the items (fwd_walk, fmha_fwd_sched.h).
template <bool F16, bool VARLEN, bool DSC>
__global__ void __launch_bounds__(256, 1) fmha_fwd8w_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef XFA_FWD8_STAMPS
    unsigned acc = 0;
#endif
    fwd_walk<kFwd8wQueue>(p, [&](int bh, int m_block) { fwd8w_item<F16, VARLEN, DSC>(p, smem, bh, m_block XFA_F8_ACC_ARG); });
#ifdef XFA_FWD8_STAMPS
    if ((threadIdx.x & 63) < 8) atomicAdd(&g_fwd8_stamps[(threadIdx.x >> 6) * 8 + (threadIdx.x & 63)], (unsigned long long)acc);
#endif
}

}  // namespace xfa
