// fmha_fwd8pp_kernel.h — 8-wave ping-pong fp8 (e4m3fn) forward, D = 128 (two waves per SIMD, 32
// query rows per wave): the phase structure of fmha_fwdpp_kernel.h (bf16) on the operand layouts
// of the 4-wave fp8 kernel (fmha_fwd8w_kernel.h, whose LDS images and helpers it uses).
//
// Same semantics as fmha_fwd_fp8_kernel.h (north_star's fp8 GEMMs; the bf16 forward of the
// reference, flash_fwd_kernel_hip.h:1023-1200, on the dequantised inputs with P rounded to e4m3
// for PV).  The item's pipeline is one generated asm statement (fmha_fwd8pp_body.h,
// tools/gen_fwd8pp.py).  This file's own: the read bases and DMA offsets of its LDS ring, and the
// descales; dense launches only.  The item geometry is fmha_fwd_geom.h's, the item schedules
// fmha_fwd_sched.h's.
#pragma once

#include "fmha_fwd8w_kernel.h"
#ifdef XFA_FWD8PP_BODY
#include XFA_FWD8PP_BODY        // an A/B variant of the generated body
#else
#include "fmha_fwd8pp_body.h"
#endif

namespace xfa {

constexpr int kFwd8ppRows = 256;           // query rows per workgroup (8 waves x 32)
constexpr FwdQueue kFwd8ppQueue = kQueueXcd; // for plan_fwd and fwd_walk
constexpr int kFwd8ppVReg = kFwd8ppRing * kFwd8wTile;      // the V ring follows the K ring
constexpr int kFwd8ppSmem = 2 * kFwd8ppRing * kFwd8wTile;  // (kFwd8ppRing: the generated body's)

// One (batch x kv head, 256-row query block) item.
template <bool F16, bool DSC>
__device__ __forceinline__ void fwd8pp_item(const FwdParams& p, char* smem, const int bh, const int m_block) {
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
    const int sq = p.seqlen_q, sk = p.seqlen_k;
    const int G = p.group;
    const int rows_total = sq * G;
    const int row0 = m_block * kFwd8ppRows;
    if (row0 >= rows_total) return;          // workgroup-uniform
    const KeyLimit lim_r{sk, sk - sq, p.wr};

    const int ntl = key_tiles(lim_r, (min(row0 + kFwd8ppRows, rows_total) - 1) / G);
    const int wrow0 = row0 + 32 * wave;
    int t_w, e_w;
    wave_tiles<32>(lim_r, wrow0, rows_total, G, ntl, t_w, e_w);
    t_w = __builtin_amdgcn_readfirstlane(t_w);
    e_w = __builtin_amdgcn_readfirstlane(e_w);

    // this lane's row (Q in fp8 bytes)
    const LaneRow lrow = lane_row<1>(p, lim_r, wrow0 + lr, rows_total, hk_i, 32 * hh, 16 * hh, hh);

    if (ntl <= 0) {
        store_empty_row(p, bidx, 0, lrow, hh);
        return;
    }

    const RowSrds srd = row_srds<1>(p, bidx, 0, sq);
    const int k_row = (int)p.k_row, v_row = (int)p.v_row;
    const char* kseq = reinterpret_cast<const char*>(p.k) + (int64_t)bidx * p.k_batch + (int64_t)hk_i * p.k_head;
    const char* vseq = reinterpret_cast<const char*>(p.v) + (int64_t)bidx * p.v_batch + (int64_t)hk_i * p.v_head;
    const int nk = min(sk, ntl * kBlockN);
    const uint32_t kvbytes = (uint32_t)((nk - 1) * k_row + HD);

    // LDS-DMA piece g = wave of each tile (K and V): rows 8g .. 8g+7 (8 x 128 bytes), lane l
    // lands at g KiB + 16 l, fetched from the source chunk the image's XOR places there
    const int r = 8 * wave + (lane >> 3);
    const int dk = r * k_row + 16 * ((lane & 7) ^ ((r >> 1) & 7));
    const int dv = r * v_row + 16 * ((lane & 7) ^ v8w_swz(r));
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
        for (int dt = 0; dt < 4; ++dt) va[dt] = sbase + kFwd8ppVReg + v8w_off(vr, 2 * dt + g) + 8 * pb8;
    }
    const int kstep = __builtin_amdgcn_readfirstlane(kBlockN * k_row);
    const int kdst = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
    const int grp = __builtin_amdgcn_readfirstlane(wave >> 2);
    const float c = p.scale_log2 * ds.q * ds.k;
    const float thr = __builtin_amdgcn_exp2f(fminf(p.max_slack, 8.f));   // P <= 256 < 448
    const int kvb = __builtin_amdgcn_readfirstlane((int)kvbytes);
    if constexpr (F16)
        fwd8pp_item_f16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), kvb, srd.q, srd.o, srd.lse, kstep, kdst,
                        ntl, t_w, e_w, grp, c, thr, ds.v, ka[0], ka[1], ka[2], ka[3], va[0], va[1], va[2], va[3], dk, dv,
                        lrow.lim, lrow.qoff, lrow.ooff, lrow.loff);
    else
        fwd8pp_item_bf16(ptr_lo(kseq), ptr_hi(kseq), ptr_lo(vseq), ptr_hi(vseq), kvb, srd.q, srd.o, srd.lse, kstep, kdst,
                         ntl, t_w, e_w, grp, c, thr, ds.v, ka[0], ka[1], ka[2], ka[3], va[0], va[1], va[2], va[3], dk, dv,
                         lrow.lim, lrow.qoff, lrow.ooff, lrow.loff);
}

// Persistent grid (one workgroup per CU) over the items (fwd_walk, fmha_fwd_sched.h).
template <bool F16, bool DSC>
__global__ void __launch_bounds__(512, 1) fmha_fwd8pp_kernel(const FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fwd_walk<kFwd8ppQueue>(p, [&](int bh, int m_block) { fwd8pp_item<F16, DSC>(p, smem, bh, m_block); });
}

}  // namespace xfa
