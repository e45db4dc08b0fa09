// fmha_fwd_sched.h — the item schedules of the forward kernels: what the host plans (plan_fwd,
// fmha_launch.h) and the one loop that walks it on the device (fwd_walk), for all six kernels
// (fmha_fwd, fmha_fwdpp, fmha_fwd4, fmha_fwd8w, fmha_fwd8pp, fmha_fwd_fp8).
//
// An item is one row block m_block (of n_mblocks) of one (batch x kv head) unit bh (of nbh).
// Causal work grows with m_block, so every schedule hands out the heaviest row blocks first.
// FwdParams::persistent names the schedule:
//   0  one workgroup per item: grid (nbh, n_mblocks, splits), the last row blocks dispatched
//      first;
//   1  boustrophedon: g resident workgroups; workgroup w's k-th item is number k g + w (even k)
//      or k g + g - 1 - w (odd k) of the heaviest-first order, so the work per workgroup
//      balances, and one item's O-store tail overlaps the next item's prologue loads instead
//      of a workgroup boundary;
//   2  XCD-grouped pairs (g % 8 == 0): pair i of a unit is the row blocks (n - 1 - i, i), equal
//      causal work, run back to back by one workgroup (steps 2j and 2j + 1; the middle block of
//      an odd count is its own pair and the odd step is skipped).  Workgroup w sits on XCD
//      w % 8, and consecutive pairs go to the workgroups of one XCD, so the pairs of a unit run
//      at the same time on one XCD and share its L2 for K / V;
//   3  dynamic queues: a workgroup claims its next item from a device counter when it finishes
//      one, so ragged (varlen) items balance.  With xcd_queues there is one queue per XCD over
//      the units bh = x (mod 8), unit-major, so a unit's row blocks run together on one XCD and
//      share its L2 (g % 8 == 0 and nbh >= 8 are checked on the host); else one global queue,
//      heaviest row block first over all units.
#pragma once

#include "fmha_common.h"

namespace xfa {

// Which schedules a kernel can walk; its launcher passes the same value to plan_fwd.
//   kQueueStatic: modes 0-2 only (no claim or reset code is compiled);
//   kQueueXcd:    also mode 3, per-XCD queues or the global one (p.xcd_queues);
//   kQueueRagged: also mode 3, the global queue only (the 8-wave fp8 kernel's packed launches).
enum FwdQueue { kQueueStatic, kQueueXcd, kQueueRagged };

// ---- the schedules as pure functions of integers (host and device; tests/test_fwd_sched.py
// walks plan_fwd's grids with them)
enum FwdStep { kStepItem, kStepSkip, kStepEnd };

// Static schedules: step k of workgroup wg of g.  Mode 2, the XCD-grouped pairs:
__host__ __device__ inline FwdStep fwd_pair_step(const int k, const int wg, const int g, const int nbh,
                                                 const int nm, int& bh, int& m_block) {
    const int npair = (nm + 1) >> 1;
    const int v = (wg & 7) * (g >> 3) + (wg >> 3);    // XCD-major rank of the workgroup
    const int q = (k >> 1) * g + v;
    if (q >= nbh * npair) return kStepEnd;
    bh = q / npair;
    const int i = q - bh * npair;
    m_block = (k & 1) ? i : nm - 1 - i;
    return ((k & 1) && i == nm - 1 - i) ? kStepSkip : kStepItem;
}
// Mode 1, the boustrophedon:
__host__ __device__ inline FwdStep fwd_snake_step(const int k, const int wg, const int g, const int nbh,
                                                  const int nm, int& bh, int& m_block) {
    const int lin = k * g + ((k & 1) ? g - 1 - wg : wg);
    if (lin >= nbh * nm) return kStepEnd;
    bh = lin % nbh;
    m_block = nm - 1 - lin / nbh;
    return kStepItem;
}

// Dynamic queues: the queue workgroup wg claims from, the queue's length, and claim q's item.
__host__ __device__ inline int fwd_queue_of(const bool xcd_queues, const int wg) { return xcd_queues ? wg & 7 : 0; }
__host__ __device__ inline int fwd_queue_len(const bool xcd_queues, const int x, const int nbh, const int nm) {
    return (xcd_queues ? (nbh - x + 7) >> 3 : nbh) * nm;
}
__host__ __device__ inline void fwd_queue_item(const bool xcd_queues, const int x, const int q, const int nbh,
                                               const int nm, int& bh, int& m_block) {
    if (xcd_queues) {   // unit-major over the units x, x + 8, ...: the heaviest block of each first
        bh = x + 8 * (q / nm);
        m_block = nm - 1 - q % nm;
    } else {            // heaviest row block first over all units
        bh = q % nbh;
        m_block = nm - 1 - q / nbh;
    }
}

// ---- the device walk
// Thread 0 claims the next index of queue x (counter p.work_ctr[2 + x]) and hands it to the
// workgroup through LDS.  The slot alternates with the step: a fast wave may make the next
// step's claim while a slow one has yet to read this one's.
__device__ __forceinline__ int fwd_claim(const FwdParams& p, const int k, const int x) {
    __shared__ int s_claim[2];
    if (threadIdx.x == 0) s_claim[k & 1] = atomicAdd(p.work_ctr + 2 + x, 1);
    __syncthreads();
    return s_claim[k & 1];
}

// Runs item(bh, m_block) for every item the plan gives this workgroup.  The loop has one call
// site, so a force-inlined item body is inlined once.  After the loop of mode 3 every workgroup
// has made its last (failed) claim; the last one to get there resets the counters for the next
// launch on the stream.
template <FwdQueue Q, class Item>
__device__ __forceinline__ void fwd_walk(const FwdParams& p, Item&& item) {
    const int nbh = p.b * p.hk;
    const int g = gridDim.x;
    for (int k = 0;; ++k) {
        int bh, m_block;
        if (Q != kQueueStatic && p.persistent == 3) {
            const bool xq = Q == kQueueXcd && p.xcd_queues;
            const int x = fwd_queue_of(xq, (int)blockIdx.x);
            const int q = fwd_claim(p, k, x);
            if (q >= fwd_queue_len(xq, x, nbh, p.n_mblocks)) break;
            fwd_queue_item(xq, x, q, nbh, p.n_mblocks, bh, m_block);
        } else if (p.persistent == 2) {
            const FwdStep s = fwd_pair_step(k, (int)blockIdx.x, g, nbh, p.n_mblocks, bh, m_block);
            if (s == kStepEnd) break;
            if (s == kStepSkip) continue;
        } else if (p.persistent) {
            if (fwd_snake_step(k, (int)blockIdx.x, g, nbh, p.n_mblocks, bh, m_block) == kStepEnd) break;
        } else {
            if (k > 0) break;
            bh = blockIdx.x;
            m_block = gridDim.y - 1 - blockIdx.y;
        }
        item(bh, m_block);
    }
    if (Q != kQueueStatic && p.persistent == 3 && threadIdx.x == 0) {
        const int total = (int)(gridDim.x * gridDim.y * gridDim.z);
        if (atomicAdd(p.work_ctr + 1, 1) == total - 1) {
            for (int i = 2; i < 10; ++i) atomicExch(p.work_ctr + i, 0);
            atomicExch(p.work_ctr + 1, 0);
        }
    }
}

}  // namespace xfa
