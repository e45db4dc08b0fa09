// fmha_merge.hip — merge partial attention states (fmha_merge_states): n parts (O_i, LSE_i) of
// one softmax row, each computed over its own keys, into the (O, LSE) of the row over all of
// them.  Per (batch, row, head), in fp32:
//
//   present_i = LSE_i is finite (+inf: this library's "no visible key"; -inf: other libraries')
//   m = max LSE_i,  w_i = exp(LSE_i - m),  den = sum w_i          over the present parts
//   O = sum (w_i / den) O_i   (rounded once),  LSE = m + log(den)
//   with a sink: O *= f, LSE = merged, from sink_merge(LSE, sink[head])
//   no part present: O = 0, LSE = +inf, whatever the sink
//
// A streaming kernel: it reads n R D elements and writes R D (R = batch rows heads), no LDS.  One
// thread per 16-byte chunk of an O row, d / 8 threads per (row, head) and 256 / (d / 8) of them
// per workgroup in (batch, row, head) order, so consecutive lanes walk the contiguous [head, d]
// run of O.  The part pointers arrive by value in the kernel arguments (no device table), the
// parts are summed in index order without atomics: bitwise reproducible.
//
// In place (o / lse = part 0's buffers): a thread reads its chunk of every part before it writes
// that chunk, and the barrier orders every read of a row's LSEs (the threads of a row may sit in
// two waves when d / 8 does not divide 64) before the row's one LSE write.
//
// The O of an absent part is loaded but never enters the sum (a select on the presence mask, not
// a product with 0: it may be NaN).  The loads and stores of O carry the non-temporal hint: every
// byte is touched once, and the hint measured 5 - 7 % less time than plain accesses (DESIGN.md
// §3.9; -DXFA_MERGE_NT=0 builds the plain form for that comparison).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_launch.h"

#ifndef XFA_MERGE_NT
#define XFA_MERGE_NT 1
#endif

namespace xfa {

// NP > 0: the part count, known at compile time (loops unroll, every load is issued up front);
// NP = 0: p.n parts at run time, up to kMergeMaxParts
template <typename T, int NP>
__global__ void __launch_bounds__(256) fmha_merge_kernel(const MergeParams p) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    constexpr int CAP = NP ? NP : kMergeMaxParts;
    const int n = NP ? NP : p.n;
    const int cpr = p.d >> 3, rpb = 256 / cpr;
    const int t = threadIdx.x, ri = t / cpr, c = t - ri * cpr;
    const int64_t rh = (int64_t)blockIdx.x * rpb + ri;
    const bool ok = ri < rpb && rh < (int64_t)p.b * p.rows * p.h;
    int head = 0;
    int64_t pli = 0, poi = 0, li = 0, oi = 0;
    if (ok) {
        head = (int)(rh % p.h);
        const int64_t r = rh / p.h;
        const int64_t bi = r / p.rows, pos = r - bi * p.rows;
        pli = bi * p.pl_batch + (int64_t)head * p.pl_head + pos;
        li = bi * p.l_batch + (int64_t)head * p.l_head + pos;
        poi = bi * p.po_batch + pos * p.po_row + (int64_t)head * p.po_head + 8 * c;
        oi = bi * p.o_batch + pos * p.o_row + (int64_t)head * p.o_head + 8 * c;
    }
    float w[CAP];
    T8 x[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        w[i] = INFINITY;
        if (ok && i < n) w[i] = p.lse_parts[i][pli];
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        x[i] = T8{};
        if (ok && i < n) {
            const T8* src = reinterpret_cast<const T8*>(reinterpret_cast<const T*>(p.o_parts[i]) + poi);
            x[i] = XFA_MERGE_NT ? __builtin_nontemporal_load(src) : *src;
        }
    }
    // presence mask, maximum, normalised weights
    unsigned present = 0u;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (fabsf(w[i]) != INFINITY) { present |= 1u << i; m = fmaxf(m, w[i]); }
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        w[i] = (present >> i & 1u) ? __expf(w[i] - m) : 0.f;
        den += w[i];
    }
    float lse = INFINITY, f = 1.f;
    if (present) {
        const float inv = 1.f / den;
#pragma unroll
        for (int i = 0; i < CAP; ++i) w[i] *= inv;
        lse = m + logf(den);
        if (p.sink) {
            const SinkMerge sm = sink_merge(lse, p.sink[head]);
            f = sm.f;
            lse = sm.lse;
        }
    }
    __syncthreads();
    if (!ok) return;
    if (p.lse && c == 0) p.lse[li] = lse;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (present >> i & 1u) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += w[i] * (float)x[i][j];
        }
    T8 y;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = (T)(acc[j] * f);
    T8* dst = reinterpret_cast<T8*>(reinterpret_cast<T*>(p.o) + oi);
    if (XFA_MERGE_NT) __builtin_nontemporal_store(y, dst);
    else *dst = y;
}

template <typename T>
static void launch_merge_t(const MergeParams& p, dim3 grid, hipStream_t st) {
    switch (p.n) {
    case 1: hipLaunchKernelGGL((fmha_merge_kernel<T, 1>), grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL((fmha_merge_kernel<T, 2>), grid, dim3(256), 0, st, p); break;
    case 3: hipLaunchKernelGGL((fmha_merge_kernel<T, 3>), grid, dim3(256), 0, st, p); break;
    case 4: hipLaunchKernelGGL((fmha_merge_kernel<T, 4>), grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL((fmha_merge_kernel<T, 0>), grid, dim3(256), 0, st, p); break;
    }
}

hipError_t launch_merge_states(const MergeParams& p, bool fp16, hipStream_t st) {
    const int rpb = 256 / (p.d / 8);
    const int64_t rh = (int64_t)p.b * p.rows * p.h;
    if (rh <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rh + rpb - 1) / rpb));
    if (fp16) launch_merge_t<_Float16>(p, grid, st);
    else launch_merge_t<__bf16>(p, grid, st);
    return hipGetLastError();
}

}  // namespace xfa
