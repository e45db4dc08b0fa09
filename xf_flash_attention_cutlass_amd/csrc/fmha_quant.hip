// fmha_quant.hip — bf16 / fp16 -> OCP fp8 e4m3fn with the descales the fp8 kernels take
// (fmha_quantize_fp8): what a caller of the fp8 forward otherwise does with a chain of torch ops
// (amax, host scalar, divide, clamp, cast: four or more passes with fp32 temporaries and a
// device-to-host sync).  Two passes over x, no allocation, no sync, capturable in a graph:
//
//   pass 1  amax[s] = max |float(x)| over scale set s          (s = 0, or (batch, head group))
//   pass 2  descale[s] = amax[s] / 448  (1.0 where amax == 0: zeros or an empty sequence)
//           x8 = e4m3_rne(clamp(float(x) * (1 / descale[s]), -448, 448))
//
// Both passes give a thread one 16-byte chunk column (head, 8 elements) of kQuantIter rows, so
// the scale set of a thread never changes over its rows.  Pass 1 keeps a running maximum per
// thread, takes the wave maximum per distinct scale set among the wave's lanes (one for a
// per-tensor scale or when a head group spans the wave; a few otherwise) and one lane issues an
// atomicMax on the bit pattern of the non-negative float: a maximum does not depend on the
// order, so the result is deterministic.  Pass 2 reads 16 bytes, converts with
// v_cvt_pk_fp8_f32 and stores 8 bytes per chunk.  Lanes past a sequence's rows (packed input)
// or past the columns read and write nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fmha_launch.h"

namespace xfa {

constexpr int kQuantIter = 32;    // rows per thread (pass 1: rows between two atomics of a wave)
constexpr int kQuantBatch = 8;    // of them loaded before the first is used (divides kQuantIter)

// The block's rows and the thread's column: block (x = column tile + tiles * row block, y =
// batch); narrow rows (fewer than 256 chunks) put 256 / cols rows side by side in a block.
struct QuantLane {
    bool ok;            // the thread has a column (and a first row slot)
    int bi, col;        // batch (or sequence), chunk column of the row: head * (d / 8) + chunk
    int r0, rstep, r1;  // rows r0, r0 + rstep, ... < r1 of this sequence
    int sidx;           // scale set
    int64_t src;        // element offset of (row 0, col) in x, dst the same in x8
    int64_t dst;
};
__device__ __forceinline__ QuantLane quant_lane(const QuantParams& p) {
    QuantLane l;
    const int cpr = p.d / 8, cols = p.h * cpr;
    const int cw = cols < 256 ? cols : 256;
    const int rpp = cols < 256 ? 256 / cols : 1;
    const int tiles = (cols + 255) / 256;
    const int ct = (int)blockIdx.x % tiles, rb = (int)blockIdx.x / tiles;
    const int t = (int)threadIdx.x;
    const int rsub = t / cw;
    l.bi = (int)blockIdx.y;
    l.col = ct * 256 + t % cw;
    l.ok = rsub < rpp && l.col < cols;
    int row_off = 0, len = p.s;
    if (p.cu) { row_off = p.cu[l.bi]; len = p.cu[l.bi + 1] - row_off; }
    l.r0 = rb * (kQuantIter * rpp) + rsub;
    l.rstep = rpp;
    l.r1 = min(len, (rb + 1) * (kQuantIter * rpp));
    const int head = l.ok ? l.col / cpr : 0;
    const int e0 = 8 * (l.ok ? l.col - head * cpr : 0);
    l.sidx = p.gran ? l.bi * (p.h / p.group) + head / p.group : 0;
    l.src = (p.cu ? (int64_t)row_off * p.x_row : (int64_t)l.bi * p.x_batch) + (int64_t)head * p.x_head + e0;
    l.dst = ((int64_t)(p.cu ? row_off : (int64_t)l.bi * p.s) * p.h + head) * p.d + e0;
    return l;
}

template <typename T>
__global__ void __launch_bounds__(256) fmha_quant_amax_kernel(const QuantParams p) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    const QuantLane l = quant_lane(p);
    float m = 0.f;
    if (l.ok && l.r0 < l.r1) {
        const T* x = reinterpret_cast<const T*>(p.x) + l.src;
        // kQuantBatch loads in flight per thread; a slot past the thread's rows reads the last
        // row of the block's range again (same column, same scale set: a maximum does not mind)
        for (int it = 0; it < kQuantIter && l.r0 + it * l.rstep < l.r1; it += kQuantBatch) {
            T8 v[kQuantBatch];
#pragma unroll
            for (int j = 0; j < kQuantBatch; ++j)
                v[j] = *reinterpret_cast<const T8*>(x + (int64_t)min(l.r0 + (it + j) * l.rstep, l.r1 - 1) * p.x_row);
#pragma unroll
            for (int j = 0; j < kQuantBatch; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf((float)v[j][i]));
        }
    }
    // one atomic per distinct scale set among the wave's lanes that saw a non-zero value (the
    // accumulator starts at zero, so a zero adds nothing)
    unsigned bits = __float_as_uint(m);
    uint64_t todo = __ballot(bits != 0u);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int s = __shfl(l.sidx, lead);
        const bool mine = bits != 0u && l.sidx == s;
        unsigned w = mine ? bits : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w = max(w, (unsigned)__shfl_xor((int)w, o));
        if ((int)(threadIdx.x & 63) == lead) atomicMax(p.amax + s, w);
        todo &= ~__ballot(mine);
    }
}

__device__ __forceinline__ float quant_descale(const unsigned amax_bits) {
    const float a = __uint_as_float(amax_bits);
    return a == 0.f ? 1.f : a / 448.f;
}
__device__ __forceinline__ float clamp448(const float v) {
    return v < -448.f ? -448.f : (v > 448.f ? 448.f : v);
}

template <typename T>
__global__ void __launch_bounds__(256) fmha_quant_cvt_kernel(const QuantParams p) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    const int nscale = p.gran ? p.b * (p.h / p.group) : 1;
    const int flat = ((int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x) * 256 + (int)threadIdx.x;
    if (flat < nscale) p.descale[flat] = quant_descale(p.amax[flat]);
    const QuantLane l = quant_lane(p);
    if (!l.ok || l.r0 >= l.r1) return;
    const float inv = 1.f / quant_descale(p.amax[l.sidx]);
    const T* x = reinterpret_cast<const T*>(p.x) + l.src;
    uint8_t* y = reinterpret_cast<uint8_t*>(p.x8) + l.dst;
    const int64_t y_row = (int64_t)p.h * p.d;
    // kQuantBatch loads in flight per thread; a slot past the thread's rows loads the range's
    // last row again and stores nothing
    for (int it = 0; it < kQuantIter && l.r0 + it * l.rstep < l.r1; it += kQuantBatch) {
        T8 v[kQuantBatch];
#pragma unroll
        for (int j = 0; j < kQuantBatch; ++j)
            v[j] = *reinterpret_cast<const T8*>(x + (int64_t)min(l.r0 + (it + j) * l.rstep, l.r1 - 1) * p.x_row);
#pragma unroll
        for (int j = 0; j < kQuantBatch; ++j) {
            const int r = l.r0 + (it + j) * l.rstep;
            float f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = clamp448((float)v[j][i] * inv);
            int lo = 0, hi = 0;
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
            if (r < l.r1) *reinterpret_cast<u32x2*>(y + (int64_t)r * y_row) = u32x2{(unsigned)lo, (unsigned)hi};
        }
    }
}

hipError_t launch_quantize_fp8(const QuantParams& p, bool fp16, hipStream_t st) {
    const int nscale = p.gran ? p.b * (p.h / p.group) : 1;
    hipError_t e = hipMemsetAsync(p.amax, 0, (size_t)nscale * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    const int cols = p.h * (p.d / 8);
    const int rpp = cols < 256 ? 256 / cols : 1;
    const int tiles = (cols + 255) / 256;
    const int rblocks = (p.s + kQuantIter * rpp - 1) / (kQuantIter * rpp);
    const dim3 grid((unsigned)(tiles * (rblocks > 0 ? rblocks : 1)), (unsigned)p.b);
    if (fp16) hipLaunchKernelGGL(fmha_quant_amax_kernel<_Float16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(fmha_quant_amax_kernel<__bf16>, grid, dim3(256), 0, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (fp16) hipLaunchKernelGGL(fmha_quant_cvt_kernel<_Float16>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(fmha_quant_cvt_kernel<__bf16>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace xfa
