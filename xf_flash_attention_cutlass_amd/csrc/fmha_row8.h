// fmha_row8.h — eight elements of a row at a time: the 16-byte load to fp32 and the fp8 store the
// append kernels share (fmha_append.hip, fmha_mla_index.hip).
#pragma once

#include "fmha_common.h"

#include <cstdint>

namespace xfa {

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&x)[8]) {
    typedef __attribute__((ext_vector_type(8))) T T8;
    const T8 v = *reinterpret_cast<const T8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (float)v[i];
}

// 8 fp32 values x inv -> 8 e4m3fn bytes (v_cvt_pk_fp8_f32: round to nearest even), one store
__device__ __forceinline__ void store8(uint8_t* p, const float (&x)[8], const float inv) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = x[i] * inv;
        f[i] = v < -448.f ? -448.f : (v > 448.f ? 448.f : v);
    }
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *reinterpret_cast<u32x2*>(p) = u32x2{(unsigned)lo, (unsigned)hi};
}

}  // namespace xfa
