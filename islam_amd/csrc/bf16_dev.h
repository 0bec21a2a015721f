// Device helpers shared by the channels-last bf16 matrix-core kernels (conv_nhwc.hip, conv_ws.hip, conv_ws32.hip, hourglass.hip):
// native vector types, a compile-time loop, and packed-bf16 conversion / ReLU.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace islam {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));     // a REAL vector value: copies of HIP's uint4 struct become memcpy
                                                                 // intrinsics that keep a register array in scratch
typedef short s16x2_t __attribute__((ext_vector_type(2)));

// Compile-time loop: the index is an integral_constant, so the register arrays it indexes are split into scalars as soon as the
// lambda is inlined.  With `#pragma unroll` the indices only become constant after the (late) unroll pass; an array that is
// still indexed dynamically when SROA runs is left to AMDGPUPromoteAlloca, which keeps anything above 128 bytes in SCRATCH -- the
// prefetched weights (nine uint4) then go through scratch_store right after their global loads, which forces a vmcnt wait
// in front of the multiply phase and serialises the two (found in the ISA; 194 -> see DESIGN.md).
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

__device__ __forceinline__ unsigned pack2(float a, float b) {      // round-to-nearest-even, one v_cvt_pk_bf16_f32
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ float lo16(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float hi16(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
// ReLU of packed bf16: a negative bf16 is a negative int16 (sign-magnitude), so max(., 0) on the int16 lanes is the ReLU: ONE v_pk_max_i16 per pair
__device__ __forceinline__ unsigned relu2(unsigned t) {
    const s16x2_t z = {0, 0};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2_t, t), z));
}

}  // namespace islam
