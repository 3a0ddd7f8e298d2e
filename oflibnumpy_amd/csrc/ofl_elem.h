// ofl_elem.h -- the element types fields and tensors are stored in (OFL_EL_*), shared by every file whose kernels are templates
// of the element type, and with_elem, which turns a checked run-time OFL_EL_* into that template argument.
#pragma once
#include "ofl_common.h"

namespace ofl {

template <int E> struct Elem;

template <> struct Elem<OFL_EL_F16> {
    typedef uint16_t T;
    static __device__ __forceinline__ float to_f32(T v) { return (float)__builtin_bit_cast(_Float16, v); }                // exact
    static __device__ __forceinline__ T from_f32(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }           // nearest even, overflow -> inf
};

template <> struct Elem<OFL_EL_BF16> {
    typedef uint16_t T;
    static __device__ __forceinline__ float to_f32(T v) { return __uint_as_float((uint32_t)v << 16); }                    // exact
    static __device__ __forceinline__ T from_f32(float f)       // nearest even on the bit pattern; every NaN becomes 0x7fc0
    {
        const uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (T)0x7fc0;
        return (T)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
};

template <> struct Elem<OFL_EL_F32> {
    typedef float T;
    static __device__ __forceinline__ float to_f32(T v) { return v; }
    static __device__ __forceinline__ T from_f32(float f) { return f; }
};

template <> struct Elem<OFL_EL_F64> {
    typedef double T;
    static __device__ __forceinline__ float to_f32(T v) { return (float)v; }                                              // nearest even
};

// f(std::integral_constant<int, elem>) for a checked elem of the three tensor types: f is a generic lambda whose argument E
// gives the template argument E.value
template <class F>
inline void with_elem(int elem, F &&f)
{
    switch (elem) {
    case OFL_EL_F16:  f(std::integral_constant<int, OFL_EL_F16>()); break;
    case OFL_EL_BF16: f(std::integral_constant<int, OFL_EL_BF16>()); break;
    default:          f(std::integral_constant<int, OFL_EL_F32>()); break;
    }
}

}  // namespace ofl
