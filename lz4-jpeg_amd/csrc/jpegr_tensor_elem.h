// jpegr_tensor_elem.h -- the element of a tensor that the crop calls deliver
// (include/jpegr.h: JPEGR_DTYPE_*): its storage type, the normalisation and
// the rounding, one text for jpeg_crop_tensor_kernel (jpegr_recon.h: a byte in)
// and jpeg_resize_tensor_kernel (jpegr_resize.hip: a resampled fp32 value in).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"

#pragma clang fp contract(off)

namespace {

// The element of one channel byte v: U8 the byte; otherwise
// f = fl32(fl32((float)v * s) + b), two fp32 operations each rounded (no
// contraction in this file), stored as fp32 bits, or rounded to nearest-even
// to f16 (the hardware conversion, subnormals kept) or to bf16 (on the fp32
// bits; f is never a NaN: v and s, b are finite).
template <int DT>
struct TensorElem {
  using type = uint16_t;
};
template <>
struct TensorElem<JPEGR_DTYPE_U8> {
  using type = uint8_t;
};
template <>
struct TensorElem<JPEGR_DTYPE_F32> {
  using type = uint32_t;
};

template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type tensor_elem(uint32_t v, float s, float b) {
  if constexpr (DT == JPEGR_DTYPE_U8) {
    return (uint8_t)v;
  } else {
    const float p = (float)v * s;
    const float f = p + b;
    if constexpr (DT == JPEGR_DTYPE_F32) {
      return __float_as_uint(f);
    } else if constexpr (DT == JPEGR_DTYPE_F16) {
      return __builtin_bit_cast(uint16_t, (_Float16)f);
    } else {
      const uint32_t u = __float_as_uint(f);
      return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
  }
}

// The same for a value that is no byte (a resampled one, finite and >= 0): U8
// rounds it to nearest-even and clamps to 0 .. 255; the others are tensor_elem
// with val in (float)v's place, not rounded to a byte first.
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::type tensor_elem_of(float val, float s, float b) {
  if constexpr (DT == JPEGR_DTYPE_U8) {
    return (uint8_t)fminf(fmaxf(rintf(val), 0.0f), 255.0f);
  } else {
    const float p = val * s;
    const float f = p + b;
    if constexpr (DT == JPEGR_DTYPE_F32) {
      return __float_as_uint(f);
    } else if constexpr (DT == JPEGR_DTYPE_F16) {
      return __builtin_bit_cast(uint16_t, (_Float16)f);
    } else {
      const uint32_t u = __float_as_uint(f);
      return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
  }
}

// scale3 and bias3 of the call, by value: kernel arguments, so a captured
// launch keeps them
struct TensorNorm {
  float s[3], b[3];
};

}  // namespace
