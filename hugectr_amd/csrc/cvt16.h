// cvt16.h -- 16-bit (fp16 / bf16) <-> fp32 on the device, in the two forms the kernels use: typed
// (float / __half / __hip_bfloat16 through the HIP conversion functions) and raw (the bits of a value
// in an unsigned short, H16<BF>).  Every fp32 -> 16-bit conversion here rounds to nearest even.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace hctr {

// ---- typed -----------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float to_f32(T v);
template <>
__device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ float to_f32<__half>(__half v) { return __half2float(v); }
template <>
__device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <typename T>
__device__ __forceinline__ T from_f32(float v);
template <>
__device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }
template <>
__device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

template <typename T>
__device__ __forceinline__ float ld_as_f32(const T* p) { return to_f32<T>(*p); }
template <typename T>
__device__ __forceinline__ void st_from_f32(T* p, float v) { *p = from_f32<T>(v); }
// v as the 16-bit type holds it
template <typename T>
__device__ __forceinline__ float round16(float v) { return to_f32<T>(from_f32<T>(v)); }

// four consecutive 16-bit values (8 bytes, 8-byte aligned)
template <typename T>
__device__ __forceinline__ float4 cvt4_as_f32(uint2 r);
template <>
__device__ __forceinline__ float4 cvt4_as_f32<__hip_bfloat16>(uint2 r) {
  return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xFFFF0000u),
                     __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xFFFF0000u));
}
template <>
__device__ __forceinline__ float4 cvt4_as_f32<__half>(uint2 r) {
  const float2 fa = __half22float2(*reinterpret_cast<const __half2*>(&r.x));
  const float2 fb = __half22float2(*reinterpret_cast<const __half2*>(&r.y));
  return make_float4(fa.x, fa.y, fb.x, fb.y);
}
template <typename T>
__device__ __forceinline__ float4 ld4_as_f32(const T* p) {
  return cvt4_as_f32<T>(*reinterpret_cast<const uint2*>(p));
}
template <typename T>
__device__ __forceinline__ void st4_from_f32(T* p, float4 v) {
  T h[4] = {from_f32<T>(v.x), from_f32<T>(v.y), from_f32<T>(v.z), from_f32<T>(v.w)};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(h);
}
// (fp32: the four values are 16 bytes, 16-byte aligned)
template <>
__device__ __forceinline__ void st4_from_f32<float>(float* p, float4 v) {
  *reinterpret_cast<float4*>(p) = v;
}

// ---- raw: kernels that move 16-bit data as unsigned short / packed words ---------------------------
template <bool BF>
struct H16Bits;
template <>
struct H16Bits<true> {
  __device__ __forceinline__ static unsigned short from_f32(float v) {
    __bf16 h = (__bf16)v;
    return *reinterpret_cast<unsigned short*>(&h);
  }
  __device__ __forceinline__ static float to_f32(unsigned short u) {
    return __uint_as_float((unsigned)u << 16);
  }
};
template <>
struct H16Bits<false> {
  __device__ __forceinline__ static unsigned short from_f32(float v) {
    _Float16 h = (_Float16)v;
    return *reinterpret_cast<unsigned short*>(&h);
  }
  __device__ __forceinline__ static float to_f32(unsigned short u) {
    _Float16 h = *reinterpret_cast<_Float16*>(&u);
    return (float)h;
  }
};

// a 32-bit word of two 16-bit values: the first one in the low half
__device__ __forceinline__ unsigned short lo16(unsigned v) { return (unsigned short)(v & 0xFFFFu); }
__device__ __forceinline__ unsigned short hi16(unsigned v) { return (unsigned short)(v >> 16); }
__device__ __forceinline__ unsigned pack16(unsigned short a, unsigned short b) {
  return (unsigned)a | ((unsigned)b << 16);
}

template <bool BF>
struct H16 : H16Bits<BF> {
  using H16Bits<BF>::from_f32;
  using H16Bits<BF>::to_f32;
  __device__ __forceinline__ static float lo(unsigned v) { return to_f32(lo16(v)); }
  __device__ __forceinline__ static float hi(unsigned v) { return to_f32(hi16(v)); }
  __device__ __forceinline__ static unsigned pack2(float a, float b) {
    return pack16(from_f32(a), from_f32(b));
  }
  __device__ __forceinline__ static uint2 pack4(float a, float b, float c, float d) {
    return make_uint2(pack2(a, b), pack2(c, d));
  }
};

}  // namespace hctr
