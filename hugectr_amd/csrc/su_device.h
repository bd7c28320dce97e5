// su_device.h -- what the kernels of both units of the sparse update inline (internal, see
// su_units.h): 4-element gradient loads, the optimizer formulas and their row registers, the mean
// combiner's scaling, D / 4 lanes per row as a compile-time constant.  All of it sits in the
// unnamed namespace, like the kernels that use it.
#pragma once
#include <cmath>

#include "su_units.h"

namespace hctr {
namespace {

constexpr int kBlock = 256;

template <typename GradT>
struct Load4;
template <>
struct Load4<float> {
  typedef float4 raw;  // 4 elements as they sit in memory
  __device__ __forceinline__ static raw ld_raw(const float* p) {
    return *reinterpret_cast<const float4*>(p);
  }
  __device__ __forceinline__ static float4 cvt(raw r) { return r; }
  __device__ __forceinline__ static float4 ld(const float* p) {
    return *reinterpret_cast<const float4*>(p);
  }
  __device__ __forceinline__ static float ld1(const float* p) { return *p; }
  __device__ __forceinline__ static float rnd(float v) { return v; }
};
template <>
struct Load4<__half> {
  typedef uint2 raw;
  __device__ __forceinline__ static raw ld_raw(const __half* p) {
    return *reinterpret_cast<const uint2*>(p);
  }
  __device__ __forceinline__ static float4 cvt(raw u) {
    __half2 a = *reinterpret_cast<__half2*>(&u.x), b = *reinterpret_cast<__half2*>(&u.y);
    float2 fa = __half22float2(a), fb = __half22float2(b);
    return make_float4(fa.x, fa.y, fb.x, fb.y);
  }
  __device__ __forceinline__ static float4 ld(const __half* p) { return cvt(ld_raw(p)); }
  __device__ __forceinline__ static float ld1(const __half* p) { return __half2float(*p); }
  __device__ __forceinline__ static float rnd(float v) { return __half2float(__float2half_rn(v)); }
};
template <>
struct Load4<__hip_bfloat16> {
  typedef uint2 raw;
  __device__ __forceinline__ static raw ld_raw(const __hip_bfloat16* p) {
    return *reinterpret_cast<const uint2*>(p);
  }
  __device__ __forceinline__ static float4 cvt(raw u) {
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
                       __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u));
  }
  __device__ __forceinline__ static float4 ld(const __hip_bfloat16* p) { return cvt(ld_raw(p)); }
  __device__ __forceinline__ static float ld1(const __hip_bfloat16* p) {
    return __bfloat162float(*p);
  }
  __device__ __forceinline__ static float rnd(float v) {
    return __bfloat162float(__float2bfloat16(v));
  }
};

// ---- the optimizer on one row -------------------------------------------------------------------
struct OptConst {
  int optimizer, update_type;
  float lr, beta1, beta2, epsilon, mf, scaler;
  float alpha_t;         // lr * adam.bias()
  float alpha_t_common;  // lr / (1 - beta1) (lazy adam)
  float ftrl_l1, ftrl_l2b;  // lambda1, lambda2 + beta / lr
  unsigned long long times;
  int state_half;  // optimizer state carries fp16 values
};

// OptimizerTensor<TypeEmbeddingComp> (R/HugeCTR/include/optimizer.hpp:284-296): with fp16 embeddings
// the reference keeps m / v / accumulators in fp16 -- every kernel converts the stored value to
// float, computes in float and converts the result back on the store; the weight update of the
// same step uses the unrounded float.  Here too (round 4): with state_half the state arrays ARE
// __half arrays (half the footprint and the traffic of the fp32 arrays rounds 1-3 kept); the
// pointers travel as float* and are re-typed where they are dereferenced (ld_state / st_state).
__device__ __forceinline__ float state_store(int state_half, float x) {
  if (!state_half) return x;
  // the fp32 result first, THEN the conversion (two roundings, as the reference's float math +
  // TypeConvertFunc does): without the barrier the compiler folds a preceding multiply into one
  // mixed-precision instruction that rounds the exact product straight to fp16
  asm volatile("" : "+v"(x));
  return __half2float(__float2half_rn(x));
}

// element f of a state array / the four elements from f on (f a multiple of 4)
__device__ __forceinline__ float ld_state1(const float* base, size_t f, int half) {
  return half ? __half2float(reinterpret_cast<const __half*>(base)[f]) : base[f];
}
__device__ __forceinline__ void st_state1(float* base, size_t f, int half, float v) {
  if (half) reinterpret_cast<__half*>(base)[f] = __float2half_rn(v);  // (v is fp16-valued: exact)
  else base[f] = v;
}
__device__ __forceinline__ float4 ld_state4(const float* base, size_t f, int half) {
  if (half)
    return Load4<__half>::cvt(
        *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(base) + f));
  return *reinterpret_cast<const float4*>(base + f);
}
__device__ __forceinline__ void st_state4(float* base, size_t f, int half, const float4& v) {
  if (half) {
    const __half2 a = __floats2half2_rn(v.x, v.y), b = __floats2half2_rn(v.z, v.w);
    uint2 u;
    u.x = *reinterpret_cast<const uint32_t*>(&a);
    u.y = *reinterpret_cast<const uint32_t*>(&b);
    *reinterpret_cast<uint2*>(reinterpret_cast<__half*>(base) + f) = u;
  } else {
    *reinterpret_cast<float4*>(base + f) = v;
  }
}

// one element of one row; formulas cite sparse_optimizer.cu
__device__ __forceinline__ void apply_opt(const OptConst& o, float gi, float& w, float* s0p,
                                          float* s1p, unsigned long long* ptp) {
  switch (o.optimizer) {
    case HCTR_OPT_SGD:  // opt_sgd_kernel :497-518
      w += -o.lr * gi;
      break;
    case kOptStoreSum:
      w = gi;
      break;
    case HCTR_OPT_FTRL: {  // FtrlOptimizer::update, ragged_static_embedding.cu:159-290 (s0 = n, s1 = z)
      float ni = *s0p;
      const float sq = sqrtf(ni + 1.1920929e-07f);
      ni = ni + gi * gi;
      const float sqn = sqrtf(ni + 1.1920929e-07f);
      const float sigma = (sqn - sq) / o.lr;
      const float zi = *s1p + gi - sigma * w;
      const float p = (1.f - 2.f * (float)signbit(zi)) * o.ftrl_l1 - zi;
      const float q = sqn / o.lr + o.ftrl_l2b;
      w = p / q * (float)signbit(o.ftrl_l1 - fabsf(zi));
      *s0p = state_store(o.state_half, ni);
      *s1p = state_store(o.state_half, zi);
    } break;
    case HCTR_OPT_ADAGRAD: {  // opt_adagrad_kernel :410-437 (Global == Local)
      float accum = *s0p + gi * gi;
      *s0p = state_store(o.state_half, accum);
      w += -o.lr * gi / (sqrtf(accum) + o.epsilon);
    } break;
    case HCTR_OPT_ADAM:
      if (o.update_type == HCTR_UPDATE_LOCAL) {  // opt_adam_kernel :379-408
        float mi = o.beta1 * *s0p + (1.0f - o.beta1) * gi;
        float vi = o.beta2 * *s1p + (1.0f - o.beta2) * gi * gi;
        *s0p = state_store(o.state_half, mi);
        *s1p = state_store(o.state_half, vi);
        w += -o.alpha_t * mi / (sqrtf(vi) + o.epsilon);
      } else if (o.update_type == HCTR_UPDATE_GLOBAL) {  // opt_adam_kernel_global :241-265
        *s0p = state_store(o.state_half, *s0p + (1.0f - o.beta1) * gi / o.beta1);
        *s1p = state_store(o.state_half, *s1p + (1.0f - o.beta2) * gi * gi / o.beta2);
      } else {  // opt_adam_kernel_lazy :524-561
        unsigned long long pt = *ptp;
        *ptp = o.times;
        unsigned long long skipped = o.times - pt;
        float b1ps = powf(o.beta1, (float)skipped);
        float a = o.alpha_t_common * sqrtf(1.0f - powf(o.beta2, (float)pt)) /
                  (1.0f - powf(o.beta1, (float)pt)) * (1.0f - b1ps);
        float mi = *s0p, vi = *s1p;
        w += -a * mi / (sqrtf(vi) + o.epsilon);
        mi = b1ps * mi + (1.0f - o.beta1) * gi;
        vi = powf(o.beta2, (float)skipped) * vi + (1.0f - o.beta2) * gi * gi;
        *s0p = state_store(o.state_half, mi);
        *s1p = state_store(o.state_half, vi);
      }
      break;
    case HCTR_OPT_MOMENTUM_SGD:
      if (o.update_type == HCTR_UPDATE_LOCAL) {  // opt_momentum_sgd_kernel :440-465
        float mo = o.mf * *s0p - o.lr * gi;
        *s0p = state_store(o.state_half, mo);
        w += mo;
      } else {  // opt_momentum_sgd_kernel_global :292-312
        *s0p = state_store(o.state_half, *s0p - o.lr * gi / o.mf);
      }
      break;
    case HCTR_OPT_NESTEROV:
      if (o.update_type == HCTR_UPDATE_LOCAL) {  // opt_nesterov_kernel :468-494
        float accm_old = *s0p;
        float accm_new = o.mf * accm_old - o.lr * gi;
        *s0p = state_store(o.state_half, accm_new);
        w += -o.mf * accm_old + (1.0f + o.mf) * accm_new;
      } else {  // nesterov_local_update_kernel_global :352-375
        float accm = *s0p;
        accm -= o.lr * gi;
        *s0p = state_store(o.state_half, accm);
        w -= (1.0f + o.mf) * (o.lr * gi);
      }
      break;
    default: break;
  }
}

__device__ __forceinline__ bool needs_s0(const OptConst& o) {
  return o.optimizer != HCTR_OPT_SGD && o.optimizer != kOptStoreSum;
}
__device__ __forceinline__ bool needs_s1(const OptConst& o) {
  return o.optimizer == HCTR_OPT_ADAM || o.optimizer == HCTR_OPT_FTRL;
}
__device__ __forceinline__ bool needs_pt(const OptConst& o) {
  return o.optimizer == HCTR_OPT_ADAM && o.update_type == HCTR_UPDATE_LAZY_GLOBAL;
}

// Row update shared by seg_apply_kernel and seg_combine_kernel, split in load / compute / store so
// that callers can keep several rows in flight: gi = acc / scaler, then the optimizer on the 4
// elements this lane owns.
struct RowRegs {
  float4 w, s0, s1;
  unsigned long long pt[4];
};

template <int LPR>
__device__ __forceinline__ void row_load(const OptConst& o, uint64_t row, int l, RowRegs& r,
                                         const float* __restrict__ table,
                                         const float* __restrict__ state0,
                                         const float* __restrict__ state1,
                                         const unsigned long long* __restrict__ prev_time) {
  constexpr int D = LPR * 4;
  const size_t f = row * (uint64_t)D + l * 4;
  r.s0 = make_float4(0.f, 0.f, 0.f, 0.f);
  r.w = r.s0;
  if (o.optimizer != kOptStoreSum) r.w = *reinterpret_cast<const float4*>(table + f);
  r.s1 = r.s0;
  r.pt[0] = r.pt[1] = r.pt[2] = r.pt[3] = 1ull;
  if (needs_s0(o)) r.s0 = ld_state4(state0, f, o.state_half);
  if (needs_s1(o)) r.s1 = ld_state4(state1, f, o.state_half);
  if (needs_pt(o)) {
#pragma unroll
    for (int t = 0; t < 4; t++) r.pt[t] = prev_time[f + t];
  }
}

__device__ __forceinline__ void row_compute(const OptConst& o, float4 gi, RowRegs& r) {
  gi.x /= o.scaler;
  gi.y /= o.scaler;
  gi.z /= o.scaler;
  gi.w /= o.scaler;
  apply_opt(o, gi.x, r.w.x, &r.s0.x, &r.s1.x, &r.pt[0]);
  apply_opt(o, gi.y, r.w.y, &r.s0.y, &r.s1.y, &r.pt[1]);
  apply_opt(o, gi.z, r.w.z, &r.s0.z, &r.s1.z, &r.pt[2]);
  apply_opt(o, gi.w, r.w.w, &r.s0.w, &r.s1.w, &r.pt[3]);
}

template <int LPR>
__device__ __forceinline__ void row_store(const OptConst& o, uint64_t row, int l, const RowRegs& r,
                                          float* __restrict__ table, float* __restrict__ state0,
                                          float* __restrict__ state1,
                                          unsigned long long* __restrict__ prev_time) {
  constexpr int D = LPR * 4;
  const size_t f = row * (uint64_t)D + l * 4;
  const bool w_written = !((o.optimizer == HCTR_OPT_ADAM || o.optimizer == HCTR_OPT_MOMENTUM_SGD) &&
                           o.update_type == HCTR_UPDATE_GLOBAL);
  if (w_written) *reinterpret_cast<float4*>(table + f) = r.w;
  if (needs_s0(o)) st_state4(state0, f, o.state_half, r.s0);
  if (needs_s1(o)) st_state4(state1, f, o.state_half, r.s1);
  if (needs_pt(o)) {
#pragma unroll
    for (int t = 0; t < 4; t++) prev_time[f + t] = r.pt[t];
  }
}

// A key that found no row (hash table overflow, or an unseen key of an index-only call) carries
// kInvalidIndex; as a 32-bit sort key that is 0xFFFFFFFF, which create() keeps out of the legal row
// range.  Such positions sort behind every live row and their run is dropped by every writer.
constexpr uint64_t kNoRow = 0xFFFFFFFFull;

template <int LPR>
__device__ __forceinline__ void apply_row_vec4(const OptConst& o, uint64_t row, int l, float4 gi,
                                               float* __restrict__ table,
                                               float* __restrict__ state0,
                                               float* __restrict__ state1,
                                               unsigned long long* __restrict__ prev_time) {
  if (row == kNoRow) return;
  RowRegs r;
  row_load<LPR>(o, row, l, r, table, state0, state1, prev_time);
  row_compute(o, gi, r);
  row_store<LPR>(o, row, l, r, table, state0, state1, prev_time);
}

// number of keys in bucket b (the mean combiner's divisor)
__device__ __forceinline__ int bucket_len(const void* row_offset_v, bool off_is_u32, uint32_t b) {
  if (off_is_u32) {
    const uint32_t* ro = (const uint32_t*)row_offset_v;
    return (int)(ro[b + 1] - ro[b]);
  }
  const long long* ro = (const long long*)row_offset_v;
  return (int)(ro[b + 1] - ro[b]);
}

template <typename GradT>
__device__ __forceinline__ float4 scaled_grad(typename Load4<GradT>::raw r, int combiner, int n) {
  float4 v = Load4<GradT>::cvt(r);
  if (combiner == 1) {
    // backward_mean_align2_kernel (backward_functor.cu:83-104): the scaler is rounded to the
    // gradient type before the multiply; fp32 gradients: rnd() is the identity
    const float sc = Load4<GradT>::rnd(n > 1 ? 1.0f / (float)n : 1.0f);
    v.x = Load4<GradT>::rnd(v.x * sc);
    v.y = Load4<GradT>::rnd(v.y * sc);
    v.z = Load4<GradT>::rnd(v.z * sc);
    v.w = Load4<GradT>::rnd(v.w * sc);
  }
  return v;
}

// D / 4 lanes per row as a compile-time constant: f(std::integral_constant<int, LPR>{}) for
// LPR = lpr in {1, 2, 4, 8, 16, 32, 64} (lpr_supported; anything else is taken as 64)
inline bool lpr_supported(int D) {
  const int lpr = D / 4;
  return D % 4 == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0;
}
template <typename F>
inline auto with_lpr(int lpr, F&& f) {
  switch (lpr) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

inline OptConst opt_const(const OptState& opt) {
  OptConst o;
  o.optimizer = opt.optimizer;
  o.update_type = opt.update_type;
  o.lr = opt.lr;
  o.beta1 = opt.beta1;
  o.beta2 = opt.beta2;
  o.epsilon = opt.epsilon;
  o.mf = opt.momentum_factor;
  o.scaler = opt.scaler;
  o.times = opt.times;
  // AdamOptHyperParams::bias() (optimizer.hpp:58-60): double pow, rounded to float, times lr
  const float bias = (float)(std::sqrt(1.0 - std::pow((double)opt.beta2, (double)opt.times)) /
                             (1.0 - std::pow((double)opt.beta1, (double)opt.times)));
  o.alpha_t = opt.lr * bias;
  o.alpha_t_common = opt.lr / (1.0f - opt.beta1);
  o.ftrl_l1 = opt.ftrl_lambda1;
  o.ftrl_l2b = opt.ftrl_lambda2 + opt.ftrl_beta / opt.lr;
  o.state_half = opt.state_half;
  return o;
}

}  // namespace
}  // namespace hctr
