// dense_ops.hip -- the dense ops next to the GEMMs: the DCN cross layers' element-wise kernels and
// the MLP edge kernels (ReLU backward + bias gradient, split-K group sums, SGD / Ftrl with the 16-bit
// shadow copy, BCE loss, the logit head, the skinny first layer).  The dot interaction is interaction.hip,
// the cross layers' GEMMs are cross_gemm.hip.
//
// MultiCrossLayer<T> (DCN v1): R/HugeCTR/src/layers/multi_cross_layer.cu:582-601 (fprop functor),
//   :671-812 (bprop) -- 4 element-wise kernels + a gemv per layer in the reference; here all layers
//   run in one launch with x0/x_l held in registers (one wavefront per row).
#include "block_prims.h"
#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

// ================================================================================================
// DCN v1 cross layers: x_{l+1} = x0 * (x_l . w_l) + b_l + x_l   (one wavefront per row)
// ================================================================================================
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <int NPL>
__global__ void __launch_bounds__(kBlock)
    cross_v1_fwd_kernel(size_t batch, int w, int layers, const float* __restrict__ x0,
                        const float* __restrict__ kernels, const float* __restrict__ biases,
                        float* __restrict__ outputs, float* __restrict__ hiddens) {
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const size_t nwaves = ((size_t)gridDim.x * kBlock) >> 6;
  for (size_t row = wave; row < batch; row += nwaves) {
    float a0[NPL], xl[NPL];
#pragma unroll
    for (int t = 0; t < NPL; t++) {
      const int i = lane + 64 * t;
      a0[t] = (i < w) ? x0[row * w + i] : 0.f;
      xl[t] = a0[t];
    }
    for (int l = 0; l < layers; l++) {
      const float* k = kernels + (size_t)l * w;
      const float* bi = biases + (size_t)l * w;
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < NPL; t++) {
        const int i = lane + 64 * t;
        if (i < w) part += xl[t] * k[i];
      }
      const float hsum = wave_sum(part);
      if (lane == 0) hiddens[(size_t)l * batch + row] = hsum;
      float* o = outputs + ((size_t)l * batch + row) * w;
#pragma unroll
      for (int t = 0; t < NPL; t++) {
        const int i = lane + 64 * t;
        if (i < w) {
          float v = a0[t] * hsum;
          v = v + xl[t];
          v = v + bi[i];
          xl[t] = v;
          o[i] = v;
        }
      }
    }
  }
}

// backward: per row local math; dW/db column sums go to per-wave partial rows in `partials`
// [num_waves][layers][2][w], reduced in fixed order by cross_v1_reduce_kernel (deterministic).
// LDS = true: one wavefront per workgroup keeps its dW/db partial rows in LDS (2*layers*w floats)
// instead of read-modify-writing them in global memory for every row -- the per-row RMW chain
// through L2 made the backward 12x slower than the forward at the DCN shape.
template <int NPL, bool LDS>
__global__ void __launch_bounds__(kBlock)
    cross_v1_bwd_kernel(size_t batch, int w, int layers, const float* __restrict__ x0,
                        const float* __restrict__ kernels, const float* __restrict__ outputs,
                        const float* __restrict__ hiddens, const float* __restrict__ out_grad,
                        float* __restrict__ in_grad, float* __restrict__ partials) {
  HCTR_DYN_LDS(float, cross_lds);
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  float* gmy = partials + wave * (size_t)layers * 2 * w;
  float* my = LDS ? cross_lds : gmy;
  for (int i = lane; i < layers * 2 * w; i += 64) my[i] = 0.f;
  // (entry i is cleared / copied out by lane i % 64 but accumulated by the lane that owns its
  //  COLUMN: the partial rows cross lanes at both ends of the row loop)
  __builtin_amdgcn_wave_barrier();
  for (size_t row = wave; row < batch; row += nwaves) {
    float a0[NPL], dy[NPL], dx0[NPL];
#pragma unroll
    for (int t = 0; t < NPL; t++) {
      const int i = lane + 64 * t;
      a0[t] = (i < w) ? x0[row * w + i] : 0.f;
      dy[t] = (i < w) ? out_grad[row * w + i] : 0.f;
      dx0[t] = 0.f;
    }
    for (int l = layers - 1; l >= 0; l--) {
      const float hsum = hiddens[(size_t)l * batch + row];
      const float* k = kernels + (size_t)l * w;
      const float* xprev = (l == 0) ? x0 + row * w : outputs + ((size_t)(l - 1) * batch + row) * w;
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < NPL; t++) {
        dx0[t] += dy[t] * hsum;  // row_scaling + matrix_add
        part += dy[t] * a0[t];   // matrix_pair_mul
      }
      const float tv = wave_sum(part);
      float* dwp = my + (size_t)l * 2 * w;
      float* dbp = dwp + w;
#pragma unroll
      for (int t = 0; t < NPL; t++) {
        const int i = lane + 64 * t;
        if (i < w) {
          dwp[i] += xprev[i] * tv;  // row_scaling_sum
          dbp[i] += dy[t];          // rows_sum
          dy[t] = dy[t] + tv * k[i];  // out_product + matrix_add
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NPL; t++) {
      const int i = lane + 64 * t;
      if (i < w) in_grad[row * w + i] = dx0[t] + dy[t];
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (LDS)
    for (int i = lane; i < layers * 2 * w; i += 64) gmy[i] = my[i];
}

// column sums of the per-wave partial rows: a workgroup owns 32 columns x 8 row groups; the 8
// group sums are added in fixed order (deterministic)
__global__ void __launch_bounds__(kBlock)
    cross_v1_reduce_kernel(size_t nwaves, int w, int layers, const float* __restrict__ partials,
                           float* __restrict__ kernel_grads, float* __restrict__ bias_grads) {
  __shared__ float red[kBlock];
  const size_t total = (size_t)layers * 2 * w;
  const size_t i = (size_t)blockIdx.x * 32 + (threadIdx.x & 31);
  const int tg = threadIdx.x >> 5;
  float s = 0.f;
  if (i < total) {
#pragma unroll 8
    for (size_t q = tg; q < nwaves; q += 8) s += partials[q * total + i];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (tg == 0 && i < total) {
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++) sum += red[k * 32 + threadIdx.x];
    const int l = (int)(i / (2 * w)), rem = (int)(i % (2 * w));
    if (rem < w) kernel_grads[(size_t)l * w + rem] = sum;
    else bias_grads[(size_t)l * w + (rem - w)] = sum;
  }
}

// ================================================================================================
// Fused ReLU backward + bias gradient for the MLP layers around the path:
//   dz[b][n] = dy[b][n] * (y[b][n] > 0),   db[n] = sum_b dz[b][n]
// PyTorch issues threshold_backward (read dy,y / write dz) and a column-sum reduction (read dz)
// as two launches; fused, dz is consumed from registers.  Two-stage, fixed-order column sums
// (deterministic): stage 1 writes partial[row_tile][n], stage 2 adds the tiles in order.
// ================================================================================================
constexpr int kRbRows = 128;  // rows per workgroup

// rows per workgroup of cross_v2_bwd_step_kernel: 128 at most, fewer (a power of two >= 16) while
// the grid would stay below ~2 k workgroups -- 64 tiles of 128 rows at batch 8192 left three
// quarters of the CUs idle
inline int cross_step_rows_per_tile(size_t batch, int width) {
  const int n8 = width / 8;
  const int cw = n8 < kBlock ? n8 : kBlock;
  const size_t col_blocks = (size_t)((n8 + cw - 1) / cw);
  int rpt = 128;
  while (rpt > 16 && ((batch + rpt - 1) / rpt) * col_blocks < 2048) rpt >>= 1;
  return rpt;
}

// thread t of a workgroup owns 16-byte column vector (t % cw) and walks rows (t / cw), +rg, ...;
// cw = min(n/8, 256), rg = 256 / cw row groups; the rg partial sums meet in LDS in fixed order.
template <bool BF>
__global__ void __launch_bounds__(kBlock)
    relu_bwd_bias_kernel(size_t rows, int n, int cw, int rg, const unsigned short* __restrict__ dy,
                         const unsigned short* __restrict__ y, unsigned short* __restrict__ dz,
                         float* __restrict__ partial) {
  using H = H16<BF>;
  __shared__ float red[kBlock * 8];
  const int n8 = n / 8;
  const int c8 = threadIdx.x % cw, g = threadIdx.x / cw;
  const bool live = g < rg;
  const size_t r0 = (size_t)blockIdx.x * kRbRows;
  const size_t r1 = r0 + kRbRows < rows ? r0 + kRbRows : rows;
  for (int cc = c8; cc - c8 < n8; cc += cw) {  // uniform trip count: every thread reaches the barriers
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live && cc < n8) {
#pragma unroll 4
      for (size_t r = r0 + g; r < r1; r += rg) {
        const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + r * n + cc * 8);
        const u32x4 av = *reinterpret_cast<const u32x4*>(y + r * n + cc * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const unsigned short g0 = (unsigned short)(gv[e] & 0xFFFFu);
          const unsigned short g1 = (unsigned short)(gv[e] >> 16);
          const float y0 = H::to_f32((unsigned short)(av[e] & 0xFFFFu));
          const float y1 = H::to_f32((unsigned short)(av[e] >> 16));
          const unsigned short z0 = y0 > 0.f ? g0 : (unsigned short)0;
          const unsigned short z1 = y1 > 0.f ? g1 : (unsigned short)0;
          acc[2 * e] += H::to_f32(z0);
          acc[2 * e + 1] += H::to_f32(z1);
          o[e] = (unsigned)z0 | ((unsigned)z1 << 16);
        }
        *reinterpret_cast<u32x4*>(dz + r * n + cc * 8) = o;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) red[e * kBlock + threadIdx.x] = acc[e];
    __syncthreads();
    if (g == 0 && cc < n8) {
      float* p = partial + (size_t)blockIdx.x * n + cc * 8;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float sum = 0.f;
        for (int k = 0; k < rg; k++) sum += red[e * kBlock + k * cw + c8];
        p[e] = sum;
      }
    }
    __syncthreads();
  }
}

// ================================================================================================
// DCN-v2 cross layer, the elementwise step of one layer's backward in the activations' 16-bit type
// (MultiCrossBackwardFunctorv2: fused_mul_fma3, R/HugeCTR/src/layers/multi_cross_layer.cu:391-424,
// 127-165 -- S0 = dY .* X0, dX += dY .* H, one rounding per element as its paired-half kernel
// rounds -- and the bias gradient db = column sums of S0, which the reference takes in the
// epilogue of the dV GEMM, :770-776): dY is read once for both products, S0 is summed from
// registers.  Thread layout and the two-stage fixed-order column sums are relu_bwd_bias_kernel's.
// FIRST (the last layer, visited first): dX = dY .* H, the accumulator is not read (nor cleared
// beforehand).
// ================================================================================================
template <bool BF, bool FIRST>
__global__ void __launch_bounds__(kBlock)
    cross_v2_bwd_step_kernel(size_t rows, int n, int cw, int rg, int rpt,
                             const unsigned short* __restrict__ dy,
                             const unsigned short* __restrict__ x0,
                             const unsigned short* __restrict__ hm, unsigned short* __restrict__ acc_io,
                             unsigned short* __restrict__ s0, float* __restrict__ partial) {
  using H = H16<BF>;
  __shared__ float red[kBlock * 8];
  const int n8 = n / 8;
  const int c8 = threadIdx.x % cw, g = threadIdx.x / cw;
  const bool live = g < rg;
  // a workgroup = rpt rows x cw 16-byte column vectors (blockIdx.y picks the column block): the
  // grid is (row tiles, column blocks), sized by the host for >= ~1 k workgroups at any batch
  const size_t r0 = (size_t)blockIdx.x * (size_t)rpt;
  const size_t r1 = r0 + (size_t)rpt < rows ? r0 + (size_t)rpt : rows;
  const int cc = (int)blockIdx.y * cw + c8;
  {
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live && cc < n8) {
#pragma unroll 4
      for (size_t r = r0 + g; r < r1; r += rg) {
        const size_t at = r * n + cc * 8;
        const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + at);
        const u32x4 xv = *reinterpret_cast<const u32x4*>(x0 + at);
        const u32x4 hv = *reinterpret_cast<const u32x4*>(hm + at);
        u32x4 av = {0u, 0u, 0u, 0u};
        if (!FIRST) av = *reinterpret_cast<const u32x4*>(acc_io + at);
        u32x4 so, ao;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float g0 = H::to_f32((unsigned short)(gv[e] & 0xFFFFu));
          const float g1 = H::to_f32((unsigned short)(gv[e] >> 16));
          // (the product of two 16-bit values is exact in fp32: one rounding, to the 16-bit type)
          const unsigned short p0 = H::from_f32(g0 * H::to_f32((unsigned short)(xv[e] & 0xFFFFu)));
          const unsigned short p1 = H::from_f32(g1 * H::to_f32((unsigned short)(xv[e] >> 16)));
          sum[2 * e] += H::to_f32(p0);
          sum[2 * e + 1] += H::to_f32(p1);
          so[e] = (unsigned)p0 | ((unsigned)p1 << 16);
          float a0 = g0 * H::to_f32((unsigned short)(hv[e] & 0xFFFFu));
          float a1 = g1 * H::to_f32((unsigned short)(hv[e] >> 16));
          if (!FIRST) {
            a0 += H::to_f32((unsigned short)(av[e] & 0xFFFFu));
            a1 += H::to_f32((unsigned short)(av[e] >> 16));
          }
          ao[e] = (unsigned)H::from_f32(a0) | ((unsigned)H::from_f32(a1) << 16);
        }
        *reinterpret_cast<u32x4*>(s0 + at) = so;
        *reinterpret_cast<u32x4*>(acc_io + at) = ao;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) red[e * kBlock + threadIdx.x] = sum[e];
    __syncthreads();
    if (g == 0 && cc < n8) {
      float* p = partial + (size_t)blockIdx.x * n + cc * 8;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float t = 0.f;
        for (int k = 0; k < rg; k++) t += red[e * kBlock + k * cw + c8];
        p[e] = t;
      }
    }
    __syncthreads();
  }
}

// db[c..c+3] = sum over tiles of partial[tile][c..c+3]: a workgroup owns 8 float4 column groups x 32
// tile groups; the 32 group sums are added in fixed order through LDS.
__global__ void __launch_bounds__(kBlock)
    colsum_partials_kernel(size_t tiles, int n, const float* __restrict__ partial,
                           float* __restrict__ db) {
  __shared__ f32x4 red[kBlock];
  const int c4 = blockIdx.x * 8 + (threadIdx.x & 7), tg = threadIdx.x >> 3;
  const bool live = c4 * 4 < n;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll 8
    for (size_t t = tg; t < tiles; t += 32)
      s += *reinterpret_cast<const f32x4*>(partial + t * n + c4 * 4);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (tg == 0 && live) {
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 32; k++) sum += red[k * 8 + threadIdx.x];
    *reinterpret_cast<f32x4*>(db + c4 * 4) = sum;
  }
}

// out[i] = sum_g in[g][i] (fixed order), 16-bit partial products of a split-K GEMM -> fp32
template <bool BF>
__global__ void __launch_bounds__(kBlock)
    sum_groups_kernel(int groups, size_t n8, const unsigned short* __restrict__ in,
                      float* __restrict__ out) {
  using H = H16<BF>;
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n8) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int g = 0; g < groups; g++) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((size_t)g * n8 + i) * 8);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      acc[2 * e] += H::to_f32((unsigned short)(v[e] & 0xFFFFu));
      acc[2 * e + 1] += H::to_f32((unsigned short)(v[e] >> 16));
    }
  }
  f32x4* o = reinterpret_cast<f32x4*>(out + i * 8);
  o[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  o[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// the dense SGD step as ONE expression for every kernel that takes it (f32x4 or float): a parameter
// rounds the same (contraction included) whichever kernel updates it
template <typename V>
__device__ __forceinline__ V sgd_apply(V w, V g, float lr, float grad_scale) {
  w -= lr * grad_scale * g;
  return w;
}

// dense SGD step fused with the refresh of the 16-bit compute copy: w -= lr * g; w16 = (T16)w
template <bool BF>
__global__ void __launch_bounds__(kBlock)
    sgd_shadow_kernel(size_t n4, float lr, float grad_scale, float* __restrict__ w,
                      const float* __restrict__ g, unsigned short* __restrict__ w16) {
  using H = H16<BF>;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * kBlock) {
    f32x4 wv = reinterpret_cast<f32x4*>(w)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    wv = sgd_apply(wv, gv, lr, grad_scale);
    reinterpret_cast<f32x4*>(w)[i] = wv;
    const unsigned lo = (unsigned)H::from_f32(wv[0]) | ((unsigned)H::from_f32(wv[1]) << 16);
    const unsigned hi = (unsigned)H::from_f32(wv[2]) | ((unsigned)H::from_f32(wv[3]) << 16);
    reinterpret_cast<uint2*>(w16)[i] = make_uint2(lo, hi);
  }
}

// ================================================================================================
// Dense Ftrl (ftrl_update_kernel and its launch, R/HugeCTR/src/optimizers/ftrl_optimizer.cu:28-43,
// 92-93).  Like sgd_apply, the step is ONE expression for every kernel that takes it (f32x4 or
// float), so a parameter rounds the same whichever kernel updates it.
//   g = grad * grad_scale;  n' = n + g*g;  z' = z + g + (sqrt(n + eps) - sqrt(n' + eps)) * w / lr
//   w' = |z'| > lambda1 ? (lambda1 * sgn(z') - z') / (sqrt(n' + eps) / lr + l2) : 0
// with eps = FLT_EPSILON, l2 = lambda2 + beta / lr (formed once on the host) and sgn = +1 for a
// clear sign bit.  A parameter whose gradient is 0 on the first step becomes 0: z' stays 0.
// ================================================================================================
struct FtrlHp {
  float lr, lambda1, l2, grad_scale;
};

__device__ __forceinline__ float ftrl_apply(float w, float& z, float& n, float grad, FtrlHp h) {
  constexpr float eps = 1.1920928955078125e-7f;  // FLT_EPSILON
  const float g = grad * h.grad_scale;
  const float n_new = n + g * g;
  const float root = sqrtf(n_new + eps);
  const float z_new = z + g + (sqrtf(n + eps) - root) * w / h.lr;
  const float x = (__builtin_signbitf(z_new) ? -h.lambda1 : h.lambda1) - z_new;
  const float y = root / h.lr + h.l2;
  n = n_new;
  z = z_new;
  return fabsf(z_new) > h.lambda1 ? x / y : 0.f;
}

__device__ __forceinline__ f32x4 ftrl_apply(f32x4 w, f32x4& z, f32x4& n, f32x4 grad, FtrlHp h) {
  f32x4 out;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    float ze = z[e], ne = n[e];
    out[e] = ftrl_apply(w[e], ze, ne, grad[e], h);
    z[e] = ze;
    n[e] = ne;
  }
  return out;
}

// the flat form: the twin of sgd_shadow_kernel (SHADOW 0: no 16-bit copy, 1: fp16, 2: bf16)
template <int SHADOW>
__global__ void __launch_bounds__(kBlock)
    ftrl_shadow_kernel(size_t n4, FtrlHp h, float* __restrict__ w, float* __restrict__ z,
                       float* __restrict__ nacc, const float* __restrict__ g,
                       unsigned short* __restrict__ w16) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * kBlock) {
    f32x4 zv = reinterpret_cast<f32x4*>(z)[i];
    f32x4 nv = reinterpret_cast<f32x4*>(nacc)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    const f32x4 wv = ftrl_apply(reinterpret_cast<f32x4*>(w)[i], zv, nv, gv, h);
    reinterpret_cast<f32x4*>(w)[i] = wv;
    reinterpret_cast<f32x4*>(z)[i] = zv;
    reinterpret_cast<f32x4*>(nacc)[i] = nv;
    if (SHADOW) {
      using H = H16<SHADOW == 2>;
      const unsigned lo = (unsigned)H::from_f32(wv[0]) | ((unsigned)H::from_f32(wv[1]) << 16);
      const unsigned hi = (unsigned)H::from_f32(wv[2]) | ((unsigned)H::from_f32(wv[3]) << 16);
      reinterpret_cast<uint2*>(w16)[i] = make_uint2(lo, hi);
    }
  }
}

// the segmented form: parameter tensors that do not live in one buffer; their gradients and the
// state do (flat g / z / n, a segment's elements at `off`).  A block takes kFtrlSegElems elements
// of one segment and finds the segment like dense_grad_finish_kernel does.  Groups of 4 go through
// the vector form when the segment allows it (w 16-byte aligned, off % 4 == 0), the tail and
// everything else through the scalar form of the same expression.
constexpr int kFtrlSegElems = HCTR_FTRL_SEG_BLOCK_ELEMS;
static_assert(kFtrlSegElems == kBlock * 4, "a thread takes 4 elements");

__global__ void __launch_bounds__(kBlock)
    ftrl_segments_kernel(const hctr_ftrl_seg* __restrict__ segs, int nseg, FtrlHp h,
                         float* __restrict__ z, float* __restrict__ nacc,
                         const float* __restrict__ g) {
  int si = -1;
  for (int base = 0; base < nseg; base += 64) {
    const int t = base + (int)(threadIdx.x & 63);
    const bool in = t < nseg && segs[t].block0 <= (long long)blockIdx.x;
    si += (int)__popcll(__ballot(in));
  }
  if (si < 0) return;  // (a table whose first segment does not start at block 0)
  const hctr_ftrl_seg sg = segs[si];
  const size_t cnt = (size_t)sg.n, off = (size_t)sg.off;
  float* w = reinterpret_cast<float*>(sg.w);
  const size_t e0 = ((size_t)((long long)blockIdx.x - sg.block0) * kBlock + threadIdx.x) * 4;
  if (e0 >= cnt) return;
  const bool vec = (sg.w & 15) == 0 && (off & 3) == 0 && e0 + 4 <= cnt;
  if (vec) {
    f32x4 zv = *reinterpret_cast<f32x4*>(z + off + e0);
    f32x4 nv = *reinterpret_cast<f32x4*>(nacc + off + e0);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + off + e0);
    const f32x4 wv = ftrl_apply(*reinterpret_cast<f32x4*>(w + e0), zv, nv, gv, h);
    *reinterpret_cast<f32x4*>(w + e0) = wv;
    *reinterpret_cast<f32x4*>(z + off + e0) = zv;
    *reinterpret_cast<f32x4*>(nacc + off + e0) = nv;
    return;
  }
  const size_t e1 = e0 + 4 < cnt ? e0 + 4 : cnt;
  for (size_t e = e0; e < e1; e++) {
    float zs = z[off + e], ns = nacc[off + e];
    w[e] = ftrl_apply(w[e], zs, ns, g[off + e], h);
    z[off + e] = zs;
    nacc[off + e] = ns;
  }
}

// ================================================================================================
// BinaryCrossEntropyLoss (R/HugeCTR/src/loss.cu:231-262): per-sample stable BCE-with-logits,
// the logit gradient scaled by grad_scale (= scaler / batch / total_gpu_count in the reference),
// and the mean loss.  The reference accumulates the block sums with atomicAdd; here the block
// partials are added in fixed order by the last launch (deterministic).
// ================================================================================================
constexpr int kBceBlocks = 256;

template <typename T>
__global__ void __launch_bounds__(kBlock)
    bce_kernel(size_t batch, const T* __restrict__ logit, const float* __restrict__ label,
               float grad_scale, T* __restrict__ dlogit, float* __restrict__ partial) {
  __shared__ float smem[kBlock / 64];
  float val = 0.f;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < batch;
       i += (size_t)gridDim.x * kBlock) {
    const float x = ld_as_f32(logit + i);
    const float y = label[i];
    float g;
    if (x >= 0.f) {
      const float e = expf(-x);
      g = (1.f - y) - e / (1.f + e);
      val += x * (1.f - y) + logf(1.f + e);
    } else {
      const float e = expf(x);
      g = -y + e / (1.f + e);
      val += -x * y + logf(1.f + e);
    }
    if (dlogit) st_from_f32(dlogit + i, g * grad_scale);
  }
  const float tot = block_reduce_sum<float, kBlock>(val, smem);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock)
    bce_finish_kernel(int blocks, size_t batch, const float* __restrict__ partial,
                      float* __restrict__ loss) {
  __shared__ float smem[kBlock / 64];
  const float v = (int)threadIdx.x < blocks ? partial[threadIdx.x] : 0.f;
  const float tot = block_reduce_sum<float, kBlock>(v, smem);
  if (threadIdx.x == 0) *loss = tot / (float)batch;
}

// ---- logit head: the last fully connected layer (K -> 1), BinaryCrossEntropyLoss and their
//      backward in ONE pass over the activations (MLPLayer's last GEMM + loss.cu:231-262).  As
//      library calls this is a GEMV forward, a rank-1 dgrad and a K = batch reduction for the weight
//      gradient -- three badly shaped GEMMs (16 + 17 + 69 us at batch 65536, K = 256) around the
//      loss kernels; here every row of x is read once: z = x.w + b, loss term, dz = (sigmoid(z) -
//      y) * grad_scale, dx = dz * w written back, dw / db / loss accumulated per wavefront and
//      reduced in fixed order (deterministic).
constexpr int kHeadBlocks = 1024;
constexpr int kHeadMaxSeg = 8;  // K <= 64 lanes * 4 elements * 8 segments = 2048

// partial layout per block: [K dw][1 db][1 loss].  A wavefront takes ROWS rows per iteration (ROWS
// independent row loads in flight); NSEG = ceil(K / 256) segments of 64 lanes x 4 elements.
template <typename T, int NSEG, int ROWS>
__global__ void __launch_bounds__(kBlock)
    logit_head_kernel(size_t batch, int K, const T* __restrict__ x, const T* __restrict__ w,
                      const T* __restrict__ bias, const float* __restrict__ label,
                      float grad_scale, T* __restrict__ dx, float* __restrict__ partial) {
  HCTR_DYN_LDS(float, lds);  // [waves][K + 2]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 wr[NSEG], acc[NSEG];
#pragma unroll
  for (int j = 0; j < NSEG; j++) {
    const int k = j * 256 + lane * 4;
    wr[j] = k < K ? ld4_as_f32<T>(w + k) : zero4;
    acc[j] = zero4;
  }
  const float b0 = ld_as_f32(bias);
  float db = 0.f, loss = 0.f;
  const size_t nw = (size_t)gridDim.x * (kBlock / 64);
  for (size_t r0 = ((size_t)blockIdx.x * (kBlock / 64) + wv) * ROWS; r0 < batch; r0 += nw * ROWS) {
    float4 xv[ROWS][NSEG];
    float dot[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
      const size_t r = r0 + i;
      dot[i] = 0.f;
#pragma unroll
      for (int j = 0; j < NSEG; j++) {
        const int k = j * 256 + lane * 4;
        xv[i][j] = (r < batch && k < K) ? ld4_as_f32<T>(x + r * (size_t)K + k) : zero4;
        dot[i] += xv[i][j].x * wr[j].x + xv[i][j].y * wr[j].y + xv[i][j].z * wr[j].z +
                  xv[i][j].w * wr[j].w;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int i = 0; i < ROWS; i++) dot[i] += __shfl_xor(dot[i], o);
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
      const size_t r = r0 + i;
      if (r >= batch) break;  // wave-uniform
      const float z = dot[i] + b0;
      const float y = label[r];
      float g, l;
      if (z >= 0.f) {
        const float e = expf(-z);
        g = (1.f - y) - e / (1.f + e);
        l = z * (1.f - y) + logf(1.f + e);
      } else {
        const float e = expf(z);
        g = -y + e / (1.f + e);
        l = -z * y + logf(1.f + e);
      }
      const float dz = g * grad_scale;
      loss += l;
      db += dz;
#pragma unroll
      for (int j = 0; j < NSEG; j++) {
        const int k = j * 256 + lane * 4;
        if (k < K) {
          acc[j].x += dz * xv[i][j].x;
          acc[j].y += dz * xv[i][j].y;
          acc[j].z += dz * xv[i][j].z;
          acc[j].w += dz * xv[i][j].w;
          if (dx)
            st4_from_f32<T>(dx + r * (size_t)K + k, make_float4(dz * wr[j].x, dz * wr[j].y,
                                                                 dz * wr[j].z, dz * wr[j].w));
        }
      }
    }
  }
  // wavefronts of the block -> LDS -> one partial per block (waves added in order)
  float* mine = lds + wv * (K + 2);
#pragma unroll
  for (int j = 0; j < NSEG; j++) {
    const int k = j * 256 + lane * 4;
    if (k < K) {
      mine[k] = acc[j].x;
      mine[k + 1] = acc[j].y;
      mine[k + 2] = acc[j].z;
      mine[k + 3] = acc[j].w;
    }
  }
  if (lane == 0) {
    mine[K] = db;
    mine[K + 1] = loss;
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * (K + 2);
  for (int k = threadIdx.x; k < K + 2; k += kBlock) {
    float t = 0.f;
    for (int q = 0; q < kBlock / 64; q++) t += lds[q * (K + 2) + k];
    out[k] = t;
  }
}

// fixed-order sum of the block partials: a 1024-thread workgroup owns 64 columns; 16 row groups sum
// consecutive chunks of the partial blocks (coalesced 256-byte reads), then the group sums are
// added in group order
__global__ void __launch_bounds__(1024)
    logit_head_finish_kernel(int blocks, int K, size_t batch, const float* __restrict__ partial,
                             float* __restrict__ dw, float* __restrict__ db,
                             float* __restrict__ loss) {
  __shared__ float part[16][64];
  const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + c;
  const int chunk = (blocks + 15) / 16;
  const int b0 = grp * chunk, b1 = min(blocks, b0 + chunk);
  float t = 0.f;
  if (k < K + 2) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {  // 8 independent loads in flight, added in order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = partial[(size_t)(b + u) * (K + 2) + k];
#pragma unroll
      for (int u = 0; u < 8; u++) t += v[u];
    }
    for (; b < b1; b++) t += partial[(size_t)b * (K + 2) + k];
  }
  part[grp][c] = t;
  __syncthreads();
  if (grp == 0 && k < K + 2) {
    float tot = 0.f;
#pragma unroll
    for (int g = 0; g < 16; g++) tot += part[g][c];
    if (k < K) dw[k] = tot;
    else if (k == K) *db = tot;
    else *loss = tot / (float)batch;
  }
}

// ---- first layer of the bottom MLP: y = relu(x W^T + b) with a handful of input features (K <= 16,
//      DLRM: 13 dense features -> 512).  As a GEMM it is all output traffic and no arithmetic
//      (library kernel: 30 us forward; ReLU backward + bias + a K = batch weight-gradient GEMM with
//      13 columns: 72 us).  Here 128 lanes own one row at a time, a lane 4 consecutive outputs
//      with their K weights in registers; the backward folds dz = dy * (y > 0) into the
//      weight-gradient sum, so dz is never written (the layer has no data gradient).
constexpr int kSkinnyK = 16;       // padded K
constexpr int kSkinnyBlocks = 256;
constexpr int kSkinnyLanes = 128;  // lanes per row, 4 outputs each (N <= 512)
constexpr int kSkinnyBwdBlock = 1024;
constexpr bool kSkinnyBwdMfmaDefault = true;
constexpr int kSkinnyUnroll = 2;   // rows per step and row group in the backward (x2 in flight)

typedef float v2f __attribute__((ext_vector_type(2)));

// x fp32 [B][K] (rounded to T on load, as the 16-bit GEMM path does), w T [N][K], bias T [N].
// A block owns R consecutive rows: their features are staged (rounded, zero-padded to kSkinnyK)
// in LDS once, so the row loop has no global load to wait on -- broadcast LDS reads, packed FMAs
// and a stream of stores.
template <typename T>
__global__ void __launch_bounds__(kBlock)
    skinny_fc_fwd_kernel(size_t batch, int K, int N, int R, const float* __restrict__ x,
                         const T* __restrict__ w, const T* __restrict__ bias, T* __restrict__ y) {
  HCTR_DYN_LDS(float, xs);  // [R][kSkinnyK]
  const int col = threadIdx.x % kSkinnyLanes;
  const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x / kSkinnyLanes);
  const bool live = col * 4 < N;
  const int n0 = live ? col * 4 : 0;
  const size_t rb = (size_t)blockIdx.x * R;
  v2f wr[4][kSkinnyK / 2];
  float br[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    br[j] = ld_as_f32(bias + (size_t)(n0 + j));
#pragma unroll
    for (int k = 0; k < kSkinnyK; k++) {
      // clamped index + select: 64 independent loads, no branch (and no wait) per element
      const float t = ld_as_f32(w + (size_t)(n0 + j) * K + (k < K ? k : K - 1));
      const float v = k < K ? t : 0.f;
      if (k & 1) wr[j][k / 2].y = v;
      else wr[j][k / 2].x = v;
    }
  }
  const size_t last = batch - 1;
  for (int idx = threadIdx.x; idx < R * kSkinnyK; idx += kBlock) {
    const int row = idx / kSkinnyK, k = idx % kSkinnyK;
    const float t = x[min(rb + row, last) * (size_t)K + (k < K ? k : K - 1)];
    xs[idx] = k < K ? round16<T>(t) : 0.f;
  }
  __syncthreads();
  constexpr int kRows = kBlock / kSkinnyLanes;
  for (int row = sub; row < R; row += kRows) {
    const size_t r = rb + row;
    if (r >= batch) break;  // scalar condition
    const float4* xp = reinterpret_cast<const float4*>(xs + row * kSkinnyK);
    v2f acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = v2f{0.f, 0.f};
#pragma unroll
    for (int q = 0; q < kSkinnyK / 4; q++) {
      const float4 xv = xp[q];  // same address in every lane: broadcast
      const v2f lo = v2f{xv.x, xv.y}, hi = v2f{xv.z, xv.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc[j] += lo * wr[j][2 * q];
        acc[j] += hi * wr[j][2 * q + 1];
      }
    }
    if (live)
      st4_from_f32<T>(y + r * (size_t)N + n0,
                      make_float4(fmaxf(acc[0].x + acc[0].y + br[0], 0.f),
                                  fmaxf(acc[1].x + acc[1].y + br[1], 0.f),
                                  fmaxf(acc[2].x + acc[2].y + br[2], 0.f),
                                  fmaxf(acc[3].x + acc[3].y + br[3], 0.f)));
  }
}

// partial per block: [N][kSkinnyK] dw and [N] db interleaved as [N][kSkinnyK + 1].  The loads of the
// next kSkinnyUnroll rows (raw 16-bit words) are issued before the current ones are consumed; row
// numbers are scalar, rows past the end are clamped for the loads and count with weight zero.
template <typename T>
__global__ void __launch_bounds__(kSkinnyBwdBlock)
    skinny_fc_bwd_kernel(size_t batch, int K, int N, const float* __restrict__ x,
                         const T* __restrict__ dy, const T* __restrict__ y,
                         float* __restrict__ partial) {
  HCTR_DYN_LDS(float, lds);  // [N * (kSkinnyK + 1)]
  const int lane = threadIdx.x & 63;
  const int col = threadIdx.x % kSkinnyLanes;
  const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x / kSkinnyLanes);
  const bool live = col * 4 < N;
  const int n0 = live ? col * 4 : 0;
  const int kl = lane < K ? lane : 0;
  v2f acc[4][kSkinnyK / 2];
  float dbv[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    dbv[j] = 0.f;
#pragma unroll
    for (int k = 0; k < kSkinnyK / 2; k++) acc[j][k] = v2f{0.f, 0.f};
  }
  constexpr int kRows = kSkinnyBwdBlock / kSkinnyLanes;
  const size_t step = (size_t)gridDim.x * kRows;
  const size_t first = (size_t)blockIdx.x * kRows + sub;
  const size_t last = batch - 1;
  uint2 g[kSkinnyUnroll], a[kSkinnyUnroll];
  float xl[kSkinnyUnroll];
#pragma unroll
  for (int u = 0; u < kSkinnyUnroll; u++) {
    const size_t r = min(first + (size_t)u * step, last);
    g[u] = *reinterpret_cast<const uint2*>(dy + r * (size_t)N + n0);
    a[u] = *reinterpret_cast<const uint2*>(y + r * (size_t)N + n0);
    xl[u] = x[r * (size_t)K + kl];
  }
  for (size_t r0 = first; r0 < batch; r0 += step * kSkinnyUnroll) {
    uint2 gn[kSkinnyUnroll], an[kSkinnyUnroll];
    float xn[kSkinnyUnroll];
#pragma unroll
    for (int u = 0; u < kSkinnyUnroll; u++) {
      const size_t r = min(r0 + (size_t)(u + kSkinnyUnroll) * step, last);
      gn[u] = *reinterpret_cast<const uint2*>(dy + r * (size_t)N + n0);
      an[u] = *reinterpret_cast<const uint2*>(y + r * (size_t)N + n0);
      xn[u] = x[r * (size_t)K + kl];
    }
#pragma unroll
    for (int u = 0; u < kSkinnyUnroll; u++) {
      if (r0 + (size_t)u * step < batch) {  // scalar condition
        // dz as the unfused path hands it to its GEMM
        const float4 gf = cvt4_as_f32<T>(g[u]), af = cvt4_as_f32<T>(a[u]);
        const float d[4] = {af.x > 0.f ? gf.x : 0.f, af.y > 0.f ? gf.y : 0.f,
                            af.z > 0.f ? gf.z : 0.f, af.w > 0.f ? gf.w : 0.f};
        const float xr = lane < K ? round16<T>(xl[u]) : 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) dbv[j] += d[j];
#pragma unroll
        for (int k = 0; k < kSkinnyK; k += 2) {
          const v2f xk = v2f{__shfl(xr, k), __shfl(xr, k + 1)};
#pragma unroll
          for (int j = 0; j < 4; j++) acc[j][k / 2] += xk * d[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSkinnyUnroll; u++) {
      g[u] = gn[u];
      a[u] = an[u];
      xl[u] = xn[u];
    }
  }
  // the block's row groups add their sums in a fixed order through LDS
  const int stride = kSkinnyK + 1;
  for (int q = 0; q < kRows; q++) {
    if (sub == q && live) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float* d = lds + (size_t)(n0 + j) * stride;
#pragma unroll
        for (int k = 0; k < kSkinnyK; k++) {
          const float v = (k & 1) ? acc[j][k / 2].y : acc[j][k / 2].x;
          d[k] = (q == 0 ? 0.f : d[k]) + v;
        }
        d[kSkinnyK] = (q == 0 ? 0.f : d[kSkinnyK]) + dbv[j];
      }
    }
    __syncthreads();
  }
  float* out = partial + (size_t)blockIdx.x * N * stride;
  for (int i = threadIdx.x; i < N * stride; i += kSkinnyBwdBlock) out[i] = lds[i];
}

// The same backward on the matrix cores.  v_mfma_f32_16x16x4_f32 takes ONE f32 per lane for A and
// for B, so nothing has to be transposed: with D[i][j] = sum_k A[i][k] B[k][j], k = 4 batch rows,
// j = input feature (16 columns: K features, then a column of ones whose sum is db), and
// i = 16 outputs, a lane that loaded 8 consecutive outputs of row (lane >> 4) feeds them to 8
// instructions -- instruction t owns the outputs {8 i + t}: which outputs form a tile is free.
// Products of 16-bit values are exact in f32; the sums are f32 in a fixed order.  A wavefront owns
// 128 outputs x a share of the rows (8 accumulators of 4 registers), 16 rows per step in flight;
// the wavefronts of a block that share outputs add up through LDS in a fixed order.
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int kMfmaUnroll = 4;  // 4-row groups per step and wavefront

template <typename T>
__global__ void __launch_bounds__(kSkinnyBwdBlock)
    skinny_fc_bwd_mfma_kernel(size_t batch, int K, int N, const float* __restrict__ x,
                              const T* __restrict__ dy, const T* __restrict__ y,
                              float* __restrict__ partial) {
  HCTR_DYN_LDS(float, lds);  // [N * (kSkinnyK + 1)]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int kWaves = kSkinnyBwdBlock / 64;
  const int ngroups = (N + 127) / 128;
  const int rsets = kWaves / ngroups;
  const int ng = wv % ngroups, rs = wv / ngroups;
  const bool active = rs < rsets;  // wave-uniform
  const int c = lane & 15, ri = lane >> 4;
  const int n0 = ng * 128 + 8 * c;
  const bool has_n = n0 < N;
  const int n0c = has_n ? n0 : 0;
  const int kc = c < K ? c : K - 1;
  v4f acc[8];
#pragma unroll
  for (int t = 0; t < 8; t++) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
  const size_t last = batch - 1;
  const size_t step = (size_t)gridDim.x * rsets;
  if (active) {
    for (size_t g16 = (size_t)blockIdx.x * rsets + rs; g16 * 16 < batch; g16 += step) {
      uint4 gq[kMfmaUnroll], aq[kMfmaUnroll];
      float xv[kMfmaUnroll];
#pragma unroll
      for (int u = 0; u < kMfmaUnroll; u++) {
        const size_t r = min(g16 * 16 + u * 4 + ri, last);
        gq[u] = *reinterpret_cast<const uint4*>(dy + r * (size_t)N + n0c);
        aq[u] = *reinterpret_cast<const uint4*>(y + r * (size_t)N + n0c);
        xv[u] = x[r * (size_t)K + kc];
      }
#pragma unroll
      for (int u = 0; u < kMfmaUnroll; u++) {
        const bool ok = has_n && g16 * 16 + u * 4 + ri < batch;
        const float4 g0 = cvt4_as_f32<T>(make_uint2(gq[u].x, gq[u].y));
        const float4 g1 = cvt4_as_f32<T>(make_uint2(gq[u].z, gq[u].w));
        const float4 a0 = cvt4_as_f32<T>(make_uint2(aq[u].x, aq[u].y));
        const float4 a1 = cvt4_as_f32<T>(make_uint2(aq[u].z, aq[u].w));
        const float d[8] = {(ok && a0.x > 0.f) ? g0.x : 0.f, (ok && a0.y > 0.f) ? g0.y : 0.f,
                            (ok && a0.z > 0.f) ? g0.z : 0.f, (ok && a0.w > 0.f) ? g0.w : 0.f,
                            (ok && a1.x > 0.f) ? g1.x : 0.f, (ok && a1.y > 0.f) ? g1.y : 0.f,
                            (ok && a1.z > 0.f) ? g1.z : 0.f, (ok && a1.w > 0.f) ? g1.w : 0.f};
        const float b = c < K ? round16<T>(xv[u]) : (c == K ? 1.f : 0.f);
#pragma unroll
        for (int t = 0; t < 8; t++)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[t], b, acc[t], 0, 0, 0);
      }
    }
  }
  // acc[t][reg] = column c of output ng * 128 + 8 * (4 * ri + reg) + t; column K carries db
  const int stride = kSkinnyK + 1;
  const int col = c == K ? kSkinnyK : c;
  for (int q = 0; q < rsets; q++) {
    if (active && rs == q && c <= K) {
#pragma unroll
      for (int t = 0; t < 8; t++) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int n = ng * 128 + 8 * (4 * ri + reg) + t;
          if (n < N) {
            float* d = lds + (size_t)n * stride + col;
            *d = (q == 0 ? 0.f : *d) + acc[t][reg];
          }
        }
      }
    }
    __syncthreads();
  }
  float* out = partial + (size_t)blockIdx.x * N * stride;
  for (int i = threadIdx.x; i < N * stride; i += kSkinnyBwdBlock) out[i] = lds[i];
}

// dw [N][K] and db [N] from the block partials: 64 elements per block, 16 groups of lanes each sum
// a consecutive chunk of the partial blocks (8 loads in flight), group sums added in group order
__global__ void __launch_bounds__(1024)
    skinny_fc_finish_kernel(int blocks, int K, int N, const float* __restrict__ partial,
                            float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float part[16][64];
  const int stride = kSkinnyK + 1;
  const int total = N * stride;
  const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  const int chunk = (blocks + 15) / 16;
  const int b0 = grp * chunk, b1 = min(blocks, b0 + chunk);
  float t = 0.f;
  if (i < total) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = partial[(size_t)(b + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; u++) t += v[u];
    }
    for (; b < b1; b++) t += partial[(size_t)b * total + i];
  }
  part[grp][c] = t;
  __syncthreads();
  if (grp == 0 && i < total) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) tot += part[q][c];
    const int n = i / stride, k = i % stride;
    if (k == kSkinnyK) db[n] = tot;
    else if (k < K) dw[(size_t)n * K + k] = tot;
  }
}

// ================================================================================================
// Gradient finish: ONE launch per step takes every fixed-order partial sum the backward's producers
// left (split-K weight-gradient products, bias tile partials, the logit head's and the skinny first
// layer's block partials) to its place in the flat gradient buffer -- or, SGD = true, straight
// through the optimizer step into the fp32 masters and their 16-bit copy.  A workgroup finds its
// segment in the table by its block number; each segment kind adds in the order of the kernel it
// stands in for (sum_groups / colsum_partials / logit_head_finish / skinny_fc_finish), term for
// term, so every gradient keeps its bits.
// ================================================================================================
template <bool SGD>
__device__ __forceinline__ void finish_store4(const hctr_dense_seg& sg, size_t at, f32x4 gv,
                                              float lr, float grad_scale) {
  if (!SGD) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(sg.g) + at) = gv;
    return;
  }
  f32x4* wp = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(sg.w) + at);
  const f32x4 wv = sgd_apply(*wp, gv, lr, grad_scale);
  *wp = wv;
  unsigned lo, hi;
  if (sg.bf16) {
    lo = (unsigned)H16<true>::from_f32(wv[0]) | ((unsigned)H16<true>::from_f32(wv[1]) << 16);
    hi = (unsigned)H16<true>::from_f32(wv[2]) | ((unsigned)H16<true>::from_f32(wv[3]) << 16);
  } else {
    lo = (unsigned)H16<false>::from_f32(wv[0]) | ((unsigned)H16<false>::from_f32(wv[1]) << 16);
    hi = (unsigned)H16<false>::from_f32(wv[2]) | ((unsigned)H16<false>::from_f32(wv[3]) << 16);
  }
  *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(sg.w16) + at) = make_uint2(lo, hi);
}

template <bool SGD>
__device__ __forceinline__ void finish_store1(const hctr_dense_seg& sg, size_t at, float gv,
                                              float lr, float grad_scale) {
  if (!SGD) {
    reinterpret_cast<float*>(sg.g)[at] = gv;
    return;
  }
  float* wp = reinterpret_cast<float*>(sg.w) + at;
  const float wv = sgd_apply(*wp, gv, lr, grad_scale);
  *wp = wv;
  reinterpret_cast<unsigned short*>(sg.w16)[at] =
      sg.bf16 ? H16<true>::from_f32(wv) : H16<false>::from_f32(wv);
}

// sum_groups_kernel's sum for element group i
template <bool BF>
__device__ __forceinline__ void finish_sum_groups(int groups, size_t n8, size_t i,
                                                  const unsigned short* __restrict__ in,
                                                  f32x4& lo, f32x4& hi) {
  using H = H16<BF>;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // (the usual 16 groups: all 16 loads in flight, added in group order)
#pragma unroll 16
  for (int g = 0; g < groups; g++) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((size_t)g * n8 + i) * 8);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      acc[2 * e] += H::to_f32((unsigned short)(v[e] & 0xFFFFu));
      acc[2 * e + 1] += H::to_f32((unsigned short)(v[e] >> 16));
    }
  }
  lo = f32x4{acc[0], acc[1], acc[2], acc[3]};
  hi = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// the chunked block sum of logit_head_finish_kernel / skinny_fc_finish_kernel for 64 consecutive
// columns: 16 chunk groups, each added in block order, then the groups in order.  Here a wavefront
// takes four of the groups, one after the other (256 threads instead of 1024): the same sums.
__device__ __forceinline__ float finish_block_chunks(float (*part)[64], int blocks, size_t stride,
                                                     size_t col, bool live,
                                                     const float* __restrict__ partial) {
  const int c = threadIdx.x & 63;
  const int chunk = (blocks + 15) / 16;
  for (int grp = threadIdx.x >> 6; grp < 16; grp += kBlock / 64) {
    const int b0 = grp * chunk, b1 = min(blocks, b0 + chunk);
    float t = 0.f;
    if (live) {
      int b = b0;
      for (; b + 8 <= b1; b += 8) {  // 8 independent loads in flight, added in order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = partial[(size_t)(b + u) * stride + col];
#pragma unroll
        for (int u = 0; u < 8; u++) t += v[u];
      }
      for (; b < b1; b++) t += partial[(size_t)b * stride + col];
    }
    part[grp][c] = t;
  }
  __syncthreads();
  float tot = 0.f;
  if (threadIdx.x < 64 && live) {
#pragma unroll
    for (int g = 0; g < 16; g++) tot += part[g][c];
  }
  return tot;
}

template <bool SGD>
__global__ void __launch_bounds__(kBlock)
    dense_grad_finish_kernel(const hctr_dense_seg* __restrict__ segs, int nseg, float lr,
                             float grad_scale, float* __restrict__ loss) {
  __shared__ f32x4 red[kBlock];  // colsum: [32 tile groups][8]; head / skinny: float [16][64]
  // the block's segment = the last one whose first block is not past it: every wavefront looks at
  // 64 table entries per step (one load latency, not one per segment)
  int si = -1;
  for (int base = 0; base < nseg; base += 64) {
    const int t = base + (int)(threadIdx.x & 63);
    const bool in = t < nseg && segs[t].block0 <= (long long)blockIdx.x;
    si += (int)__popcll(__ballot(in));
  }
  const hctr_dense_seg sg = segs[si];
  const int blk = (int)((long long)blockIdx.x - sg.block0);
  const size_t dst = (size_t)sg.dst, dst2 = (size_t)sg.dst2;
  switch ((int)sg.kind) {
    case HCTR_DENSE_SEG_SUM_GROUPS: {
      const size_t n8 = (size_t)sg.n / 8;
      const size_t i = (size_t)blk * kBlock + threadIdx.x;
      if (i >= n8) return;
      const unsigned short* in = reinterpret_cast<const unsigned short*>(sg.src);
      f32x4 lo, hi;
      if (sg.src_bf16) finish_sum_groups<true>((int)sg.count, n8, i, in, lo, hi);
      else finish_sum_groups<false>((int)sg.count, n8, i, in, lo, hi);
      finish_store4<SGD>(sg, dst + i * 8, lo, lr, grad_scale);
      finish_store4<SGD>(sg, dst + i * 8 + 4, hi, lr, grad_scale);
      return;
    }
    case HCTR_DENSE_SEG_COLSUM: {  // colsum_partials_kernel
      const float* partial = reinterpret_cast<const float*>(sg.src);
      const size_t tiles = (size_t)sg.count;
      const int n = (int)sg.n;
      const int c4 = blk * 8 + (threadIdx.x & 7), tg = threadIdx.x >> 3;
      const bool live = c4 * 4 < n;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      if (live) {
#pragma unroll 8
        for (size_t t = tg; t < tiles; t += 32)
          s += *reinterpret_cast<const f32x4*>(partial + t * n + c4 * 4);
      }
      red[threadIdx.x] = s;
      __syncthreads();
      if (tg == 0 && live) {
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 32; k++) sum += red[k * 8 + threadIdx.x];
        finish_store4<SGD>(sg, dst + (size_t)c4 * 4, sum, lr, grad_scale);
      }
      return;
    }
    case HCTR_DENSE_SEG_LOGIT_HEAD: {  // logit_head_finish_kernel; partial [blocks][K + 2]
      const int K = (int)sg.n;
      const int k = blk * 64 + (int)(threadIdx.x & 63);
      const bool live = k < K + 2;
      const float tot = finish_block_chunks(reinterpret_cast<float(*)[64]>(red), (int)sg.count,
                                            (size_t)(K + 2), (size_t)k, live,
                                            reinterpret_cast<const float*>(sg.src));
      if (threadIdx.x < 64 && live) {
        if (k < K) finish_store1<SGD>(sg, dst + k, tot, lr, grad_scale);
        else if (k == K) finish_store1<SGD>(sg, dst2, tot, lr, grad_scale);
        else if (loss) *loss = tot / (float)(size_t)sg.k;
      }
      return;
    }
    case HCTR_DENSE_SEG_SKINNY: {  // skinny_fc_finish_kernel; partial [blocks][N][kSkinnyK + 1]
      const int stride = kSkinnyK + 1;
      const int K = (int)sg.k, total = (int)sg.n * stride;
      const int i = blk * 64 + (int)(threadIdx.x & 63);
      const bool live = i < total;
      const float tot = finish_block_chunks(reinterpret_cast<float(*)[64]>(red), (int)sg.count,
                                            (size_t)total, (size_t)i, live,
                                            reinterpret_cast<const float*>(sg.src));
      if (threadIdx.x < 64 && live) {
        const int n = i / stride, kk = i % stride;
        if (kk == kSkinnyK) finish_store1<SGD>(sg, dst2 + n, tot, lr, grad_scale);
        else if (kk < K) finish_store1<SGD>(sg, dst + (size_t)n * K + kk, tot, lr, grad_scale);
      }
      return;
    }
    default: {  // HCTR_DENSE_SEG_DIRECT: the gradient is in g already; only the step is left
      if (!SGD) return;
      const size_t i = (size_t)blk * kBlock + threadIdx.x;
      if (i >= (size_t)sg.n / 4) return;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(sg.g) + dst + i * 4);
      finish_store4<SGD>(sg, dst + i * 4, gv, lr, grad_scale);
      return;
    }
  }
}

constexpr int kCrossBwdWaves = 256 * 4;  // waves used by the cross backward (deterministic reduce)

}  // namespace
}  // namespace hctr

using namespace hctr;

extern "C" {

#define HCTR_CROSS_DISPATCH(MACRO)       \
  if (npl <= 1) MACRO(1)                 \
  else if (npl <= 2) MACRO(2)            \
  else if (npl <= 4) MACRO(4)            \
  else if (npl <= 8) MACRO(8)            \
  else if (npl <= 16) MACRO(16)          \
  else if (npl <= 32) MACRO(32)          \
  else MACRO(64)

int hctr_cross_v1_fwd(size_t batch, int width, int layers, const float* x0, const float* kernels,
                      const float* biases, float* outputs, float* hiddens, hctr_stream_t stream) {
  HCTR_REQUIRE(width >= 1 && layers >= 1, "shape");
  HCTR_REQUIRE(width <= 64 * 64, "cross v1: width > 4096 not supported");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(x0 && kernels && biases && outputs && hiddens, "null pointer");
  hipStream_t s = as_stream(stream);
  const int npl = (width + 63) / 64;
  const int grid = grid_for(batch * 64, kBlock);
#define HCTR_CF(N_)                                                                            \
  hipLaunchKernelGGL(cross_v1_fwd_kernel<N_>, dim3(grid), dim3(kBlock), 0, s, batch, width,    \
                     layers, x0, kernels, biases, outputs, hiddens);
  HCTR_CROSS_DISPATCH(HCTR_CF)
#undef HCTR_CF
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_cross_v1_bwd_workspace_bytes(size_t batch, int width, int layers) {
  (void)batch;
  return (size_t)kCrossBwdWaves * layers * 2 * width * sizeof(float);
}

int hctr_cross_v1_bwd(size_t batch, int width, int layers, const float* x0, const float* kernels,
                      const float* outputs, const float* hiddens, const float* out_grad,
                      float* in_grad, float* kernel_grads, float* bias_grads, float* workspace,
                      hctr_stream_t stream) {
  HCTR_REQUIRE(width >= 1 && layers >= 1, "shape");
  HCTR_REQUIRE(width <= 64 * 64, "cross v1: width > 4096 not supported");
  HCTR_REQUIRE(x0 && kernels && outputs && hiddens && out_grad && in_grad && kernel_grads &&
                   bias_grads && workspace,
               "null pointer");
  hipStream_t s = as_stream(stream);
  const int npl = (width + 63) / 64;
  const int grid = kCrossBwdWaves / kWavesPerBlock;
  const size_t lds_bytes = (size_t)layers * 2 * width * sizeof(float);
  if (lds_bytes <= 60 * 1024) {
#define HCTR_CB(N_)                                                                           \
  hipLaunchKernelGGL((cross_v1_bwd_kernel<N_, true>), dim3(kCrossBwdWaves), dim3(64), lds_bytes, \
                     s, batch, width, layers, x0, kernels, outputs, hiddens, out_grad, in_grad,  \
                     workspace);
    HCTR_CROSS_DISPATCH(HCTR_CB)
#undef HCTR_CB
  } else {
#define HCTR_CB(N_)                                                                           \
  hipLaunchKernelGGL((cross_v1_bwd_kernel<N_, false>), dim3(grid), dim3(kBlock), 0, s, batch, \
                     width, layers, x0, kernels, outputs, hiddens, out_grad, in_grad, workspace);
    HCTR_CROSS_DISPATCH(HCTR_CB)
#undef HCTR_CB
  }
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cross_v1_reduce_kernel,
                     dim3((unsigned)ceil_div<size_t>((size_t)layers * 2 * width, 32)),
                     dim3(kBlock), 0, s, (size_t)kCrossBwdWaves, width, layers, workspace,
                     kernel_grads, bias_grads);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_relu_bwd_bias_workspace_bytes(size_t rows, int n) {
  return ceil_div<size_t>(rows, (size_t)kRbRows) * (size_t)n * sizeof(float);
}

// finish = false: the tile partials stay in the workspace (hctr_dense_grad_finish adds them)
static int relu_bwd_bias_impl(size_t rows, int n, const void* dy, const void* y, void* dz, float* db,
                              float* workspace, int dtype, bool finish, hctr_stream_t stream) {
  HCTR_REQUIRE(n > 0 && n % 8 == 0, "n must be a multiple of 8");
  HCTR_REQUIRE(dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16, "16-bit dtypes only");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(dy && y && dz && (db || !finish) && workspace, "null pointer");
  hipStream_t s = as_stream(stream);
  const size_t tiles = ceil_div<size_t>(rows, (size_t)kRbRows);
  const int cw = n / 8 < kBlock ? n / 8 : kBlock;
  const int rg = kBlock / cw;
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(relu_bwd_bias_kernel<true>, dim3((unsigned)tiles), dim3(kBlock), 0, s, rows,
                       n, cw, rg, (const unsigned short*)dy, (const unsigned short*)y,
                       (unsigned short*)dz, workspace);
  else
    hipLaunchKernelGGL(relu_bwd_bias_kernel<false>, dim3((unsigned)tiles), dim3(kBlock), 0, s,
                       rows, n, cw, rg, (const unsigned short*)dy, (const unsigned short*)y,
                       (unsigned short*)dz, workspace);
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div<int>(n, 32)), dim3(kBlock), 0, s,
                     tiles, n, workspace, db);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_relu_bwd_bias(size_t rows, int n, const void* dy, const void* y, void* dz, float* db,
                       float* workspace, int dtype, hctr_stream_t stream) {
  return relu_bwd_bias_impl(rows, n, dy, y, dz, db, workspace, dtype, true, stream);
}

int hctr_relu_bwd_bias_partials(size_t rows, int n, const void* dy, const void* y, void* dz,
                                float* workspace, int dtype, hctr_stream_t stream) {
  return relu_bwd_bias_impl(rows, n, dy, y, dz, nullptr, workspace, dtype, false, stream);
}

size_t hctr_cross_v2_bwd_step_workspace_bytes(size_t batch, int width) {
  if (batch == 0 || width <= 0) return 0;
  return ceil_div<size_t>(batch, (size_t)cross_step_rows_per_tile(batch, width)) * (size_t)width *
         sizeof(float);
}

int hctr_cross_v2_bwd_step(size_t batch, int width, const void* dy, const void* x0, const void* h,
                           void* acc, void* s0, float* db, float* workspace, int first, int dtype,
                           hctr_stream_t stream) {
  HCTR_REQUIRE(width > 0 && width % 8 == 0, "width must be a multiple of 8");
  HCTR_REQUIRE(dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16, "16-bit dtypes only");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(dy && x0 && h && acc && s0 && db && workspace, "null pointer");
  hipStream_t s = as_stream(stream);
  const int cw = width / 8 < kBlock ? width / 8 : kBlock;
  const int rg = kBlock / cw;
  const int rpt = cross_step_rows_per_tile(batch, width);
  const size_t tiles = ceil_div<size_t>(batch, (size_t)rpt);
  const unsigned col_blocks = (unsigned)ceil_div<int>(width / 8, cw);
#define HCTR_CROSS_STEP(BF_, FIRST_)                                                              \
  hipLaunchKernelGGL((cross_v2_bwd_step_kernel<BF_, FIRST_>), dim3((unsigned)tiles, col_blocks),   \
                     dim3(kBlock), 0, s, batch, width, cw, rg, rpt, (const unsigned short*)dy,     \
                     (const unsigned short*)x0, (const unsigned short*)h, (unsigned short*)acc,    \
                     (unsigned short*)s0, workspace)
  if (dtype == HCTR_EMB_BF16) {
    if (first) HCTR_CROSS_STEP(true, true);
    else HCTR_CROSS_STEP(true, false);
  } else {
    if (first) HCTR_CROSS_STEP(false, true);
    else HCTR_CROSS_STEP(false, false);
  }
#undef HCTR_CROSS_STEP
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div<int>(width, 32)), dim3(kBlock), 0, s,
                     tiles, width, workspace, db);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_sum_groups(int groups, size_t n, const void* in, int dtype, float* out,
                    hctr_stream_t stream) {
  HCTR_REQUIRE(groups > 0 && n % 8 == 0, "n must be a multiple of 8");
  HCTR_REQUIRE(dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16, "16-bit dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(in && out, "null pointer");
  hipStream_t s = as_stream(stream);
  const size_t n8 = n / 8;
  const dim3 grid((unsigned)ceil_div<size_t>(n8, (size_t)kBlock));
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(sum_groups_kernel<true>, grid, dim3(kBlock), 0, s, groups, n8,
                       (const unsigned short*)in, out);
  else
    hipLaunchKernelGGL(sum_groups_kernel<false>, grid, dim3(kBlock), 0, s, groups, n8,
                       (const unsigned short*)in, out);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_sgd_shadow(size_t n, float lr, float grad_scale, float* w, const float* g, void* w16,
                    int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(n % 4 == 0, "n must be a multiple of 4");
  HCTR_REQUIRE(dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16, "16-bit shadow dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(w && g && w16, "null pointer");
  hipStream_t s = as_stream(stream);
  const dim3 grid(grid_for(n / 4, kBlock, 4096));
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(sgd_shadow_kernel<true>, grid, dim3(kBlock), 0, s, n / 4, lr, grad_scale, w,
                       g, (unsigned short*)w16);
  else
    hipLaunchKernelGGL(sgd_shadow_kernel<false>, grid, dim3(kBlock), 0, s, n / 4, lr, grad_scale,
                       w, g, (unsigned short*)w16);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

static int ftrl_check(float lr, float beta, float lambda1, float lambda2, float grad_scale) {
  HCTR_REQUIRE(lr > 0.f && lr < INFINITY, "ftrl: lr must be positive and finite");
  HCTR_REQUIRE(beta >= 0.f && lambda1 >= 0.f && lambda2 >= 0.f,
               "ftrl: beta, lambda1 and lambda2 must not be negative");
  HCTR_REQUIRE(grad_scale == grad_scale && fabsf(grad_scale) < INFINITY, "ftrl: grad_scale");
  return HCTR_OK;
}

static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int hctr_ftrl_shadow(size_t n, float lr, float beta, float lambda1, float lambda2, float grad_scale,
                     float* w, float* z, float* nacc, const float* g, void* w16, int dtype,
                     hctr_stream_t stream) {
  HCTR_REQUIRE(n % 4 == 0, "n must be a multiple of 4");
  HCTR_TRY(ftrl_check(lr, beta, lambda1, lambda2, grad_scale));
  HCTR_REQUIRE(!w16 || dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16,
               "16-bit shadow dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(w && z && nacc && g, "null pointer");
  HCTR_REQUIRE(aligned16(w) && aligned16(z) && aligned16(nacc) && aligned16(g) && aligned16(w16),
               "16-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const FtrlHp h = {lr, lambda1, lambda2 + beta / lr, grad_scale};
  const dim3 grid(grid_for(n / 4, kBlock, 4096));
  if (!w16)
    hipLaunchKernelGGL(ftrl_shadow_kernel<0>, grid, dim3(kBlock), 0, s, n / 4, h, w, z, nacc, g,
                       (unsigned short*)nullptr);
  else if (dtype == HCTR_EMB_F16)
    hipLaunchKernelGGL(ftrl_shadow_kernel<1>, grid, dim3(kBlock), 0, s, n / 4, h, w, z, nacc, g,
                       (unsigned short*)w16);
  else
    hipLaunchKernelGGL(ftrl_shadow_kernel<2>, grid, dim3(kBlock), 0, s, n / 4, h, w, z, nacc, g,
                       (unsigned short*)w16);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_ftrl_segments(const hctr_ftrl_seg* segs, int nseg, size_t nblocks, float lr, float beta,
                       float lambda1, float lambda2, float grad_scale, float* z, float* nacc,
                       const float* g, hctr_stream_t stream) {
  HCTR_REQUIRE(nseg >= 0 && nblocks <= 0x7FFFFFFFu, "ftrl segments: segment / block count");
  HCTR_TRY(ftrl_check(lr, beta, lambda1, lambda2, grad_scale));
  if (nseg == 0 || nblocks == 0) return HCTR_OK;
  HCTR_REQUIRE(segs && z && nacc && g, "null pointer");
  HCTR_REQUIRE(aligned16(z) && aligned16(nacc) && aligned16(g), "16-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const FtrlHp h = {lr, lambda1, lambda2 + beta / lr, grad_scale};
  hipLaunchKernelGGL(ftrl_segments_kernel, dim3((unsigned)nblocks), dim3(kBlock), 0, s, segs, nseg,
                     h, z, nacc, g);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_bce_loss_workspace_bytes(void) { return kBceBlocks * sizeof(float); }

int hctr_bce_loss(size_t batch, const void* logit, const float* label, float grad_scale,
                  void* dlogit, float* loss, float* workspace, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(batch > 0, "empty batch");
  HCTR_REQUIRE(logit && label && loss && workspace, "null pointer");
  hipStream_t s = as_stream(stream);
  const int blocks = (int)(ceil_div<size_t>(batch, (size_t)kBlock) < (size_t)kBceBlocks
                               ? ceil_div<size_t>(batch, (size_t)kBlock)
                               : (size_t)kBceBlocks);
  switch (dtype) {
    case HCTR_EMB_F32:
      hipLaunchKernelGGL(bce_kernel<float>, dim3(blocks), dim3(kBlock), 0, s, batch,
                         (const float*)logit, label, grad_scale, (float*)dlogit, workspace);
      break;
    case HCTR_EMB_F16:
      hipLaunchKernelGGL(bce_kernel<__half>, dim3(blocks), dim3(kBlock), 0, s, batch,
                         (const __half*)logit, label, grad_scale, (__half*)dlogit, workspace);
      break;
    case HCTR_EMB_BF16:
      hipLaunchKernelGGL(bce_kernel<__hip_bfloat16>, dim3(blocks), dim3(kBlock), 0, s, batch,
                         (const __hip_bfloat16*)logit, label, grad_scale, (__hip_bfloat16*)dlogit,
                         workspace);
      break;
    default:
      HCTR_REQUIRE(false, "bad dtype");
  }
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(kBlock), 0, s, blocks, batch, workspace, loss);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_logit_head_workspace_bytes(int k) { return (size_t)kHeadBlocks * (k + 2) * sizeof(float); }

static int logit_head_rows(int k) {
  const int nseg = (k + 255) / 256;
  return nseg <= 1 ? 8 : (nseg <= 2 ? 4 : (nseg <= 4 ? 2 : 1));
}

int hctr_logit_head_blocks(size_t batch, int k) {
  HCTR_REQUIRE(batch > 0 && k >= 4 && k % 4 == 0 && k <= 256 * kHeadMaxSeg,
               "logit head: K must be a multiple of 4 and <= 2048");
  return (int)std::min<size_t>((size_t)kHeadBlocks,
                               ceil_div<size_t>(batch, (size_t)(kBlock / 64) * logit_head_rows(k)));
}

// finish = false: the block partials stay in the workspace (hctr_dense_grad_finish adds them)
static int logit_head_impl(size_t batch, int k, const void* x, const void* w, const void* bias,
                           const float* label, float grad_scale, void* dx, float* dw, float* db,
                           float* loss, float* workspace, int dtype, bool finish,
                           hctr_stream_t stream) {
  HCTR_REQUIRE(batch > 0 && k >= 4 && k % 4 == 0 && k <= 256 * kHeadMaxSeg,
               "logit head: K must be a multiple of 4 and <= 2048");
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "16-bit activations");
  HCTR_REQUIRE(x && w && bias && label && ((dw && db && loss) || !finish) && workspace,
               "null pointer");
  HCTR_REQUIRE(reinterpret_cast<uintptr_t>(x) % 8 == 0 && reinterpret_cast<uintptr_t>(w) % 8 == 0 &&
                   (dx == nullptr || reinterpret_cast<uintptr_t>(dx) % 8 == 0),
               "8-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const int nseg = (k + 255) / 256;
  const int blocks = hctr_logit_head_blocks(batch, k);
  const size_t lds = (size_t)(kBlock / 64) * (k + 2) * sizeof(float);
#define HCTR_HEAD(T_, NSEG_, ROWS_)                                                               \
  hipLaunchKernelGGL((logit_head_kernel<T_, NSEG_, ROWS_>), dim3(blocks), dim3(kBlock), lds, s,   \
                     batch, k, (const T_*)x, (const T_*)w, (const T_*)bias, label, grad_scale,    \
                     (T_*)dx, workspace)
#define HCTR_HEAD_T(T_)                       \
  if (nseg <= 1) HCTR_HEAD(T_, 1, 8);         \
  else if (nseg <= 2) HCTR_HEAD(T_, 2, 4);    \
  else if (nseg <= 4) HCTR_HEAD(T_, 4, 2);    \
  else HCTR_HEAD(T_, 8, 1);
  if (dtype == HCTR_EMB_BF16) {
    HCTR_HEAD_T(__hip_bfloat16)
  } else {
    HCTR_HEAD_T(__half)
  }
#undef HCTR_HEAD_T
#undef HCTR_HEAD
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  hipLaunchKernelGGL(logit_head_finish_kernel, dim3(ceil_div<int>(k + 2, 64)), dim3(1024), 0, s,
                     blocks, k, batch, workspace, dw, db, loss);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_logit_head(size_t batch, int k, const void* x, const void* w, const void* bias,
                    const float* label, float grad_scale, void* dx, float* dw, float* db,
                    float* loss, float* workspace, int dtype, hctr_stream_t stream) {
  return logit_head_impl(batch, k, x, w, bias, label, grad_scale, dx, dw, db, loss, workspace,
                         dtype, true, stream);
}

int hctr_logit_head_partials(size_t batch, int k, const void* x, const void* w, const void* bias,
                             const float* label, float grad_scale, void* dx, float* workspace,
                             int dtype, hctr_stream_t stream) {
  return logit_head_impl(batch, k, x, w, bias, label, grad_scale, dx, nullptr, nullptr, nullptr,
                         workspace, dtype, false, stream);
}

static int skinny_check(size_t batch, int k, int n, int dtype) {
  HCTR_REQUIRE(batch > 0 && k >= 1 && k <= kSkinnyK, "skinny fc: 1 <= K <= 16");
  HCTR_REQUIRE(n >= 4 && n % 4 == 0 && n <= 512, "skinny fc: N a multiple of 4, <= 512");
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "16-bit weights / activations");
  return HCTR_OK;
}

int hctr_skinny_fc_fwd(size_t batch, int k, int n, const float* x, const void* w, const void* bias,
                       void* y, int dtype, hctr_stream_t stream) {
  HCTR_TRY(skinny_check(batch, k, n, dtype));
  HCTR_REQUIRE(x && w && bias && y, "null pointer");
  HCTR_REQUIRE(reinterpret_cast<uintptr_t>(y) % 8 == 0, "8-byte aligned output");
  hipStream_t s = as_stream(stream);
  // R consecutive rows per block (even, <= 256: 16 KB of LDS), about 4 blocks per CU
  size_t rows = ceil_div<size_t>(batch, 1024);
  rows = std::min<size_t>(256, (rows + 1) / 2 * 2);
  const int blocks = (int)ceil_div<size_t>(batch, rows);
  const size_t lds = rows * kSkinnyK * sizeof(float);
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(skinny_fc_fwd_kernel<__hip_bfloat16>, dim3(blocks), dim3(kBlock), lds, s,
                       batch, k, n, (int)rows, x, (const __hip_bfloat16*)w,
                       (const __hip_bfloat16*)bias, (__hip_bfloat16*)y);
  else
    hipLaunchKernelGGL(skinny_fc_fwd_kernel<__half>, dim3(blocks), dim3(kBlock), lds, s, batch, k, n,
                       (int)rows, x, (const __half*)w, (const __half*)bias, (__half*)y);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_skinny_fc_bwd_workspace_bytes(int n) {
  return (size_t)kSkinnyBlocks * n * (kSkinnyK + 1) * sizeof(float);
}

// which form of the backward runs and how many block partials it leaves
static int skinny_bwd_blocks(size_t batch, int k, int n, const void* dy, const void* y, bool* mfma) {
  // matrix-core form: needs a spare input column for db and 16-byte rows (HCTR_SKINNY_BWD=valu|mfma)
  const char* mode = getenv("HCTR_SKINNY_BWD");
  const bool want_mfma = mode ? strcmp(mode, "valu") != 0 : kSkinnyBwdMfmaDefault;
  *mfma = want_mfma && k < kSkinnyK && n % 8 == 0 && reinterpret_cast<uintptr_t>(dy) % 16 == 0 &&
          reinterpret_cast<uintptr_t>(y) % 16 == 0;
  if (*mfma) {
    const int rsets = (kSkinnyBwdBlock / 64) / ceil_div<int>(n, 128);
    return (int)std::min<size_t>((size_t)kSkinnyBlocks, ceil_div<size_t>(batch, (size_t)rsets * 16));
  }
  return (int)std::min<size_t>((size_t)kSkinnyBlocks,
                               ceil_div<size_t>(batch, kSkinnyBwdBlock / kSkinnyLanes));
}

int hctr_skinny_fc_bwd_blocks(size_t batch, int k, int n, const void* dy, const void* y) {
  HCTR_REQUIRE(batch > 0 && k >= 1 && k <= kSkinnyK, "skinny fc: 1 <= K <= 16");
  HCTR_REQUIRE(n >= 4 && n % 4 == 0 && n <= 512, "skinny fc: N a multiple of 4, <= 512");
  bool mfma;
  return skinny_bwd_blocks(batch, k, n, dy, y, &mfma);
}

// finish = false: the block partials stay in the workspace (hctr_dense_grad_finish adds them)
static int skinny_fc_bwd_impl(size_t batch, int k, int n, const float* x, const void* dy,
                              const void* y, float* dw, float* db, float* workspace, int dtype,
                              bool finish, hctr_stream_t stream) {
  HCTR_TRY(skinny_check(batch, k, n, dtype));
  HCTR_REQUIRE(x && dy && y && ((dw && db) || !finish) && workspace, "null pointer");
  HCTR_REQUIRE(reinterpret_cast<uintptr_t>(dy) % 8 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0,
               "8-byte aligned activations");
  hipStream_t s = as_stream(stream);
  const size_t lds = (size_t)n * (kSkinnyK + 1) * sizeof(float);
  bool mfma;
  const int blocks = skinny_bwd_blocks(batch, k, n, dy, y, &mfma);
  if (mfma) {
    if (dtype == HCTR_EMB_BF16)
      hipLaunchKernelGGL(skinny_fc_bwd_mfma_kernel<__hip_bfloat16>, dim3(blocks),
                         dim3(kSkinnyBwdBlock), lds, s, batch, k, n, x, (const __hip_bfloat16*)dy,
                         (const __hip_bfloat16*)y, workspace);
    else
      hipLaunchKernelGGL(skinny_fc_bwd_mfma_kernel<__half>, dim3(blocks), dim3(kSkinnyBwdBlock), lds,
                         s, batch, k, n, x, (const __half*)dy, (const __half*)y, workspace);
    HCTR_LAUNCH_CHECK();
    if (!finish) return HCTR_OK;
    hipLaunchKernelGGL(skinny_fc_finish_kernel, dim3(ceil_div<int>(n * (kSkinnyK + 1), 64)),
                       dim3(1024), 0, s, blocks, k, n, workspace, dw, db);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(skinny_fc_bwd_kernel<__hip_bfloat16>, dim3(blocks), dim3(kSkinnyBwdBlock), lds, s,
                       batch, k, n, x, (const __hip_bfloat16*)dy, (const __hip_bfloat16*)y,
                       workspace);
  else
    hipLaunchKernelGGL(skinny_fc_bwd_kernel<__half>, dim3(blocks), dim3(kSkinnyBwdBlock), lds, s, batch, k, n,
                       x, (const __half*)dy, (const __half*)y, workspace);
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  hipLaunchKernelGGL(skinny_fc_finish_kernel, dim3(ceil_div<int>(n * (kSkinnyK + 1), 64)),
                     dim3(1024), 0, s, blocks, k, n, workspace, dw, db);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_skinny_fc_bwd(size_t batch, int k, int n, const float* x, const void* dy, const void* y,
                       float* dw, float* db, float* workspace, int dtype, hctr_stream_t stream) {
  return skinny_fc_bwd_impl(batch, k, n, x, dy, y, dw, db, workspace, dtype, true, stream);
}

int hctr_skinny_fc_bwd_partials(size_t batch, int k, int n, const float* x, const void* dy,
                                const void* y, float* workspace, int dtype, hctr_stream_t stream) {
  return skinny_fc_bwd_impl(batch, k, n, x, dy, y, nullptr, nullptr, workspace, dtype, false,
                            stream);
}

int hctr_dense_seg_blocks(int kind, size_t n) {
  switch (kind) {
    case HCTR_DENSE_SEG_SUM_GROUPS: return (int)ceil_div<size_t>(n / 8, (size_t)kBlock);
    case HCTR_DENSE_SEG_COLSUM: return (int)ceil_div<size_t>(n, 32);
    case HCTR_DENSE_SEG_LOGIT_HEAD: return (int)ceil_div<size_t>(n + 2, 64);
    case HCTR_DENSE_SEG_SKINNY: return (int)ceil_div<size_t>(n * (kSkinnyK + 1), 64);
    case HCTR_DENSE_SEG_DIRECT: return (int)ceil_div<size_t>(n / 4, (size_t)kBlock);
    default: HCTR_REQUIRE(false, "dense finish: unknown segment kind");
  }
}

int hctr_dense_grad_finish(const hctr_dense_seg* segs, int nseg, size_t nblocks, int sgd, float lr,
                           float grad_scale, float* loss, hctr_stream_t stream) {
  HCTR_REQUIRE(nseg >= 0 && nblocks <= 0x7FFFFFFFu, "dense finish: segment / block count");
  if (nseg == 0 || nblocks == 0) return HCTR_OK;
  HCTR_REQUIRE(segs, "null pointer");
  hipStream_t s = as_stream(stream);
  if (sgd)
    hipLaunchKernelGGL(dense_grad_finish_kernel<true>, dim3((unsigned)nblocks), dim3(kBlock), 0, s,
                       segs, nseg, lr, grad_scale, loss);
  else
    hipLaunchKernelGGL(dense_grad_finish_kernel<false>, dim3((unsigned)nblocks), dim3(kBlock), 0, s,
                       segs, nseg, lr, grad_scale, loss);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
