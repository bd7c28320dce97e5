// dense_ops.hip -- the dense ops next to the GEMMs: the DCN cross layers' element-wise kernels and
// the MLP edge kernels (ReLU backward + bias gradient, split-K group sums, SGD / Ftrl with the 16-bit
// shadow copy, BCE loss, the logit head, the skinny first layer).  The dot interaction is interaction.hip,
// the cross layers' GEMMs are cross_gemm.hip.  By family: cross v1, column-tile producers, loss and
// logit head, skinny first layer, optimizers, fixed-order sums and the finish launch; then the
// host entries in the same order.
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
constexpr int kCrossBwdWaves = 256 * 4;  // waves used by the cross backward (deterministic reduce)

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
// Column-tile producers: an elementwise pass over 16-bit rows that also leaves the column sums of
// what it wrote, as one fp32 partial row per row tile (the tiles are added in fixed order by the
// COLSUM finish below: deterministic).  A workgroup owns a tile of rows x cw 16-byte column
// vectors: thread t owns column vector c8 = t % cw and walks the rows g = t / cw, + rg, ...;
// cw = min(n / 8, 256), rg = 256 / cw row groups, whose sums meet in LDS in group order.
// ================================================================================================
struct Terms8 {
  float v[8];
};

// one column block of one tile: term(at) handles the vector at element offset `at` of row r and
// returns its eight fp32 terms; their sums over the tile's rows go to partial[blockIdx.x][...].
// Every thread of the workgroup calls this (two barriers), whether it owns a vector or not.
template <typename F>
__device__ __forceinline__ void col_tile_sum(float* red, size_t rows, int n, int cw, int rg, int rpt,
                                             int col0, float* __restrict__ partial, F&& term) {
  const int c8 = threadIdx.x % cw, g = threadIdx.x / cw;
  const int cc = col0 + c8;
  const bool live = g < rg && cc < n / 8;
  const size_t r0 = (size_t)blockIdx.x * (size_t)rpt;
  const size_t r1 = r0 + (size_t)rpt < rows ? r0 + (size_t)rpt : rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll 4
    for (size_t r = r0 + g; r < r1; r += rg) {
      const Terms8 t = term(r * n + cc * 8);
#pragma unroll
      for (int e = 0; e < 8; e++) acc[e] += t.v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; e++) red[e * kBlock + threadIdx.x] = acc[e];
  __syncthreads();
  if (g == 0 && cc < n / 8) {
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

// Fused ReLU backward + bias gradient for the MLP layers around the path:
//   dz[b][n] = dy[b][n] * (y[b][n] > 0),   db[n] = sum_b dz[b][n]
// PyTorch issues threshold_backward (read dy,y / write dz) and a column-sum reduction (read dz)
// as two launches; fused, dz is consumed from registers.
constexpr int kRbRows = 128;  // rows per workgroup

template <bool BF>
__global__ void __launch_bounds__(kBlock)
    relu_bwd_bias_kernel(size_t rows, int n, int cw, int rg, const unsigned short* __restrict__ dy,
                         const unsigned short* __restrict__ y, unsigned short* __restrict__ dz,
                         float* __restrict__ partial) {
  using H = H16<BF>;
  __shared__ float red[kBlock * 8];
  // a workgroup takes the column blocks one after the other: uniform trip count
  for (int col0 = 0; col0 < n / 8; col0 += cw)
    col_tile_sum(red, rows, n, cw, rg, kRbRows, col0, partial, [&](size_t at) {
      const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + at);
      const u32x4 av = *reinterpret_cast<const u32x4*>(y + at);
      u32x4 o;
      Terms8 t;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const unsigned short z0 = H::lo(av[e]) > 0.f ? lo16(gv[e]) : (unsigned short)0;
        const unsigned short z1 = H::hi(av[e]) > 0.f ? hi16(gv[e]) : (unsigned short)0;
        t.v[2 * e] = H::to_f32(z0);
        t.v[2 * e + 1] = H::to_f32(z1);
        o[e] = pack16(z0, z1);
      }
      *reinterpret_cast<u32x4*>(dz + at) = o;
      return t;
    });
}

// DCN-v2 cross layer, the elementwise step of one layer's backward in the activations' 16-bit type
// (MultiCrossBackwardFunctorv2: fused_mul_fma3, R/HugeCTR/src/layers/multi_cross_layer.cu:391-424,
// 127-165 -- S0 = dY .* X0, dX += dY .* H, one rounding per element as its paired-half kernel
// rounds -- and the bias gradient db = column sums of S0, which the reference takes in the
// epilogue of the dV GEMM, :770-776): dY is read once for both products, S0 is summed from
// registers.  FIRST (the last layer, visited first): dX = dY .* H, the accumulator is not read (nor
// cleared beforehand).

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

// the grid is (row tiles of rpt rows, column blocks): blockIdx.y picks the column block
template <bool BF, bool FIRST>
__global__ void __launch_bounds__(kBlock)
    cross_v2_bwd_step_kernel(size_t rows, int n, int cw, int rg, int rpt,
                             const unsigned short* __restrict__ dy,
                             const unsigned short* __restrict__ x0,
                             const unsigned short* __restrict__ hm, unsigned short* __restrict__ acc_io,
                             unsigned short* __restrict__ s0, float* __restrict__ partial) {
  using H = H16<BF>;
  __shared__ float red[kBlock * 8];
  col_tile_sum(red, rows, n, cw, rg, rpt, (int)blockIdx.y * cw, partial, [&](size_t at) {
    const u32x4 gv = *reinterpret_cast<const u32x4*>(dy + at);
    const u32x4 xv = *reinterpret_cast<const u32x4*>(x0 + at);
    const u32x4 hv = *reinterpret_cast<const u32x4*>(hm + at);
    u32x4 av = {0u, 0u, 0u, 0u};
    if (!FIRST) av = *reinterpret_cast<const u32x4*>(acc_io + at);
    u32x4 so, ao;
    Terms8 t;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float g0 = H::lo(gv[e]), g1 = H::hi(gv[e]);
      // (the product of two 16-bit values is exact in fp32: one rounding, to the 16-bit type)
      const unsigned short p0 = H::from_f32(g0 * H::lo(xv[e]));
      const unsigned short p1 = H::from_f32(g1 * H::hi(xv[e]));
      t.v[2 * e] = H::to_f32(p0);
      t.v[2 * e + 1] = H::to_f32(p1);
      so[e] = pack16(p0, p1);
      float a0 = g0 * H::lo(hv[e]);
      float a1 = g1 * H::hi(hv[e]);
      if (!FIRST) {
        a0 += H::lo(av[e]);
        a1 += H::hi(av[e]);
      }
      ao[e] = H::pack2(a0, a1);
    }
    *reinterpret_cast<u32x4*>(s0 + at) = so;
    *reinterpret_cast<u32x4*>(acc_io + at) = ao;
    return t;
  });
}

// ================================================================================================
// BinaryCrossEntropyLoss (R/HugeCTR/src/loss.cu:231-262): per-sample stable BCE-with-logits,
// the logit gradient scaled by grad_scale (= scaler / batch / total_gpu_count in the reference),
// and the mean loss.  The reference accumulates the block sums with atomicAdd; here the block
// partials are added in fixed order by the last launch (deterministic).
// ================================================================================================
constexpr int kBceBlocks = 256;

// one sample: *loss = bce(z, y), *grad = sigmoid(z) - y, both through exp(-|z|)
__device__ __forceinline__ void bce_term(float z, float y, float* grad, float* loss) {
  if (z >= 0.f) {
    const float e = expf(-z);
    *grad = (1.f - y) - e / (1.f + e);
    *loss = z * (1.f - y) + logf(1.f + e);
  } else {
    const float e = expf(z);
    *grad = -y + e / (1.f + e);
    *loss = -z * y + logf(1.f + e);
  }
}

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
    float g, l;
    bce_term(x, y, &g, &l);
    val += l;
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
      // bce_term written out: through the function this kernel's <T, 1, 8> form schedules 24
      // instructions differently and measured 1 - 3 % slower (profiles/dense_refactor_ab.txt)
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


// ================================================================================================
// Skinny first layer of the bottom MLP: y = relu(x W^T + b) with a handful of input features
// (K <= 16, DLRM: 13 dense features -> 512).  As a GEMM it is all output traffic and no arithmetic
// (library kernel: 30 us forward; ReLU backward + bias + a K = batch weight-gradient GEMM with
// 13 columns: 72 us).  Here 128 lanes own one row at a time, a lane 4 consecutive outputs
// with their K weights in registers; the backward folds dz = dy * (y > 0) into the
// weight-gradient sum, so dz is never written (the layer has no data gradient).
// ================================================================================================
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

// ================================================================================================
// Optimizers of the dense layers: SGD and Ftrl on the fp32 masters, with the refresh of the 16-bit
// compute copy.  The dense SGD step is ONE expression for every kernel that takes it (f32x4 or
// float): a parameter rounds the same (contraction included) whichever kernel updates it.
// ================================================================================================
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
    reinterpret_cast<uint2*>(w16)[i] = H::pack4(wv[0], wv[1], wv[2], wv[3]);
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
      reinterpret_cast<uint2*>(w16)[i] = H::pack4(wv[0], wv[1], wv[2], wv[3]);
    }
  }
}

// a workgroup's entry in a table of segments (hctr_ftrl_seg, hctr_dense_seg): the last one whose
// first block is not past it, -1 if there is none.  Every wavefront looks at 64 table entries per
// step (one load latency, not one per segment).
template <typename Seg>
__device__ __forceinline__ int find_segment(const Seg* __restrict__ segs, int nseg) {
  int si = -1;
  for (int base = 0; base < nseg; base += 64) {
    const int t = base + (int)(threadIdx.x & 63);
    const bool in = t < nseg && segs[t].block0 <= (long long)blockIdx.x;
    si += (int)__popcll(__ballot(in));
  }
  return si;
}

// the segmented form: parameter tensors that do not live in one buffer; their gradients and the
// state do (flat g / z / n, a segment's elements at `off`).  A block takes kFtrlSegElems elements
// of one segment.  Groups of 4 go through the vector form when the segment allows it (w 16-byte
// aligned, off % 4 == 0), the tail and everything else through the scalar form of the same
// expression.
constexpr int kFtrlSegElems = HCTR_FTRL_SEG_BLOCK_ELEMS;
static_assert(kFtrlSegElems == kBlock * 4, "a thread takes 4 elements");

__global__ void __launch_bounds__(kBlock)
    ftrl_segments_kernel(const hctr_ftrl_seg* __restrict__ segs, int nseg, FtrlHp h,
                         float* __restrict__ z, float* __restrict__ nacc,
                         const float* __restrict__ g) {
  const int si = find_segment(segs, nseg);
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
// Fixed-order sums and the gradient finish.  Every partial sum the backward's producers leave
// (split-K weight-gradient products, bias tile partials, the logit head's and the skinny first
// layer's block partials) is described by one hctr_dense_seg and added by ONE body per kind, a
// function of (segment, block number within the segment, store policy).  Two kernels call them:
// dense_grad_finish_kernel, ONE launch per step over a table of segments, which stores into the
// flat gradient buffer or, SGD = true, straight through the optimizer step into the fp32 masters
// and their 16-bit copy; and dense_seg_finish_kernel, one segment for the stand-alone entries
// (hctr_sum_groups, the db of hctr_relu_bwd_bias / hctr_cross_v2_bwd_step, hctr_logit_head,
// hctr_skinny_fc_bwd).  The order of additions is the body's, so a gradient has the same bits
// whichever way it was finished.
// ================================================================================================
// a segment's source or gradient address as a pointer.  The table holds integers, and a pointer
// made from an integer is a flat one (flat_load / flat_store); these addresses are global memory,
// and saying so gives the global instructions a kernel's pointer arguments get.
template <typename T>
__device__ __forceinline__ T* seg_ptr(int64_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (T*)reinterpret_cast<__attribute__((address_space(1))) T*>(addr);
#else
  return reinterpret_cast<T*>(addr);
#endif
}

template <bool SGD>
__device__ __forceinline__ void finish_store4(const hctr_dense_seg& sg, size_t at, f32x4 gv,
                                              float lr, float grad_scale) {
  if (!SGD) {
    *reinterpret_cast<f32x4*>(seg_ptr<float>(sg.g) + at) = gv;
    return;
  }
  f32x4* wp = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(sg.w) + at);
  const f32x4 wv = sgd_apply(*wp, gv, lr, grad_scale);
  *wp = wv;
  *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(sg.w16) + at) =
      sg.bf16 ? H16<true>::pack4(wv[0], wv[1], wv[2], wv[3])
              : H16<false>::pack4(wv[0], wv[1], wv[2], wv[3]);
}

template <bool SGD>
__device__ __forceinline__ void finish_store1(const hctr_dense_seg& sg, size_t at, float gv,
                                              float lr, float grad_scale) {
  if (!SGD) {
    seg_ptr<float>(sg.g)[at] = gv;
    return;
  }
  float* wp = reinterpret_cast<float*>(sg.w) + at;
  const float wv = sgd_apply(*wp, gv, lr, grad_scale);
  *wp = wv;
  reinterpret_cast<unsigned short*>(sg.w16)[at] =
      sg.bf16 ? H16<true>::from_f32(wv) : H16<false>::from_f32(wv);
}

// SUM_GROUPS: out[i] = sum_g in[g][i], g = 0 .. count - 1 in order; 16-bit partial products of a
// split-K GEMM -> fp32.  A thread owns 8 consecutive elements, a block 256 * 8.
// UNROLL loads in flight, added in group order whatever UNROLL is.
template <bool BF, int UNROLL>
__device__ __forceinline__ void sum_groups8(int groups, size_t n8, size_t i,
                                            const unsigned short* __restrict__ in, f32x4& lo,
                                            f32x4& hi) {
  using H = H16<BF>;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll UNROLL
  for (int g = 0; g < groups; g++) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((size_t)g * n8 + i) * 8);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      acc[2 * e] += H::lo(v[e]);
      acc[2 * e + 1] += H::hi(v[e]);
    }
  }
  lo = f32x4{acc[0], acc[1], acc[2], acc[3]};
  hi = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// SRC: the products' type, 1 bf16, 0 fp16, -1 as the segment says (a table mixes both)
template <bool SGD, int UNROLL, int SRC = -1>
__device__ __forceinline__ void finish_sum_groups(const hctr_dense_seg& sg, int blk, float lr,
                                                  float grad_scale) {
  const size_t n8 = (size_t)sg.n / 8;
  const size_t i = (size_t)blk * kBlock + threadIdx.x;
  if (i >= n8) return;
  const unsigned short* in = seg_ptr<const unsigned short>(sg.src);
  f32x4 lo, hi;
  if (SRC < 0 ? sg.src_bf16 != 0 : SRC == 1) sum_groups8<true, UNROLL>((int)sg.count, n8, i, in, lo, hi);
  else sum_groups8<false, UNROLL>((int)sg.count, n8, i, in, lo, hi);
  finish_store4<SGD>(sg, (size_t)sg.dst + i * 8, lo, lr, grad_scale);
  finish_store4<SGD>(sg, (size_t)sg.dst + i * 8 + 4, hi, lr, grad_scale);
}

// COLSUM: db[c .. c + 3] = sum over tiles of partial[tile][c .. c + 3].  A block of 256 threads
// owns 8 float4 column groups x 32 tile groups: tile group tg adds tiles tg, tg + 32, ... in order,
// then the 32 group sums are added in group order through LDS (red: 256 f32x4).
template <bool SGD>
__device__ __forceinline__ void finish_colsum(const hctr_dense_seg& sg, int blk, f32x4* red,
                                              float lr, float grad_scale) {
  const float* partial = seg_ptr<const float>(sg.src);
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
    finish_store4<SGD>(sg, (size_t)sg.dst + (size_t)c4 * 4, sum, lr, grad_scale);
  }
}

// The chunked block sum of the logit head's and the skinny first layer's block partials
// (partial[block][stride], this block's 64 consecutive columns, `col` the thread's): 16 chunk
// groups of ceil(blocks / 16) consecutive blocks, each added in block order with 8 loads in flight,
// then the 16 group sums in group order through LDS (part: float [16][64]).  The groups are dealt
// to the block's WAVES wavefronts -- a template argument, which the caller keeps equal to
// blockDim.x / 64: one each at 1024 threads (straight-line code), four each, one after the other,
// at 256 -- the same sums.  The total is valid in the first wavefront.
template <int WAVES>
__device__ __forceinline__ float finish_block_chunks(float (*part)[64], int blocks, size_t stride,
                                                     size_t col, bool live,
                                                     const float* __restrict__ partial) {
  const int c = threadIdx.x & 63;
  const int chunk = (blocks + 15) / 16;
  for (int grp = threadIdx.x >> 6; grp < 16; grp += WAVES) {
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

// LOGIT_HEAD: partial [count blocks][K + 2] = dw, db, loss; *loss = sum / batch (sg.k)
template <bool SGD, int WAVES>
__device__ __forceinline__ void finish_logit_head(const hctr_dense_seg& sg, int blk,
                                                  float (*part)[64], float lr, float grad_scale,
                                                  float* __restrict__ loss) {
  const int K = (int)sg.n;
  const int k = blk * 64 + (int)(threadIdx.x & 63);
  const bool live = k < K + 2;
  const float tot = finish_block_chunks<WAVES>(part, (int)sg.count, (size_t)(K + 2), (size_t)k, live,
                                        seg_ptr<const float>(sg.src));
  if (threadIdx.x < 64 && live) {
    if (k < K) finish_store1<SGD>(sg, (size_t)sg.dst + k, tot, lr, grad_scale);
    else if (k == K) finish_store1<SGD>(sg, (size_t)sg.dst2, tot, lr, grad_scale);
    else if (loss) *loss = tot / (float)(size_t)sg.k;
  }
}

// SKINNY: partial [count blocks][N][kSkinnyK + 1] -> dw [N][K] and db [N]
template <bool SGD, int WAVES>
__device__ __forceinline__ void finish_skinny(const hctr_dense_seg& sg, int blk, float (*part)[64],
                                              float lr, float grad_scale) {
  const int stride = kSkinnyK + 1;
  const int K = (int)sg.k, total = (int)sg.n * stride;
  const int i = blk * 64 + (int)(threadIdx.x & 63);
  const bool live = i < total;
  const float tot = finish_block_chunks<WAVES>(part, (int)sg.count, (size_t)total, (size_t)i, live,
                                        seg_ptr<const float>(sg.src));
  if (threadIdx.x < 64 && live) {
    const int n = i / stride, kk = i % stride;
    if (kk == kSkinnyK) finish_store1<SGD>(sg, (size_t)sg.dst2 + n, tot, lr, grad_scale);
    else if (kk < K) finish_store1<SGD>(sg, (size_t)sg.dst + (size_t)n * K + kk, tot, lr, grad_scale);
  }
}

template <bool SGD>
__global__ void __launch_bounds__(kBlock)
    dense_grad_finish_kernel(const hctr_dense_seg* __restrict__ segs, int nseg, float lr,
                             float grad_scale, float* __restrict__ loss) {
  __shared__ f32x4 red[kBlock];  // colsum: [32 tile groups][8]; head / skinny: float [16][64]
  const hctr_dense_seg sg = segs[find_segment(segs, nseg)];
  const int blk = (int)((long long)blockIdx.x - sg.block0);
  switch ((int)sg.kind) {
    // (the usual 16 groups: all 16 loads in flight)
    case HCTR_DENSE_SEG_SUM_GROUPS: return finish_sum_groups<SGD, 16>(sg, blk, lr, grad_scale);
    case HCTR_DENSE_SEG_COLSUM: return finish_colsum<SGD>(sg, blk, red, lr, grad_scale);
    case HCTR_DENSE_SEG_LOGIT_HEAD:
      return finish_logit_head<SGD, kWavesPerBlock>(sg, blk, reinterpret_cast<float(*)[64]>(red), lr,
                                                    grad_scale, loss);
    case HCTR_DENSE_SEG_SKINNY:
      return finish_skinny<SGD, kWavesPerBlock>(sg, blk, reinterpret_cast<float(*)[64]>(red), lr,
                                                grad_scale);
    default: {  // HCTR_DENSE_SEG_DIRECT: the gradient is in g already; only the step is left
      if (!SGD) return;
      const size_t i = (size_t)blk * kBlock + threadIdx.x;
      if (i >= (size_t)sg.n / 4) return;
      const size_t at = (size_t)sg.dst + i * 4;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(sg.g) + at);
      finish_store4<SGD>(sg, at, gv, lr, grad_scale);
      return;
    }
  }
}

// one segment of kind KIND, gradients only: the finish of a stand-alone entry.  256 threads for the
// group and column sums, 1024 for the chunked block sums (one chunk group per wavefront).  KIND is a
// template argument, like the wavefront count of the chunked sums, and the group sum keeps 4 loads
// in flight here: as measured, a switch on the kind inside one kernel, blockDim.x for the wavefront
// count and 16 loads in flight were each slower (profiles/dense_refactor_ab.txt).
constexpr int seg_finish_threads(int kind) {
  return kind == HCTR_DENSE_SEG_LOGIT_HEAD || kind == HCTR_DENSE_SEG_SKINNY ? 1024 : kBlock;
}

template <int KIND, int SRC>
__global__ void __launch_bounds__(seg_finish_threads(KIND))
    dense_seg_finish_kernel(const hctr_dense_seg sg, float* __restrict__ loss) {
  __shared__ f32x4 red[kBlock];
  const int blk = (int)blockIdx.x;
  constexpr int WAVES = seg_finish_threads(KIND) / 64;
  float(*part)[64] = reinterpret_cast<float(*)[64]>(red);
  if (KIND == HCTR_DENSE_SEG_SUM_GROUPS) finish_sum_groups<false, 4, SRC>(sg, blk, 0.f, 0.f);
  if (KIND == HCTR_DENSE_SEG_COLSUM) finish_colsum<false>(sg, blk, red, 0.f, 0.f);
  if (KIND == HCTR_DENSE_SEG_LOGIT_HEAD)
    finish_logit_head<false, WAVES>(sg, blk, part, 0.f, 0.f, loss);
  if (KIND == HCTR_DENSE_SEG_SKINNY)
    finish_skinny<false, WAVES>(sg, blk, part, 0.f, 0.f);
}

}  // namespace
}  // namespace hctr

using namespace hctr;

// ================================================================================================
// Host entries, in the order of the kernels above.  Run-time value -> template argument as in
// common.h (with_bool / with_dtype).
// ================================================================================================
namespace {

template <int N>
using int_c = std::integral_constant<int, N>;

// the 16-bit element type of a dtype the caller has required to be HCTR_EMB_BF16 or HCTR_EMB_F16
template <bool BF>
using T16 = std::conditional_t<BF, __hip_bfloat16, __half>;

inline bool is16(int dtype) { return dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16; }
inline bool aligned(const void* p, size_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// f(int_c<NPL>{}): the 64-lane column slots per lane of the cross v1 kernels, a power of two
template <typename F>
void with_npl(int npl, F&& f) {
  if (npl <= 1) f(int_c<1>{});
  else if (npl <= 2) f(int_c<2>{});
  else if (npl <= 4) f(int_c<4>{});
  else if (npl <= 8) f(int_c<8>{});
  else if (npl <= 16) f(int_c<16>{});
  else if (npl <= 32) f(int_c<32>{});
  else f(int_c<64>{});
}

// f(int_c<NSEG>{}, int_c<ROWS>{}) of the logit head: NSEG 256-element segments cover K, a
// wavefront then takes ROWS = 8 / NSEG rows per iteration
template <typename F>
void with_head_shape(int k, F&& f) {
  const int nseg = (k + 255) / 256;
  if (nseg <= 1) f(int_c<1>{}, int_c<8>{});
  else if (nseg <= 2) f(int_c<2>{}, int_c<4>{});
  else if (nseg <= 4) f(int_c<4>{}, int_c<2>{});
  else f(int_c<8>{}, int_c<1>{});
}

// The finish of a stand-alone entry: the entry's partial sums as ONE gradients-only segment of kind
// KIND, handed to dense_seg_finish_kernel<KIND> by value.  out stands for the flat buffer (dst = 0;
// 16-byte aligned where the kind stores float4, as the entries always required).  out2 is addressed
// from it: dst2 is its signed distance in elements (both are float arrays), which the device adds to
// out as a 64-bit offset, so out2 may lie below out.
template <int KIND, int SRC = -1>
int finish_one(const void* src, size_t count, size_t n, size_t k, float* out, float* out2,
               float* loss, hipStream_t s) {
  hctr_dense_seg sg = {};
  sg.kind = KIND;
  sg.src = (int64_t)reinterpret_cast<uintptr_t>(src);
  sg.count = (int64_t)count;
  sg.n = (int64_t)n;
  sg.k = (int64_t)k;
  sg.g = (int64_t)reinterpret_cast<uintptr_t>(out);
  if (out2) sg.dst2 = ((int64_t)reinterpret_cast<uintptr_t>(out2) - sg.g) / (int64_t)sizeof(float);
  sg.src_bf16 = SRC == 1;
  hipLaunchKernelGGL((dense_seg_finish_kernel<KIND, SRC>), dim3(hctr_dense_seg_blocks(KIND, n)),
                     dim3(seg_finish_threads(KIND)), 0, s, sg, loss);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace

extern "C" {

// ---- cross v1 --------------------------------------------------------------------------------------
int hctr_cross_v1_fwd(size_t batch, int width, int layers, const float* x0, const float* kernels,
                      const float* biases, float* outputs, float* hiddens, hctr_stream_t stream) {
  HCTR_REQUIRE(width >= 1 && layers >= 1, "shape");
  HCTR_REQUIRE(width <= 64 * 64, "cross v1: width > 4096 not supported");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(x0 && kernels && biases && outputs && hiddens, "null pointer");
  hipStream_t s = as_stream(stream);
  with_npl((width + 63) / 64, [&](auto npl) {
    hipLaunchKernelGGL(cross_v1_fwd_kernel<decltype(npl)::value>, dim3(grid_for(batch * 64, kBlock)),
                       dim3(kBlock), 0, s, batch, width, layers, x0, kernels, biases, outputs,
                       hiddens);
  });
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
  // one wavefront per workgroup with its partial rows in LDS while they fit, else in the workspace
  const size_t lds_bytes = (size_t)layers * 2 * width * sizeof(float);
  with_npl((width + 63) / 64, [&](auto npl) {
    with_bool(lds_bytes <= 60 * 1024, [&](auto lds) {
      constexpr bool LDS = decltype(lds)::value;
      hipLaunchKernelGGL((cross_v1_bwd_kernel<decltype(npl)::value, LDS>),
                         dim3(LDS ? kCrossBwdWaves : kCrossBwdWaves / kWavesPerBlock),
                         dim3(LDS ? 64 : kBlock), LDS ? lds_bytes : 0, s, batch, width, layers, x0,
                         kernels, outputs, hiddens, out_grad, in_grad, workspace);
    });
  });
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cross_v1_reduce_kernel,
                     dim3((unsigned)ceil_div<size_t>((size_t)layers * 2 * width, 32)),
                     dim3(kBlock), 0, s, (size_t)kCrossBwdWaves, width, layers, workspace,
                     kernel_grads, bias_grads);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// ---- column-tile producers -------------------------------------------------------------------------
size_t hctr_relu_bwd_bias_workspace_bytes(size_t rows, int n) {
  return ceil_div<size_t>(rows, (size_t)kRbRows) * (size_t)n * sizeof(float);
}

// finish = false: the tile partials stay in the workspace (hctr_dense_grad_finish adds them)
static int relu_bwd_bias_impl(size_t rows, int n, const void* dy, const void* y, void* dz, float* db,
                              float* workspace, int dtype, bool finish, hctr_stream_t stream) {
  HCTR_REQUIRE(n > 0 && n % 8 == 0, "n must be a multiple of 8");
  HCTR_REQUIRE(is16(dtype), "16-bit dtypes only");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(dy && y && dz && (db || !finish) && workspace, "null pointer");
  hipStream_t s = as_stream(stream);
  const size_t tiles = ceil_div<size_t>(rows, (size_t)kRbRows);
  const int cw = n / 8 < kBlock ? n / 8 : kBlock;
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    hipLaunchKernelGGL(relu_bwd_bias_kernel<decltype(bf)::value>, dim3((unsigned)tiles),
                       dim3(kBlock), 0, s, rows, n, cw, kBlock / cw, (const unsigned short*)dy,
                       (const unsigned short*)y, (unsigned short*)dz, workspace);
  });
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  return finish_one<HCTR_DENSE_SEG_COLSUM>(workspace, tiles, (size_t)n, 0, db, nullptr, nullptr,
                                           s);
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
  HCTR_REQUIRE(is16(dtype), "16-bit dtypes only");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(dy && x0 && h && acc && s0 && db && workspace, "null pointer");
  hipStream_t s = as_stream(stream);
  const int cw = width / 8 < kBlock ? width / 8 : kBlock;
  const int rpt = cross_step_rows_per_tile(batch, width);
  const size_t tiles = ceil_div<size_t>(batch, (size_t)rpt);
  const unsigned col_blocks = (unsigned)ceil_div<int>(width / 8, cw);
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    with_bool(first != 0, [&](auto f) {
      hipLaunchKernelGGL((cross_v2_bwd_step_kernel<decltype(bf)::value, decltype(f)::value>),
                         dim3((unsigned)tiles, col_blocks), dim3(kBlock), 0, s, batch, width, cw,
                         kBlock / cw, rpt, (const unsigned short*)dy, (const unsigned short*)x0,
                         (const unsigned short*)h, (unsigned short*)acc, (unsigned short*)s0,
                         workspace);
    });
  });
  HCTR_LAUNCH_CHECK();
  return finish_one<HCTR_DENSE_SEG_COLSUM>(workspace, tiles, (size_t)width, 0, db, nullptr,
                                           nullptr, s);
}

// ---- loss and logit head ---------------------------------------------------------------------------
size_t hctr_bce_loss_workspace_bytes(void) { return kBceBlocks * sizeof(float); }

int hctr_bce_loss(size_t batch, const void* logit, const float* label, float grad_scale,
                  void* dlogit, float* loss, float* workspace, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(batch > 0, "empty batch");
  HCTR_REQUIRE(logit && label && loss && workspace, "null pointer");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || is16(dtype), "bad dtype");
  hipStream_t s = as_stream(stream);
  const int blocks = (int)std::min<size_t>(ceil_div<size_t>(batch, (size_t)kBlock), (size_t)kBceBlocks);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(bce_kernel<T>, dim3(blocks), dim3(kBlock), 0, s, batch, (const T*)logit, label,
                       grad_scale, (T*)dlogit, workspace);
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(kBlock), 0, s, blocks, batch, workspace, loss);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_logit_head_workspace_bytes(int k) { return (size_t)kHeadBlocks * (k + 2) * sizeof(float); }

static int logit_head_check(size_t batch, int k) {
  HCTR_REQUIRE(batch > 0 && k >= 4 && k % 4 == 0 && k <= 256 * kHeadMaxSeg,
               "logit head: K must be a multiple of 4 and <= 2048");
  return HCTR_OK;
}

int hctr_logit_head_blocks(size_t batch, int k) {
  HCTR_TRY(logit_head_check(batch, k));
  int rows = 0;
  with_head_shape(k, [&](auto, auto r) { rows = decltype(r)::value; });
  return (int)std::min<size_t>((size_t)kHeadBlocks,
                               ceil_div<size_t>(batch, (size_t)(kBlock / 64) * rows));
}

// finish = false: the block partials stay in the workspace (hctr_dense_grad_finish adds them)
static int logit_head_impl(size_t batch, int k, const void* x, const void* w, const void* bias,
                           const float* label, float grad_scale, void* dx, float* dw, float* db,
                           float* loss, float* workspace, int dtype, bool finish,
                           hctr_stream_t stream) {
  HCTR_TRY(logit_head_check(batch, k));
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "16-bit activations");
  HCTR_REQUIRE(x && w && bias && label && ((dw && db && loss) || !finish) && workspace,
               "null pointer");
  HCTR_REQUIRE(aligned(x, 8) && aligned(w, 8) && aligned(dx, 8), "8-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const int blocks = hctr_logit_head_blocks(batch, k);
  const size_t lds = (size_t)(kBlock / 64) * (k + 2) * sizeof(float);
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    using T = T16<decltype(bf)::value>;
    with_head_shape(k, [&](auto nseg, auto rows) {
      hipLaunchKernelGGL((logit_head_kernel<T, decltype(nseg)::value, decltype(rows)::value>),
                         dim3(blocks), dim3(kBlock), lds, s, batch, k, (const T*)x, (const T*)w,
                         (const T*)bias, label, grad_scale, (T*)dx, workspace);
    });
  });
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  return finish_one<HCTR_DENSE_SEG_LOGIT_HEAD>(workspace, (size_t)blocks, (size_t)k, batch, dw,
                                               db, loss, s);
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

// ---- skinny first layer ----------------------------------------------------------------------------
static int skinny_check(size_t batch, int k, int n) {
  HCTR_REQUIRE(batch > 0 && k >= 1 && k <= kSkinnyK, "skinny fc: 1 <= K <= 16");
  HCTR_REQUIRE(n >= 4 && n % 4 == 0 && n <= 512, "skinny fc: N a multiple of 4, <= 512");
  return HCTR_OK;
}

int hctr_skinny_fc_fwd(size_t batch, int k, int n, const float* x, const void* w, const void* bias,
                       void* y, int dtype, hctr_stream_t stream) {
  HCTR_TRY(skinny_check(batch, k, n));
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "16-bit weights / activations");
  HCTR_REQUIRE(x && w && bias && y, "null pointer");
  HCTR_REQUIRE(aligned(y, 8), "8-byte aligned output");
  hipStream_t s = as_stream(stream);
  // R consecutive rows per block (even, <= 256: 16 KB of LDS), about 4 blocks per CU
  size_t rows = ceil_div<size_t>(batch, 1024);
  rows = std::min<size_t>(256, (rows + 1) / 2 * 2);
  const int blocks = (int)ceil_div<size_t>(batch, rows);
  const size_t lds = rows * kSkinnyK * sizeof(float);
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    using T = T16<decltype(bf)::value>;
    hipLaunchKernelGGL(skinny_fc_fwd_kernel<T>, dim3(blocks), dim3(kBlock), lds, s, batch, k, n,
                       (int)rows, x, (const T*)w, (const T*)bias, (T*)y);
  });
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
  *mfma = want_mfma && k < kSkinnyK && n % 8 == 0 && aligned(dy, 16) && aligned(y, 16);
  const int rows = *mfma ? (kSkinnyBwdBlock / 64) / ceil_div<int>(n, 128) * 16
                         : kSkinnyBwdBlock / kSkinnyLanes;
  return (int)std::min<size_t>((size_t)kSkinnyBlocks, ceil_div<size_t>(batch, (size_t)rows));
}

int hctr_skinny_fc_bwd_blocks(size_t batch, int k, int n, const void* dy, const void* y) {
  HCTR_TRY(skinny_check(batch, k, n));
  bool mfma;
  return skinny_bwd_blocks(batch, k, n, dy, y, &mfma);
}

// finish = false: the block partials stay in the workspace (hctr_dense_grad_finish adds them)
static int skinny_fc_bwd_impl(size_t batch, int k, int n, const float* x, const void* dy,
                              const void* y, float* dw, float* db, float* workspace, int dtype,
                              bool finish, hctr_stream_t stream) {
  HCTR_TRY(skinny_check(batch, k, n));
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "16-bit weights / activations");
  HCTR_REQUIRE(x && dy && y && ((dw && db) || !finish) && workspace, "null pointer");
  HCTR_REQUIRE(aligned(dy, 8) && aligned(y, 8), "8-byte aligned activations");
  hipStream_t s = as_stream(stream);
  const size_t lds = (size_t)n * (kSkinnyK + 1) * sizeof(float);
  bool mfma;
  const int blocks = skinny_bwd_blocks(batch, k, n, dy, y, &mfma);
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    using T = T16<decltype(bf)::value>;
    with_bool(mfma, [&](auto m) {
      constexpr auto kernel =
          decltype(m)::value ? skinny_fc_bwd_mfma_kernel<T> : skinny_fc_bwd_kernel<T>;
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kSkinnyBwdBlock), lds, s, batch, k, n, x,
                         (const T*)dy, (const T*)y, workspace);
    });
  });
  HCTR_LAUNCH_CHECK();
  if (!finish) return HCTR_OK;
  return finish_one<HCTR_DENSE_SEG_SKINNY>(workspace, (size_t)blocks, (size_t)n, (size_t)k, dw,
                                           db, nullptr, s);
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

// ---- optimizers ------------------------------------------------------------------------------------
int hctr_sgd_shadow(size_t n, float lr, float grad_scale, float* w, const float* g, void* w16,
                    int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(n % 4 == 0, "n must be a multiple of 4");
  HCTR_REQUIRE(is16(dtype), "16-bit shadow dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(w && g && w16, "null pointer");
  hipStream_t s = as_stream(stream);
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    hipLaunchKernelGGL(sgd_shadow_kernel<decltype(bf)::value>, dim3(grid_for(n / 4, kBlock, 4096)),
                       dim3(kBlock), 0, s, n / 4, lr, grad_scale, w, g, (unsigned short*)w16);
  });
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

int hctr_ftrl_shadow(size_t n, float lr, float beta, float lambda1, float lambda2, float grad_scale,
                     float* w, float* z, float* nacc, const float* g, void* w16, int dtype,
                     hctr_stream_t stream) {
  HCTR_REQUIRE(n % 4 == 0, "n must be a multiple of 4");
  HCTR_TRY(ftrl_check(lr, beta, lambda1, lambda2, grad_scale));
  HCTR_REQUIRE(!w16 || is16(dtype), "16-bit shadow dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(w && z && nacc && g, "null pointer");
  HCTR_REQUIRE(aligned(w, 16) && aligned(z, 16) && aligned(nacc, 16) && aligned(g, 16) &&
                   aligned(w16, 16),
               "16-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const FtrlHp h = {lr, lambda1, lambda2 + beta / lr, grad_scale};
  const dim3 grid(grid_for(n / 4, kBlock, 4096));
  // SHADOW 0: no 16-bit copy, 1: fp16, 2: bf16
  auto launch = [&](auto shadow) {
    hipLaunchKernelGGL(ftrl_shadow_kernel<decltype(shadow)::value>, grid, dim3(kBlock), 0, s, n / 4,
                       h, w, z, nacc, g, (unsigned short*)w16);
  };
  if (!w16) launch(int_c<0>{});
  else if (dtype == HCTR_EMB_F16) launch(int_c<1>{});
  else launch(int_c<2>{});
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
  HCTR_REQUIRE(aligned(z, 16) && aligned(nacc, 16) && aligned(g, 16), "16-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const FtrlHp h = {lr, lambda1, lambda2 + beta / lr, grad_scale};
  hipLaunchKernelGGL(ftrl_segments_kernel, dim3((unsigned)nblocks), dim3(kBlock), 0, s, segs, nseg,
                     h, z, nacc, g);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// ---- fixed-order sums and the finish launch --------------------------------------------------------
int hctr_sum_groups(int groups, size_t n, const void* in, int dtype, float* out,
                    hctr_stream_t stream) {
  HCTR_REQUIRE(groups > 0 && n % 8 == 0, "n must be a multiple of 8");
  HCTR_REQUIRE(is16(dtype), "16-bit dtypes only");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(in && out, "null pointer");
  int rc = HCTR_OK;
  with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
    rc = finish_one<HCTR_DENSE_SEG_SUM_GROUPS, decltype(bf)::value ? 1 : 0>(
        in, (size_t)groups, n, 0, out, nullptr, nullptr, as_stream(stream));
  });
  return rc;
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
  with_bool(sgd != 0, [&](auto sg) {
    hipLaunchKernelGGL(dense_grad_finish_kernel<decltype(sg)::value>, dim3((unsigned)nblocks),
                       dim3(kBlock), 0, s, segs, nseg, lr, grad_scale, loss);
  });
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
