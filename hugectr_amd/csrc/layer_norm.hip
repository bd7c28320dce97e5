// layer_norm.hip -- LayerNormLayer<T> (R/HugeCTR/src/layers/layer_norm_layer.cu) with the residual
// add in front of it folded in, forward and backward, for gfx950 (wave 64).  Per row of `hidden`
// elements, z = x or x + residual:
//   mean = sum(z) / hidden,  var = sum((z - mean)^2) / hidden (two passes around the mean),
//   rstd = 1 / sqrt(var + eps),  y = (z - mean) rstd gamma + beta
//   t = dy gamma, xh = (z - mean) rstd:  dz = rstd (t - mean(t) - xh mean(t xh)),
//   dgamma = sum_rows dy xh,  dbeta = sum_rows dy;  dz is the gradient of x AND of residual.
// Activations fp32 / fp16 / bf16; gamma, beta, their gradients and all arithmetic fp32.
//
// The operator is HBM traffic and nothing else, and its rows are narrow (hidden 16 .. 256, millions
// of rows), so the design is about who owns a row.  A row is cut into chunks of 16 bytes (V = 4 fp32
// or 8 16-bit elements) and owned by a GROUP of G lanes; lane l of the group holds chunks l, l + G,
// ... (K of them, E = K V elements) in registers from the row's one read to its one write:
//   hidden <= V G, G = 1, 2, 4 .. 64   one chunk a lane (E = V); 64 / G rows share a wavefront and
//                                      256 / G a workgroup; every lane issues one 16-byte load
//   hidden <= 1024, <= 2048            G = 64, E = 16, 32: a wavefront owns the row
//   hidden <= 4096, <= 8192            G = 256, E = 16, 32: the workgroup owns the row, its four
//                                      wavefronts' partial sums meet in LDS (block_reduce_sum)
// A row sum is a butterfly over the group's lanes (group_reduce_sum: no LDS, no barrier, no atomic;
// every lane ends with the same bits), so with the row in registers the second pass around the mean
// costs no memory access.  A width that is no multiple of V (or a misaligned buffer) takes the same
// kernels with element loads and stores -- its rows do not start on 16-byte boundaries.  Chunks
// past the row's end read column 0 (in bounds) and count as zeros.  Workgroups of 256 threads walk
// the rows grid-stride; gamma and beta are read once per lane, before the walk.
//
// Forward: y, and when the caller wants a gradient, (mean, rstd) as fp32 [rows][2].  Backward, one
// kernel: reads x (+ residual), dy and the statistics again, recomputes xh, writes dz, and keeps the
// lane's E column partials of dgamma / dbeta in registers across all rows the workgroup walks.  At
// the end the groups of a wavefront add theirs by a butterfly over the lanes G, 2 G .. 32 apart,
// the four wavefronts' sums meet in LDS and are added in wavefront order, and the workgroup writes
// one [2][hidden] fp32 partial into the caller's scratch.  ln_finish_kernel adds the partials in
// ascending workgroup order (eight contiguous slices per column, the slices then in order).  The
// grids depend on (rows, hidden, dtype) only and nothing is atomic: two runs give the same bits.
#include <cmath>
#include <type_traits>

#include "block_prims.h"
#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace ln {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxHidden = 8192;
constexpr int kFwdGrid = 2048;     // 8 workgroups a CU
constexpr int kBwdGrid = 1024;     // the backward holds five rows' worth of registers
constexpr int kFinishCols = 32, kFinishSlices = kThreads / kFinishCols;

// V consecutive elements, 16-byte aligned: one or two 16-byte accesses
template <typename S, int V>
struct alignas(16) Pack {
  S e[V];
};

// how the lanes of a workgroup own rows: G lanes a row, E elements a lane in chunks of V
template <typename T, int G_, int E_ = 16 / (int)sizeof(T)>
struct Lanes {
  static constexpr int G = G_;
  static constexpr int V = 16 / (int)sizeof(T);
  static constexpr int E = E_;
  static constexpr int K = E / V;
  static constexpr int kRows = G >= kThreads ? 1 : kThreads / G;  // rows of one workgroup trip
  static_assert(G == kThreads || (G <= 64 && (G & (G - 1)) == 0), "G: 1, 2, 4 .. 64 or the workgroup");
  // the first column of the lane's chunk k
  __device__ __forceinline__ static int col(int lane, int k) { return (k * G + lane) * V; }
};

// the lane's E elements of a row (or of gamma / beta: S = float) as fp32; what lies past the row's
// end is 0.  All loads are issued before the first conversion
template <typename L, typename S>
__device__ __forceinline__ void load_row(const S* __restrict__ row, int lane, int hidden, bool vec,
                                         float (&f)[L::E]) {
  if (vec) {
    Pack<S, L::V> p[L::K];
#pragma unroll
    for (int k = 0; k < L::K; k++) {
      const int c = L::col(lane, k);
      p[k] = *reinterpret_cast<const Pack<S, L::V>*>(row + (c < hidden ? c : 0));
    }
#pragma unroll
    for (int k = 0; k < L::K; k++)
#pragma unroll
      for (int e = 0; e < L::V; e++)
        f[k * L::V + e] = L::col(lane, k) < hidden ? to_f32<S>(p[k].e[e]) : 0.f;
  } else {
#pragma unroll
    for (int k = 0; k < L::K; k++)
#pragma unroll
      for (int e = 0; e < L::V; e++) {
        const int c = L::col(lane, k) + e;
        const float v = to_f32<S>(row[c < hidden ? c : 0]);
        f[k * L::V + e] = c < hidden ? v : 0.f;
      }
  }
}

template <typename L, typename S>
__device__ __forceinline__ void store_row(S* __restrict__ row, int lane, int hidden, bool vec,
                                          const float (&f)[L::E]) {
#pragma unroll
  for (int k = 0; k < L::K; k++) {
    const int c = L::col(lane, k);
    if (vec) {
      Pack<S, L::V> p;
#pragma unroll
      for (int e = 0; e < L::V; e++) p.e[e] = from_f32<S>(f[k * L::V + e]);
      if (c < hidden) *reinterpret_cast<Pack<S, L::V>*>(row + c) = p;
    } else {
#pragma unroll
      for (int e = 0; e < L::V; e++)
        if (c + e < hidden) row[c + e] = from_f32<S>(f[k * L::V + e]);
    }
  }
}

// a row's sum over its owners: the group's butterfly, or the workgroup's four wavefronts through LDS
template <typename L>
__device__ __forceinline__ float row_sum(float v, float* red) {
  if constexpr (L::G <= 64) return group_reduce_sum<L::G>(v);
  else return block_reduce_sum<float, kThreads>(v, red);
}

template <typename T, typename L>
__global__ __launch_bounds__(kThreads) void ln_fwd_kernel(
    size_t rows, int hidden, const T* __restrict__ x, const T* __restrict__ residual,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    T* __restrict__ y, float* __restrict__ stats, bool vec) {
  constexpr int E = L::E;
  __shared__ float red[kThreads / 64];
  const int lane = threadIdx.x % L::G, grp = threadIdx.x / L::G;
  float g[E], b[E];
  load_row<L>(gamma, lane, hidden, vec, g);
  load_row<L>(beta, lane, hidden, vec, b);
  const float h = (float)hidden;
  for (size_t base = (size_t)blockIdx.x * L::kRows; base < rows; base += (size_t)gridDim.x * L::kRows) {
    // (a group past the last row reads the trip's first row again and writes nothing: the loop,
    //  the shuffles and the barriers stay uniform)
    const bool live = base + grp < rows;
    const size_t row = live ? base + grp : base;
    float z[E];
    load_row<L>(x + row * hidden, lane, hidden, vec, z);
    if (residual) {
      float r[E];
      load_row<L>(residual + row * hidden, lane, hidden, vec, r);
#pragma unroll
      for (int e = 0; e < E; e++) z[e] += r[e];
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) s += z[e];
    const float mean = row_sum<L>(s, red) / h;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) {
      z[e] = L::col(lane, e / L::V) + e % L::V < hidden ? z[e] - mean : 0.f;
      q += z[e] * z[e];
    }
    const float rstd = 1.f / sqrtf(row_sum<L>(q, red) / h + eps);
    if (!live) continue;
#pragma unroll
    for (int e = 0; e < E; e++) z[e] = z[e] * rstd * g[e] + b[e];
    store_row<L>(y + row * hidden, lane, hidden, vec, z);
    if (stats && lane == 0) *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(mean, rstd);
  }
}

template <typename T, typename L>
__global__ __launch_bounds__(kThreads) void ln_bwd_kernel(
    size_t rows, int hidden, const T* __restrict__ x, const T* __restrict__ residual,
    const float* __restrict__ gamma, const float* __restrict__ stats, const T* __restrict__ dy,
    T* __restrict__ dz, float* __restrict__ partial, bool vec) {
  constexpr int E = L::E, G = L::G;
  // the wavefronts' column partials, [wavefront][element][lane]; G = 256: block_reduce_sum's slots
  __shared__ float red[G <= 64 ? (kThreads / 64) * G * E : kThreads / 64];
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  float g[E], dg[E], db[E];
  load_row<L>(gamma, lane, hidden, vec, g);
#pragma unroll
  for (int e = 0; e < E; e++) dg[e] = db[e] = 0.f;
  const float h = (float)hidden;
  for (size_t base = (size_t)blockIdx.x * L::kRows; base < rows; base += (size_t)gridDim.x * L::kRows) {
    const bool live = base + grp < rows;
    const size_t row = live ? base + grp : base;
    float xh[E], d[E];
    load_row<L>(x + row * hidden, lane, hidden, vec, xh);
    load_row<L>(dy + row * hidden, lane, hidden, vec, d);
    if (residual) {
      float r[E];
      load_row<L>(residual + row * hidden, lane, hidden, vec, r);
#pragma unroll
      for (int e = 0; e < E; e++) xh[e] += r[e];
    }
    const float2 st = *reinterpret_cast<const float2*>(stats + 2 * row);  // (mean, rstd)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) {
      xh[e] = L::col(lane, e / L::V) + e % L::V < hidden ? (xh[e] - st.x) * st.y : 0.f;
      const float t = d[e] * g[e];
      s1 += t;
      s2 += t * xh[e];
    }
    s1 = row_sum<L>(s1, red) / h;
    s2 = row_sum<L>(s2, red) / h;
    if (!live) continue;
    float o[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      o[e] = st.y * (d[e] * g[e] - s1 - xh[e] * s2);
      dg[e] += d[e] * xh[e];
      db[e] += d[e];
    }
    store_row<L>(dz + row * hidden, lane, hidden, vec, o);
  }

  float* out = partial + (size_t)blockIdx.x * 2 * hidden;  // [dgamma | dbeta][hidden]
  if constexpr (G == kThreads) {  // every thread is the only owner of its columns
    store_row<L>(out, lane, hidden, vec, dg);
    store_row<L>(out + hidden, lane, hidden, vec, db);
  } else {
    const int wave = threadIdx.x / 64;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      float (&acc)[E] = pass ? db : dg;
#pragma unroll
      for (int e = 0; e < E; e++) {
        float v = acc[e];  // over the wavefront's groups
#pragma unroll
        for (int dist = 32; dist >= G; dist >>= 1) v += __shfl_xor(v, dist, 64);
        if ((threadIdx.x & 63) < G) red[(wave * E + e) * G + lane] = v;
      }
      __syncthreads();
      for (int j = threadIdx.x; j < G * E; j += kThreads) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < kThreads / 64; w++) s += red[w * E * G + j];
        const int e = j / G, c = L::col(j % G, e / L::V) + e % L::V;
        if (c < hidden) out[pass * hidden + c] = s;
      }
      __syncthreads();
    }
  }
}

// dgamma | dbeta [2 hidden] = the workgroups' partials [n][2 hidden] added in ascending order: a
// workgroup takes 32 columns, eight threads a column, each a contiguous slice of the partials
__global__ __launch_bounds__(kThreads) void ln_finish_kernel(int n, int hidden,
                                                             const float* __restrict__ partial,
                                                             float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  __shared__ float red[kFinishSlices][kFinishCols];
  const int cl = threadIdx.x % kFinishCols, slice = threadIdx.x / kFinishCols;
  const int c = blockIdx.x * kFinishCols + cl, width = 2 * hidden;
  const int per = (n + kFinishSlices - 1) / kFinishSlices;
  const int lo = slice * per, hi = lo + per < n ? lo + per : n;
  float s = 0.f;
  if (c < width)
    for (int w = lo; w < hi; w++) s += partial[(size_t)w * width + c];
  red[slice][cl] = s;
  __syncthreads();
  if (slice == 0 && c < width) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kFinishSlices; i++) t += red[i][cl];
    if (c < hidden) dgamma[c] = t;
    else dbeta[c - hidden] = t;
  }
}

// ================================================================================================
// Host side
// ================================================================================================
// what every entry point refuses, by name, before anything else
int ln_check(size_t rows, int hidden, int dtype) {
  HCTR_REQUIRE(hidden >= 1 && hidden <= kMaxHidden, "layer_norm: hidden 1 .. 8192");
  HCTR_REQUIRE(rows <= (size_t)0x7FFFFFFF / (size_t)hidden, "layer_norm: rows * hidden < 2^31");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "layer_norm: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}

// (hidden, element type) -> f(Lanes): the one place where a shape picks its kernel
template <typename T, typename F>
int with_lanes(int hidden, F&& f) {
  constexpr int V = 16 / (int)sizeof(T);
  if (hidden <= V) return f(Lanes<T, 1>{});
  if (hidden <= 2 * V) return f(Lanes<T, 2>{});
  if (hidden <= 4 * V) return f(Lanes<T, 4>{});
  if (hidden <= 8 * V) return f(Lanes<T, 8>{});
  if (hidden <= 16 * V) return f(Lanes<T, 16>{});
  if (hidden <= 32 * V) return f(Lanes<T, 32>{});
  if (hidden <= 64 * V) return f(Lanes<T, 64>{});
  if (hidden <= 64 * 16) return f(Lanes<T, 64, 16>{});
  if (hidden <= 64 * 32) return f(Lanes<T, 64, 32>{});
  if (hidden <= kThreads * 16) return f(Lanes<T, kThreads, 16>{});
  return f(Lanes<T, kThreads, 32>{});
}

int grid_of(size_t rows, int rows_per_trip, int cap) {
  const size_t g = ceil_div<size_t>(rows, (size_t)rows_per_trip);
  return (int)(g < (size_t)cap ? g : (size_t)cap);
}

// 16-byte accesses need rows that start on 16-byte boundaries
template <typename... P>
bool vec_ok(int hidden, int V, const P*... p) {
  return hidden % V == 0 && ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}

int fwd(size_t rows, int hidden, const void* x, const void* residual, const float* gamma,
        const float* beta, float eps, void* y, float* stats, int dtype, hctr_stream_t stream) {
  HCTR_TRY(ln_check(rows, hidden, dtype));
  HCTR_REQUIRE(eps > 0.f, "layer_norm: eps > 0");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(x && gamma && beta && y, "null pointer");
  HCTR_REQUIRE(reinterpret_cast<uintptr_t>(stats) % 8 == 0, "layer_norm: 8-byte aligned stats");
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    return with_lanes<T>(hidden, [&](auto lanes) -> int {
      using L = decltype(lanes);
      const bool vec = vec_ok(hidden, L::V, x, residual, gamma, beta, y);
      hipLaunchKernelGGL((ln_fwd_kernel<T, L>), dim3(grid_of(rows, L::kRows, kFwdGrid)),
                         dim3(kThreads), 0, s, rows, hidden, (const T*)x, (const T*)residual, gamma,
                         beta, eps, (T*)y, stats, vec);
      return HCTR_OK;
    });
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// the backward's grid: a function of (rows, hidden, element type) alone
template <typename L>
int bwd_grid(size_t rows) {
  return grid_of(rows, L::kRows, kBwdGrid);
}

size_t bwd_scratch_bytes(size_t rows, int hidden) {
  if (hidden < 1 || hidden > kMaxHidden) return 0;
  const size_t n = rows < (size_t)kBwdGrid ? (rows < 1 ? 1 : rows) : (size_t)kBwdGrid;
  return n * 2 * (size_t)hidden * sizeof(float);  // (no grid is larger, whatever the element type)
}

int bwd(size_t rows, int hidden, const void* x, const void* residual, const float* gamma,
        const float* stats, const void* dy, void* dz, float* dgamma, float* dbeta, void* scratch,
        int dtype, hctr_stream_t stream) {
  HCTR_TRY(ln_check(rows, hidden, dtype));
  if (rows == 0 && !(dgamma && dbeta)) return HCTR_OK;
  HCTR_REQUIRE(dgamma && dbeta, "null pointer");
  HCTR_REQUIRE(rows == 0 || (x && gamma && stats && dy && dz && scratch), "null pointer");
  HCTR_REQUIRE(reinterpret_cast<uintptr_t>(stats) % 8 == 0, "layer_norm: 8-byte aligned stats");
  hipStream_t s = as_stream(stream);
  int n = 0;  // workgroups = partials
  if (rows > 0) {
    HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
      using T = std::remove_pointer_t<decltype(t)>;
      return with_lanes<T>(hidden, [&](auto lanes) -> int {
        using L = decltype(lanes);
        const bool vec = vec_ok(hidden, L::V, x, residual, gamma, dy, dz, scratch);
        n = bwd_grid<L>(rows);
        hipLaunchKernelGGL((ln_bwd_kernel<T, L>), dim3(n), dim3(kThreads), 0, s, rows, hidden,
                           (const T*)x, (const T*)residual, gamma, stats, (const T*)dy, (T*)dz,
                           (float*)scratch, vec);
        return HCTR_OK;
      });
    }));
    HCTR_LAUNCH_CHECK();
  }
  // (no rows: no partials, the gradients of gamma and beta are zeros)
  hipLaunchKernelGGL(ln_finish_kernel, dim3(ceil_div(2 * hidden, kFinishCols)), dim3(kThreads), 0, s,
                     n, hidden, (const float*)scratch, dgamma, dbeta);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace
}  // namespace ln
}  // namespace hctr

extern "C" {

int hctr_layer_norm_fwd(size_t rows, int hidden, const void* x, const void* residual,
                        const float* gamma, const float* beta, float eps, void* y, float* stats,
                        int dtype, hctr_stream_t stream) {
  return hctr::ln::fwd(rows, hidden, x, residual, gamma, beta, eps, y, stats, dtype, stream);
}

int hctr_layer_norm_bwd(size_t rows, int hidden, const void* x, const void* residual,
                        const float* gamma, const float* stats, const void* dy, void* dz,
                        float* dgamma, float* dbeta, void* scratch, int dtype,
                        hctr_stream_t stream) {
  return hctr::ln::bwd(rows, hidden, x, residual, gamma, stats, dy, dz, dgamma, dbeta, scratch,
                       dtype, stream);
}

size_t hctr_layer_norm_bwd_scratch_bytes(size_t rows, int hidden) {
  return hctr::ln::bwd_scratch_bytes(rows, hidden);
}

}  // extern "C"
