// sequence_ops.hip -- the three dense layers the sequence models (DIN, BST) need besides attention
// and the norms, for gfx950 (wave 64), forward and backward, fp32 / fp16 / bf16:
//   MatrixMultiplyLayer<T>      R/HugeCTR/src/layers/matrix_multiply_layer.cu
//   ReduceMeanLayer<T>          R/HugeCTR/src/layers/reduce_mean_layer.cu
//   FusedReshapeConcatLayer<T>  R/HugeCTR/src/layers/fused_reshape_concat_layer.cu
// Nothing here is atomic and every grid depends on the shapes alone: two runs give the same bits.
//
// ---- batched matrix multiply -------------------------------------------------------------------
// One product form serves the forward and both gradients: per batch item, C [M][N] = X . Y with
// X(i, p) and Y(p, j) read from memory as stored or transposed, the sum over p = 0 .. K - 1 in fp32
// and one rounding on the store:
//   forward  C  = A  . B    (M, N, K) = (m, k, n)   X = A  kept [M][K]   Y = B  kept [K][N]
//   dA       dA = dC . B^T  (M, N, K) = (m, n, k)   X = dC kept [M][K]   Y = B  kept [N][K]
//   dB       dB = A^T . dC  (M, N, K) = (n, k, m)   X = A  kept [K][M]   Y = dC kept [K][N]
// No transposed copy is written anywhere; "kept [K][M]" only changes how LDS is indexed.
//
// Two bodies, picked by (m, n, k) alone (packed_shape): no keyword, no environment variable.
//
// mm_tile_kernel (MFMA).  A workgroup of four wavefronts owns a 64 x 64 tile of one item's C, each
// wavefront a 32 x 32 block of it; tiles of all items are walked grid-stride.  The sum index moves
// in steps of 16.  Per step each operand's 64 x 16 tile is fetched by 16-byte global loads in the
// orientation memory has it (one chunk a thread for 16-bit types, two for fp32), parked in
// registers while the MFMAs of the step before run, and then stored into the other of two LDS
// buffers: one barrier a step.  A tile whose sum index is contiguous is kept [64][16 + V], one
// whose sum index is the memory row [16][64 + V] (V = elements in 16 bytes; the pad keeps rows
// 16-byte aligned and off each other's banks).  An operand fragment is one 16-byte LDS read in the
// first case and eight (fp32: one) strided element reads in the second: that is the whole
// transposition.  16-bit types run v_mfma_f32_32x32x16_{f16,bf16}, one instruction a step; fp32 runs
// v_mfma_f32_16x16x4_f32 on true fp32 operands, 2 x 2 sub-blocks x four instructions a step.  A row
// pitch or pointer that is not 16-byte aligned (odd k in a 16-bit type) takes element loads into
// the same registers; whatever lies past an edge in M, N or K is a zero in LDS and is never read
// from memory.  A wavefront whose block lies wholly outside C skips the MFMAs but not the loads.
//
// mm_packed_kernel (VALU).  For items far smaller than a tile (DIN's 1 x 10 x 36): a workgroup
// takes a SLAB of consecutive items -- their X and their Y are two contiguous runs of memory, so
// they are staged in LDS by flat 16-byte loads whatever the row pitch (slabs are multiples of
// eight items, which keeps every slab 16-byte aligned) -- and then walks the slab's outputs in
// memory order, a thread an output: the lanes that share an output row read the same X element (an
// LDS broadcast) and consecutive Y elements, K fp32 FMAs each, and the stores are coalesced.
// Transposition is two strides per operand.  The body moves every byte once: it is bound by HBM.
//
// ---- reduce mean ---------------------------------------------------------------------------------
// x [outer][len][inner] -> y [outer][1][inner], fp32 sums / len.  inner == 1 (rm_row_kernel): a
// group of G = 1, 4, 16 or 64 lanes (by len) owns an output, strides its contiguous row and meets
// in a butterfly.  inner > 1 (rm_col_kernel): a lane owns a 16-byte chunk of columns of one outer
// index and walks len; when there are few such chunks and len is long, `ns` threads share a chunk,
// each a contiguous slab of rows, and the slabs' partials are added through LDS in slab order.
// The backward writes dy / len into every row.
//
// ---- fused reshape + concat ----------------------------------------------------------------------
// `num` inputs [B][S][w_i], as a by-value table in the kernel arguments, side by side into rows of
// W = sum w_i: slots 0 .. S - 2 of every sample -> item [B (S - 1)][W], slot S - 1 -> ad [B][W].
// A group of lanes moves one output row, 16 bytes a lane when every width and pointer allows,
// elements otherwise; the backward is the same walk with the copy turned round.
#include <type_traits>

#include "block_prims.h"
#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace seq {
namespace {

constexpr int kThreads = 256;
constexpr size_t kMaxElems = 0x7FFFFFFF;
constexpr int kLdsBytes = 32768;  // of the packed body's slab: five workgroups a CU

// V consecutive elements moved as one access: 16 bytes, 16-byte aligned, when V is a chunk's worth
template <typename S, int V>
struct alignas(sizeof(S) * V) Pack {
  S e[V];
};

template <typename... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}

// ================================================================================================
// Matrix multiply, MFMA body
// ================================================================================================
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kMmDim = 4096;
constexpr int kTile = 64;  // C tile of a workgroup (2 x 2 wavefronts of 32 x 32)
constexpr int kStep = 16;  // sum indices a step
constexpr int kTileGrid = 2048;

// the bits of an element as the tile kernel moves them, and the tile geometry
template <typename T>
struct Tile {
  using S = std::conditional_t<std::is_same<T, float>::value, float, unsigned short>;
  static constexpr int V = 16 / (int)sizeof(S);
  static constexpr int kPitchK = kStep + V;  // tile kept [64][16]: the sum index is contiguous
  static constexpr int kPitchR = kTile + V;  // tile kept [16][64]: the sum index is the row
  static constexpr int kElems = kTile * kPitchK > kStep * kPitchR ? kTile * kPitchK : kStep * kPitchR;
  static constexpr int kChunks = kTile * kStep / V;          // 16-byte chunks of one tile
  static constexpr int kPerThread = 2 * kChunks / kThreads;  // of both tiles: 1 (16-bit), 2 (fp32)
  static_assert(2 * kChunks % kThreads == 0, "whole chunks a thread");
};

// chunk q of a tile: its row and first column in the tile as memory (and LDS) has it
template <int V, bool KC>
__device__ __forceinline__ void chunk_rc(int q, int& r, int& c) {
  constexpr int per_row = (KC ? kStep : kTile) / V;
  r = q / per_row;
  c = (q % per_row) * V;
}

// chunk q of the tile at (e0, k0) of one item's operand: E rows or columns of C by K sum indices,
// kept [E][K] (KC) or [K][E].  Past an edge: zeros, and no access
template <typename S, int V, bool KC>
__device__ __forceinline__ Pack<S, V> load_chunk(const S* __restrict__ mat, int E, int K, int e0,
                                                 int k0, int q, bool vec) {
  int r, c;
  chunk_rc<V, KC>(q, r, c);
  const int rows = KC ? E : K, cols = KC ? K : E;
  const int gr = (KC ? e0 : k0) + r, gc = (KC ? k0 : e0) + c;
  Pack<S, V> p;
  if (vec && gr < rows && gc + V <= cols) {
    p = *reinterpret_cast<const Pack<S, V>*>(mat + (size_t)gr * cols + gc);
  } else {
#pragma unroll
    for (int e = 0; e < V; e++)
      p.e[e] = (gr < rows && gc + e < cols) ? mat[(size_t)gr * cols + gc + e] : (S)0;
  }
  return p;
}

template <typename S, int V, bool KC>
__device__ __forceinline__ void store_chunk(S* tile, int q, const Pack<S, V>& p) {
  int r, c;
  chunk_rc<V, KC>(q, r, c);
  constexpr int pitch = KC ? kStep + V : kTile + V;
  *reinterpret_cast<Pack<S, V>*>(tile + r * pitch + c) = p;
}

// element (idx, kk) of a tile: row or column idx of C's tile, sum index kk of the step
template <typename S, int V, bool KC>
__device__ __forceinline__ S tile_at(const S* tile, int idx, int kk) {
  return KC ? tile[idx * (kStep + V) + kk] : tile[kk * (kTile + V) + idx];
}

// the eight sum indices kh .. kh + 7 of row / column idx: a 32x32x16 operand fragment
template <bool KC>
__device__ __forceinline__ Pack<unsigned short, 8> frag16(const unsigned short* tile, int idx, int kh) {
  Pack<unsigned short, 8> p;
  if (KC) {
    p = *reinterpret_cast<const Pack<unsigned short, 8>*>(tile + idx * (kStep + 8) + kh);
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++) p.e[e] = tile[(kh + e) * (kTile + 8) + idx];
  }
  return p;
}

__device__ __forceinline__ f32x16 mfma16(const __half*, const Pack<unsigned short, 8>& a,
                                         const Pack<unsigned short, 8>& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a),
                                                *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma16(const __hip_bfloat16*, const Pack<unsigned short, 8>& a,
                                         const Pack<unsigned short, 8>& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a),
                                                 *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
}

// a wavefront's 32 x 32 block of C in the accumulator registers of its element type's MFMA
template <typename T>
struct Block {  // 16-bit: one 32x32x16 accumulator
  f32x16 acc;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
  }
  // A[i][k]: lane i + 32 (k / 8), element k % 8; B[k][j]: lane j + 32 (k / 8), element k % 8
  template <bool XK, bool YK>
  __device__ __forceinline__ void step(const unsigned short* xs, const unsigned short* ys, int wm,
                                       int wn, int lane) {
    const int i = lane & 31, kh = (lane >> 5) * 8;
    acc = mfma16((const T*)nullptr, frag16<XK>(xs, wm * 32 + i, kh), frag16<YK>(ys, wn * 32 + i, kh),
                 acc);
  }
  // D[i][j]: lane j + 32 ((i / 4) % 2), register 4 (i / 8) + i % 4
  template <typename F>
  __device__ __forceinline__ void for_each(int lane, F&& f) const {
#pragma unroll
    for (int r = 0; r < 16; r++) f((r / 4) * 8 + (lane >> 5) * 4 + r % 4, lane & 31, acc[r]);
  }
};
template <>
struct Block<float> {  // fp32: 2 x 2 sub-blocks of 16x16x4
  f32x4 acc[2][2];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < 4; s++) acc[s / 2][s % 2] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // A[i][k]: lane i + 16 k; B[k][j]: lane j + 16 k
  template <bool XK, bool YK>
  __device__ __forceinline__ void step(const float* xs, const float* ys, int wm, int wn, int lane) {
    const int i = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < kStep / 4; ks++) {
      float a[2], b[2];
#pragma unroll
      for (int s = 0; s < 2; s++) {
        a[s] = tile_at<float, 4, XK>(xs, wm * 32 + s * 16 + i, ks * 4 + kq);
        b[s] = tile_at<float, 4, YK>(ys, wn * 32 + s * 16 + i, ks * 4 + kq);
      }
#pragma unroll
      for (int s = 0; s < 2; s++)
#pragma unroll
        for (int t = 0; t < 2; t++)
          acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[t], acc[s][t], 0, 0, 0);
    }
  }
  // D[i][j]: lane j + 16 (i / 4), register i % 4
  template <typename F>
  __device__ __forceinline__ void for_each(int lane, F&& f) const {
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          f(s * 16 + 4 * (lane >> 4) + r, t * 16 + (lane & 15), acc[s][t][r]);
  }
};

// C [batch][M][N] = X . Y per item; XK: X kept [M][K], else [K][M]; YK: Y kept [N][K], else [K][N];
// vx, vy: the operand's rows start on 16-byte boundaries
template <typename T, bool XK, bool YK>
__global__ __launch_bounds__(kThreads) void mm_tile_kernel(size_t batch, int M, int N, int K,
                                                           const T* __restrict__ x,
                                                           const T* __restrict__ y,
                                                           T* __restrict__ c, bool vx, bool vy) {
  using G = Tile<T>;
  using S = typename G::S;
  constexpr int V = G::V;
  __shared__ uint4 raw[4 * G::kElems * sizeof(S) / 16];  // [buffer][X | Y][kElems]
  S* lds = reinterpret_cast<S*>(raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int tn = (N + kTile - 1) / kTile, per_item = ((M + kTile - 1) / kTile) * tn;
  const size_t tiles = batch * (size_t)per_item;
  const int steps = (K + kStep - 1) / kStep;

  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const size_t item = t / (size_t)per_item;
    const int rem = (int)(t % (size_t)per_item), m0 = (rem / tn) * kTile, n0 = (rem % tn) * kTile;
    const S* xi = reinterpret_cast<const S*>(x) + item * (size_t)M * K;
    const S* yi = reinterpret_cast<const S*>(y) + item * (size_t)K * N;
    T* ci = c + item * (size_t)M * N;
    const bool live = m0 + wm * 32 < M && n0 + wn * 32 < N;  // (wave-uniform)

    Pack<S, V> regs[G::kPerThread];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int u = 0; u < G::kPerThread; u++) {
        const int q = threadIdx.x + u * kThreads;  // chunks 0 .. of X, then of Y (wave-uniform)
        if (q < G::kChunks) regs[u] = load_chunk<S, V, XK>(xi, M, K, m0, k0, q, vx);
        else regs[u] = load_chunk<S, V, YK>(yi, N, K, n0, k0, q - G::kChunks, vy);
      }
    };
    auto park = [&](int buf) {
      S* xs = lds + buf * 2 * G::kElems;
#pragma unroll
      for (int u = 0; u < G::kPerThread; u++) {
        const int q = threadIdx.x + u * kThreads;
        if (q < G::kChunks) store_chunk<S, V, XK>(xs, q, regs[u]);
        else store_chunk<S, V, YK>(xs + G::kElems, q - G::kChunks, regs[u]);
      }
    };

    Block<T> blk;
    blk.clear();
    fetch(0);
    park(0);
    __syncthreads();
    for (int s = 0; s < steps; s++) {
      if (s + 1 < steps) fetch((s + 1) * kStep);  // in flight under this step's MFMAs
      const S* xs = lds + (s & 1) * 2 * G::kElems;
      if (live) blk.template step<XK, YK>(xs, xs + G::kElems, wm, wn, lane);
      if (s + 1 < steps) park((s + 1) & 1);  // (that buffer was last read before the last barrier)
      __syncthreads();
    }
    if (live)
      blk.for_each(lane, [&](int i, int j, float v) {
        const int row = m0 + wm * 32 + i, col = n0 + wn * 32 + j;
        if (row < M && col < N) ci[(size_t)row * N + col] = from_f32<T>(v);
      });
  }
}

// ================================================================================================
// Matrix multiply, packed body
// ================================================================================================
constexpr int kPackedElems = 1024;  // m n + n k + m k at most: eight fp32 items fit the slab
constexpr int kPackedGrid = 2048;
constexpr int kPackedSlab = 1024;   // items at most

__host__ __device__ inline int round_up(int v, int to) { return (v + to - 1) / to * to; }

template <typename T>
__device__ __forceinline__ void copy_in(T* dst, const T* __restrict__ src, int n, bool vec) {
  constexpr int V = 16 / (int)sizeof(T);
  int done = 0;
  if (vec) {
    const int nv = n / V;
    for (int q = threadIdx.x; q < nv; q += kThreads)
      reinterpret_cast<Pack<T, V>*>(dst)[q] = reinterpret_cast<const Pack<T, V>*>(src)[q];
    done = nv * V;
  }
  for (int e = done + threadIdx.x; e < n; e += kThreads) dst[e] = src[e];
}

// X(i, p) = x[i sxi + p sxp], Y(p, j) = y[p syp + j syj] inside an item; `slab` items a trip, a
// multiple of 8 (every slab then starts on a 16-byte boundary when the tensor does: vec)
template <typename T>
__global__ __launch_bounds__(kThreads) void mm_packed_kernel(size_t batch, int M, int N, int K,
                                                             int slab, const T* __restrict__ x,
                                                             const T* __restrict__ y,
                                                             T* __restrict__ c, int sxi, int sxp,
                                                             int syp, int syj, bool vec) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ uint4 raw[kLdsBytes / 16];
  const int szx = M * K, szy = K * N, szc = M * N;
  T* xs = reinterpret_cast<T*>(raw);
  T* ys = xs + round_up(slab * szx, V);
  const size_t slabs = (batch + slab - 1) / slab;
  for (size_t sl = blockIdx.x; sl < slabs; sl += gridDim.x) {
    const size_t b0 = sl * (size_t)slab;
    const int cnt = (int)(batch - b0 < (size_t)slab ? batch - b0 : (size_t)slab);
    copy_in(xs, x + b0 * szx, cnt * szx, vec);
    copy_in(ys, y + b0 * szy, cnt * szy, vec);
    __syncthreads();
    T* co = c + b0 * szc;
    for (int o = threadIdx.x; o < cnt * szc; o += kThreads) {
      const int it = o / szc, r = o - it * szc, i = r / N, j = r - i * N;
      const T* xa = xs + it * szx + i * sxi;
      const T* ya = ys + it * szy + j * syj;
      float acc = 0.f;
      for (int p = 0; p < K; p++) acc = fmaf(to_f32<T>(xa[p * sxp]), to_f32<T>(ya[p * syp]), acc);
      co[o] = from_f32<T>(acc);
    }
    __syncthreads();
  }
}

// ---- host ----------------------------------------------------------------------------------------
// the one dispatch rule: an item whose three matrices together hold at most kPackedElems elements
// is packed, everything else is tiled
bool packed_shape(int m, int n, int k) { return m * n + n * k + m * k <= kPackedElems; }

int mm_check(size_t batch, int m, int n, int k, int dtype) {
  HCTR_REQUIRE(m >= 1 && m <= kMmDim, "matmul: m 1 .. 4096");
  HCTR_REQUIRE(n >= 1 && n <= kMmDim, "matmul: inner dimension n 1 .. 4096");
  HCTR_REQUIRE(k >= 1 && k <= kMmDim, "matmul: k 1 .. 4096");
  size_t most = (size_t)m * n;
  if ((size_t)n * k > most) most = (size_t)n * k;
  if ((size_t)m * k > most) most = (size_t)m * k;
  HCTR_REQUIRE(batch <= kMaxElems / most, "matmul: batch * m * n, batch * n * k, batch * m * k < 2^31");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "matmul: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}

// C [batch][M][N] = X . Y; xk: X kept [M][K] (else [K][M]); yk: Y kept [N][K] (else [K][N])
template <typename T, bool XK, bool YK>
void product(size_t batch, int M, int N, int K, const void* x, const void* y, void* c, bool packed,
             hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  if (packed) {
    int slab = (kLdsBytes / (int)sizeof(T) - V) / (M * K + K * N) / 8 * 8;
    if (slab > kPackedSlab) slab = kPackedSlab;
    // (a small batch is spread over the grid rather than packed into a few full slabs)
    const size_t spread = ceil_div<size_t>(ceil_div<size_t>(batch, (size_t)kPackedGrid), 8) * 8;
    if ((size_t)slab > spread) slab = (int)spread;
    hipLaunchKernelGGL(mm_packed_kernel<T>,
                       dim3(grid_for(ceil_div<size_t>(batch, (size_t)slab), 1, kPackedGrid)),
                       dim3(kThreads), 0, s, batch, M, N, K, slab, (const T*)x, (const T*)y, (T*)c,
                       XK ? K : 1, XK ? 1 : M, YK ? 1 : N, YK ? K : 1, aligned16(x, y));
  } else {
    const size_t tiles = batch * (size_t)ceil_div(M, kTile) * (size_t)ceil_div(N, kTile);
    hipLaunchKernelGGL((mm_tile_kernel<T, XK, YK>), dim3(grid_for(tiles, 1, kTileGrid)),
                       dim3(kThreads), 0, s, batch, M, N, K, (const T*)x, (const T*)y, (T*)c,
                       (XK ? K : M) % V == 0 && aligned16(x), (YK ? K : N) % V == 0 && aligned16(y));
  }
}

int mm_fwd(size_t batch, int m, int n, int k, const void* a, const void* b, void* c, int dtype,
           hctr_stream_t stream) {
  HCTR_TRY(mm_check(batch, m, n, k, dtype));
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(a && b && c, "null pointer");
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    product<T, true, false>(batch, m, k, n, a, b, c, packed_shape(m, n, k), as_stream(stream));
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int mm_bwd(size_t batch, int m, int n, int k, const void* a, const void* b, const void* dc, void* da,
           void* db, int dtype, hctr_stream_t stream) {
  HCTR_TRY(mm_check(batch, m, n, k, dtype));
  if (batch == 0 || !(da || db)) return HCTR_OK;
  HCTR_REQUIRE(dc && (!da || b) && (!db || a), "null pointer");
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    const bool packed = packed_shape(m, n, k);
    if (da) product<T, true, true>(batch, m, n, k, dc, b, da, packed, as_stream(stream));
    if (db) product<T, false, false>(batch, n, k, m, a, dc, db, packed, as_stream(stream));
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// ================================================================================================
// Reduce mean
// ================================================================================================
constexpr int kReduceGrid = 1024;
constexpr int kMaxSlabs = 64;       // threads that share one column chunk
constexpr int kSlabRows = 16;       // rows a slab at least
constexpr size_t kBusyThreads = 65536;

// inner == 1: a group of G lanes per output
template <typename T, int G>
__global__ __launch_bounds__(kThreads) void rm_row_kernel(size_t outer, int len,
                                                          const T* __restrict__ x,
                                                          T* __restrict__ y) {
  constexpr int kRows = kThreads / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  for (size_t base = (size_t)blockIdx.x * kRows; base < outer; base += (size_t)gridDim.x * kRows) {
    // (a group past the last output reads the trip's first row again: the shuffles stay uniform)
    const bool live = base + grp < outer;
    const size_t row = live ? base + grp : base;
    const T* xr = x + row * (size_t)len;
    float s = 0.f;
    for (int l = lane; l < len; l += G) s += to_f32<T>(xr[l]);
    s = group_reduce_sum<G>(s);
    if (live && lane == 0) y[row] = from_f32<T>(s / (float)len);
  }
}

// inner > 1: a thread per 16-byte chunk of columns and row slab; ns slabs (a power of two) share a
// chunk and meet in LDS, added in slab order
template <typename T>
__global__ __launch_bounds__(kThreads) void rm_col_kernel(size_t outer, int len, int inner, int ns,
                                                          const T* __restrict__ x,
                                                          T* __restrict__ y, bool vec) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ float part[kThreads * V];  // [slab][chunk of the trip][V]
  const int ipw = kThreads / ns, slab = threadIdx.x / ipw, loc = threadIdx.x % ipw;
  const int chunks = (inner + V - 1) / V;
  const size_t items = outer * (size_t)chunks;
  const int per = (len + ns - 1) / ns, l0 = slab * per, l1 = l0 + per < len ? l0 + per : len;
  for (size_t base = (size_t)blockIdx.x * ipw; base < items; base += (size_t)gridDim.x * ipw) {
    const size_t it = base + loc;
    const bool live = it < items;
    const size_t o = it / (size_t)chunks;
    const int c0 = (int)(it % (size_t)chunks) * V;
    float s[V];
#pragma unroll
    for (int e = 0; e < V; e++) s[e] = 0.f;
    if (live) {
      const T* xp = x + o * (size_t)len * inner + c0;
      for (int l = l0; l < l1; l++) {
        if (vec) {
          const Pack<T, V> p = *reinterpret_cast<const Pack<T, V>*>(xp + (size_t)l * inner);
#pragma unroll
          for (int e = 0; e < V; e++) s[e] += to_f32<T>(p.e[e]);
        } else {
#pragma unroll
          for (int e = 0; e < V; e++)
            if (c0 + e < inner) s[e] += to_f32<T>(xp[(size_t)l * inner + e]);
        }
      }
    }
    if (ns > 1) {  // (uniform over the workgroup, as is the trip count)
#pragma unroll
      for (int e = 0; e < V; e++) part[threadIdx.x * V + e] = s[e];
      __syncthreads();
      if (slab == 0)
        for (int k = 1; k < ns; k++)
#pragma unroll
          for (int e = 0; e < V; e++) s[e] += part[(k * ipw + loc) * V + e];
      __syncthreads();
    }
    if (live && slab == 0) {
      T* yp = y + o * (size_t)inner + c0;
      if (vec) {
        Pack<T, V> p;
#pragma unroll
        for (int e = 0; e < V; e++) p.e[e] = from_f32<T>(s[e] / (float)len);
        *reinterpret_cast<Pack<T, V>*>(yp) = p;
      } else {
#pragma unroll
        for (int e = 0; e < V; e++)
          if (c0 + e < inner) yp[e] = from_f32<T>(s[e] / (float)len);
      }
    }
  }
}

// dx [outer][len][inner] = dy [outer][inner] / len; a thread per 16-byte chunk (VEC: inner is a
// multiple of V, so a chunk stays inside a row) or per element
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void rm_bwd_kernel(size_t n, int len, int inner,
                                                          const T* __restrict__ dy,
                                                          T* __restrict__ dx) {
  constexpr int W = VEC ? 16 / (int)sizeof(T) : 1;
  const size_t per_outer = (size_t)len * inner;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < n; q += (size_t)gridDim.x * kThreads) {
    const size_t e0 = q * W, o = e0 / per_outer, i = e0 % (size_t)inner;
    Pack<T, W> p = *reinterpret_cast<const Pack<T, W>*>(dy + o * inner + i);
#pragma unroll
    for (int e = 0; e < W; e++) p.e[e] = from_f32<T>(to_f32<T>(p.e[e]) / (float)len);
    *reinterpret_cast<Pack<T, W>*>(dx + e0) = p;
  }
}

int rm_check(size_t outer, size_t len, size_t inner, int dtype) {
  HCTR_REQUIRE(len >= 1, "reduce_mean: len >= 1 (the reduced axis is not empty)");
  HCTR_REQUIRE(len <= kMaxElems && inner <= kMaxElems / len &&
                   (inner == 0 || outer <= kMaxElems / (len * inner)),
               "reduce_mean: outer * len * inner < 2^31");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "reduce_mean: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}

int rm_fwd(size_t outer, size_t len, size_t inner, const void* x, void* y, int dtype,
           hctr_stream_t stream) {
  HCTR_TRY(rm_check(outer, len, inner, dtype));
  if (outer == 0 || inner == 0) return HCTR_OK;
  HCTR_REQUIRE(x && y, "null pointer");
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    constexpr int V = 16 / (int)sizeof(T);
    if (inner == 1) {
      auto launch = [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL((rm_row_kernel<T, G>), dim3(grid_for(outer, kThreads / G, kReduceGrid)),
                           dim3(kThreads), 0, s, outer, (int)len, (const T*)x, (T*)y);
      };
      if (len <= 8) launch(std::integral_constant<int, 1>{});
      else if (len <= 64) launch(std::integral_constant<int, 4>{});
      else if (len <= 512) launch(std::integral_constant<int, 16>{});
      else launch(std::integral_constant<int, 64>{});
    } else {
      const size_t items = outer * ceil_div<size_t>(inner, V);
      int ns = 1;  // a function of the shape and the element type alone
      while (ns < kMaxSlabs && items * ns < kBusyThreads && len >= (size_t)(2 * ns * kSlabRows)) ns *= 2;
      hipLaunchKernelGGL(rm_col_kernel<T>, dim3(grid_for(items, kThreads / ns, kReduceGrid)),
                         dim3(kThreads), 0, s, outer, (int)len, (int)inner, ns, (const T*)x, (T*)y,
                         inner % V == 0 && aligned16(x, y));
    }
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int rm_bwd(size_t outer, size_t len, size_t inner, const void* dy, void* dx, int dtype,
           hctr_stream_t stream) {
  HCTR_TRY(rm_check(outer, len, inner, dtype));
  if (outer == 0 || inner == 0) return HCTR_OK;
  HCTR_REQUIRE(dy && dx, "null pointer");
  hipStream_t s = as_stream(stream);
  const size_t total = outer * len * inner;
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    constexpr int V = 16 / (int)sizeof(T);
    with_bool(inner % V == 0 && aligned16(dy, dx), [&](auto vec) {
      const size_t n = total / (decltype(vec)::value ? V : 1);
      hipLaunchKernelGGL((rm_bwd_kernel<T, decltype(vec)::value>), dim3(grid_for(n, kThreads)),
                         dim3(kThreads), 0, s, n, (int)len, (int)inner, (const T*)dy, (T*)dx);
    });
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// ================================================================================================
// Fused reshape + concat
// ================================================================================================
constexpr int kFrcInputs = 8;
constexpr int kFrcGrid = 2048;

struct FrcTable {  // by value in the kernel arguments
  void* p[kFrcInputs];
  int w[kFrcInputs];    // width of input k
  int off[kFrcInputs];  // its first column in the output row
};

// S: the bits of an element; VEC: 16 bytes a lane (every width a multiple of V, every pointer
// aligned); BWD: the copy runs from item / ad into the inputs' gradients.  G lanes a row
template <typename S, bool VEC, bool BWD>
__global__ __launch_bounds__(kThreads) void frc_kernel(FrcTable tab, int num, size_t rows, int slots,
                                                       int W, int G, S* __restrict__ item,
                                                       S* __restrict__ ad) {
  constexpr int V = VEC ? 16 / (int)sizeof(S) : 1;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G, per_trip = kThreads / G;
  const int nc = W / V;
  for (size_t base = (size_t)blockIdx.x * per_trip; base < rows; base += (size_t)gridDim.x * per_trip) {
    const size_t row = base + grp;
    if (row >= rows) continue;
    const size_t b = row / (size_t)slots;
    const int slot = (int)(row % (size_t)slots);
    S* out = slot == slots - 1 ? ad + b * W : item + (b * (size_t)(slots - 1) + slot) * W;
    for (int c = lane; c < nc; c += G) {
      const int col = c * V;
      S* in = static_cast<S*>(tab.p[0]);
      int w = tab.w[0], off = 0;
#pragma unroll
      for (int k = 1; k < kFrcInputs; k++)  // (static indices: the table stays in scalar registers)
        if (k < num && col >= tab.off[k]) {
          in = static_cast<S*>(tab.p[k]);
          w = tab.w[k];
          off = tab.off[k];
        }
      Pack<S, V>* src = reinterpret_cast<Pack<S, V>*>(in + row * (size_t)w + (col - off));
      Pack<S, V>* dst = reinterpret_cast<Pack<S, V>*>(out + col);
      if (BWD) *src = *dst;
      else *dst = *src;
    }
  }
}

int frc_run(bool bwd, size_t batch, int slots, int num, void* const* inputs, const int* widths,
            void* item, void* ad, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(num >= 1 && num <= kFrcInputs, "fused_reshape_concat: num 1 .. 8 inputs");
  HCTR_REQUIRE(slots >= 1, "fused_reshape_concat: slots S >= 1");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "fused_reshape_concat: dtype (f32 / f16 / bf16)");
  HCTR_REQUIRE(batch <= kMaxElems / (size_t)slots, "fused_reshape_concat: rows = B * S, rows * W < 2^31");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(inputs && widths, "null pointer");
  const size_t rows = batch * (size_t)slots;
  FrcTable tab = {};
  size_t W = 0;
  const int size = dtype == HCTR_EMB_F32 ? 4 : 2, V = 16 / size;
  bool vec = aligned16(item, ad);
  for (int k = 0; k < num; k++) {
    HCTR_REQUIRE(widths[k] >= 1, "fused_reshape_concat: width >= 1");
    tab.p[k] = inputs[k];
    tab.w[k] = widths[k];
    tab.off[k] = (int)W;
    W += (size_t)widths[k];
    HCTR_REQUIRE(W <= kMaxElems / rows, "fused_reshape_concat: rows = B * S, rows * W < 2^31");
    vec = vec && widths[k] % V == 0 && aligned16(inputs[k]);
  }
  for (int k = 0; k < num; k++) HCTR_REQUIRE(inputs[k], "null pointer");
  HCTR_REQUIRE(ad && (item || slots == 1), "null pointer");
  const int nc = (int)W / (vec ? V : 1);
  int G = 1;
  while (G < 64 && G < nc) G *= 2;
  const int grid = grid_for(rows, kThreads / G, kFrcGrid);
  hipStream_t s = as_stream(stream);
  auto launch = [&](auto* t) {
    using S = std::remove_pointer_t<decltype(t)>;
    with_bool(vec, [&](auto v) {
      with_bool(bwd, [&](auto d) {
        hipLaunchKernelGGL((frc_kernel<S, decltype(v)::value, decltype(d)::value>), dim3(grid),
                           dim3(kThreads), 0, s, tab, num, rows, slots, (int)W, G, (S*)item, (S*)ad);
      });
    });
  };
  if (size == 4) launch((unsigned int*)nullptr);
  else launch((unsigned short*)nullptr);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace
}  // namespace seq
}  // namespace hctr

extern "C" {

int hctr_matmul_fwd(size_t batch, int m, int n, int k, const void* a, const void* b, void* c,
                    int dtype, hctr_stream_t stream) {
  return hctr::seq::mm_fwd(batch, m, n, k, a, b, c, dtype, stream);
}

int hctr_matmul_bwd(size_t batch, int m, int n, int k, const void* a, const void* b, const void* dc,
                    void* da, void* db, int dtype, hctr_stream_t stream) {
  return hctr::seq::mm_bwd(batch, m, n, k, a, b, dc, da, db, dtype, stream);
}

int hctr_reduce_mean_fwd(size_t outer, size_t len, size_t inner, const void* x, void* y, int dtype,
                         hctr_stream_t stream) {
  return hctr::seq::rm_fwd(outer, len, inner, x, y, dtype, stream);
}

int hctr_reduce_mean_bwd(size_t outer, size_t len, size_t inner, const void* dy, void* dx, int dtype,
                         hctr_stream_t stream) {
  return hctr::seq::rm_bwd(outer, len, inner, dy, dx, dtype, stream);
}

int hctr_fused_reshape_concat_fwd(size_t batch, int slots, int num, const void* const* inputs,
                                  const int* widths, void* item, void* ad, int dtype,
                                  hctr_stream_t stream) {
  return hctr::seq::frc_run(false, batch, slots, num, const_cast<void* const*>(inputs), widths, item,
                            ad, dtype, stream);
}

int hctr_fused_reshape_concat_bwd(size_t batch, int slots, int num, void* const* dinputs,
                                  const int* widths, const void* ditem, const void* dad, int dtype,
                                  hctr_stream_t stream) {
  return hctr::seq::frc_run(true, batch, slots, num, dinputs, widths, const_cast<void*>(ditem),
                            const_cast<void*>(dad), dtype, stream);
}

}  // extern "C"
