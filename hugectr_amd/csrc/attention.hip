// attention.hip -- multi-head attention (forward, backward) and the sequence mask:
// kernels, host dispatch, hctr_mha_fwd / hctr_mha_bwd / hctr_sequence_mask, and the *_len_* entries
// of both families, which take the two length vectors in the place of the mask and run the same
// kernel bodies (template parameter LEN: the 0 / 1 decision is formed in registers from the
// sample's two floats -- LenBounds below -- and no mask tensor is read).
//
// Two kernel families.  This file holds the first, for seq_from, seq_to <= 128 and size_per_head
// <= 64: a whole (sample, head) in one wavefront's LDS, described below.  attention_tiled.hip, taken
// in at the end, holds the second (hctr_mha_tiled_fwd / hctr_mha_tiled_bwd): blocks of 128 rows over
// streamed 16-bit tiles, any shape up to 4096 x 4096 x 128.  The entry points do not choose: each
// runs its own family and refuses what that family has no kernel for; the rule that picks is
// hugectr_amd/layers.py's (the first family wherever it fits, the second for everything else).
//
// MultiHeadAttentionLayer<T> + MaskedSoftmaxLayer<T> + SequenceMaskLayer<T> of the reference
// (R/HugeCTR/src/layers/multi_head_attention_layer.cu, masked_softmax_layer.cu,
// sequence_mask_layer.cu: four transposes, two strided-batched GEMMs, a softmax launch, two
// copies, three [B, H, m, n] tensors kept for the backward).  Here one wavefront owns one
// (sample, head):
//   * Q_h [m][d], K_h, V_h [n][d] (backward: dO_h too) are read once from the [B, seq, H d] layout
//     with 16-byte loads into LDS tiles of fp32 (a 16-bit value is exact in fp32); rows are padded
//     to 32 and columns to 16 with zeros, which are the MFMA's K padding; no transposed copy exists:
//     an operand whose k runs down a tile's rows is gathered from its column (col8);
//   * all products run on v_mfma_f32_32x32x16 (fp16 / bf16 operands, fp32 accumulate); an fp32
//     operand goes in as a (hi, lo) pair of bf16 -- three MFMAs, ~2^-16 relative, as interaction.hip
//     does -- so there is one kernel body per direction for the three element types;
//   * the scores of 32 query rows are produced TRANSPOSED (A = K rows, B = Q rows): lane (q, h)
//     then holds half of row q's scores in its accumulator registers, and scale, mask, max, sum and
//     the normalisation run on registers with one cross-lane exchange (lane ^ 32) per reduction;
//   * P goes back through a [32][n] fp32 LDS block as the A operand of P V; O_h is staged in LDS
//     and leaves as 16-byte stores into head h's columns of O.
// Between the steps everything stays fp32; a value is rounded to the element type only where it
// becomes an MFMA operand or an output (the reference rounds S and P to the type in HBM).
//
// Softmax: s = q.k / sqrt(d) - ((1 - mask) 10000 - r), p = exp(s - max s) / (sum + 1e-6), where r
// is the row's smallest penalty: a shift common to a row cancels in the softmax, so this is the
// reference's formula without the fp32 cancellation of (s - 10000) in a fully masked row.
//
// Backward: the forward saves NOTHING beyond its inputs.  P is recomputed from Q, K and the mask:
//   pass 1, per 32 query rows: S, P, dP = dO V^T, delta = rowsum(dP o P), dS = P o (dP - delta);
//           the rows' max, 1 / (sum + 1e-6), delta and r stay in LDS; dQ = dS K / sqrt(d) leaves;
//   pass 2, per 32 keys: over the query blocks the S and dP tiles are computed again, P and dS go
//           through LDS transposed, dV += P^T dO and dK += dS^T Q / sqrt(d) accumulate in registers
//           (two tiles each) and leave once.
// The second evaluation of S and dP (7 tile products instead of 5) is what keeps the accumulators
// at four tiles and the LDS at four input tiles and one block; one wavefront writes all of a
// head's gradients, no atomics.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace mha {  // (its own: a build that takes this file into interaction.hip's unit shares no name)
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kMaxSeq = 128;        // m, n: four 32-wide tiles -> four accumulators per row block
constexpr int kMaxHeadSize = 64;    // d: two 32-wide column tiles
constexpr int kSeqTiles = kMaxSeq / 32;
constexpr int kColTiles = kMaxHeadSize / 32;
constexpr int kTileLd = 36;         // row stride (floats) of pass 2's [32][32] P^T / dS^T tiles
constexpr float kMaskPenalty = 10000.f;
constexpr float kSoftmaxEps = 1e-6f;

// one (sample, head): the tiles' geometry and the LDS layout of both kernels (floats)
struct MhaShape {
  int heads, m, n, d;
  int mp, np;  // m, n rounded up to the 32 rows of an MFMA tile (rows past m / n stay zero)
  int dk;      // d rounded up to the MFMA's K of 16 (columns d .. dk stay zero)
  int n16;     // n rounded up to 16: the k range of a product over the keys
  int ld;      // row stride of the Q / K / V / dO tiles: +16 B against b128 bank conflicts
  int sld;     // row stride of the [32][np] P / dS block
  __host__ __device__ MhaShape(int heads_, int m_, int n_, int d_)
      : heads(heads_), m(m_), n(n_), d(d_), mp((m_ + 31) & ~31), np((n_ + 31) & ~31),
        dk((d_ + 15) & ~15), n16((n_ + 15) & ~15), ld(dk + 4), sld(np + 4) {}
  __host__ __device__ int row_stride() const { return heads * d; }  // elements between two rows
  // forward: Q [mp][ld], K, V [np][ld], P block [32][sld], staged O block [32][ld]
  __host__ __device__ int fwd_floats() const { return (mp + 2 * np) * ld + 32 * sld + 32 * ld; }
  // backward: Q, dO [mp][ld], K, V [np][ld], the dS block of pass 1 = the two tiles of pass 2,
  // four row statistics [mp]
  __host__ __device__ int bwd_block() const {
    return 32 * sld > 2 * 32 * kTileLd ? 32 * sld : 2 * 32 * kTileLd;
  }
  __host__ __device__ int bwd_floats() const { return 2 * (mp + np) * ld + bwd_block() + 4 * mp; }
};

// ---- MFMA operands ---------------------------------------------------------------------------------
// Op<T>::make(x): eight fp32 values as the operand fragment of element type T; Op<T>::mma: the
// product of two fragments added to a 32 x 32 accumulator
template <typename T>
struct Op;
template <>
struct Op<__half> {
  struct frag {
    f16x8 v;
  };
  __device__ __forceinline__ static frag make(const float (&x)[8]) {
    frag f;
#pragma unroll
    for (int e = 0; e < 8; e++) f.v[e] = (_Float16)x[e];
    return f;
  }
  __device__ __forceinline__ static f32x16 mma(const frag& a, const frag& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a.v, b.v, c, 0, 0, 0);
  }
};
template <>
struct Op<__hip_bfloat16> {
  struct frag {
    bf16x8 v;
  };
  __device__ __forceinline__ static frag make(const float (&x)[8]) {
    frag f;
#pragma unroll
    for (int e = 0; e < 8; e++) f.v[e] = (__bf16)x[e];
    return f;
  }
  __device__ __forceinline__ static f32x16 mma(const frag& a, const frag& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, c, 0, 0, 0);
  }
};
// fp32: x ~= hi + lo with |x - hi - lo| <= 2^-17 |x|; hi hi + hi lo + lo hi reproduces the fp32
// product to ~2^-16 relative (interaction.hip: split8)
template <>
struct Op<float> {
  struct frag {
    bf16x8 hi, lo;
  };
  __device__ __forceinline__ static frag make(const float (&x)[8]) {
    frag f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const __bf16 h = (__bf16)x[e];
      f.hi[e] = h;
      f.lo[e] = (__bf16)(x[e] - (float)h);
    }
    return f;
  }
  __device__ __forceinline__ static f32x16 mma(const frag& a, const frag& b, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, c, 0, 0, 0);
  }
};

// eight consecutive values of a row / eight values down a column of an LDS tile
__device__ __forceinline__ void row8(const float* t, int ld, int row, int k0, float (&x)[8]) {
  const f32x4 p = *reinterpret_cast<const f32x4*>(t + row * ld + k0);
  const f32x4 q = *reinterpret_cast<const f32x4*>(t + row * ld + k0 + 4);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    x[e] = p[e];
    x[4 + e] = q[e];
  }
}
__device__ __forceinline__ void col8(const float* t, int ld, int k0, int col, float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e++) x[e] = t[(k0 + e) * ld + col];
}

// C[i][j] = sum_k A[arow0 + i][k] B[brow0 + j][k], k < 16 ksteps: both operands by rows.
// Lane (r, h) = (lane & 31, lane >> 5) feeds row r, k = 16 t + 8 h .. + 7, and receives column
// j = r, rows i = tile_row(reg, h) in its 16 registers.
template <typename T>
__device__ __forceinline__ f32x16 tile_rr(const float* a, int lda, int arow0, const float* b,
                                          int ldb, int brow0, int ksteps, int lane) {
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ksteps; t++) {
    float x[8], y[8];
    row8(a, lda, arow0 + r, 16 * t + 8 * h, x);
    row8(b, ldb, brow0 + r, 16 * t + 8 * h, y);
    acc = Op<T>::mma(Op<T>::make(x), Op<T>::make(y), acc);
  }
  return acc;
}
// acc[i][j] += sum_k A[arow0 + i][k] B[bk0 + k][bcol]: B by columns (bcol = this lane's column of
// B, clamped by the caller to one that exists)
template <typename T>
__device__ __forceinline__ f32x16 tile_rc(f32x16 acc, const float* a, int lda, int arow0,
                                          const float* b, int ldb, int bk0, int bcol, int ksteps,
                                          int lane) {
  const int r = lane & 31, h = lane >> 5;
  for (int t = 0; t < ksteps; t++) {
    float x[8], y[8];
    row8(a, lda, arow0 + r, 16 * t + 8 * h, x);
    col8(b, ldb, bk0 + 16 * t + 8 * h, bcol, y);
    acc = Op<T>::mma(Op<T>::make(x), Op<T>::make(y), acc);
  }
  return acc;
}
// row of a 32 x 32 accumulator that register `reg` of a lane of half h holds
__device__ __forceinline__ int tile_row(int reg, int h) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * h;
}

// ---- global <-> LDS --------------------------------------------------------------------------------
template <typename T>
struct Chunk {  // 16 bytes of T
  static constexpr int N = 16 / sizeof(T);
  __device__ __forceinline__ static void to_f32(const u32x4& v, float (&f)[N]) {
    const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int i = 0; i < N; i++) f[i] = hctr::to_f32<T>(e[i]);
  }
  __device__ __forceinline__ static u32x4 from_f32(const float (&f)[N]) {
    u32x4 v;
    T* e = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int i = 0; i < N; i++) e[i] = hctr::from_f32<T>(f[i]);
    return v;
  }
};

// tile[row][0 .. d) <- g[row * stride + 0 .. d), rows < `rows`, 16 bytes per lane per load
template <typename T>
__device__ __forceinline__ void load_rows(float* tile, int ld, const T* __restrict__ g,
                                          size_t stride, int rows, int d, int lane) {
  constexpr int N = Chunk<T>::N;
  const int cpr = d / N;
  for (int i = lane; i < rows * cpr; i += 64) {
    const int row = i / cpr, c = (i % cpr) * N;
    float f[N];
    Chunk<T>::to_f32(*reinterpret_cast<const u32x4*>(g + row * stride + c), f);
#pragma unroll
    for (int e = 0; e < N; e += 4)
      *reinterpret_cast<f32x4*>(tile + row * ld + c + e) = (f32x4){f[e], f[e + 1], f[e + 2], f[e + 3]};
  }
}
// g[row * stride + 0 .. d) <- tile[row][0 .. d) rounded to T, rows < `rows`, 16-byte stores
template <typename T>
__device__ __forceinline__ void store_rows(T* __restrict__ g, size_t stride, const float* tile,
                                           int ld, int rows, int d, int lane) {
  constexpr int N = Chunk<T>::N;
  const int cpr = d / N;
  for (int i = lane; i < rows * cpr; i += 64) {
    const int row = i / cpr, c = (i % cpr) * N;
    float f[N];
#pragma unroll
    for (int e = 0; e < N; e++) f[e] = tile[row * ld + c + e];
    *reinterpret_cast<u32x4*>(g + row * stride + c) = Chunk<T>::from_f32(f);
  }
}
// a 32-row accumulator whose lanes hold columns (j = column c0 + r, registers = rows) straight to
// g[(row0 + i) * stride + c], scaled: rows < rows_end, columns < d
template <typename T>
__device__ __forceinline__ void store_acc(T* __restrict__ g, size_t stride, const f32x16& acc,
                                          float scale, int row0, int rows_end, int c, int d,
                                          int lane) {
  const int h = lane >> 5;
  if (c >= d) return;
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    const int row = row0 + tile_row(reg, h);
    if (row < rows_end) g[row * stride + c] = hctr::from_f32<T>(acc[reg] * scale);
  }
}

// ---- the softmax of 32 query rows, on the accumulators ---------------------------------------------
// the penalty of (query row, key): (1 - mask) 10000; no mask, or a row past m: 0
template <typename T>
__device__ __forceinline__ float penalty(const T* mrow, int key) {
  return mrow ? (1.f - hctr::to_f32<T>(mrow[key])) * kMaskPenalty : 0.f;
}
// the row's smallest penalty over its n keys (the two lanes of a row hold half of the keys each)
template <typename T>
__device__ __forceinline__ float row_min_penalty(const T* mrow, int nt, int n, int h) {
  float pmin = INFINITY;
#pragma unroll
  for (int jt = 0; jt < kSeqTiles; jt++) {
    if (jt < nt) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int key = jt * 32 + tile_row(reg, h);
        if (key < n) pmin = fminf(pmin, penalty(mrow, key));
      }
    }
  }
  return pmin;
}
// acc[jt][reg]: raw q.k of (this lane's query row, key jt * 32 + tile_row(reg, h)) -> the logit
// s = q.k * scale - (penalty - pmin), -inf for a key past n
template <typename T>
__device__ __forceinline__ float logit(float qk, float scale, const T* mrow, float pmin, int key,
                                       int n) {
  if (key >= n) return -INFINITY;
  return qk * scale - (penalty(mrow, key) - pmin);
}
// ---- the mask as two lengths (the *_len_* entries) ---------------------------------------------------
// valid(b, i, j) = (float)i < len_from[b] && (float)j < len_to[b], sequence_mask_kernel's comparison,
// formed from the two floats of a sample; no mask tensor is read.
// how many of the integers 0 .. hi - 1 lie, as floats, below len: clamp(ceil(len), 0, hi), 0 for NaN
__device__ __forceinline__ int count_below(float len, int hi) {
  return len > 0.f ? (len < (float)hi ? (int)ceilf(len) : hi) : 0;
}
// one sample: keys 0 .. nv - 1 are valid; rows from first_plain on (and every row when no key is
// valid) are plain: their penalty is common to the row and cancels, so they attend to all n keys.
// Every other row treats a key >= nv like a key >= n: logit -inf, weight exactly 0
struct LenBounds {
  int nv, first_plain, n;
  __device__ __forceinline__ LenBounds(const float* len_from, const float* len_to, size_t b, int m,
                                       int n_)
      : nv(count_below(len_to[b], n_)), first_plain(nv == 0 ? 0 : count_below(len_from[b], m)),
        n(n_) {}
  // where the keys of `row` end (>= 1)
  __device__ __forceinline__ int key_end(int row) const { return row < first_plain ? nv : n; }
  // the largest key_end among the rows below row_end (<= m)
  __device__ __forceinline__ int key_end_upto(int row_end) const {
    return row_end > first_plain ? n : nv;
  }
};

// acc: raw q.k -> P; returns the row's max and 1 / (sum + eps) through rmax / rinv
template <typename T>
__device__ __forceinline__ void softmax_rows(f32x16 (&acc)[kSeqTiles], int nt, int n, float scale,
                                             const T* mrow, float pmin, int h, float& rmax,
                                             float& rinv) {
  float mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < kSeqTiles; jt++) {
    if (jt < nt) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const float s = logit(acc[jt][reg], scale, mrow, pmin, jt * 32 + tile_row(reg, h), n);
        acc[jt][reg] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int jt = 0; jt < kSeqTiles; jt++) {
    if (jt < nt) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const float e = __expf(acc[jt][reg] - mx);
        acc[jt][reg] = e;
        sum += e;
      }
    }
  }
  sum += __shfl_xor(sum, 32);
  rmax = mx;
  rinv = 1.f / (sum + kSoftmaxEps);
#pragma unroll
  for (int jt = 0; jt < kSeqTiles; jt++) {
    if (jt < nt) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) acc[jt][reg] *= rinv;
    }
  }
}
// block[q][key] <- acc (lane = query row q, registers = keys): four consecutive keys per store
__device__ __forceinline__ void put_block(float* block, int sld, const f32x16 (&acc)[kSeqTiles],
                                          int nt, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int jt = 0; jt < kSeqTiles; jt++) {
    if (jt < nt) {
#pragma unroll
      for (int g = 0; g < 4; g++)
        *reinterpret_cast<f32x4*>(block + r * sld + jt * 32 + 8 * g + 4 * h) =
            (f32x4){acc[jt][4 * g], acc[jt][4 * g + 1], acc[jt][4 * g + 2], acc[jt][4 * g + 3]};
    }
  }
}

// where head hd of sample b starts in a [B, seq, H d] tensor
__device__ __forceinline__ size_t head_offset(const MhaShape& s, size_t b, int hd, int seq) {
  return (b * seq * s.heads + hd) * (size_t)s.d;
}

// ================================================================================================
// Forward
// ================================================================================================
// LEN: the mask comes from len_from / len_to (fp32 [B]) and `dense` is not read; otherwise from
// `dense` (or no mask) and the lengths are not read
template <typename T, bool LEN>
__global__ void __launch_bounds__(64)
    mha_fwd_kernel(size_t n_heads_total, MhaShape s, const T* __restrict__ q,
                   const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dense,
                   const float* __restrict__ len_from, const float* __restrict__ len_to,
                   T* __restrict__ out, float scale) {
  const T* mask = LEN ? nullptr : dense;
  HCTR_DYN_LDS16(float, smem);
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  float* qt = smem;
  float* kt = qt + s.mp * s.ld;
  float* vt = kt + s.np * s.ld;
  float* pb = vt + s.np * s.ld;  // [32][sld]
  float* ob = pb + 32 * s.sld;   // [32][ld]
  for (int i = lane; i < s.fwd_floats(); i += 64) smem[i] = 0.f;  // the zero padding, once
  __syncthreads();
  const int nt = s.np / 32, ksd = s.dk / 16, ksn = s.n16 / 16;
  const size_t stride = s.row_stride();

  for (size_t p = blockIdx.x; p < n_heads_total; p += gridDim.x) {
    const size_t b = p / s.heads;
    const int hd = (int)(p % s.heads);
    int nv = s.n, first_plain = s.m;  // (no lengths: every row's keys end at n)
    if (LEN) {
      const LenBounds lb(len_from, len_to, b, s.m, s.n);
      nv = lb.nv, first_plain = lb.first_plain;
    }
    load_rows(qt, s.ld, q + head_offset(s, b, hd, s.m), stride, s.m, s.d, lane);
    load_rows(kt, s.ld, k + head_offset(s, b, hd, s.n), stride, s.n, s.d, lane);
    load_rows(vt, s.ld, v + head_offset(s, b, hd, s.n), stride, s.n, s.d, lane);
    __syncthreads();
    for (int q0 = 0; q0 < s.mp; q0 += 32) {
      const T* mrow = (mask && q0 + r < s.m) ? mask + (b * s.m + q0 + r) * (size_t)s.n : nullptr;
      f32x16 acc[kSeqTiles];
#pragma unroll
      for (int jt = 0; jt < kSeqTiles; jt++)
        if (jt < nt) acc[jt] = tile_rr<T>(kt, s.ld, jt * 32, qt, s.ld, q0, ksd, lane);
      float pmin = mask ? row_min_penalty(mrow, nt, s.n, h) : 0.f;
      if (mask) pmin = fminf(pmin, __shfl_xor(pmin, 32));
      float rmax, rinv;
      // lengths: the minimum is known to be 0; a key past the row's end is a key past n
      softmax_rows(acc, nt, LEN && q0 + r < first_plain ? nv : s.n, scale, mrow, pmin, h, rmax,
                   rinv);
      put_block(pb, s.sld, acc, nt, lane);
      __syncthreads();
      // O block = P V: lane = column c of O_h, registers = query rows
#pragma unroll
      for (int ct = 0; ct < kColTiles; ct++) {
        if (ct * 32 < s.d) {
          const int c = ct * 32 + r;
          f32x16 o = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          o = tile_rc<T>(o, pb, s.sld, 0, vt, s.ld, 0, c < s.d ? c : 0, ksn, lane);
          if (c < s.d) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) ob[tile_row(reg, h) * s.ld + c] = o[reg];
          }
        }
      }
      __syncthreads();
      const int rows = s.m - q0 < 32 ? s.m - q0 : 32;
      store_rows(out + head_offset(s, b, hd, s.m) + q0 * stride, stride, ob, s.ld, rows, s.d, lane);
      __syncthreads();
    }
  }
}

// ================================================================================================
// Backward
// ================================================================================================
template <typename T, bool LEN>
__global__ void __launch_bounds__(64)
    mha_bwd_kernel(size_t n_heads_total, MhaShape s, const T* __restrict__ q,
                   const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dense,
                   const float* __restrict__ len_from, const float* __restrict__ len_to,
                   const T* __restrict__ top, T* __restrict__ dq, T* __restrict__ dk,
                   T* __restrict__ dv, float scale) {
  const T* mask = LEN ? nullptr : dense;
  HCTR_DYN_LDS16(float, smem);
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  float* qt = smem;
  float* gt = qt + s.mp * s.ld;  // dO
  float* kt = gt + s.mp * s.ld;
  float* vt = kt + s.np * s.ld;
  float* blk = vt + s.np * s.ld;     // pass 1: dS [32][sld]; pass 2: P^T, dS^T [32][kTileLd] each
  float* st = blk + s.bwd_block();   // rows' max, 1 / (sum + eps), delta, smallest penalty: [4][mp]
  for (int i = lane; i < s.bwd_floats(); i += 64) smem[i] = 0.f;
  __syncthreads();
  const int nt = s.np / 32, ksd = s.dk / 16, ksn = s.n16 / 16;
  const size_t stride = s.row_stride();

  for (size_t p = blockIdx.x; p < n_heads_total; p += gridDim.x) {
    const size_t b = p / s.heads;
    const int hd = (int)(p % s.heads);
    const size_t off_m = head_offset(s, b, hd, s.m), off_n = head_offset(s, b, hd, s.n);
    int nv = s.n, first_plain = s.m;
    if (LEN) {
      const LenBounds lb(len_from, len_to, b, s.m, s.n);
      nv = lb.nv, first_plain = lb.first_plain;
    }
    load_rows(qt, s.ld, q + off_m, stride, s.m, s.d, lane);
    load_rows(gt, s.ld, top + off_m, stride, s.m, s.d, lane);
    load_rows(kt, s.ld, k + off_n, stride, s.n, s.d, lane);
    load_rows(vt, s.ld, v + off_n, stride, s.n, s.d, lane);
    __syncthreads();

    // ---- pass 1: row statistics and dQ, 32 query rows at a time ----------------------------------
    for (int q0 = 0; q0 < s.mp; q0 += 32) {
      const T* mrow = (mask && q0 + r < s.m) ? mask + (b * s.m + q0 + r) * (size_t)s.n : nullptr;
      f32x16 acc[kSeqTiles];
#pragma unroll
      for (int jt = 0; jt < kSeqTiles; jt++)
        if (jt < nt) acc[jt] = tile_rr<T>(kt, s.ld, jt * 32, qt, s.ld, q0, ksd, lane);
      float pmin = mask ? row_min_penalty(mrow, nt, s.n, h) : 0.f;
      if (mask) pmin = fminf(pmin, __shfl_xor(pmin, 32));
      float rmax, rinv;
      // lengths: the minimum is known to be 0; a key past the row's end is a key past n
      softmax_rows(acc, nt, LEN && q0 + r < first_plain ? nv : s.n, scale, mrow, pmin, h, rmax,
                   rinv);
      // dP = dO V^T in the same layout, delta = rowsum(dP o P), acc <- dS = P o (dP - delta)
      f32x16 dp[kSeqTiles];
      float delta = 0.f;
#pragma unroll
      for (int jt = 0; jt < kSeqTiles; jt++) {
        if (jt < nt) {
          dp[jt] = tile_rr<T>(vt, s.ld, jt * 32, gt, s.ld, q0, ksd, lane);
#pragma unroll
          for (int reg = 0; reg < 16; reg++) delta += dp[jt][reg] * acc[jt][reg];
        }
      }
      delta += __shfl_xor(delta, 32);
#pragma unroll
      for (int jt = 0; jt < kSeqTiles; jt++) {
        if (jt < nt) {
#pragma unroll
          for (int reg = 0; reg < 16; reg++) acc[jt][reg] *= dp[jt][reg] - delta;
        }
      }
      if (h == 0) {
        st[q0 + r] = rmax;
        st[s.mp + q0 + r] = rinv;
        st[2 * s.mp + q0 + r] = delta;
        st[3 * s.mp + q0 + r] = pmin;
      }
      put_block(blk, s.sld, acc, nt, lane);
      __syncthreads();
      // dQ block = dS K * scale: lane = column c, registers = query rows
#pragma unroll
      for (int ct = 0; ct < kColTiles; ct++) {
        if (ct * 32 < s.d) {
          const int c = ct * 32 + r;
          f32x16 g = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          g = tile_rc<T>(g, blk, s.sld, 0, kt, s.ld, 0, c < s.d ? c : 0, ksn, lane);
          store_acc(dq + off_m, stride, g, scale, q0, s.m, c, s.d, lane);
        }
      }
      __syncthreads();
    }

    // ---- pass 2: dV and dK, 32 keys at a time ----------------------------------------------------
    float* ptt = blk;                   // P^T  [key][query]
    float* dst = blk + 32 * kTileLd;    // dS^T [key][query]
    for (int k0 = 0; k0 < s.np; k0 += 32) {
      f32x16 gv[kColTiles], gk[kColTiles];
#pragma unroll
      for (int ct = 0; ct < kColTiles; ct++) {
        gv[ct] = (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        gk[ct] = gv[ct];
      }
      for (int q0 = 0; q0 < s.mp; q0 += 32) {
        const int qi = q0 + r;
        const T* mrow = (mask && qi < s.m) ? mask + (b * s.m + qi) * (size_t)s.n : nullptr;
        const float rmax = st[qi], rinv = st[s.mp + qi], delta = st[2 * s.mp + qi],
                    pmin = st[3 * s.mp + qi];
        const int kend = LEN && qi < first_plain ? nv : s.n;
        const f32x16 sc = tile_rr<T>(kt, s.ld, k0, qt, s.ld, q0, ksd, lane);
        const f32x16 dp = tile_rr<T>(vt, s.ld, k0, gt, s.ld, q0, ksd, lane);
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int kl = tile_row(reg, h);
          const float pr = __expf(logit(sc[reg], scale, mrow, pmin, k0 + kl, kend) - rmax) * rinv;
          ptt[kl * kTileLd + r] = pr;
          dst[kl * kTileLd + r] = pr * (dp[reg] - delta);
        }
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < kColTiles; ct++) {
          if (ct * 32 < s.d) {
            const int c = ct * 32 + r < s.d ? ct * 32 + r : 0;
            gv[ct] = tile_rc<T>(gv[ct], ptt, kTileLd, 0, gt, s.ld, q0, c, 2, lane);
            gk[ct] = tile_rc<T>(gk[ct], dst, kTileLd, 0, qt, s.ld, q0, c, 2, lane);
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int ct = 0; ct < kColTiles; ct++) {
        if (ct * 32 < s.d) {
          store_acc(dv + off_n, stride, gv[ct], 1.f, k0, s.n, ct * 32 + r, s.d, lane);
          store_acc(dk + off_n, stride, gk[ct], scale, k0, s.n, ct * 32 + r, s.d, lane);
        }
      }
    }
    __syncthreads();  // the next head's loads overwrite the tiles
  }
}

// ================================================================================================
// Sequence mask: mask[b][0][i][j] = i < len_from[b] && j < len_to[b]
// ================================================================================================
template <typename T>
__global__ void __launch_bounds__(256)
    sequence_mask_kernel(size_t total, int max_from, int max_to, const T* __restrict__ len_from,
                         const T* __restrict__ len_to, T* __restrict__ mask) {
  constexpr int N = Chunk<T>::N;
  const size_t per = (size_t)max_from * max_to;
  const size_t chunks = (total + N - 1) / N;
  for (size_t ch = blockIdx.x * (size_t)blockDim.x + threadIdx.x; ch < chunks;
       ch += (size_t)gridDim.x * blockDim.x) {
    float f[N];
#pragma unroll
    for (int e = 0; e < N; e++) {
      const size_t idx = ch * N + e < total ? ch * N + e : total - 1;
      const size_t b = idx / per;
      const int i = (int)((idx % per) / max_to), j = (int)(idx % max_to);
      f[e] = ((float)i < hctr::to_f32<T>(len_from[b]) && (float)j < hctr::to_f32<T>(len_to[b]))
                 ? 1.f : 0.f;
    }
    if (ch * N + N <= total) {
      *reinterpret_cast<u32x4*>(mask + ch * N) = Chunk<T>::from_f32(f);
    } else {
      for (int e = 0; ch * N + e < total; e++) mask[ch * N + e] = hctr::from_f32<T>(f[e]);
    }
  }
}

// ================================================================================================
// Host side
// ================================================================================================
template <typename... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}
bool known_dtype(int dtype) {
  return dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16;
}
// what both attention entry points refuse, by name, before anything else
int mha_check(int heads, int seq_from, int seq_to, int size_per_head, int dtype) {
  HCTR_REQUIRE(heads >= 1, "mha: heads >= 1");
  HCTR_REQUIRE(seq_from >= 1 && seq_from <= kMaxSeq, "mha: seq_from 1 .. 128");
  HCTR_REQUIRE(seq_to >= 1 && seq_to <= kMaxSeq, "mha: seq_to 1 .. 128");
  HCTR_REQUIRE(size_per_head >= 8 && size_per_head % 8 == 0 && size_per_head <= kMaxHeadSize,
               "mha: size_per_head a multiple of 8, 8 .. 64");
  HCTR_REQUIRE(known_dtype(dtype), "mha: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}
// a workgroup (one wavefront) per (sample, head), strided over them; at most 8 resident per CU
int mha_grid(size_t n_heads_total) {
  const size_t gmax = 256 * 8;
  return (int)(n_heads_total < gmax ? n_heads_total : gmax);
}
// a kernel that is launched with more than 64 KB of dynamic LDS has to be told first
template <typename K>
int allow_dyn_lds(K kernel, size_t lds) {
  if (lds > 65536)
    HCTR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  return HCTR_OK;
}


// where a call's mask comes from: a dense tensor (NULL: no mask), or the two fp32 [B] length vectors
// of the *_len_* entries (no alignment asked of them: they are read a float at a time)
struct MaskSrc {
  const void* dense;
  const float *len_from, *len_to;
  bool lengths;
  bool complete() const { return !lengths || (len_from && len_to); }  // for a batch that is not empty
};
// f(std::true_type) for lengths, f(std::false_type) for a dense mask: the kernels' LEN
template <typename F>
int with_mask_src(const MaskSrc& ms, F&& f) {
  return ms.lengths ? f(std::true_type{}) : f(std::false_type{});
}

int fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head, const void* q,
        const void* k, const void* v, const MaskSrc& ms, void* out, int dtype,
        hctr_stream_t stream) {
  HCTR_TRY(mha_check(heads, seq_from, seq_to, size_per_head, dtype));
  HCTR_REQUIRE(aligned16(q, k, v, ms.dense, out), "mha: 16-byte aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(q && k && v && out && ms.complete(), "null pointer");
  const MhaShape sh(heads, seq_from, seq_to, size_per_head);
  const size_t lds = (size_t)sh.fwd_floats() * 4, total = batch * (size_t)heads;
  const float scale = 1.f / sqrtf((float)size_per_head);
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    return with_mask_src(ms, [&](auto len) -> int {
      auto kernel = mha_fwd_kernel<T, decltype(len)::value>;
      HCTR_TRY(allow_dyn_lds(kernel, lds));
      hipLaunchKernelGGL(kernel, dim3(mha_grid(total)), dim3(64), lds, s, total, sh, (const T*)q,
                         (const T*)k, (const T*)v, (const T*)ms.dense, ms.len_from, ms.len_to,
                         (T*)out, scale);
      return HCTR_OK;
    });
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head, const void* q,
        const void* k, const void* v, const MaskSrc& ms, const void* top_grad, void* dq, void* dk,
        void* dv, int dtype, hctr_stream_t stream) {
  HCTR_TRY(mha_check(heads, seq_from, seq_to, size_per_head, dtype));
  HCTR_REQUIRE(aligned16(q, k, v, ms.dense, top_grad, dq, dk, dv), "mha: 16-byte aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(q && k && v && top_grad && dq && dk && dv && ms.complete(), "null pointer");
  const MhaShape sh(heads, seq_from, seq_to, size_per_head);
  const size_t lds = (size_t)sh.bwd_floats() * 4, total = batch * (size_t)heads;
  const float scale = 1.f / sqrtf((float)size_per_head);
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    return with_mask_src(ms, [&](auto len) -> int {
      auto kernel = mha_bwd_kernel<T, decltype(len)::value>;
      HCTR_TRY(allow_dyn_lds(kernel, lds));
      hipLaunchKernelGGL(kernel, dim3(mha_grid(total)), dim3(64), lds, s, total, sh, (const T*)q,
                         (const T*)k, (const T*)v, (const T*)ms.dense, ms.len_from, ms.len_to,
                         (const T*)top_grad, (T*)dq, (T*)dk, (T*)dv, scale);
      return HCTR_OK;
    });
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int sequence_mask(size_t batch, int max_from, int max_to, const void* len_from,
                  const void* len_to, void* mask, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(max_from >= 1 && max_to >= 1, "sequence_mask: max_from, max_to >= 1");
  HCTR_REQUIRE(known_dtype(dtype), "sequence_mask: dtype (f32 / f16 / bf16)");
  HCTR_REQUIRE(aligned16(mask), "sequence_mask: 16-byte aligned mask");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(len_from && len_to && mask, "null pointer");
  const size_t total = batch * (size_t)max_from * (size_t)max_to;
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(sequence_mask_kernel<T>, dim3(grid_for(total / Chunk<T>::N + 1, 256)),
                       dim3(256), 0, s, total, max_from, max_to, (const T*)len_from,
                       (const T*)len_to, (T*)mask);
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// the second kernel family: blocks of rows over streamed 16-bit tiles, any shape up to 4096 x 128
#include "attention_tiled.hip"

}  // namespace
}  // namespace mha
}  // namespace hctr

extern "C" {

int hctr_mha_fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                 const void* q, const void* k, const void* v, const void* mask, void* out,
                 int dtype, hctr_stream_t stream) {
  return hctr::mha::fwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                        {mask, nullptr, nullptr, false}, out, dtype, stream);
}

int hctr_mha_len_fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                     const void* q, const void* k, const void* v, const float* len_from,
                     const float* len_to, void* out, int dtype, hctr_stream_t stream) {
  return hctr::mha::fwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                        {nullptr, len_from, len_to, true}, out, dtype, stream);
}

int hctr_mha_bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                 const void* q, const void* k, const void* v, const void* mask,
                 const void* top_grad, void* dq, void* dk, void* dv, int dtype,
                 hctr_stream_t stream) {
  return hctr::mha::bwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                        {mask, nullptr, nullptr, false}, top_grad, dq, dk, dv, dtype, stream);
}

int hctr_mha_len_bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                     const void* q, const void* k, const void* v, const float* len_from,
                     const float* len_to, const void* top_grad, void* dq, void* dk, void* dv,
                     int dtype, hctr_stream_t stream) {
  return hctr::mha::bwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                        {nullptr, len_from, len_to, true}, top_grad, dq, dk, dv, dtype, stream);
}

int hctr_mha_tiled_fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                       const void* q, const void* k, const void* v, const void* mask, void* out,
                       void* stats, int dtype, hctr_stream_t stream) {
  return hctr::mha::tiled_fwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                              {mask, nullptr, nullptr, false}, out, stats, dtype, stream);
}

int hctr_mha_tiled_len_fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                           const void* q, const void* k, const void* v, const float* len_from,
                           const float* len_to, void* out, void* stats, int dtype,
                           hctr_stream_t stream) {
  return hctr::mha::tiled_fwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                              {nullptr, len_from, len_to, true}, out, stats, dtype, stream);
}

int hctr_mha_tiled_bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                       const void* q, const void* k, const void* v, const void* mask,
                       const void* out, void* stats, const void* top_grad, void* dq, void* dk,
                       void* dv, int dtype, hctr_stream_t stream) {
  return hctr::mha::tiled_bwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                              {mask, nullptr, nullptr, false}, out, stats, top_grad, dq, dk, dv,
                              dtype, stream);
}

int hctr_mha_tiled_len_bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head,
                           const void* q, const void* k, const void* v, const float* len_from,
                           const float* len_to, const void* out, void* stats,
                           const void* top_grad, void* dq, void* dk, void* dv, int dtype,
                           hctr_stream_t stream) {
  return hctr::mha::tiled_bwd(batch, heads, seq_from, seq_to, size_per_head, q, k, v,
                              {nullptr, len_from, len_to, true}, out, stats, top_grad, dq, dk, dv,
                              dtype, stream);
}

int hctr_sequence_mask(size_t batch, int max_from, int max_to, const void* len_from,
                       const void* len_to, void* mask, int dtype, hctr_stream_t stream) {
  return hctr::mha::sequence_mask(batch, max_from, max_to, len_from, len_to, mask, dtype, stream);
}

}  // extern "C"
