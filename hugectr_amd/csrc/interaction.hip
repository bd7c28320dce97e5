// interaction.hip -- the DLRM dot interaction: kernels, host dispatch, hctr_interaction_* entries.
//
// InteractionLayer<T>::fprop/bprop: R/HugeCTR/src/layers/interaction_layer.cu:1046-1237
//   (generic path = concat kernel + cublasGemmStridedBatched X.X^T + gather kernel, three
//   round trips through HBM; fused WMMA path only for fp16).  Here one wavefront owns one sample:
//   the 27x128 tile is staged once in LDS, X.X^T runs on the fp32 MFMA (v_mfma_f32_32x32x2_f32,
//   exact fp32 fma chain), the strict lower triangle is gathered in LDS and the 480-float output
//   row leaves as 16-byte stores.  No `concat` / `mat` intermediates exist.
#include <type_traits>

#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGenericBlock = 256;
constexpr int kGenericWaves = kGenericBlock / 64;

// one sample: n_ins = n_emb + 1 rows (the MLP output, then the embeddings), their n_pairs products
// below the diagonal, output row = [mlp W | pairs | one zero pad column]
struct InterShape {
  int n_ins, n_pairs, out_len;
  InterShape(int n_emb, int width)
      : n_ins(n_emb + 1), n_pairs(n_ins * (n_ins - 1) / 2), out_len(width + n_pairs + 1) {}
};

// ================================================================================================
// Interaction forward, fp32, MFMA path: n_ins <= 32, W % 8 == 0, W <= 256
// LDS per wave: X tile [32][W+4] floats (rows >= n_ins stay zero) + out row staging
// ================================================================================================
template <int W>
struct InterCfg {
  static constexpr int LD = W + 4;             // row stride (floats): +16 B breaks b128 conflicts
  static constexpr int XT = 32 * LD;           // X tile floats
  static constexpr int GS = 36;  // G row stride (floats): 16 lanes of a ds_read_b128 -> 16 slots
  // forward: X [(n_ins + 1) rows][LD] + the staged output row; backward: X [32][LD], G [32][GS],
  // the (n, m) of every pair as 16-bit words
  static size_t fwd_lds(const InterShape& s) {
    return (size_t)((s.n_ins + 1) * LD + ((s.out_len + 3) & ~3)) * 4;
  }
  static size_t bwd_lds(const InterShape& s) {
    return (size_t)(XT + 32 * GS) * 4 + (size_t)((s.n_pairs + 7) & ~7) * 2;
  }
};

__device__ __forceinline__ int tri_index(int n, int m) { return n * (n - 1) / 2 + m; }  // n > m

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// fp32 -> (hi, lo) bf16 pair: x ~= hi + lo with |x - hi - lo| <= 2^-17 |x|.  Three bf16 MFMAs
// (hi*hi + hi*lo + lo*hi) then reproduce the fp32 product to ~2^-16 relative, at 3/16 of the
// fp32-MFMA cycle cost -- which is what lets the kernel run at the HBM roofline instead of the
// fp32 matrix-pipe limit (MI355X_MICROARCH: f32 MFMA = 1/16 of the bf16 rate).
__device__ __forceinline__ void split8(const float4& p, const float4& q, bf16x8& hi, bf16x8& lo) {
  const float v[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const __bf16 h = (__bf16)v[i];
    hi[i] = h;
    lo[i] = (__bf16)(v[i] - (float)h);
  }
}

// registers <- one sample's [n_ins][W] tile (row 0 = mlp, rows 1.. = emb), 16 B per lane per load.
// Lanes past the tile re-read element 0 so that `pre` stays in registers (no predicated array
// writes -> no scratch).
template <int W, int NPRE>
__device__ __forceinline__ void load_sample_tile(f32x4 (&pre)[NPRE], const float* __restrict__ mlp,
                                                 const float* __restrict__ emb, size_t b, int n_emb,
                                                 int n_vec, int lane) {
  constexpr int W4 = W / 4;
  const f32x4* m4 = reinterpret_cast<const f32x4*>(mlp + b * W);
  const f32x4* e4 = reinterpret_cast<const f32x4*>(emb + b * (size_t)n_emb * W) - W4;
#pragma unroll
  for (int q = 0; q < NPRE; q++) {
    int i = lane + 64 * q;
    i = i < n_vec ? i : 0;
    const f32x4* src = (i < W4) ? m4 : e4;
    pre[q] = src[i];
  }
}

// One wavefront (= one 64-thread workgroup) per sample, software-pipelined over samples:
//   registers <- global (sample i+1, 16-byte coalesced)   ||   MFMA on the LDS tile of sample i
// LDS per workgroup: X tile [(n_ins+1) rows][W+4] (last row = zeros for the padded MFMA rows) +
// the staged output row.
template <int W>
__global__ void __launch_bounds__(64, 2)
    interaction_fwd_mfma_kernel(size_t batch, int n_emb, const float* __restrict__ mlp,
                                const float* __restrict__ emb, float* __restrict__ out,
                                int out_len) {
  using C = InterCfg<W>;
  HCTR_DYN_LDS16(float, smem);
  const int lane = threadIdx.x;
  const int n_ins = n_emb + 1;
  float* xt = smem;
  float* stage = smem + (n_ins + 1) * C::LD;
  constexpr int W4 = W / 4;
  constexpr int NPRE = (32 * W4 + 63) / 64;  // float4 per lane for up to 32 rows
  const int n_vec = n_ins * W4;
  for (int i = lane; i < C::LD; i += 64) xt[n_ins * C::LD + i] = 0.f;  // the zero row

  const int r = lane & 31, h = lane >> 5;
  const int rr = r < n_ins ? r : n_ins;
  f32x4 pre[NPRE];
  size_t b = blockIdx.x;
  if (b < batch) load_sample_tile<W, NPRE>(pre, mlp, emb, b, n_emb, n_vec, lane);
  for (; b < batch; b += gridDim.x) {
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W4, c4 = i % W4;
        *reinterpret_cast<f32x4*>(xt + row * C::LD + c4 * 4) = pre[q];
      }
    }
    __syncthreads();
    const size_t nb = b + gridDim.x;
    if (nb < batch) load_sample_tile<W, NPRE>(pre, mlp, emb, nb, n_emb, n_vec, lane);

    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // lane (r,h) feeds X[r][h*W/2 + 8t .. +7] at k-step t; A == B fragment (product is X.X^T)
    const float* xr = xt + rr * C::LD + h * (W / 2);
#pragma unroll
    for (int t = 0; t < W / 16; t++) {
      const float4 p = *reinterpret_cast<const float4*>(xr + t * 8);
      const float4 q = *reinterpret_cast<const float4*>(xr + t * 8 + 4);
      bf16x8 hi, lo;
      split8(p, q, hi, lo);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi, hi, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi, lo, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo, hi, acc, 0, 0, 0);
    }
    // C layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (row > r && row < n_ins) stage[W + tri_index(row, r)] = acc[reg];
    }
    for (int i = lane; i < W; i += 64) stage[i] = xt[i];  // mlp passthrough
    if (lane == 0) stage[out_len - 1] = 0.f;              // zero pad column
    __syncthreads();
    float* o = out + b * (size_t)out_len;
    if ((out_len & 3) == 0) {
      for (int i = lane; i < out_len / 4; i += 64)
        reinterpret_cast<float4*>(o)[i] = reinterpret_cast<const float4*>(stage)[i];
    } else {
      for (int i = lane; i < out_len; i += 64) o[i] = stage[i];
    }
    __syncthreads();
  }
}

// ================================================================================================
// 16-bit (bf16 / fp16) interaction: same one-wavefront-per-sample pipeline, a single MFMA chain
// (inputs are already 16-bit), fp32 accumulate, 16-bit output.  This is the reference's mixed
// precision mode (InteractionLayer<__half>, interaction_layer.cu:47-756) with bf16 added.
// ================================================================================================
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool BF>
struct Mfma16;
template <>
struct Mfma16<true> : H16<true> {
  typedef bf16x8 vec8;
  // two fp32 values rounded to the type, a in the low half of the word.  Both Mfma16<BF>::pack2 hide
  // H16<BF>::pack2 of cvt16.h (the fp16 one is another instruction choice, this one its twin): call
  // them through Mfma16 only -- the inherited pack4 goes through the base's.
  __device__ __forceinline__ static unsigned pack2(float a, float b) {
    return (unsigned)from_f32(a) | ((unsigned)from_f32(b) << 16);
  }
  __device__ __forceinline__ static f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma16<false> : H16<false> {
  typedef f16x8 vec8;
  __device__ __forceinline__ static unsigned pack2(float a, float b) {  // (one v_cvt_pk_f16_f32)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 v = __builtin_convertvector((f32x2){a, b}, f16x2);
    return __builtin_bit_cast(unsigned, v);
  }
  __device__ __forceinline__ static f32x16 mfma(vec8 a, vec8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

template <int W>
struct InterCfg16 {
  static constexpr int LD = W + 8;   // forward: row stride in 16-bit elements (+16 B against conflicts)
  static constexpr int XT = 32 * W;  // backward: the tile's elements (rows unpadded, chunks swizzled)
  static constexpr int GS = 40;      // G row stride (elements): 80 B -> 16 distinct 16-B slots
  // The backward's tile is read three ways: by rows in 16-byte chunks (tile write, gradient rows
  // out), by columns through the transposed read (4 rows x 32 columns per half wave) and written
  // back 8 bytes per lane, lane = row, one half chunk for all.  Chunk ch of row `row` lies at chunk
  // ch ^ bwd_swz(row) of that row: the 16 chunks of a transposed read then cover all 64 banks
  // once, the 16 rows of an 8-byte write the 32 banks twice (2-way, hidden behind the store's
  // register transfer), and a row's chunks stay a permutation of themselves.
  __host__ __device__ static constexpr int bwd_swz(int row) {
    return W == 128 ? (((row & 3) << 2) | ((row >> 2) & 3))
           : W == 64 ? ((((row >> 1) & 1) << 2) | ((row >> 2) & 3))
                     : ((row >> 1) & 3);
  }
  // element offset of 16-byte chunk ch of row `row` in the backward's tile
  __host__ __device__ static constexpr int bwd_off(int row, int ch) {
    return row * W + ((ch ^ bwd_swz(row)) << 3);
  }
  // the layouts of InterCfg<W>, in 16-bit elements
  static size_t fwd_lds(const InterShape& s) {
    return (size_t)((s.n_ins + 1) * LD + ((s.out_len + 7) & ~7)) * 2;
  }
  static size_t bwd_lds(const InterShape& s) {
    return (size_t)(XT + 32 * GS + ((s.n_pairs + 7) & ~7)) * 2;
  }
};

// row_of == nullptr: emb is the dense [batch][n_emb][W] tensor.  row_of != nullptr (unique-row
// exchange): emb is a table of distinct rows [R][W] and embedding row s of sample b is
// emb[row_of[b * n_emb + s]] -- the receiver never materialises the expanded tensor.
template <int W, int NPRE>
__device__ __forceinline__ void load_sample_tile16(u32x4 (&pre)[NPRE],
                                                   const unsigned short* __restrict__ mlp,
                                                   const unsigned short* __restrict__ emb,
                                                   const uint32_t* __restrict__ row_of, size_t b,
                                                   int n_emb, int n_vec, int lane) {
  constexpr int W8 = W / 8;
  const u32x4* m4 = reinterpret_cast<const u32x4*>(mlp + b * W);
  if (row_of == nullptr) {
    const u32x4* e4 = reinterpret_cast<const u32x4*>(emb + b * (size_t)n_emb * W) - W8;
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      int i = lane + 64 * q;
      i = i < n_vec ? i : 0;
      const u32x4* src = (i < W8) ? m4 : e4;
      pre[q] = src[i];
    }
  } else {
    const u32x4* r4 = reinterpret_cast<const u32x4*>(emb);
    const uint32_t* ro = row_of + b * (size_t)n_emb;
    uint32_t idx[NPRE];
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      int i = lane + 64 * q;
      i = i < n_vec ? i : 0;
      const int row = i / W8;
      idx[q] = ro[row > 0 ? row - 1 : 0];
    }
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      int i = lane + 64 * q;
      i = i < n_vec ? i : 0;
      const int row = i / W8, c8 = i % W8;
      pre[q] = (row == 0) ? m4[c8] : r4[(size_t)idx[q] * W8 + c8];
    }
  }
}

// What both 16-bit forward kernels do once a sample's tile lies in LDS (xt, behind a barrier):
// X.X^T on the MFMA (lane (r, h) feeds X[r][h*W/2 + 8t .. +7] at k-step t; A == B fragment), the
// strict lower triangle, the MLP pass-through and the zero pad column staged as the output row,
// which leaves as 16-byte stores where its length allows.  Ends behind a barrier: xt and stage are
// free again.
template <int W, typename H>
__device__ __forceinline__ void inter_fwd16_finish(const unsigned short* xt, unsigned short* stage,
                                                   int n_ins, int lane,
                                                   unsigned short* o, int out_len) {
  using C = InterCfg16<W>;
  const int r = lane & 31, h = lane >> 5;
  const int rr = r < n_ins ? r : n_ins;  // rows past the tile read the zero row
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const unsigned short* xr = xt + rr * C::LD + h * (W / 2);
#pragma unroll
  for (int t = 0; t < W / 16; t++) {
    const typename H::vec8 f = *reinterpret_cast<const typename H::vec8*>(xr + t * 8);
    acc = H::mfma(f, f, acc);
  }
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (row > r && row < n_ins) stage[W + tri_index(row, r)] = H::from_f32(acc[reg]);
  }
  for (int i = lane; i < W; i += 64) stage[i] = xt[i];
  if (lane == 0) stage[out_len - 1] = 0;
  __syncthreads();
  if ((out_len & 7) == 0) {
    for (int i = lane; i < out_len / 8; i += 64)
      reinterpret_cast<u32x4*>(o)[i] = reinterpret_cast<const u32x4*>(stage)[i];
  } else {
    for (int i = lane; i < out_len; i += 64) o[i] = stage[i];
  }
  __syncthreads();
}

template <int W, bool BF>
__global__ void __launch_bounds__(64, 2)
    interaction_fwd16_kernel(size_t batch, int n_emb, const unsigned short* __restrict__ mlp,
                             const unsigned short* __restrict__ emb,
                             const uint32_t* __restrict__ row_of,
                             unsigned short* __restrict__ out, int out_len) {
  using C = InterCfg16<W>;
  using H = Mfma16<BF>;
  HCTR_DYN_LDS16(unsigned short, smem16);
  const int lane = threadIdx.x;
  const int n_ins = n_emb + 1;
  unsigned short* xt = smem16;
  unsigned short* stage = smem16 + (n_ins + 1) * C::LD;
  constexpr int W8 = W / 8;
  constexpr int NPRE = (32 * W8 + 63) / 64;
  const int n_vec = n_ins * W8;
  for (int i = lane; i < C::LD; i += 64) xt[n_ins * C::LD + i] = 0;  // zero row

  u32x4 pre[NPRE];
  size_t b = blockIdx.x;
  if (b < batch) load_sample_tile16<W, NPRE>(pre, mlp, emb, row_of, b, n_emb, n_vec, lane);
  for (; b < batch; b += gridDim.x) {
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W8, c8 = i % W8;
        *reinterpret_cast<u32x4*>(xt + row * C::LD + c8 * 8) = pre[q];
      }
    }
    __syncthreads();
    const size_t nb = b + gridDim.x;
    if (nb < batch) load_sample_tile16<W, NPRE>(pre, mlp, emb, row_of, nb, n_emb, n_vec, lane);

    inter_fwd16_finish<W, H>(xt, stage, n_ins, lane, out + b * (size_t)out_len, out_len);
  }
}

// ---- gather fused into the interaction (one GPU, one key per bucket, sum combiner) ---------------
// The pooled vector of a one-hot bucket IS its table row (rounded to the 16-bit type), and the
// interaction stages each sample's rows in LDS anyway: this kernel reads the fp32 table rows
// through value_index straight into the tile and runs the same MFMA chain and output stage as
// interaction_fwd16_kernel -- bit-identical to pool_vec4_kernel + interaction_fwd16_kernel, without
// the pass that re-reads the pooled vectors (B * n_emb * W * 2 bytes).  STORE: the pooled
// [batch][n_emb][W] vectors are written once as well, for a backward that reads them; without it
// the backward rebuilds the same tile from the table (interaction_bwd16_kernel<.., GATHER>).
// A missing row (kInvalidIndex: evaluation miss / full table) pools as zeros.
template <int W, int NPRE>
__device__ __forceinline__ void load_gather_idx(uint64_t (&idx)[NPRE],
                                                const uint64_t* __restrict__ value_index,
                                                size_t b, int n_emb, int n_vec, int lane) {
  constexpr int W8 = W / 8;
  const uint64_t* vi = value_index + b * (size_t)n_emb;
#pragma unroll
  for (int q = 0; q < NPRE; q++) {
    int i = lane + 64 * q;
    i = i < n_vec ? i : 0;
    const int row = i / W8;
    idx[q] = vi[row > 0 ? row - 1 : 0];
  }
}

template <int W, int NPRE>
__device__ __forceinline__ void load_gather_rows(f32x4 (&lo)[NPRE], f32x4 (&hi)[NPRE],
                                                 const uint64_t (&idx)[NPRE],
                                                 const unsigned short* __restrict__ mlp,
                                                 const float* __restrict__ table, size_t b,
                                                 int n_vec, int lane) {
  constexpr int W8 = W / 8;
  const f32x4* m4 = reinterpret_cast<const f32x4*>(mlp + b * W);  // (16 bytes = 8 halves)
#pragma unroll
  for (int q = 0; q < NPRE; q++) {
    int i = lane + 64 * q;
    i = i < n_vec ? i : 0;
    const int row = i / W8, c8 = i % W8;
    const uint64_t r = idx[q] != kInvalidIndex ? idx[q] : 0ull;  // always a legal read
    const f32x4* t4 = reinterpret_cast<const f32x4*>(table + r * (uint64_t)W + c8 * 8);
    lo[q] = (row == 0) ? m4[c8] : t4[0];
    hi[q] = (row == 0) ? m4[c8] : t4[1];
  }
}

// load_gather_rows for the backward, whose prefetch registers are scarcer: lane s < n_emb holds
// the row number of embedding s (my_idx, loaded a sample ahead), each entry takes its own from that
// lane; returns the entries' live bits (row number != kInvalidIndex).  The lane's row number for the
// sample after (*my_next) is asked for once the current one has been handed out and in front of the
// rows: it takes my_idx's place without a copy that would have to wait for it.
template <int W, int NPRE>
__device__ __forceinline__ uint32_t load_gather_rows_lane(f32x4 (&lo)[NPRE], f32x4 (&hi)[NPRE],
                                                          uint64_t& my_idx,
                                                          const uint64_t* __restrict__ my_next,
                                                          const unsigned short* __restrict__ mlp,
                                                          const float* __restrict__ table, size_t b,
                                                          int n_vec, int lane) {
  constexpr int W8 = W / 8;
  uint64_t idx[NPRE];
#pragma unroll
  for (int q = 0; q < NPRE; q++) {
    int i = lane + 64 * q;
    i = i < n_vec ? i : 0;
    const int row = i / W8;
    idx[q] = __shfl(my_idx, row > 0 ? row - 1 : 0);
  }
  my_idx = *my_next;
  load_gather_rows<W, NPRE>(lo, hi, idx, mlp, table, b, n_vec, lane);
  uint32_t live = 0;
#pragma unroll
  for (int q = 0; q < NPRE; q++) live |= (idx[q] != kInvalidIndex ? 1u : 0u) << q;
  return live;
}

// 8 values of a gathered tile row as the 16-bit vector the tile holds: row 0 (the MLP output) as
// loaded, an embedding row rounded from fp32 (a missing row -> +0)
template <typename H>
__device__ __forceinline__ u32x4 gather_tile_vec(const f32x4& lo, const f32x4& hi, bool live,
                                                 int row) {
  if (row == 0) return *reinterpret_cast<const u32x4*>(&lo);
  float f[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  unsigned short u[8];
#pragma unroll
  for (int k = 0; k < 8; k++) u[k] = H::from_f32(0.f + (live ? f[k] : 0.f));
  u32x4 v;
  v[0] = (uint32_t)u[0] | ((uint32_t)u[1] << 16);
  v[1] = (uint32_t)u[2] | ((uint32_t)u[3] << 16);
  v[2] = (uint32_t)u[4] | ((uint32_t)u[5] << 16);
  v[3] = (uint32_t)u[6] | ((uint32_t)u[7] << 16);
  return v;
}

template <int W, bool BF, bool STORE>
__global__ void __launch_bounds__(64, 2)
    interaction_fwd16_gather_kernel(size_t batch, int n_emb,
                                    const unsigned short* __restrict__ mlp,
                                    const float* __restrict__ table,
                                    const uint64_t* __restrict__ value_index,
                                    unsigned short* __restrict__ pooled,
                                    unsigned short* __restrict__ out, int out_len) {
  using C = InterCfg16<W>;
  using H = Mfma16<BF>;
  HCTR_DYN_LDS16(unsigned short, smem16);
  const int lane = threadIdx.x;
  const int n_ins = n_emb + 1;
  unsigned short* xt = smem16;
  unsigned short* stage = smem16 + (n_ins + 1) * C::LD;
  constexpr int W8 = W / 8;
  constexpr int NPRE = (32 * W8 + 63) / 64;
  const int n_vec = n_ins * W8;
  for (int i = lane; i < C::LD; i += 64) xt[n_ins * C::LD + i] = 0;  // zero row

  f32x4 lo[NPRE], hi[NPRE];
  uint64_t idx[NPRE], idx_nxt[NPRE];
  size_t b = blockIdx.x;
  const size_t last = batch - 1;
  // row indices run one sample ahead of the rows, the rows one sample ahead of the MFMA chain
  load_gather_idx<W, NPRE>(idx, value_index, b < batch ? b : last, n_emb, n_vec, lane);
  load_gather_rows<W, NPRE>(lo, hi, idx, mlp, table, b < batch ? b : last, n_vec, lane);
  {
    const size_t nb = b + gridDim.x;
    load_gather_idx<W, NPRE>(idx_nxt, value_index, nb < batch ? nb : last, n_emb, n_vec, lane);
  }
  for (; b < batch; b += gridDim.x) {
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W8, c8 = i % W8;
        const u32x4 v = gather_tile_vec<H>(lo[q], hi[q], idx[q] != kInvalidIndex, row);
        if (STORE && row != 0)
          *reinterpret_cast<u32x4*>(pooled + (b * (size_t)n_emb + (row - 1)) * W + c8 * 8) = v;
        *reinterpret_cast<u32x4*>(xt + row * C::LD + c8 * 8) = v;
      }
    }
    __syncthreads();
    const size_t nb = b + gridDim.x, nb2 = nb + gridDim.x;
#pragma unroll
    for (int q = 0; q < NPRE; q++) idx[q] = idx_nxt[q];
    if (nb < batch) load_gather_rows<W, NPRE>(lo, hi, idx, mlp, table, nb, n_vec, lane);
    load_gather_idx<W, NPRE>(idx_nxt, value_index, nb2 < batch ? nb2 : last, n_emb, n_vec, lane);

    inter_fwd16_finish<W, H>(xt, stage, n_ins, lane, out + b * (size_t)out_len, out_len);
  }
}

template <int W, bool BF, bool GATHER>
__global__ void __launch_bounds__(64, 2)
    interaction_bwd16_kernel(size_t batch, int n_emb, const unsigned short* __restrict__ mlp,
                             const unsigned short* __restrict__ emb,
                             const uint32_t* __restrict__ row_of,
                             const float* __restrict__ table,
                             const uint64_t* __restrict__ value_index,
                             const unsigned short* __restrict__ top_grad,
                             unsigned short* __restrict__ mlp_grad,
                             unsigned short* __restrict__ emb_grad, int out_len,
                             const uint32_t* __restrict__ grad_map) {
  // grad_map != nullptr: the gradient of embedding s of sample b goes to row
  // grad_map[b * n_emb + s] of emb_grad (the all-to-all send layout: no reorder pass behind it)
  // GATHER: the tile is rebuilt from the fp32 table through value_index exactly as
  // interaction_fwd16_gather_kernel built it (emb / row_of unused) -- the pooled vectors are never
  // stored; row numbers run one sample ahead of the rows, which are rounded when the tile is written.
  // Everything a sample reads from global memory (rows, both parts of the top gradient, the row
  // numbers of the sample after) is asked for by one unconditional prefetch a sample ahead, oldest
  // first in the order it is needed: the vector-memory counter retires in order, so a load issued
  // behind the prefetch, or a branch around it, would turn the next wait into a wait for all of it
  using C = InterCfg16<W>;
  using H = Mfma16<BF>;
  constexpr int GS = C::GS;
  HCTR_DYN_LDS16(unsigned short, smem16);
  const int lane = threadIdx.x;
  const int n_ins = n_emb + 1;
  unsigned short* xt = smem16;            // [32][W] X (chunks at C::bwd_off), reused for dX
  unsigned short* gm = smem16 + C::XT;    // [32][GS]
  unsigned short* pair_nm = gm + 32 * GS; // [n_pairs]
  constexpr int W8 = W / 8;
  constexpr int NT = W / 32;
  constexpr int NPRE = (32 * W8 + 63) / 64;
  constexpr int NG = 8;
  const int n_vec = n_ins * W8;
  const int n_pairs = n_ins * (n_ins - 1) / 2;
  for (int i = lane; i < C::XT + 32 * GS; i += 64) smem16[i] = 0;
  for (int p = lane; p < n_pairs; p += 64) {
    int n = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (n * (n - 1) / 2 > p) n--;
    while ((n + 1) * n / 2 <= p) n++;
    pair_nm[p] = (unsigned short)((n << 8) | (p - n * (n - 1) / 2));
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  u32x4 pre[NPRE];
  f32x4 lo[NPRE], hi[NPRE];
  uint32_t live = 0;
  uint64_t idx_nxt = 0;
  unsigned short gpre[NG];
  u32x4 gt_nxt = {0u, 0u, 0u, 0u};  // the sample's pass-through gradient (row 0: lanes < W8)
  size_t b = blockIdx.x;
  const size_t last = batch - 1;
  const int my_s = lane < n_emb ? lane : 0;
  // (a macro: as a lambda or a function it moves the registers of every instantiation and, through
  // the loader they share, interaction_fwd16_kernel's: profiles/interaction_refactor_resources.txt)
#define HCTR_BWD16_PREFETCH(bb)                                                       \
  {                                                                                   \
    if constexpr (GATHER) {                                                           \
      const size_t nx__ = (bb) + gridDim.x;                                           \
      live = load_gather_rows_lane<W, NPRE>(                                          \
          lo, hi, idx_nxt, value_index + (nx__ < batch ? nx__ : last) * (size_t)n_emb + my_s, \
          mlp, table, (bb), n_vec, lane);                                             \
    } else                                                                            \
      load_sample_tile16<W, NPRE>(pre, mlp, emb, row_of, (bb), n_emb, n_vec, lane);   \
    gt_nxt = reinterpret_cast<const u32x4*>(top_grad + (bb) * (size_t)out_len)[lane < W8 ? lane : 0]; \
    const unsigned short* g__ = top_grad + (bb) * (size_t)out_len + W;                \
    _Pragma("unroll") for (int q = 0; q < NG; q++) {                                  \
      int p__ = lane + 64 * q;                                                        \
      p__ = p__ < n_pairs ? p__ : 0;                                                  \
      gpre[q] = g__[p__];                                                             \
    }                                                                                 \
  }
  if constexpr (GATHER) idx_nxt = value_index[(b < batch ? b : last) * (size_t)n_emb + my_s];
  if (b < batch) HCTR_BWD16_PREFETCH(b)
  for (; b < batch; b += gridDim.x) {
    const u32x4 gt = gt_nxt;
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W8, c8 = i % W8;
        *reinterpret_cast<u32x4*>(xt + C::bwd_off(row, c8)) =
            GATHER ? gather_tile_vec<H>(lo[q], hi[q], (live >> q) & 1u, row) : pre[q];
      }
    }
#pragma unroll
    for (int q = 0; q < NG; q++) {
      const int p = lane + 64 * q;
      if (p < n_pairs) {
        const int nm = pair_nm[p];
        const int n = nm >> 8, m = nm & 0xFF;
        gm[n * GS + m] = gpre[q];
        gm[m * GS + n] = gpre[q];
      }
    }
    __syncthreads();
    // the next sample's rows and gradients; behind the last one the last sample's again (legal
    // reads nobody uses): a branch around the prefetch would make every wait behind it, for a load
    // issued in front of it, a wait for everything
    const size_t nb = b + gridDim.x < batch ? b + gridDim.x : last;
    HCTR_BWD16_PREFETCH(nb)

    // dX^T = X^T G on the MFMA (G is symmetric: its fragment is the same as either operand): lane
    // (r, h) feeds column T*32 + r of X rows k0 .. k0+7 -- two transposed reads, lane 4q + p of each
    // 16 supplying row q, columns 4p .. 4p+3 of its block -- and receives row r of dX, columns
    // T*32 + 8g + 4h .. +3 in registers 4g .. 4g+3, which go back to the tile as one 8-byte store
    constexpr int HP = NT >= 2 ? 2 : 1;
    const int tq = (lane >> 2) & 3, tp = lane & 3, tj = (lane >> 4) & 1;
#pragma unroll
    for (int pn = 0; pn < NT / HP; pn++) {
      f32x16 acc[HP];
#pragma unroll
      for (int t = 0; t < HP; t++)
        acc[t] = (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                          0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s2 = 0; s2 < 2; s2++) {
        const int k0 = 16 * s2 + 8 * h;
        const typename H::vec8 gf = *reinterpret_cast<const typename H::vec8*>(gm + r * GS + k0);
#pragma unroll
        for (int t = 0; t < HP; t++) {
          const int T = pn * HP + t;
          const int col = T * 32 + r;
          hctr_u32x2 x2[2];
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const int r0 = k0 + 4 * j;
            x2[j] = HCTR_LDS_READ_TR16_B64(
                xt, C::bwd_off(r0 + tq, 4 * T + 2 * tj + (tp >> 1)) + 4 * (tp & 1),
                C::bwd_off(r0, col >> 3) + (col & 7), C::bwd_off(r0 + 1, col >> 3) + (col & 7),
                C::bwd_off(r0 + 2, col >> 3) + (col & 7), C::bwd_off(r0 + 3, col >> 3) + (col & 7));
          }
          const u32x4 packed = {x2[0][0], x2[0][1], x2[1][0], x2[1][1]};
          const typename H::vec8 xf = *reinterpret_cast<const typename H::vec8*>(&packed);
          acc[t] = H::mfma(xf, gf, acc[t]);
        }
      }
      __syncthreads();
      if (r < n_ins) {
#pragma unroll
        for (int t = 0; t < HP; t++) {
#pragma unroll
          for (int g = 0; g < 4; g++) {
            hctr_u32x2 w2;
            w2[0] = H::pack2(acc[t][4 * g], acc[t][4 * g + 1]);
            w2[1] = H::pack2(acc[t][4 * g + 2], acc[t][4 * g + 3]);
            *reinterpret_cast<hctr_u32x2*>(xt + C::bwd_off(r, 4 * (pn * HP + t) + g) + 4 * h) = w2;
          }
        }
      }
    }
    __syncthreads();
    u32x4* mg4 = reinterpret_cast<u32x4*>(mlp_grad + b * W);
    u32x4* eg4 = reinterpret_cast<u32x4*>(emb_grad + b * (size_t)n_emb * W);
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W8, c8 = i % W8;
        u32x4 v = *reinterpret_cast<const u32x4*>(xt + C::bwd_off(row, c8));
        if (row == 0) {
          u32x4 o4;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float a0 = H::to_f32((unsigned short)(v[e] & 0xFFFFu)) +
                             H::to_f32((unsigned short)(gt[e] & 0xFFFFu));
            const float a1 = H::to_f32((unsigned short)(v[e] >> 16)) +
                             H::to_f32((unsigned short)(gt[e] >> 16));
            o4[e] = (unsigned)H::from_f32(a0) | ((unsigned)H::from_f32(a1) << 16);
          }
          mg4[c8] = o4;
        } else if (grad_map == nullptr) {
          eg4[i - W8] = v;
        } else {
          const uint32_t dst = grad_map[b * (size_t)n_emb + (row - 1)];
          reinterpret_cast<u32x4*>(emb_grad + (size_t)dst * W)[c8] = v;
        }
      }
    }
    __syncthreads();
  }
#undef HCTR_BWD16_PREFETCH
}

// any shape / dtype: one wavefront per sample, VALU dot products (fp32 accumulate)
template <typename T>
__global__ void __launch_bounds__(kGenericBlock)
    interaction_fwd_generic_kernel(size_t batch, int n_emb, int W, const T* __restrict__ mlp,
                                   const T* __restrict__ emb, T* __restrict__ out, int out_len) {
  HCTR_DYN_LDS16(float, smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_ins = n_emb + 1;
  float* xt = smem + wave * (n_ins * (W + 1));
  const size_t waves_total = (size_t)gridDim.x * kGenericWaves;
  const size_t iters = (batch + waves_total - 1) / waves_total;
  const int n_pairs = n_ins * (n_ins - 1) / 2;
  for (size_t it = 0; it < iters; it++) {
    const size_t b = it * waves_total + (size_t)blockIdx.x * kGenericWaves + wave;
    const bool valid = b < batch;
    if (valid) {
      for (int i = lane; i < n_ins * W; i += 64) {
        const int row = i / W, c = i % W;
        xt[row * (W + 1) + c] =
            to_f32<T>(row == 0 ? mlp[b * W + c] : emb[(b * n_emb + (row - 1)) * (size_t)W + c]);
      }
    }
    __syncthreads();
    if (valid) {
      T* o = out + b * (size_t)out_len;
      for (int i = lane; i < W; i += 64) o[i] = from_f32<T>(xt[i]);
      for (int p = lane; p < n_pairs; p += 64) {
        // invert p = n(n-1)/2 + m
        int n = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
        while (n * (n - 1) / 2 > p) n--;
        while ((n + 1) * n / 2 <= p) n++;
        const int m = p - n * (n - 1) / 2;
        float a = 0.f;
        for (int k = 0; k < W; k++) a += xt[m * (W + 1) + k] * xt[n * (W + 1) + k];
        o[W + p] = from_f32<T>(a);
      }
      if (lane == 0) o[out_len - 1] = from_f32<T>(0.f);
    }
    __syncthreads();
  }
}

// ================================================================================================
// Interaction backward, fp32 MFMA path.  G = dM + dM^T (symmetric, zero diagonal) in LDS,
// dX = G . X : M = 32 (n_ins padded), N = W, K = 32.
//   mlp_grad[b] = top_grad[b][0:W] + dX[0];  emb_grad[b][i-1] = dX[i]
// ================================================================================================
template <int W>
__global__ void __launch_bounds__(64, 2)
    interaction_bwd_mfma_kernel(size_t batch, int n_emb, const float* __restrict__ mlp,
                                const float* __restrict__ emb, const float* __restrict__ top_grad,
                                float* __restrict__ mlp_grad, float* __restrict__ emb_grad,
                                int out_len) {
  using C = InterCfg<W>;
  constexpr int GS = C::GS;
  HCTR_DYN_LDS16(float, smem);
  const int lane = threadIdx.x;
  const int n_ins = n_emb + 1;
  float* xt = smem;                 // [32][LD]  X, later reused for dX
  float* gm = smem + C::XT;         // [32][GS]  G = dM + dM^T
  unsigned short* pair_nm = reinterpret_cast<unsigned short*>(gm + 32 * GS);  // [n_pairs]
  constexpr int W4 = W / 4;
  constexpr int NT = W / 32;
  constexpr int NPRE = (32 * W4 + 63) / 64;
  constexpr int NG = 8;  // ceil(496 / 64) gradient words per lane
  const int n_vec = n_ins * W4;
  const int n_pairs = n_ins * (n_ins - 1) / 2;
  for (int i = lane; i < C::XT + 32 * GS; i += 64) smem[i] = 0.f;
  for (int p = lane; p < n_pairs; p += 64) {
    int n = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (n * (n - 1) / 2 > p) n--;
    while ((n + 1) * n / 2 <= p) n++;
    pair_nm[p] = (unsigned short)((n << 8) | (p - n * (n - 1) / 2));
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  f32x4 pre[NPRE];
  float gpre[NG];
  size_t b = blockIdx.x;
  auto prefetch = [&](size_t bb) {  // registers <- sample bb's tile and pair gradients
    load_sample_tile<W, NPRE>(pre, mlp, emb, bb, n_emb, n_vec, lane);
    const float* g = top_grad + bb * (size_t)out_len + W;
#pragma unroll
    for (int q = 0; q < NG; q++) {
      int p = lane + 64 * q;
      p = p < n_pairs ? p : 0;
      gpre[q] = g[p];
    }
  };
  if (b < batch) prefetch(b);
  for (; b < batch; b += gridDim.x) {
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W4, c4 = i % W4;
        *reinterpret_cast<f32x4*>(xt + row * C::LD + c4 * 4) = pre[q];
      }
    }
#pragma unroll
    for (int q = 0; q < NG; q++) {
      const int p = lane + 64 * q;
      if (p < n_pairs) {
        const int nm = pair_nm[p];
        const int n = nm >> 8, m = nm & 0xFF;
        gm[n * GS + m] = gpre[q];
        gm[m * GS + n] = gpre[q];
      }
    }
    __syncthreads();
    const size_t nb = b + gridDim.x;
    if (nb < batch) prefetch(nb);

    // dX = G . X : A = G [32 x 32], B = X [32 x W]; K = 32 -> two k-steps of 16.  The output is
    // produced in column panels of HP*32 columns (32 accumulator registers instead of 64); panel
    // p only reads columns of X that earlier panels did not overwrite, so dX replaces X in place.
    constexpr int HP = NT >= 2 ? 2 : 1;  // N tiles per panel
#pragma unroll
    for (int pn = 0; pn < NT / HP; pn++) {
      f32x16 acc[HP];
#pragma unroll
      for (int t = 0; t < HP; t++)
        acc[t] = (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                          0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s2 = 0; s2 < 2; s2++) {
        const int k0 = 16 * s2 + 8 * h;
        const float4 ga = *reinterpret_cast<const float4*>(gm + r * GS + k0);
        const float4 gb = *reinterpret_cast<const float4*>(gm + r * GS + k0 + 4);
        bf16x8 ah, al;
        split8(ga, gb, ah, al);
#pragma unroll
        for (int t = 0; t < HP; t++) {
          const int col = (pn * HP + t) * 32 + r;
          float xv[8];
#pragma unroll
          for (int e = 0; e < 8; e++) xv[e] = xt[(k0 + e) * C::LD + col];
          bf16x8 bh, bl;
          split8(make_float4(xv[0], xv[1], xv[2], xv[3]), make_float4(xv[4], xv[5], xv[6], xv[7]),
                 bh, bl);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
        }
      }
      __syncthreads();  // every lane is done reading this panel's columns of X
#pragma unroll
      for (int t = 0; t < HP; t++) {
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
          if (row < n_ins) xt[row * C::LD + (pn * HP + t) * 32 + r] = acc[t][reg];
        }
      }
    }
    __syncthreads();
    const float4* gtop4 = reinterpret_cast<const float4*>(top_grad + b * (size_t)out_len);
    float4* mg4 = reinterpret_cast<float4*>(mlp_grad + b * W);
    float4* eg4 = reinterpret_cast<float4*>(emb_grad + b * (size_t)n_emb * W);
#pragma unroll
    for (int q = 0; q < NPRE; q++) {
      const int i = lane + 64 * q;
      if (i < n_vec) {
        const int row = i / W4, c4 = i % W4;
        float4 v = *reinterpret_cast<const float4*>(xt + row * C::LD + c4 * 4);
        if (row == 0) {
          const float4 gt = gtop4[c4];
          v.x += gt.x;
          v.y += gt.y;
          v.z += gt.z;
          v.w += gt.w;
          mg4[c4] = v;
        } else {
          eg4[i - W4] = v;
        }
      }
    }
    __syncthreads();
    // rows >= n_ins of the tile were never written; rows < n_ins are rewritten next iteration
  }
}

template <typename T>
__global__ void __launch_bounds__(kGenericBlock)
    interaction_bwd_generic_kernel(size_t batch, int n_emb, int W, const T* __restrict__ mlp,
                                   const T* __restrict__ emb, const T* __restrict__ top_grad,
                                   T* __restrict__ mlp_grad, T* __restrict__ emb_grad,
                                   int out_len) {
  HCTR_DYN_LDS16(float, smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_ins = n_emb + 1;
  float* xt = smem + wave * (n_ins * (W + 1) + n_ins * n_ins);
  float* gm = xt + n_ins * (W + 1);
  const size_t waves_total = (size_t)gridDim.x * kGenericWaves;
  const size_t iters = (batch + waves_total - 1) / waves_total;
  for (size_t it = 0; it < iters; it++) {
    const size_t b = it * waves_total + (size_t)blockIdx.x * kGenericWaves + wave;
    const bool valid = b < batch;
    if (valid) {
      for (int i = lane; i < n_ins * W; i += 64) {
        const int row = i / W, c = i % W;
        xt[row * (W + 1) + c] =
            to_f32<T>(row == 0 ? mlp[b * W + c] : emb[(b * n_emb + (row - 1)) * (size_t)W + c]);
      }
      const T* g = top_grad + b * (size_t)out_len + W;
      for (int i = lane; i < n_ins * n_ins; i += 64) {
        const int m = i / n_ins, n = i % n_ins;
        float v = 0.f;
        if (m != n) {
          const int hi = m > n ? m : n, lo = m > n ? n : m;
          v = to_f32<T>(g[hi * (hi - 1) / 2 + lo]);
        }
        gm[i] = v;
      }
    }
    __syncthreads();
    if (valid) {
      const T* gtop = top_grad + b * (size_t)out_len;
      for (int i = lane; i < n_ins * W; i += 64) {
        const int m = i / W, n = i % W;
        float a = 0.f;
        for (int k = 0; k < n_ins; k++) a += gm[m * n_ins + k] * xt[k * (W + 1) + n];
        if (m == 0) mlp_grad[b * W + n] = from_f32<T>(to_f32<T>(gtop[n]) + a);
        else emb_grad[(b * n_emb + (m - 1)) * (size_t)W + n] = from_f32<T>(a);
      }
    }
    __syncthreads();
  }
}

// ================================================================================================
// Host side: one dispatch for the seven entries
// ================================================================================================
// single-wavefront workgroups per CU of the 16-bit interaction kernels (which: 0 forward,
// 1 backward); HCTR_INTER_WAVES=f,b overrides (measurements)
int inter_waves_per_cu(int which) {
  static const int v[2] = {env_int("HCTR_INTER_WAVES", 8, 0), env_int("HCTR_INTER_WAVES", 8, 1)};
  return v[which];
}
// a kernel that is launched with more than 64 KB of dynamic LDS has to be told first (per device
// and cheap: asked on every such launch rather than remembered per process)
template <typename K>
int allow_dyn_lds(K kernel, size_t lds) {
  if (lds > 65536)
    HCTR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  return HCTR_OK;
}

bool is16(int dtype) { return dtype == HCTR_EMB_BF16 || dtype == HCTR_EMB_F16; }
template <int... Vs>
bool one_of(int v) {
  return ((v == Vs) || ...);
}
template <typename... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}
// grid of the one-wavefront-per-sample kernels: a workgroup per sample, at most waves_per_cu of
// them resident on each of the 256 CUs
int sample_grid(size_t batch, int waves_per_cu) {
  const size_t gmax = (size_t)256 * (size_t)waves_per_cu;
  return (int)(batch < gmax ? batch : gmax);
}

// run-time value -> template argument (see with_bool / with_dtype, common.h):
// f(std::integral_constant<int, W>{}) for the W of Ws that equals width (the caller has checked
// that one does)
template <int... Ws, typename F>
void with_width(int width, F&& f) {
  (void)((width == Ws && (f(std::integral_constant<int, Ws>{}), true)) || ...);
}

int interaction_fwd_impl(size_t batch, int n_emb, int width, const void* mlp, const void* emb,
                         const uint32_t* row_of, void* out, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(n_emb >= 1 && width >= 1, "shape");
  const InterShape sh(n_emb, width);
  const bool a16 = aligned16(mlp, emb, out);
  HCTR_REQUIRE(row_of == nullptr ||
                   (is16(dtype) && sh.n_ins <= 32 && one_of<128, 64, 32>(width) && a16),
               "indexed interaction: 16-bit rows, width 32/64/128, <= 31 embeddings, 16-byte "
               "aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(mlp && emb && out, "null pointer");
  hipStream_t s = as_stream(stream);
  const bool tile = sh.n_ins <= 32 && a16 && one_of<128, 64, 32, 16>(width);
  if (dtype == HCTR_EMB_F32 && tile) {
    with_width<128, 64, 32, 16>(width, [&](auto w) {
      constexpr int W = decltype(w)::value;
      hipLaunchKernelGGL(interaction_fwd_mfma_kernel<W>, dim3(sample_grid(batch, 8)), dim3(64),
                         InterCfg<W>::fwd_lds(sh), s, batch, n_emb, (const float*)mlp,
                         (const float*)emb, (float*)out, sh.out_len);
    });
  } else if (is16(dtype) && tile) {
    with_width<128, 64, 32, 16>(width, [&](auto w) {
      with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((interaction_fwd16_kernel<W, decltype(bf)::value>),
                           dim3(sample_grid(batch, inter_waves_per_cu(0))), dim3(64),
                           InterCfg16<W>::fwd_lds(sh), s, batch, n_emb, (const unsigned short*)mlp,
                           (const unsigned short*)emb, row_of, (unsigned short*)out, sh.out_len);
      });
    });
  } else {
    const size_t lds = (size_t)kGenericWaves * sh.n_ins * (width + 1) * 4;
    HCTR_REQUIRE(lds <= 160 * 1024, "interaction: tile does not fit LDS");
    HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
      using T = std::remove_pointer_t<decltype(t)>;
      HCTR_TRY(allow_dyn_lds(interaction_fwd_generic_kernel<T>, lds));
      hipLaunchKernelGGL(interaction_fwd_generic_kernel<T>,
                         dim3(grid_for(batch, kGenericWaves, 256 * 2)), dim3(kGenericBlock), lds, s,
                         batch, n_emb, width, (const T*)mlp, (const T*)emb, (T*)out, sh.out_len);
      return HCTR_OK;
    }));
  }
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// GATHER: the tile comes from table / value_index (emb, row_of, grad_map unused); otherwise from
// emb, through row_of if there is one (table, value_index unused)
template <bool GATHER>
void launch_bwd16(size_t batch, int n_emb, int width, const InterShape& sh, int dtype,
                  const void* mlp, const void* emb, const uint32_t* row_of, const float* table,
                  const uint64_t* value_index, const void* top_grad, void* mlp_grad, void* emb_grad,
                  const uint32_t* grad_map, hipStream_t s) {
  with_width<128, 64, 32>(width, [&](auto w) {
    with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
      constexpr int W = decltype(w)::value;
      hipLaunchKernelGGL((interaction_bwd16_kernel<W, decltype(bf)::value, GATHER>),
                         dim3(sample_grid(batch, inter_waves_per_cu(1))), dim3(64),
                         InterCfg16<W>::bwd_lds(sh), s, batch, n_emb, (const unsigned short*)mlp,
                         (const unsigned short*)emb, row_of, table, value_index,
                         (const unsigned short*)top_grad, (unsigned short*)mlp_grad,
                         (unsigned short*)emb_grad, sh.out_len, grad_map);
    });
  });
}

int interaction_bwd_impl(size_t batch, int n_emb, int width, const void* mlp, const void* emb,
                         const uint32_t* row_of, const void* top_grad, void* mlp_grad,
                         void* emb_grad, int dtype, hctr_stream_t stream,
                         const uint32_t* grad_map = nullptr) {
  HCTR_REQUIRE(n_emb >= 1 && width >= 1, "shape");
  const InterShape sh(n_emb, width);
  const bool a16 = aligned16(mlp, emb), g16 = aligned16(top_grad, mlp_grad, emb_grad);
  HCTR_REQUIRE(row_of == nullptr || (is16(dtype) && sh.n_ins <= 32 && one_of<128, 64, 32>(width) &&
                                     sh.out_len % 8 == 0 && a16 && g16),
               "indexed interaction: 16-bit rows, width 32/64/128, <= 31 embeddings, output "
               "length % 8 == 0, 16-byte aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(mlp && emb && top_grad && mlp_grad && emb_grad, "null pointer");
  hipStream_t s = as_stream(stream);
  const bool tile = sh.n_ins <= 32 && a16 && g16 && one_of<128, 64, 32>(width);
  if (dtype == HCTR_EMB_F32 && tile && sh.out_len % 4 == 0) {
    with_width<128, 64, 32>(width, [&](auto w) {
      constexpr int W = decltype(w)::value;
      hipLaunchKernelGGL(interaction_bwd_mfma_kernel<W>, dim3(sample_grid(batch, 8)), dim3(64),
                         InterCfg<W>::bwd_lds(sh), s, batch, n_emb, (const float*)mlp,
                         (const float*)emb, (const float*)top_grad, (float*)mlp_grad,
                         (float*)emb_grad, sh.out_len);
    });
  } else if (is16(dtype) && tile && sh.out_len % 8 == 0) {
    launch_bwd16<false>(batch, n_emb, width, sh, dtype, mlp, emb, row_of, nullptr, nullptr,
                        top_grad, mlp_grad, emb_grad, grad_map, s);
  } else {
    const size_t lds =
        (size_t)kGenericWaves * (sh.n_ins * (width + 1) + sh.n_ins * sh.n_ins) * 4;
    HCTR_REQUIRE(lds <= 160 * 1024, "interaction: tile does not fit LDS");
    HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
      using T = std::remove_pointer_t<decltype(t)>;
      HCTR_TRY(allow_dyn_lds(interaction_bwd_generic_kernel<T>, lds));
      hipLaunchKernelGGL(interaction_bwd_generic_kernel<T>,
                         dim3(grid_for(batch, kGenericWaves, 256 * 2)), dim3(kGenericBlock), lds, s,
                         batch, n_emb, width, (const T*)mlp, (const T*)emb, (const T*)top_grad,
                         (T*)mlp_grad, (T*)emb_grad, sh.out_len);
      return HCTR_OK;
    }));
  }
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace
}  // namespace hctr

using namespace hctr;

extern "C" {

int hctr_interaction_fwd(size_t batch, int n_emb, int width, const void* mlp, const void* emb,
                         void* out, int dtype, hctr_stream_t stream) {
  return interaction_fwd_impl(batch, n_emb, width, mlp, emb, nullptr, out, dtype, stream);
}

int hctr_interaction_fwd_indexed(size_t batch, int n_emb, int width, const void* mlp,
                                 const void* rows, const uint32_t* row_of, void* out, int dtype,
                                 hctr_stream_t stream) {
  HCTR_REQUIRE(row_of, "null pointer");
  return interaction_fwd_impl(batch, n_emb, width, mlp, rows, row_of, out, dtype, stream);
}

int hctr_interaction_fwd_gather(size_t batch, int n_emb, int width, const void* mlp,
                                const float* table, const uint64_t* value_index, void* pooled,
                                void* out, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(n_emb >= 1 && n_emb <= 31, "interaction_fwd_gather: 1 .. 31 embeddings");
  HCTR_REQUIRE(is16(dtype), "interaction_fwd_gather: 16-bit vectors (fp16 / bf16)");
  HCTR_REQUIRE((one_of<128, 64, 32, 16>(width)),
               "interaction_fwd_gather: width 16 / 32 / 64 / 128");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(mlp && table && value_index && out, "null pointer");
  HCTR_REQUIRE(aligned16(mlp, table, pooled, out),
               "interaction_fwd_gather: 16-byte aligned buffers");
  hipStream_t s = as_stream(stream);
  const InterShape sh(n_emb, width);
  // resident wavefronts per CU: every one keeps a sample's rows (14 x 16 B per lane) in flight,
  // and with random rows an iteration lasts as long as that round trip -- more waves, more of
  // them overlapped (HCTR_GATHER_WAVES overrides)
  static const int waves = env_int("HCTR_GATHER_WAVES", 8);
  with_width<128, 64, 32, 16>(width, [&](auto w) {
    with_bool(dtype == HCTR_EMB_BF16, [&](auto bf) {
      with_bool(pooled != nullptr, [&](auto store) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL(
            (interaction_fwd16_gather_kernel<W, decltype(bf)::value, decltype(store)::value>),
            dim3(sample_grid(batch, waves)), dim3(64), InterCfg16<W>::fwd_lds(sh), s, batch, n_emb,
            (const unsigned short*)mlp, table, value_index, (unsigned short*)pooled,
            (unsigned short*)out, sh.out_len);
      });
    });
  });
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_interaction_bwd_gather(size_t batch, int n_emb, int width, const void* mlp,
                                const float* table, const uint64_t* value_index,
                                const void* top_grad, void* mlp_grad, void* emb_grad, int dtype,
                                hctr_stream_t stream) {
  const InterShape sh(n_emb, width);
  HCTR_REQUIRE(n_emb >= 1 && n_emb <= 31, "interaction_bwd_gather: 1 .. 31 embeddings");
  HCTR_REQUIRE(is16(dtype), "interaction_bwd_gather: 16-bit vectors (fp16 / bf16)");
  HCTR_REQUIRE((one_of<128, 64, 32>(width)) && sh.out_len % 8 == 0,
               "interaction_bwd_gather: width 32 / 64 / 128, output length % 8 == 0");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(mlp && table && value_index && top_grad && mlp_grad && emb_grad, "null pointer");
  HCTR_REQUIRE(aligned16(mlp, table, top_grad, mlp_grad, emb_grad),
               "interaction_bwd_gather: 16-byte aligned buffers");
  launch_bwd16<true>(batch, n_emb, width, sh, dtype, mlp, nullptr, nullptr, table, value_index,
                     top_grad, mlp_grad, emb_grad, nullptr, as_stream(stream));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_interaction_bwd(size_t batch, int n_emb, int width, const void* mlp, const void* emb,
                         const void* top_grad, void* mlp_grad, void* emb_grad, int dtype,
                         hctr_stream_t stream) {
  return interaction_bwd_impl(batch, n_emb, width, mlp, emb, nullptr, top_grad, mlp_grad, emb_grad,
                              dtype, stream);
}

int hctr_interaction_bwd_indexed(size_t batch, int n_emb, int width, const void* mlp,
                                 const void* rows, const uint32_t* row_of, const void* top_grad,
                                 void* mlp_grad, void* emb_grad, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(row_of, "null pointer");
  return interaction_bwd_impl(batch, n_emb, width, mlp, rows, row_of, top_grad, mlp_grad, emb_grad,
                              dtype, stream);
}

int hctr_interaction_bwd_indexed_scatter(size_t batch, int n_emb, int width, const void* mlp,
                                         const void* rows, const uint32_t* row_of,
                                         const void* top_grad, void* mlp_grad, void* grad_rows,
                                         int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(row_of, "null pointer");
  return interaction_bwd_impl(batch, n_emb, width, mlp, rows, row_of, top_grad, mlp_grad, grad_rows,
                              dtype, stream, row_of);
}

}  // extern "C"
