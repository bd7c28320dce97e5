// cross_gemm.hip -- the GEMMs of MultiCrossLayer v2 (DCN v2) as this library's own MFMA kernel, with
// the elementwise work the reference fuses into its GEMM epilogues.
//
// Reference: MultiCrossForwardFunctorv2 / MultiCrossBackwardFunctorv2
// (R/HugeCTR/src/layers/multi_cross_layer.cu:582-700, 732-812): per layer  P = X_l U,
// H = P V + b (bias in the second GEMM's epilogue, :640-700),  X_{l+1} = X_0 .* H + X_l
// (fused_mul_fma3, :391-424); backward S1 = S0 V^T and dY_{l-1} = S1 U^T + dY_l (the residual in
// the GEMM's epilogue, :760-812).  The reference searches cuBLASLt algorithms per shape; the shapes
// are skinny (K = 3456 -> N = 512 and K = 512 -> N = 3456 at the MLPerf DCNv2 size), which a
// library's 256 x 256 tiles fill badly (64 tiles for B = 8192 on 256 CUs: measured 0.16 of the
// matrix peak, round 4).
//
// One kernel, "NT" form:  C[M][N] = A[M][K] . Bt[N][K]^T  (+ epilogue), 16-bit operands (fp16 or
// bf16), fp32 accumulation on v_mfma_f32_32x32x16_{f16,bf16}.  Both operands are K-contiguous, so
// every MFMA fragment is one 16-byte LDS read; the forward's weights arrive transposed (they are
// converted to the 16-bit type once per step anyway), the backward's are used as they lie.
//   * tile: a GemmTile description (rows, columns, wavefronts along M and N) is all that differs
//     between the three shapes; K step 64, a wavefront owns (BM / WM) x (BN / WN) of C as MFMA tiles
//     of 32 x 32:
//       64 x 128 and 128 x 128, 4 wavefronts as 2 x 2: the skinny products above;
//       256 x 256, 8 wavefronts as 2 x 4 (a wavefront owns 128 x 64: 6 fragment reads per 8 MFMAs
//       instead of 4 per 4), two staging buffers of 64 KB, EPI_PLAIN and EPI_DRELU only.  What it
//       is for: the K = 3456 -> N = 512 products at batch 65536 are bound by what the L2 can feed
//       the LDS, not by the matrix pipe -- 2048 tiles of 128 x 128 move 2048 x 54 x 32 KB = 3.6 GB
//       through the L2 (12 TB/s at the measured 302 us); tiles of 256 x 256 move half of that.  One
//       workgroup per CU (128 KB of LDS), so it is taken only while there are at least as many
//       tiles as CUs;
//   * staging: global_load_lds 16 bytes per lane (no VGPR round trip) into a ring of STAGES LDS
//     buffers (dynamic LDS: 3 x 32 KB at BM = 128), one barrier per K step: tiles k + 1 ..
//     k + STAGES - 1 stream in while tile k is multiplied -- with two buffers a K step cannot be
//     shorter than a trip to L2 / HBM (measured, X1 shape: 545 TFLOP/s at K = 3456), so the wait
//     in front of the barrier is a COUNTED one (vmcnt = the loads of the tiles still allowed in
//     flight) and the barrier a raw s_barrier that does not drain the queue.  The LDS image of a
//     tile is row-major [rows][64] 16-bit = 128 bytes a row, 16-byte chunk c of row r stored at
//     chunk position c ^ ((r >> 1) & 7): the 16 rows a quarter-wave reads together fall into 16
//     different bank groups.  The DMA writes lane-linear, so the permutation is applied to the
//     lanes' SOURCE addresses (inside one 128-byte row segment: coalescing is untouched);
//   * epilogue: the accumulators go through LDS (fp32, the K loop's buffers: as many rows per pass
//     as the ring holds, so the 256 x 256 tile leaves in two passes of 128 rows) and leave as
//     row-contiguous 16-byte stores, which is also where bias / X_0 / X_l / the residual are read
//     as 16-byte vectors:
//       EPI_PLAIN     C = (T)acc
//       EPI_CROSS     H = (T)(acc + b[n]);  C = (T)(X_l + X_0 * H)      (H is stored too: backward)
//       EPI_RESIDUAL  C = (T)(acc + R)
//       EPI_DRELU     C = y > 0 ? (T)acc : 0, and the column sums of what the tile stored as one
//                     fp32 row per row tile (the data gradient of a Linear layer with the ReLU
//                     mask and the bias gradient of the layer below: hctr_gemm_nt16_drelu)
//     EPI_DRELU (hctr_gemm_nt16_drelu) is the data gradient of an MLP layer: A = dz of the layer
//     above, Bt = W^T (FusedMLP keeps it, transpose16_segments_kernel below), y = the ReLU output of
//     the layer below; its column sums are added per thread over its rows and then over the 16 row
//     groups in group order through the same LDS image: deterministic, no atomics;
//   * block id -> tile: column tiles of one row panel are consecutive on ONE XCD (block b runs on
//     XCD b % 8), so the panel of A is fetched from HBM once per XCD L2.
#include <initializer_list>

#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace {

typedef _Float16 cg_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float cg_f32x16 __attribute__((ext_vector_type(16)));
typedef float cg_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int cg_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kGemmBN = 128;  // what N must be a multiple of (the narrowest tile)
constexpr int kGemmBK = 64;   // 16-bit elements: 128 bytes per LDS row
constexpr int kEpiPlain = 0, kEpiCross = 1, kEpiResidual = 2, kEpiDrelu = 3;

// a tile shape: BM x BN of C per workgroup, WM x WN wavefronts; the rest follows
template <int BM_, int BN_, int WM_, int WN_>
struct GemmTile {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_;
  static constexpr int WAVES = WM * WN, THREADS = 64 * WAVES;
  static constexpr int MI = BM / WM / 32, NJ = BN / WN / 32;  // MFMA tiles of a wavefront
  static constexpr int A_TILE = BM * kGemmBK, STAGE = (BM + BN) * kGemmBK;  // 16-bit elements
  static constexpr int DMAS = (BM + BN) / 8 / WAVES;  // DMA instructions per wavefront and K tile
  // epilogue: as many passes as the fp32 tile needs to fit the shallowest ring (two stages)
  static constexpr int PASSES = (BM * BN * 4 + 2 * STAGE * 2 - 1) / (2 * STAGE * 2);
  static constexpr int EPI_ROWS = BM / PASSES;
  static constexpr int CPR = BN / 8;                       // 16-byte chunks (8 columns) per row
  static constexpr int GROUPS = THREADS / CPR;             // rows the threads cover at once
  static constexpr int NCH = EPI_ROWS * CPR / THREADS;     // chunks per thread and pass
  static constexpr int lds_bytes(int stages) { return stages * STAGE * 2; }
  // (the wavefronts of one wm hold exactly one pass's rows, or there is one pass)
  static_assert(PASSES == 1 || EPI_ROWS == BM / WM, "epilogue passes");
  static_assert(EPI_ROWS * BN * 4 <= 2 * STAGE * 2 && GROUPS * BN * 4 <= 2 * STAGE * 2, "epilogue LDS");
  static_assert(BN <= THREADS && EPI_ROWS % GROUPS == 0, "column sums");
};
using Tile64 = GemmTile<64, 128, 2, 2>;
using Tile128 = GemmTile<128, 128, 2, 2>;
using Tile256 = GemmTile<256, 256, 2, 4>;

// H16<BF> (cvt16.h) with the type's MFMA on packed words
template <bool BF>
struct Cg16;
template <>
struct Cg16<false> : hctr::H16<false> {
  __device__ __forceinline__ static cg_f32x16 mfma(cg_u32x4 a, cg_u32x4 b, cg_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<cg_f16x8*>(&a),
                                                  *reinterpret_cast<cg_f16x8*>(&b), c, 0, 0, 0);
  }
};
template <>
struct Cg16<true> : hctr::H16<true> {
  __device__ __forceinline__ static cg_f32x16 mfma(cg_u32x4 a, cg_u32x4 b, cg_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<cg_bf16x8*>(&a),
                                                   *reinterpret_cast<cg_bf16x8*>(&b), c, 0, 0, 0);
  }
};

// 16 bytes per lane from global memory straight into LDS: lane l's bytes land at lds + 16 l
__device__ __forceinline__ void cg_load_lds16(const unsigned short* g, unsigned short* lds_wave_base) {
  HCTR_GLOBAL_LOAD_LDS16(g, lds_wave_base);
}

struct GemmArgs {
  int M, N, K;
  const unsigned short* A;   // [M][lda]
  const unsigned short* Bt;  // [N][ldb]
  unsigned short* C;         // [M][ldc]
  int lda, ldb, ldc;
  const unsigned short* bias;  // EPI_CROSS: [N] (16-bit)
  const unsigned short* X0;    // EPI_CROSS: [M][ldc]
  const unsigned short* XL;    // EPI_CROSS: [M][ldc]; EPI_RESIDUAL: R [M][ldc]; EPI_DRELU: y [M][ldc]
  unsigned short* H;           // EPI_CROSS: [M][ldc]; EPI_DRELU: the partial rows, fp32 [tiles_m][N]
  int tiles_n;                 // N / BN
  int tiles_m;                 // ceil(M / BM)
};

// rows [row0, row0 + ROWS) x K step k0 of a row-major matrix into an LDS tile image (see the
// header): ROWS / 8 DMA instructions of 8 rows each, spread over the NW wavefronts
template <int ROWS, int NW>
__device__ __forceinline__ void cg_stage(const unsigned short* __restrict__ src, int ld, int row0,
                                         int rows_total, int k0, unsigned short* tile, int wave,
                                         int lane) {
  constexpr int PER_WAVE = ROWS / 8 / NW;  // DMA instructions per wavefront
  static_assert(ROWS % (8 * NW) == 0, "tile rows");
#pragma unroll
  for (int j = 0; j < PER_WAVE; j++) {
    const int r8 = (wave * PER_WAVE + j) * 8;  // first row of this instruction's 8 (tile-local)
    const int r = r8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);  // the chunk this lane's LDS position holds
    int gr = row0 + r;
    gr = gr < rows_total ? gr : rows_total - 1;  // (rows past the end: a legal read, never stored)
    cg_load_lds16(src + (size_t)gr * ld + k0 + c * 8, tile + (size_t)r8 * kGemmBK);
  }
}

// block id -> tile: XCD x takes row panels x, x + 8, ...; a panel's column tiles are consecutive
// blocks of that XCD
__device__ __forceinline__ void cg_tile_of_block(int b, int tiles_m, int tiles_n, int& tile_m,
                                                 int& tile_n) {
  if ((tiles_m & 7) == 0) {
    const int xcd = b & 7, slot = b >> 3;  // slot-th block of this XCD
    tile_m = (slot / tiles_n) * 8 + xcd;
    tile_n = slot % tiles_n;
  } else {  // (panel count not a multiple of 8: plain row-major order)
    tile_m = b / tiles_n;
    tile_n = b % tiles_n;
  }
}

// one K step of a wavefront: the tile images at / bt (row r, logical 16-byte chunk c at
// (r, c ^ ((r >> 1) & 7))) times each other into the wavefront's MI x NJ accumulators; arow / brow =
// this lane's fragment row of the wavefront's first MFMA tile
template <class H16, int MI, int NJ>
__device__ __forceinline__ void cg_mfma_step(const unsigned short* at, const unsigned short* bt,
                                             int arow, int brow, int fk, cg_f32x16 (&acc)[MI][NJ]) {
#pragma unroll
  for (int s = 0; s < kGemmBK / 16; s++) {
    cg_u32x4 af[MI], bf[NJ];
#pragma unroll
    for (int i = 0; i < MI; i++) {
      const int r = arow + i * 32;
      const int c = (2 * s + fk) ^ ((r >> 1) & 7);
      af[i] = *reinterpret_cast<const cg_u32x4*>(at + r * kGemmBK + c * 8);
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int r = brow + j * 32;
      const int c = (2 * s + fk) ^ ((r >> 1) & 7);
      bf[j] = *reinterpret_cast<const cg_u32x4*>(bt + r * kGemmBK + c * 8);
    }
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) acc[i][j] = H16::mfma(af[i], bf[j], acc[i][j]);
  }
}

// element e of the eight 16-bit values of a 16-byte epilogue operand
__device__ __forceinline__ unsigned short cg_elem(cg_u32x4 v, int e) {
  return (unsigned short)(v[e >> 1] >> ((e & 1) * 16));
}

// tile kt has landed once at most `behind` (the tiles after it that were issued) x the wave's DMA
// instructions per tile are still out; the immediate has to be a literal
#define CG_WAIT_BEHIND(behind, one, two)            \
  do {                                              \
    if ((behind) >= 2) HCTR_WAIT_VMCNT(two);        \
    else if ((behind) == 1) HCTR_WAIT_VMCNT(one);   \
    else HCTR_WAIT_VMCNT(0);                        \
  } while (0)

template <class T, bool BF, int EPI, int STAGES>
__global__ void __launch_bounds__(T::THREADS)
    cross_gemm_nt16_kernel(GemmArgs g) {
  using H16 = Cg16<BF>;
  constexpr int BM = T::BM, BN = T::BN, MI = T::MI, NJ = T::NJ, NCH = T::NCH;
  static_assert(T::DMAS == 8 || T::DMAS == 6, "counted waits below");
  // one object for all of it (a second __shared__ array makes hipcc drain the DMA queue before
  // every LDS read): the staging ring, reused by the epilogue as [EPI_ROWS][BN] fp32
  HCTR_DYN_LDS16(unsigned char, lds_raw);
  unsigned short* lds = reinterpret_cast<unsigned short*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / T::WN, wn = wave % T::WN;
  int tile_m, tile_n;
  cg_tile_of_block(blockIdx.x, g.tiles_m, g.tiles_n, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int KT = g.K / kGemmBK;

  cg_f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  const int fr = lane & 31, fk = lane >> 5;
  auto stage_tile = [&](int kt) {
    unsigned short* buf = lds + (kt % STAGES) * T::STAGE;
    cg_stage<BM, T::WAVES>(g.A, g.lda, m0, g.M, kt * kGemmBK, buf, wave, lane);
    cg_stage<BN, T::WAVES>(g.Bt, g.ldb, n0, g.N, kt * kGemmBK, buf + T::A_TILE, wave, lane);
  };
  stage_tile(0);  // (K >= 64, the host checks it: unconditional, so the accumulator clear overlaps it)
#pragma unroll
  for (int p = 1; p < STAGES - 1; p++)
    if (p < KT) stage_tile(p);
  for (int kt = 0; kt < KT; kt++) {
    // every wave waits for its own loads of tile kt, the barrier makes it everybody's
    const int behind = (KT - 1 - kt) < (STAGES - 2) ? (KT - 1 - kt) : (STAGES - 2);
    if constexpr (STAGES == 2) HCTR_WAIT_VMCNT(0);
    else if constexpr (T::DMAS == 8) CG_WAIT_BEHIND(behind, 8, 16);
    else CG_WAIT_BEHIND(behind, 6, 12);
    HCTR_RAW_BARRIER();  // (also: everybody is done reading the buffer tile kt + STAGES - 1 takes)
    if (kt + STAGES - 1 < KT) stage_tile(kt + STAGES - 1);
    const unsigned short* at = lds + (kt % STAGES) * T::STAGE;
    cg_mfma_step<H16>(at, at + T::A_TILE, wm * (BM / T::WM) + fr, wn * (BN / T::WN) + fr, fk, acc);
  }
  // ---- epilogue: accumulators -> LDS [EPI_ROWS][BN] fp32 -> row-contiguous 16-byte stores, pass
  //      by pass (the wavefronts that hold the pass's rows store, all threads write out) ----------
  // What a pass reads from memory (X_0, X_l / the residual / y, the bias) is requested FIRST, all
  // chunks of this thread at once: one trip that overlaps the accumulators' way through LDS (a
  // load -> wait -> store chain per chunk was measured at 8 dependent trips, 4 x the K loop of a
  // K = 512 product).  Raw barriers: they do not wait for these loads (no DMA is outstanding any
  // more: the last K step waited for all of it).
  float* ct = reinterpret_cast<float*>(lds_raw);
  const int cc = tid % T::CPR, rg = tid / T::CPR;  // this thread's column chunk and row group
  const int gn = n0 + cc * 8;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // EPI_DRELU: this thread's column sums
#pragma unroll 1
  for (int p = 0; p < T::PASSES; p++) {
    const int pm0 = m0 + p * T::EPI_ROWS;
    cg_u32x4 ex0[NCH], exl[NCH], bv;
    if constexpr (EPI != kEpiPlain) {
#pragma unroll
      for (int i = 0; i < NCH; i++) {
        int gm = pm0 + (i * T::THREADS + tid) / T::CPR;
        gm = gm < g.M ? gm : g.M - 1;  // (clamped: a legal read; the store below is predicated)
        const size_t off = (size_t)gm * g.ldc + gn;
        exl[i] = *reinterpret_cast<const cg_u32x4*>(g.XL + off);
        if constexpr (EPI == kEpiCross) ex0[i] = *reinterpret_cast<const cg_u32x4*>(g.X0 + off);
      }
      if constexpr (EPI == kEpiCross) bv = *reinterpret_cast<const cg_u32x4*>(g.bias + gn);
    }
    HCTR_RAW_BARRIER();  // (the K loop's / the previous pass's reads of the buffer are done)
    if (T::PASSES == 1 || wm == p) {
#pragma unroll
      for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = wm * (BM / T::WM) % T::EPI_ROWS + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
            const int col = wn * (BN / T::WN) + j * 32 + fr;
            ct[row * BN + col] = acc[i][j][r];
          }
    }
    HCTR_RAW_BARRIER();
#pragma unroll
    for (int i = 0; i < NCH; i++) {
      const int row = (i * T::THREADS + tid) / T::CPR;
      const int gm = pm0 + row;
      const cg_f32x4 v0 = *reinterpret_cast<const cg_f32x4*>(ct + row * BN + cc * 8);
      const cg_f32x4 v1 = *reinterpret_cast<const cg_f32x4*>(ct + row * BN + cc * 8 + 4);
      const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      const size_t off = (size_t)gm * g.ldc + gn;
      unsigned short o[8];
      if constexpr (EPI == kEpiPlain) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = H16::from_f32(v[e]);
      } else if constexpr (EPI == kEpiResidual) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = H16::from_f32(v[e] + H16::to_f32(cg_elem(exl[i], e)));
      } else if constexpr (EPI == kEpiDrelu) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
          o[e] = H16::to_f32(cg_elem(exl[i], e)) > 0.f ? H16::from_f32(v[e])
                                                       : (unsigned short)0;  // (a NaN y masks)
          if (gm < g.M) cs[e] += H16::to_f32(o[e]);  // (as stored; rows past M add nothing)
        }
      } else {
        unsigned short h[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          h[e] = H16::from_f32(v[e] + H16::to_f32(cg_elem(bv, e)));
          o[e] = H16::from_f32(H16::to_f32(cg_elem(exl[i], e)) +
                               H16::to_f32(cg_elem(ex0[i], e)) * H16::to_f32(h[e]));
        }
        cg_u32x4 hv;
#pragma unroll
        for (int e = 0; e < 4; e++) hv[e] = pack16(h[2 * e], h[2 * e + 1]);
        if (gm < g.M) *reinterpret_cast<cg_u32x4*>(g.H + off) = hv;
      }
      cg_u32x4 ov;
#pragma unroll
      for (int e = 0; e < 4; e++) ov[e] = pack16(o[2 * e], o[2 * e + 1]);
      if (gm < g.M) *reinterpret_cast<cg_u32x4*>(g.C + off) = ov;
    }
  }
  if constexpr (EPI == kEpiDrelu) {
    // column sums of the tile: a thread summed rows rg, rg + GROUPS, ... of every pass for its column
    // chunk (in that order); the row groups meet in LDS ([GROUPS][BN] fp32, the image above is read
    // out) and are added in group order
    HCTR_RAW_BARRIER();
    const cg_f32x4 s0 = {cs[0], cs[1], cs[2], cs[3]}, s1 = {cs[4], cs[5], cs[6], cs[7]};
    *reinterpret_cast<cg_f32x4*>(ct + rg * BN + cc * 8) = s0;
    *reinterpret_cast<cg_f32x4*>(ct + rg * BN + cc * 8 + 4) = s1;
    HCTR_RAW_BARRIER();
    if (tid < BN) {
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < T::GROUPS; k++) sum += ct[k * BN + tid];
      reinterpret_cast<float*>(g.H)[(size_t)tile_m * g.N + n0 + tid] = sum;
    }
  }
}

#undef CG_WAIT_BEHIND

// one tile of 32 x 32 (origin r0, c0) of a [rows][cols] matrix, whose 16-bit element (r, c) is
// load(r, c), through LDS to dst_t [cols][rows] (nullptr: nothing is stored); 256 threads as 32 x 8
template <class Load>
__device__ __forceinline__ void transpose16_tile(int rows, int cols, int r0, int c0,
                                                 unsigned short* __restrict__ dst_t, Load load) {
  __shared__ unsigned short tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + 8 * k][tx] = load(r, c);
  }
  __syncthreads();
  if (dst_t == nullptr) return;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;
    if (r < rows && c < cols) dst_t[(size_t)c * rows + r] = tile[tx][ty + 8 * k];
  }
}

// fp32 master weights [batch][rows][cols] -> the 16-bit copy as it lies AND its transpose
// [batch][cols][rows] in one pass (the forward wants both operands K-contiguous, the backward takes
// the weights as they lie; torch's generic transpose was 28 us per tensor at the MLPerf size)
template <bool BF>
__global__ void __launch_bounds__(256)
    convert_transpose16_kernel(int rows, int cols, const float* __restrict__ src,
                               unsigned short* __restrict__ dst, unsigned short* __restrict__ dst_t) {
  const size_t base = (size_t)blockIdx.z * rows * cols;
  transpose16_tile(rows, cols, blockIdx.y * 32, blockIdx.x * 32, dst_t ? dst_t + base : nullptr,
                   [&](int r, int c) {
                     const size_t at = base + (size_t)r * cols + c;
                     const unsigned short v = Cg16<BF>::from_f32(src[at]);
                     if (dst != nullptr) dst[at] = v;
                     return v;
                   });
}

// The 16-bit weights W [rows][cols] of several layers -> their transposes [cols][rows], one launch:
// a block of 256 threads moves one tile of 32 x 32 of the segment it falls into (the table is a
// handful of segments: a linear search)
__global__ void __launch_bounds__(256)
    transpose16_segments_kernel(const hctr_transpose16_seg* __restrict__ segs, int nseg) {
  int si = 0;
  while (si + 1 < nseg && (int64_t)blockIdx.x >= segs[si + 1].block0) si++;
  const hctr_transpose16_seg sg = segs[si];
  const unsigned short* __restrict__ src = reinterpret_cast<const unsigned short*>(sg.src);
  const int rows = (int)sg.rows, cols = (int)sg.cols;
  const int blk = (int)((int64_t)blockIdx.x - sg.block0), tiles_c = (cols + 31) / 32;
  transpose16_tile(rows, cols, blk / tiles_c * 32, blk % tiles_c * 32,
                   reinterpret_cast<unsigned short*>(sg.dst),
                   [&](int r, int c) { return src[(size_t)r * cols + c]; });
}

template <class T, bool BF, int EPI, int STAGES>
int gemm_launch_one(const GemmArgs& g, hipStream_t s) {
  constexpr int lds = T::lds_bytes(STAGES);
  if (lds > 65536)  // (above 64 KB the kernel has to be told -- per device, so on every launch)
    HCTR_HIP(hipFuncSetAttribute((const void*)cross_gemm_nt16_kernel<T, BF, EPI, STAGES>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((cross_gemm_nt16_kernel<T, BF, EPI, STAGES>),
                     dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(T::THREADS), lds, s, g);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace
}  // namespace hctr

using namespace hctr;

// tile height a product is launched with: 256 = the 256 x 256 kernel (plain and dReLU epilogues).
// HCTR_GEMM_BM = 64 / 128 / 256 forces one (measurements; 256 only where that kernel is legal)
static int gemm_tile_height(size_t m, int n, int epilogue) {
  const char* bm_env = getenv("HCTR_GEMM_BM");
  // products with at least a tile of 256 x 256 per CU: half the L2 -> LDS traffic per flop
  const size_t tiles256 = ceil_div<size_t>(m, 256) * (size_t)(n / 256);
  // (dReLU at N = 256: 128-row tiles measured 16.5 us against 19.0 at M = 65536, K = 128 -- the
  //  epilogue's y read and dz store are most of that kernel; from N = 512 on the 256-row kernel
  //  ties or wins, profiles/dgrad_relu_shapes.txt)
  const bool big_auto = tiles256 >= 256 && (epilogue != kEpiDrelu || n >= 512);
  if ((epilogue == kEpiPlain || epilogue == kEpiDrelu) && n % 256 == 0 &&
      (bm_env ? atoi(bm_env) == 256 : big_auto))
    return 256;
  // 128-row tiles while they give every CU two workgroups, 64-row tiles for the small products
  // (B = 8192 x N = 512: 256 tiles of 128 rows = one per CU, nothing to overlap a barrier with)
  const size_t tiles128 = ceil_div<size_t>(m, 128) * (size_t)(n / kGemmBN);
  return (bm_env ? atoi(bm_env) == 64 : tiles128 < 512) ? 64 : 128;
}

// what both entry points ask of a product.  `extra`: the epilogue's operands, each with whether
// this epilogue needs it (`missing` is the message when one of those is null)
struct GemmOperand {
  const void* p;
  bool needed;
};
static int gemm_nt16_check(size_t m, int n, int k, const void* a, int lda, const void* bt, int ldb,
                           const void* c, int ldc, int dtype, const char* missing,
                           std::initializer_list<GemmOperand> extra) {
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "gemm_nt16: 16-bit types only");
  if (m == 0) return HCTR_OK;
  HCTR_REQUIRE(a && bt && c, "null pointer");
  HCTR_REQUIRE(n > 0 && k > 0 && n % kGemmBN == 0 && k % kGemmBK == 0,
               "gemm_nt16: N % 128 == 0 and K % 64 == 0");
  HCTR_REQUIRE(lda >= k && ldb >= k && ldc >= n && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0,
               "gemm_nt16: leading dimensions (multiples of 8 elements)");
  HCTR_REQUIRE(m <= (size_t)0x7FFFFF00, "gemm_nt16: M");
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };  // (null passes)
  bool aligned = al16(a) && al16(bt) && al16(c), there = true;
  for (const GemmOperand& o : extra) {
    aligned = aligned && al16(o.p);
    there = there && (o.p != nullptr || !o.needed);
  }
  HCTR_REQUIRE(aligned, "gemm_nt16: 16-byte aligned buffers");
  HCTR_REQUIRE(there, missing);
  return HCTR_OK;
}

// (arguments checked; h_out: H of the cross epilogue, the partial rows of the dReLU epilogue)
static int gemm_nt16_launch(size_t m, int n, int k, const void* a, int lda, const void* bt, int ldb,
                            void* c, int ldc, int epilogue, const void* bias, const void* x0,
                            const void* xl, void* h_out, int dtype, hctr_stream_t stream) {
  GemmArgs g;
  g.M = (int)m;
  g.N = n;
  g.K = k;
  g.A = (const unsigned short*)a;
  g.Bt = (const unsigned short*)bt;
  g.C = (unsigned short*)c;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.bias = (const unsigned short*)bias;
  g.X0 = (const unsigned short*)x0;
  g.XL = (const unsigned short*)xl;
  g.H = (unsigned short*)h_out;
  hipStream_t s = as_stream(stream);
  const bool bf = dtype == HCTR_EMB_BF16;
  const int bm = gemm_tile_height(m, n, epilogue);
  g.tiles_m = (int)ceil_div<size_t>(m, (size_t)bm);
  g.tiles_n = n / (bm == 256 ? Tile256::BN : kGemmBN);
  // depth of the staging ring (HCTR_GEMM_STAGES: 2 / 3 / 4, measurements): the 256 x 256 tile has
  // LDS for two buffers, 128 rows for three (4 x 32 KB + nothing else: 128 KB of the CU's 160)
  const char* st_env = getenv("HCTR_GEMM_STAGES");
  int stages = st_env ? atoi(st_env) : 2;
  if (stages != 3 && stages != 4) stages = 2;
  if (bm == 256) stages = 2;
  if (bm == 128 && stages == 4) stages = 3;
  // every instantiation that can be launched, and no other
#define CG_CASE(T, STAGES, EPI)                                 \
  case (T::BM * 8 + STAGES) * 4 + EPI:                          \
    return bf ? gemm_launch_one<T, true, EPI, STAGES>(g, s)     \
              : gemm_launch_one<T, false, EPI, STAGES>(g, s);
#define CG_CASES(T, STAGES)                                     \
  CG_CASE(T, STAGES, kEpiPlain) CG_CASE(T, STAGES, kEpiCross)   \
  CG_CASE(T, STAGES, kEpiResidual) CG_CASE(T, STAGES, kEpiDrelu)
  switch ((bm * 8 + stages) * 4 + epilogue) {
    CG_CASES(Tile64, 2) CG_CASES(Tile64, 3) CG_CASES(Tile64, 4)
    CG_CASES(Tile128, 2) CG_CASES(Tile128, 3)
    CG_CASE(Tile256, 2, kEpiPlain) CG_CASE(Tile256, 2, kEpiDrelu)
  }
#undef CG_CASES
#undef CG_CASE
  set_error("gemm_nt16: no kernel for this tile height, ring depth and epilogue");
  return HCTR_ERR_INVALID_ARG;
}

extern "C" {

int hctr_gemm_nt16(size_t m, int n, int k, const void* a, int lda, const void* bt, int ldb, void* c,
                   int ldc, int epilogue, const void* bias, const void* x0, const void* xl,
                   void* h_out, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "gemm_nt16: 16-bit types only");
  HCTR_REQUIRE(epilogue >= kEpiPlain && epilogue <= kEpiResidual, "gemm_nt16: epilogue");
  const bool cross = epilogue == kEpiCross, residual = epilogue == kEpiResidual;  // (plain needs none)
  HCTR_TRY(gemm_nt16_check(
      m, n, k, a, lda, bt, ldb, c, ldc, dtype,
      cross ? "gemm_nt16: cross epilogue operands" : "gemm_nt16: residual operand",
      {{bias, cross}, {x0, cross}, {xl, cross || residual}, {h_out, cross}}));
  if (m == 0) return HCTR_OK;
  return gemm_nt16_launch(m, n, k, a, lda, bt, ldb, c, ldc, epilogue, bias, x0, xl, h_out, dtype,
                          stream);
}

int hctr_gemm_nt16_drelu_tiles(size_t m, int n) {
  HCTR_REQUIRE(n > 0 && n % kGemmBN == 0, "gemm_nt16: N % 128 == 0 and K % 64 == 0");
  HCTR_REQUIRE(m <= (size_t)0x7FFFFF00, "gemm_nt16: M");
  if (m == 0) return 0;
  return (int)ceil_div<size_t>(m, (size_t)gemm_tile_height(m, n, kEpiDrelu));
}

int hctr_gemm_nt16_drelu(size_t m, int n, int k, const void* a, int lda, const void* bt, int ldb,
                         const void* y, void* dz, int ldc, float* partials, int dtype,
                         hctr_stream_t stream) {
  HCTR_TRY(gemm_nt16_check(m, n, k, a, lda, bt, ldb, dz, ldc, dtype, "null pointer",
                           {{y, true}, {partials, true}}));
  if (m == 0) return HCTR_OK;
  return gemm_nt16_launch(m, n, k, a, lda, bt, ldb, dz, ldc, kEpiDrelu, nullptr, nullptr, y, partials,
                          dtype, stream);
}

int hctr_convert_transpose16(size_t batch, int rows, int cols, const float* src, void* dst,
                             void* dst_t, int dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "convert_transpose16: 16-bit types only");
  if (batch == 0 || rows <= 0 || cols <= 0) return HCTR_OK;
  HCTR_REQUIRE(src && (dst || dst_t), "null pointer");
  HCTR_REQUIRE(batch <= 65535, "convert_transpose16: batch");
  const dim3 grid((unsigned)ceil_div(cols, 32), (unsigned)ceil_div(rows, 32), (unsigned)batch);
  if (dtype == HCTR_EMB_BF16)
    hipLaunchKernelGGL(convert_transpose16_kernel<true>, grid, dim3(256), 0, as_stream(stream), rows,
                       cols, src, (unsigned short*)dst, (unsigned short*)dst_t);
  else
    hipLaunchKernelGGL(convert_transpose16_kernel<false>, grid, dim3(256), 0, as_stream(stream), rows,
                       cols, src, (unsigned short*)dst, (unsigned short*)dst_t);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_transpose16_segments(const hctr_transpose16_seg* segs, int nseg, size_t nblocks,
                               hctr_stream_t stream) {
  if (nseg == 0 || nblocks == 0) return HCTR_OK;
  HCTR_REQUIRE(segs && nseg > 0, "transpose16_segments: segment table");
  HCTR_REQUIRE(nblocks <= (size_t)0x7FFFFFFF, "transpose16_segments: blocks");
  hipLaunchKernelGGL(transpose16_segments_kernel, dim3((unsigned)nblocks), dim3(256), 0,
                     as_stream(stream), segs, nseg);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
