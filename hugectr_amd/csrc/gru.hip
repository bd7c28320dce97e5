// gru.hip -- GRULayer<T> (R/HugeCTR/src/layers/gru_layer.cu: a cuDNN GRU, one layer, one direction,
// single input bias, linear input, initial state zero) for gfx950 (wave 64), forward and backward,
// fp32 / fp16 / bf16.  Nothing here is atomic and every grid depends on the shapes alone: two runs
// give the same bits.
//
//   x [S][B][V] -> y [S][B][H]; one flat weight: Wr Wz Wn [H][V], Rr Rz Rn [H][H], br bz bn [H]
//   r = sig(Wr x + Rr h + br)   z = sig(Wz x + Rz h + bz)   n = tanh(Wn x + r o (Rn h) + bn)
//   h_t = (1 - z) o n + z o h_{t-1},  h_0 = 0,  y_t = h_t
// Rows of x and y are addressed as s * stride_s + b * stride_b, so [B][S][.] (batch_first) is read
// and written in place.  Products are summed in fp32, the gates are fp32; the state that enters the
// next step is y_t as stored (fp32: exact; 16-bit: rounded once a step).
//
// ---- tiling ---------------------------------------------------------------------------------------
// Batch rows never meet, so a workgroup of four wavefronts owns a tile of kRows batch rows (32 for the
// 16-bit types, 16 for fp32: one MFMA's rows) for all S steps and walks time by itself; tiles are
// walked grid-stride.  The gate columns are cut into blocks of kCols (32 / 16) and wavefront w owns
// blocks w, w + 4, ..: for each of its blocks it keeps the accumulators of r, z, n_x and n_h (apart,
// because r multiplies n_h only), so the four values of one (row, j) sit in the same lane and
// register and the gates are computed from the registers.  16-bit types run
// v_mfma_f32_32x32x16_{f16,bf16}, fp32 runs v_mfma_f32_16x16x4_f32 on true fp32 operands.
//
// Forward, per time step: a K loop over V ([x_t] against W, into r, z, n_x) and a K loop over H
// ([h_{t-1}] against R, into r, z, n_h), in steps of kStep sum indices (16 / 8: 32 bytes a row).  A
// step's operands -- kStep columns of the 3 Hc weight rows and, in the V loop, of the tile's x rows --
// are fetched by 16-byte global loads (the weights come from L2, where they stay), parked in
// registers under the MFMAs of the step before and stored into the other of two LDS buffers: one
// barrier a step, and the chain of steps runs on across time steps without a bubble.  h is held in
// LDS twice, [2][kRows][Hc + pad] in the operand type: step t reads one copy and its epilogue writes
// the other, which needs no barrier of its own.  Edges in B, V and H are zeros in LDS and are never
// read from memory; a pitch or pointer that is not 16-byte aligned takes element loads into the
// same registers.  When a backward will follow the epilogue stores the reserve, fp32
// [S][B][4][H]: r, z, n and Rn h_{t-1}.
//
// Backward, t = S - 1 .. 0, same tiles: dh is carried in the accumulator registers of the
// dh_{t-1} product (a lane keeps its (row, j) for the whole walk).  Per step each lane forms, for its
// elements, g = dy_t + dh and from the reserve and h_{t-1} = y_{t-1} (0 at t = 0)
//   dn' = g (1 - z)(1 - n^2)   dz' = g (h_{t-1} - n) z (1 - z)   dr' = dn' (Rn h_{t-1}) r (1 - r)
// keeps g z as the carry, writes the four planes [dr' | dz' | dn' | dn' o r] into LDS in the operand
// type and, in fp32, into the gate-gradient scratch [S][B][4][H]; then
//   dx_t      = [dr', dz', dn']     . W   (sum over the gate index: the weight chunk's ROW)
//   dh_{t-1} += [dr', dz', dn' o r] . R
// with kStep weight rows a step through the same two-buffer pipeline.
//
// Two instances, picked by (V, H, dtype) alone (resident<T>()): what is described above is the
// streamed one; in the resident one the weights are loaded once a workgroup and stay in LDS, the
// forward keeps the tile's whole x_t twice, and a time step has one barrier (backward: two).
//
// Weight gradient: dW = sum dGx^T x, dR = sum dGh^T h_{t-1}, db = sum dGx over the S B rows -- a short
// output [3H][V + H + 1] under a long sum.  The rows are cut into slabs whose number depends on the
// shapes alone; a workgroup forms the 64 x 64 fp32-MFMA partial of one output tile over one slab
// (the bias is the column of a ones operand) into scratch, and a finishing kernel adds the partials
// in slab order (runs of 32, then the runs) and rounds once.
#include <type_traits>

#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace gru {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxH = 256, kMaxV = 1024;
constexpr size_t kMaxElems = 0x7FFFFFFF;
constexpr int kTileGrid = 512;  // recurrent kernels: 256 CUs x the two workgroups the resident instance fits
constexpr int kRegs = 8;        // 16-byte chunks a thread parks per K step, at most

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename S, int V>
struct alignas(sizeof(S) * V) Pack {
  S e[V];
};

__host__ __device__ inline int round_up(int v, int to) { return (v + to - 1) / to * to; }

template <typename... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}

// the bits of an element as the kernels move them, and the geometry of the recurrent kernels
template <typename T>
struct Geo {
  static constexpr bool kF32 = std::is_same<T, float>::value;
  using S = std::conditional_t<kF32, float, unsigned short>;
  static constexpr int kVec = 16 / (int)sizeof(S);   // elements in 16 bytes: 4 / 8
  static constexpr int kStep = 2 * kVec;             // sum indices a step: 8 / 16
  static constexpr int kPitch = kStep + kVec;        // a staged row with the sum index contiguous
  static constexpr int kRows = kF32 ? 16 : 32;       // batch rows of a tile
  static constexpr int kCols = kF32 ? 16 : 32;       // columns of an accumulator block
  static constexpr int kGateBlocks = kMaxH / kCols / 4;  // blocks a wavefront, over H: 4 / 2
  static constexpr int kInBlocks = kF32 ? 16 : 4;        // over V (dx), a pass: 64 / 16 registers
};

template <typename T>
__device__ __forceinline__ float bits_f32(typename Geo<T>::S u) {
  return to_f32<T>(*reinterpret_cast<const T*>(&u));
}
template <typename T>
__device__ __forceinline__ typename Geo<T>::S f32_bits(float v) {
  const T h = from_f32<T>(v);
  return *reinterpret_cast<const typename Geo<T>::S*>(&h);
}

// elements k .. k + V - 1 of a row of `ext` elements; no row, or past its end: zeros, and no access
template <typename S, int V>
__device__ __forceinline__ Pack<S, V> load_chunk(const S* __restrict__ row, int ext, int k, bool vec) {
  Pack<S, V> p;
  if (row && vec && k + V <= ext) {
    p = *reinterpret_cast<const Pack<S, V>*>(row + k);
  } else {
#pragma unroll
    for (int e = 0; e < V; e++) p.e[e] = (row && k + e < ext) ? row[k + e] : (S)0;
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

// a wavefront's kRows x kCols block in the accumulator registers of its element type's MFMA; one
// mma() is one K step.  a: [kRows][ap], the sum index contiguous.  b: [kCols][bp] with the sum index
// contiguous (kc) or [kStep][bp] with the sum index the row (kr)
template <typename T>
struct Acc {  // 16-bit: one 32x32x16 accumulator
  static constexpr int kN = 16;
  f32x16 v;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = 0.f;
  }
  // A[i][k]: lane i + 32 (k / 8), element k % 8; B[k][j]: lane j + 32 (k / 8), element k % 8
  __device__ __forceinline__ void mma_kc(const unsigned short* a, int ap, const unsigned short* b,
                                         int bp, int lane) {
    const int i = lane & 31, kh = (lane >> 5) * 8;
    v = mfma16((const T*)nullptr, *reinterpret_cast<const Pack<unsigned short, 8>*>(a + i * ap + kh),
               *reinterpret_cast<const Pack<unsigned short, 8>*>(b + i * bp + kh), v);
  }
  __device__ __forceinline__ void mma_kr(const unsigned short* a, int ap, const unsigned short* b,
                                         int bp, int lane) {
    const int i = lane & 31, kh = (lane >> 5) * 8;
    Pack<unsigned short, 8> pb;
#pragma unroll
    for (int e = 0; e < 8; e++) pb.e[e] = b[(kh + e) * bp + i];
    v = mfma16((const T*)nullptr, *reinterpret_cast<const Pack<unsigned short, 8>*>(a + i * ap + kh),
               pb, v);
  }
  // D[i][j]: lane j + 32 ((i / 4) % 2), register 4 (i / 8) + i % 4
  __device__ __forceinline__ static void pos(int r, int lane, int& i, int& j) {
    i = (r / 4) * 8 + (lane >> 5) * 4 + r % 4;
    j = lane & 31;
  }
};
template <>
struct Acc<float> {  // fp32: one 16x16x4 accumulator, two instructions a step
  static constexpr int kN = 4;
  f32x4 v;
  __device__ __forceinline__ void clear() { v = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // A[i][k]: lane i + 16 k; B[k][j]: lane j + 16 k
  __device__ __forceinline__ void mma_kc(const float* a, int ap, const float* b, int bp, int lane) {
    const int i = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
      v = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i * ap + ks * 4 + kq], b[i * bp + ks * 4 + kq], v, 0,
                                               0, 0);
  }
  __device__ __forceinline__ void mma_kr(const float* a, int ap, const float* b, int bp, int lane) {
    const int i = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
      v = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i * ap + ks * 4 + kq], b[(ks * 4 + kq) * bp + i], v,
                                               0, 0, 0);
  }
  // D[i][j]: lane j + 16 (i / 4), register i % 4
  __device__ __forceinline__ static void pos(int r, int lane, int& i, int& j) {
    i = 4 * (lane >> 4) + r;
    j = lane & 15;
  }
};

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// ================================================================================================
// The two instances
// ================================================================================================
// resident: the concatenated weights [3 Hc][Vc + Hc + pad] (row g Hc + j: W's row, then R's; Vc, Hc
// = V, H rounded up to the block) stay in LDS for the life of the workgroup.  The pad of kVec
// elements makes the pitch an odd number of 16-byte units, so the rows a fragment read touches fall
// on different banks.  Taken when both recurrent kernels then need at most kResidentLds bytes: two
// workgroups a CU.  streamed: everything else.  SMALL (one block a wavefront over H and over V)
// only sizes the register arrays.
constexpr size_t kResidentLds = 80 * 1024;

template <typename T>
size_t fwd_lds(int V, int H, bool res) {
  using G = Geo<T>;
  const int Hc = round_up(H, G::kCols), Vc = round_up(V, G::kCols);
  const size_t h = 2 * G::kRows * (Hc + G::kVec);
  const size_t rest = res ? (size_t)3 * Hc * (Vc + Hc + G::kVec) + 2 * G::kRows * (Vc + G::kVec)
                          : (size_t)2 * (3 * Hc + G::kRows) * G::kPitch;
  return (h + rest) * sizeof(typename G::S);
}
template <typename T>
size_t bwd_lds(int V, int H, bool res) {
  using G = Geo<T>;
  const int Hc = round_up(H, G::kCols), Vc = round_up(V, G::kCols);
  const size_t g = G::kRows * (4 * Hc + G::kVec);
  const size_t rest = res ? (size_t)3 * Hc * (Vc + Hc + G::kVec)
                          : (size_t)2 * G::kStep * ((Vc > Hc ? Vc : Hc) + G::kVec);
  return (g + rest) * sizeof(typename G::S);
}
// the one dispatch rule, of (V, H, dtype) alone
template <typename T>
bool resident(int V, int H) {
  return fwd_lds<T>(V, H, true) <= kResidentLds && bwd_lds<T>(V, H, true) <= kResidentLds;
}
template <typename T>
bool small_shape(int V, int H) {
  return H <= 4 * Geo<T>::kCols && V <= 4 * Geo<T>::kCols;
}

// the resident weights, once a workgroup
template <typename T>
__device__ __forceinline__ void preload_weights(typename Geo<T>::S* wres, const typename Geo<T>::S* wg,
                                                int V, int H, int Vc, int Hc, bool vw, bool vr) {
  using S = typename Geo<T>::S;
  constexpr int VE = Geo<T>::kVec;
  const S* rg = wg + (size_t)3 * H * V;
  const int Kp = Vc + Hc + VE, cpr = (Vc + Hc) / VE;
  for (int q = threadIdx.x; q < 3 * Hc * cpr; q += kThreads) {
    const int row = q / cpr, col = (q % cpr) * VE, j = row % Hc, wr = (row / Hc) * H + j;
    const bool inx = col < Vc;
    const S* src = j >= H ? nullptr : inx ? wg + (size_t)wr * V : rg + (size_t)wr * H;
    *reinterpret_cast<Pack<S, VE>*>(wres + row * Kp + col) =
        load_chunk<S, VE>(src, inx ? V : H, inx ? col : col - Vc, inx ? vw : vr);
  }
}

// ================================================================================================
// Forward
// ================================================================================================
// LDS (elements of S): h [2][kRows][Hc + kVec], then
//   streamed: stage [2][3 Hc + kRows][kPitch]; a stage holds the step's kStep columns of the weight
//             rows g Hc + j and then of the tile's x rows
//   resident: weights [3 Hc][Vc + Hc + kVec] | x [2][kRows][Vc + kVec]
// fp32 sums are kept on two levels: every 16 K steps (128 terms) and at the end of each K loop the
// running accumulator is added into a second one, which keeps the chains of additions short
template <typename T, bool RES, bool SMALL>
__global__ __launch_bounds__(kThreads) void gru_fwd_kernel(int B, int S_, int V, int H,
                                                           const T* __restrict__ x, size_t xs,
                                                           size_t xb, const T* __restrict__ w,
                                                           T* __restrict__ y, size_t ys, size_t yb,
                                                           float* __restrict__ reserve, bool vx,
                                                           bool vw, bool vr) {
  using G = Geo<T>;
  using S = typename G::S;
  constexpr int KS = G::kStep, P = G::kPitch, RT = G::kRows, CB = G::kCols, VE = G::kVec;
  constexpr int NB = SMALL ? 1 : G::kGateBlocks;
  constexpr bool TWO = G::kF32;
  HCTR_DYN_LDS16(unsigned char, gru_lds);
  const int Hc = round_up(H, CB), Vc = round_up(V, CB), HP = Hc + VE;
  const int srows = 3 * Hc + RT, nq = 2 * srows;   // streamed: a stage
  const int Kp = Vc + Hc + VE, XP = Vc + VE;       // resident: the pitches of weights and x
  S* hbuf = reinterpret_cast<S*>(gru_lds);
  S* stage = hbuf + 2 * RT * HP;
  S* wres = stage;
  S* xres = wres + 3 * Hc * Kp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = (V + KS - 1) / KS, nk = nv + (H + KS - 1) / KS, ncb = Hc / CB;
  const S* xg = reinterpret_cast<const S*>(x);
  const S* wg = reinterpret_cast<const S*>(w);
  const S* rg = wg + (size_t)3 * H * V;
  const S* bg = rg + (size_t)3 * H * H;
  S* yg = reinterpret_cast<S*>(y);

  // chunk q = thread + 256 u.  streamed: half q & 1 of stage row q >> 1; sel: the weight row g H + j
  // it comes from (>= 0), zeros (-1), or row -2 - sel of the tile's x rows.  resident: chunk
  // q % (Vc / kVec) of x row q / (Vc / kVec) (sel = row, col = first column; -1: none)
  int sel[kRegs], col[kRegs];
#pragma unroll
  for (int u = 0; u < kRegs; u++) {
    const int q = threadIdx.x + u * kThreads;
    if (RES) {
      const int cpx = Vc / VE;
      sel[u] = q < RT * cpx ? q / cpx : -1;
      col[u] = (q % cpx) * VE;
    } else {
      const int row = q >> 1;
      col[u] = (q & 1) * VE;
      if (row < 3 * Hc) sel[u] = row % Hc < H ? (row / Hc) * H + row % Hc : -1;
      else sel[u] = row < srows ? -2 - (row - 3 * Hc) : -1;
    }
  }
  float bias[NB][3];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) {
    const int c = (wave + 4 * nb) * CB + (lane & (CB - 1));
#pragma unroll
    for (int g = 0; g < 3; g++) bias[nb][g] = c < H ? bits_f32<T>(bg[g * H + c]) : 0.f;
  }
  if (RES) preload_weights<T>(wres, wg, V, H, Vc, Hc, vw, vr);  // (the tile's first barrier covers it)

  const int tiles = (B + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int b0 = tile * RT;
    // (the h-operand's pad columns and the rows past B stay zero for the whole walk)
    for (int e = threadIdx.x; e < 2 * RT * HP; e += kThreads) hbuf[e] = (S)0;

    Pack<S, VE> regs[kRegs];
    Acc<T> acc[NB][4];              // r, z, n_x, n_h
    Acc<T> hi[TWO ? NB : 1][4];     // (fp32) their second level
    auto begin_t = [&]() {
#pragma unroll
      for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          acc[nb][g].clear();
          if (TWO) hi[nb][g].clear();
        }
    };
    // K step s of time step t: a [kRows][ap] the x or h columns, b the weights' columns of the step
    auto step = [&](int s, const S* a, int ap, const S* b, int bp) {
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const int cb = wave + 4 * nb;
        if (cb >= ncb) continue;  // (wave-uniform)
        acc[nb][0].mma_kc(a, ap, b + (cb * CB) * bp, bp, lane);
        acc[nb][1].mma_kc(a, ap, b + (Hc + cb * CB) * bp, bp, lane);
        if (s < nv) acc[nb][2].mma_kc(a, ap, b + (2 * Hc + cb * CB) * bp, bp, lane);
        else acc[nb][3].mma_kc(a, ap, b + (2 * Hc + cb * CB) * bp, bp, lane);
        if (TWO && ((s & 15) == 15 || s == nv - 1 || s == nk - 1)) {
#pragma unroll
          for (int g = 0; g < 4; g++) {
            hi[TWO ? nb : 0][g].v += acc[nb][g].v;
            acc[nb][g].clear();
          }
        }
      }
    };
    // the gates, from the registers; the new state into the other copy of h
    auto epilogue = [&](int t) {
      const S* hcur = hbuf + (t & 1) * RT * HP;
      S* hnext = hbuf + ((t + 1) & 1) * RT * HP;
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const int cb = wave + 4 * nb;
        if (cb >= ncb) continue;
        const Acc<T>* sum = TWO ? hi[TWO ? nb : 0] : acc[nb];
#pragma unroll
        for (int r = 0; r < Acc<T>::kN; r++) {
          int i, j;
          Acc<T>::pos(r, lane, i, j);
          const int c = cb * CB + j, b = b0 + i;
          if (c >= H || b >= B) continue;
          const float rr = sigmoid(sum[0].v[r] + bias[nb][0]);
          const float zz = sigmoid(sum[1].v[r] + bias[nb][1]);
          const float nh = sum[3].v[r];
          const float nn = tanhf(sum[2].v[r] + bias[nb][2] + rr * nh);
          const float hp = bits_f32<T>(hcur[i * HP + c]);
          const S hb = f32_bits<T>((1.f - zz) * nn + zz * hp);
          hnext[i * HP + c] = hb;
          yg[(size_t)t * ys + (size_t)b * yb + c] = hb;
          if (reserve) {
            float* rp = reserve + ((size_t)t * B + b) * 4 * H + c;
            rp[0] = rr;
            rp[H] = zz;
            rp[2 * H] = nn;
            rp[3 * H] = nh;
          }
        }
      }
    };

    if (RES) {
      auto fetch_x = [&](int t) {
#pragma unroll
        for (int u = 0; u < kRegs; u++) {
          if (sel[u] < 0) continue;
          const bool live = b0 + sel[u] < B;
          regs[u] = load_chunk<S, VE>(live ? xg + (size_t)t * xs + (size_t)(b0 + sel[u]) * xb : nullptr,
                                      V, col[u], vx);
        }
      };
      auto park_x = [&](int buf) {
#pragma unroll
        for (int u = 0; u < kRegs; u++)
          if (sel[u] >= 0)
            *reinterpret_cast<Pack<S, VE>*>(xres + buf * RT * XP + sel[u] * XP + col[u]) = regs[u];
      };
      fetch_x(0);
      park_x(0);
      __syncthreads();
      for (int t = 0; t < S_; t++) {
        if (t + 1 < S_) fetch_x(t + 1);  // in flight under this time step's MFMAs
        const S* xcur = xres + (t & 1) * RT * XP;
        const S* hcur = hbuf + (t & 1) * RT * HP;
        begin_t();
        for (int s = 0; s < nv; s++) step(s, xcur + s * KS, XP, wres + s * KS, Kp);
        for (int s = nv; s < nk; s++) step(s, hcur + (s - nv) * KS, HP, wres + Vc + (s - nv) * KS, Kp);
        epilogue(t);
        if (t + 1 < S_) park_x((t + 1) & 1);  // (that copy was last read before the last barrier)
        __syncthreads();
      }
    } else {
      auto fetch = [&](int t, int s) {
        const bool inx = s < nv;
        const int k0 = (inx ? s : s - nv) * KS;
#pragma unroll
        for (int u = 0; u < kRegs; u++) {
          if (threadIdx.x + u * kThreads >= nq) continue;
          const S* row = nullptr;
          bool vec = false;
          if (sel[u] >= 0) {
            row = inx ? wg + (size_t)sel[u] * V : rg + (size_t)sel[u] * H;
            vec = inx ? vw : vr;
          } else if (sel[u] <= -2 && inx && b0 + (-2 - sel[u]) < B) {
            row = xg + (size_t)t * xs + (size_t)(b0 + (-2 - sel[u])) * xb;
            vec = vx;
          }
          regs[u] = load_chunk<S, VE>(row, inx ? V : H, k0 + col[u], vec);
        }
      };
      auto park = [&](int buf) {
        S* st = stage + buf * srows * P;
#pragma unroll
        for (int u = 0; u < kRegs; u++) {
          const int q = threadIdx.x + u * kThreads;
          if (q < nq) *reinterpret_cast<Pack<S, VE>*>(st + (q >> 1) * P + col[u]) = regs[u];
        }
      };
      const long long total = (long long)S_ * nk;
      fetch(0, 0);
      park(0);
      __syncthreads();
      int t = 0, s = 0;
      for (long long it = 0; it < total; it++) {
        const int sn = s + 1 < nk ? s + 1 : 0, tn = sn ? t : t + 1;
        if (it + 1 < total) fetch(tn, sn);  // in flight under this step's MFMAs
        const S* st = stage + (int)(it & 1) * srows * P;
        if (s == 0) begin_t();
        if (s < nv) step(s, st + 3 * Hc * P, P, st, P);
        else step(s, hbuf + (t & 1) * RT * HP + (s - nv) * KS, HP, st, P);
        if (s == nk - 1) epilogue(t);
        if (it + 1 < total) park((int)((it + 1) & 1));  // (last read before the last barrier)
        __syncthreads();
        t = tn;
        s = sn;
      }
    }
  }
}

// ================================================================================================
// Backward: dx and the gate gradients
// ================================================================================================
// LDS (elements of S): gate gradients [kRows][4 Hc + kVec] (planes dr', dz', dn', dn' o r), then
//   streamed: stage [2][kStep][max(Vc, Hc) + kVec]: kStep rows of one gate's W (Vc columns) or R
//   resident: weights [3 Hc][Vc + Hc + kVec], as the forward's
// dx is formed in passes of NBV blocks a wavefront (16-bit: 4, so V > 512 takes two and streams W
// twice): more would push the accumulators out of the registers.  The gate-gradient arithmetic
// follows the order in which autograd evaluates the same expressions
template <typename T, bool RES, bool SMALL>
__global__ __launch_bounds__(kThreads) void gru_bwd_kernel(int B, int S_, int V, int H,
                                                           const T* __restrict__ w,
                                                           const T* __restrict__ y, size_t ys,
                                                           size_t yb, const float* __restrict__ reserve,
                                                           const T* __restrict__ dy,
                                                           T* __restrict__ dx, size_t xs, size_t xb,
                                                           float* __restrict__ dgates, bool vw,
                                                           bool vr) {
  using G = Geo<T>;
  using S = typename G::S;
  constexpr int KS = G::kStep, RT = G::kRows, CB = G::kCols, VE = G::kVec;
  constexpr int NBH = SMALL ? 1 : G::kGateBlocks, NBV = SMALL ? 1 : G::kInBlocks;
  constexpr bool TWO = G::kF32;
  HCTR_DYN_LDS16(unsigned char, gru_lds);
  const int Hc = round_up(H, CB), Vc = round_up(V, CB), GP = 4 * Hc + VE;
  const int NP = (Vc > Hc ? Vc : Hc) + VE, Kp = Vc + Hc + VE;
  S* gbuf = reinterpret_cast<S*>(gru_lds);
  S* stage = gbuf + RT * GP;
  S* wres = stage;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nk = (H + KS - 1) / KS, nvb = Vc / CB, npass = (nvb + 4 * NBV - 1) / (4 * NBV);
  const int per_t = (3 * npass + 3) * nk;  // K steps: W's three gates a pass, then R's
  const S* wg = reinterpret_cast<const S*>(w);
  const S* rg = wg + (size_t)3 * H * V;
  const S* yg = reinterpret_cast<const S*>(y);
  const S* dyg = reinterpret_cast<const S*>(dy);
  S* dxg = reinterpret_cast<S*>(dx);
  // streamed, chunk u of a thread: row kr of the step's kStep weight rows, 16-byte column chunk cc
  const int kr0 = G::kF32 ? 0 : threadIdx.x >> 7, krs = G::kF32 ? 1 : 2;
  const int cc = G::kF32 ? threadIdx.x : threadIdx.x & 127;
  static_assert(kRegs * (G::kF32 ? 1 : 2) == G::kStep && kMaxV / G::kVec == (G::kF32 ? 256 : 128),
                "eight chunks a thread cover a step's rows");
  if (RES) preload_weights<T>(wres, wg, V, H, Vc, Hc, vw, vr);  // (the tile's first barrier covers it)

  const int tiles = (B + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int b0 = tile * RT;
    // (the planes' pad columns and the rows past B stay zero for the whole walk)
    for (int e = threadIdx.x; e < RT * GP; e += kThreads) gbuf[e] = (S)0;

    Acc<T> carry[NBH];  // dh of the lane's (row, j)
    Acc<T> dha[TWO ? NBH : 1];  // (fp32) the R product's running sum, added into the carry every 16 steps
    Acc<T> dxa[NBV];
#pragma unroll
    for (int nb = 0; nb < NBH; nb++) {
      carry[nb].clear();
      if (TWO) dha[nb].clear();
    }
    // the step's gate gradients, a lane its own (row, j)
    auto gates = [&](int t) {
#pragma unroll
      for (int nb = 0; nb < NBH; nb++) {
        const int cb = wave + 4 * nb;
        if (cb >= Hc / CB) continue;
#pragma unroll
        for (int r = 0; r < Acc<T>::kN; r++) {
          int i, j;
          Acc<T>::pos(r, lane, i, j);
          const int c = cb * CB + j, b = b0 + i;
          if (c >= H || b >= B) continue;
          const size_t row = (size_t)t * B + b;
          const float* rp = reserve + row * 4 * H + c;
          const float rr = rp[0], zz = rp[H], nn = rp[2 * H], nh = rp[3 * H];
          const size_t yo = (size_t)b * yb + c;
          const float g = bits_f32<T>(dyg[(size_t)t * ys + yo]) + carry[nb].v[r];
          const float hp = t > 0 ? bits_f32<T>(yg[(size_t)(t - 1) * ys + yo]) : 0.f;
          carry[nb].v[r] = g * zz;
          const float dn = g * (1.f - zz) * (1.f - nn * nn);
          const float dz = (g * hp - g * nn) * (1.f - zz) * zz;
          const float dr = dn * nh * (1.f - rr) * rr;
          const float dnr = dn * rr;
          S* gp = gbuf + i * GP + c;
          gp[0] = f32_bits<T>(dr);
          gp[Hc] = f32_bits<T>(dz);
          gp[2 * Hc] = f32_bits<T>(dn);
          gp[3 * Hc] = f32_bits<T>(dnr);
          float* dg = dgates + row * 4 * H + c;
          dg[0] = dr;
          dg[H] = dz;
          dg[2 * H] = dn;
          dg[3 * H] = dnr;
        }
      }
    };
    // K step s of a time step: kStep weight rows at b (the sum index is the row, pitch bp; the block's
    // columns start at b + cb kCols)
    auto step = [&](int t, int s, const S* b, int bp) {
      const int p = s / nk, j0 = (s % nk) * KS;
      if (p < 3 * npass) {
        const int pass = p / 3, gate = p % 3;
        const S* a = gbuf + gate * Hc + j0;
        if (gate == 0 && j0 == 0) {
#pragma unroll
          for (int nb = 0; nb < NBV; nb++) dxa[nb].clear();
        }
#pragma unroll
        for (int nb = 0; nb < NBV; nb++) {
          const int cb = wave + 4 * (nb + pass * NBV);
          if (cb < nvb) dxa[nb].mma_kr(a, GP, b + cb * CB, bp, lane);
        }
        if (gate == 2 && j0 + KS >= H) {
#pragma unroll
          for (int nb = 0; nb < NBV; nb++) {
            const int cb = wave + 4 * (nb + pass * NBV);
            if (cb >= nvb) continue;
#pragma unroll
            for (int r = 0; r < Acc<T>::kN; r++) {
              int i, j;
              Acc<T>::pos(r, lane, i, j);
              const int c = cb * CB + j, bb = b0 + i;
              if (c < V && bb < B) dxg[(size_t)t * xs + (size_t)bb * xb + c] = f32_bits<T>(dxa[nb].v[r]);
            }
          }
        }
      } else {
        const int gate = p - 3 * npass;
        const S* a = gbuf + (gate == 2 ? 3 : gate) * Hc + j0;
        const bool flush = TWO && ((s & 15) == 15 || s == per_t - 1);
#pragma unroll
        for (int nb = 0; nb < NBH; nb++) {
          const int cb = wave + 4 * nb;
          if (cb >= Hc / CB) continue;
          if (TWO) dha[nb].mma_kr(a, GP, b + cb * CB, bp, lane);
          else carry[nb].mma_kr(a, GP, b + cb * CB, bp, lane);
          if (flush) {
            carry[nb].v += dha[TWO ? nb : 0].v;
            dha[TWO ? nb : 0].clear();
          }
        }
      }
    };

    if (RES) {
      __syncthreads();
      for (int t = S_ - 1; t >= 0; t--) {
        gates(t);
        __syncthreads();
        for (int s = 0; s < per_t; s++) {
          const int p = s / nk, j0 = (s % nk) * KS;
          const int gate = p < 3 * npass ? p % 3 : p - 3 * npass;
          step(t, s, wres + (gate * Hc + j0) * Kp + (p < 3 * npass ? 0 : Vc), Kp);
        }
        __syncthreads();  // (the next step's gate gradients overwrite what these MFMAs read)
      }
    } else {
      Pack<S, VE> regs[kRegs];
      auto fetch = [&](int s) {
        const int p = s / nk, j0 = (s % nk) * KS, inw = p < 3 * npass;
        const int gate = inw ? p % 3 : p - 3 * npass, N = inw ? V : H;
        const S* base = inw ? wg : rg;
        const bool vec = inw ? vw : vr;
        if (cc * VE >= (inw ? Vc : Hc)) return;
#pragma unroll
        for (int u = 0; u < kRegs; u++) {
          const int j = j0 + kr0 + u * krs;
          regs[u] =
              load_chunk<S, VE>(j < H ? base + (size_t)(gate * H + j) * N : nullptr, N, cc * VE, vec);
        }
      };
      auto park = [&](int s, int buf) {
        if (cc * VE >= (s / nk < 3 * npass ? Vc : Hc)) return;
        S* st = stage + buf * KS * NP + cc * VE;
#pragma unroll
        for (int u = 0; u < kRegs; u++)
          *reinterpret_cast<Pack<S, VE>*>(st + (kr0 + u * krs) * NP) = regs[u];
      };
      const long long total = (long long)S_ * per_t;
      fetch(0);
      park(0, 0);
      __syncthreads();
      int t = S_ - 1, s = 0;
      for (long long it = 0; it < total; it++) {
        const int sn = s + 1 < per_t ? s + 1 : 0;
        if (s == 0) {
          gates(t);
          __syncthreads();
        }
        if (it + 1 < total) fetch(sn);  // in flight under this step's MFMAs
        step(t, s, stage + (int)(it & 1) * KS * NP, NP);
        if (it + 1 < total) park(sn, (int)((it + 1) & 1));  // (last read before the last barrier)
        __syncthreads();
        if (sn == 0) t--;
        s = sn;
      }
    }
  }
}


// ================================================================================================
// Backward: the weight gradient
// ================================================================================================
constexpr int kWgTile = 64;      // output tile of a workgroup (2 x 2 wavefronts of 32 x 32)
constexpr int kWgStep = 16;      // rows of the sum a step
constexpr int kWgPitch = kWgTile + 4;
constexpr int kWgGrid = 1024;
constexpr int kWgItems = 2048;   // (tile, slab) items aimed at
constexpr int kWgSlabRows = 64;  // rows a slab at least

struct WgPlan {
  int ctiles, nt0, nt1, slabs;
  size_t slab_rows;
};
// a function of the shapes alone
WgPlan wg_plan(size_t rows, int V, int H) {
  WgPlan p;
  p.ctiles = ceil_div(3 * H, kWgTile);
  p.nt0 = ceil_div(V + 1, kWgTile);
  p.nt1 = ceil_div(H, kWgTile);
  const size_t tiles = (size_t)p.ctiles * (p.nt0 + p.nt1);
  size_t slabs = ceil_div<size_t>(rows, kWgSlabRows), most = kWgItems / tiles;
  if (most < 1) most = 1;
  if (slabs > most) slabs = most;
  if (slabs < 1) slabs = 1;
  p.slab_rows = ceil_div<size_t>(ceil_div<size_t>(rows, slabs), kWgStep) * kWgStep;
  p.slabs = (int)ceil_div<size_t>(rows, p.slab_rows);
  if (p.slabs < 1) p.slabs = 1;
  return p;
}

// part [slab][3H][V + H + 1]: columns 0 .. V - 1 dW, V .. V + H - 1 dR, V + H db.  An item is one
// 64 x 64 tile of [3H] x [V + 1] (gate gradients dr' dz' dn' against x and a column of ones) or of
// [3H] x [H] (dr' dz' dn' o r against h_{t-1}) over one slab of the S B rows; both operands are kept
// with the sum index as the row, as memory has them.  fp32 MFMA for every element type: the gate
// gradients are fp32
template <typename T>
__global__ __launch_bounds__(kThreads) void gru_wgrad_kernel(int B, size_t rows, int V, int H,
                                                             const T* __restrict__ x, size_t xs,
                                                             size_t xb, const T* __restrict__ y,
                                                             size_t ys, size_t yb,
                                                             const float* __restrict__ dgates,
                                                             float* __restrict__ part, WgPlan plan) {
  __shared__ float4 raw[2 * 2 * kWgStep * kWgPitch / 4];  // [buffer][gates | input][16][64 + 4]
  float* lds = reinterpret_cast<float*>(raw);
  constexpr int kElems = kWgStep * kWgPitch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int kr = threadIdx.x >> 4, e4 = (threadIdx.x & 15) * 4;
  const int tiles = plan.ctiles * (plan.nt0 + plan.nt1), W1 = V + H + 1;
  const size_t items = (size_t)tiles * plan.slabs;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int slab = (int)(item / tiles), tl = (int)(item % tiles);
    const int nt = tl % (plan.nt0 + plan.nt1), c0 = (tl / (plan.nt0 + plan.nt1)) * kWgTile;
    const bool hpart = nt >= plan.nt0;
    const int n0 = (hpart ? nt - plan.nt0 : nt) * kWgTile, N = hpart ? H : V + 1;
    const size_t r0 = (size_t)slab * plan.slab_rows;
    const size_t r1 = r0 + plan.slab_rows < rows ? r0 + plan.slab_rows : rows;
    const int steps = (int)((r1 - r0 + kWgStep - 1) / kWgStep);

    float ra[4], rb[4];
    auto fetch = [&](int st) {
      const size_t row = r0 + (size_t)st * kWgStep + kr;
      const bool live = row < r1;
      const size_t s = row / (size_t)B, b = row % (size_t)B;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int c = c0 + e4 + e, n = n0 + e4 + e;
        ra[e] = live && c < 3 * H ? dgates[row * 4 * H + (hpart && c >= 2 * H ? c + H : c)] : 0.f;
        if (hpart) rb[e] = live && n < H && s > 0 ? to_f32<T>(y[(s - 1) * ys + b * yb + n]) : 0.f;
        else rb[e] = live && n < V ? to_f32<T>(x[s * xs + b * xb + n]) : live && n == V ? 1.f : 0.f;
      }
    };
    auto park = [&](int buf) {
      float* d = lds + buf * 2 * kElems + kr * kWgPitch + e4;
      *reinterpret_cast<float4*>(d) = make_float4(ra[0], ra[1], ra[2], ra[3]);
      *reinterpret_cast<float4*>(d + kElems) = make_float4(rb[0], rb[1], rb[2], rb[3]);
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q / 2][q % 2] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (steps > 0) {
      fetch(0);
      park(0);
    }
    __syncthreads();
    for (int st = 0; st < steps; st++) {
      if (st + 1 < steps) fetch(st + 1);
      const float* as = lds + (st & 1) * 2 * kElems;
      const float* bs = as + kElems;
      const int i = lane & 15, kq = lane >> 4;
#pragma unroll
      for (int ks = 0; ks < kWgStep / 4; ks++) {
        float a[2], b[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
          a[q] = as[(ks * 4 + kq) * kWgPitch + wm * 32 + q * 16 + i];
          b[q] = bs[(ks * 4 + kq) * kWgPitch + wn * 32 + q * 16 + i];
        }
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
          for (int p = 0; p < 2; p++)
            acc[q][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[p], acc[q][p], 0, 0, 0);
      }
      if (st + 1 < steps) park((st + 1) & 1);
      __syncthreads();
    }
    // D[i][j]: lane j + 16 (i / 4), register i % 4
    float* out = part + (size_t)slab * 3 * H * W1;
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int p = 0; p < 2; p++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int c = c0 + wm * 32 + q * 16 + 4 * (lane >> 4) + r;
          const int n = n0 + wn * 32 + p * 16 + (lane & 15);
          if (c < 3 * H && n < N) out[(size_t)c * W1 + (hpart ? V + n : n < V ? n : V + H)] = acc[q][p][r];
        }
  }
}

// dweight (W | R | b, the weight's layout) = the slabs' partials added in slab order, rounded once
template <typename T>
__global__ __launch_bounds__(kThreads) void gru_wgrad_finish_kernel(int V, int H, int slabs,
                                                                    const float* __restrict__ part,
                                                                    T* __restrict__ dw) {
  const int W1 = V + H + 1, n = 3 * H * W1;
  for (int o = blockIdx.x * kThreads + threadIdx.x; o < n; o += gridDim.x * kThreads) {
    float sum = 0.f;  // (on two levels: runs of 32 slabs, then the runs)
    for (int k0 = 0; k0 < slabs; k0 += 32) {
      float run = 0.f;
      for (int k = k0; k < slabs && k < k0 + 32; k++) run += part[(size_t)k * n + o];
      sum += run;
    }
    const int c = o / W1, col = o % W1;
    const size_t at = col < V ? (size_t)c * V + col
                      : col < V + H ? (size_t)3 * H * V + (size_t)c * H + (col - V)
                                    : (size_t)3 * H * (V + H) + c;
    dw[at] = from_f32<T>(sum);
  }
}

// ---- host ----------------------------------------------------------------------------------------
int gru_check(size_t batch, int seq, int vec, int hidden, int dtype) {
  HCTR_REQUIRE(hidden >= 1 && hidden <= kMaxH, "gru: hidden H 1 .. 256");
  HCTR_REQUIRE(vec >= 1 && vec <= kMaxV, "gru: vector size V 1 .. 1024");
  HCTR_REQUIRE(seq >= 1, "gru: seq S >= 1");
  HCTR_REQUIRE(batch <= kMaxElems / ((size_t)seq * (size_t)(vec > hidden ? vec : hidden)),
               "gru: S * B * V and S * B * H < 2^31");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "gru: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}

size_t reserve_bytes(size_t batch, int seq, int hidden) {
  return (size_t)seq * batch * 4 * hidden * sizeof(float);
}
// gate gradients [S][B][4][H], then the weight gradient's partials
size_t scratch_bytes(size_t batch, int seq, int vec, int hidden) {
  if (batch == 0) return 0;
  const WgPlan p = wg_plan((size_t)seq * batch, vec, hidden);
  return reserve_bytes(batch, seq, hidden) +
         (size_t)p.slabs * 3 * hidden * (vec + hidden + 1) * sizeof(float);
}

// a kernel that is launched with more than 64 KB of dynamic LDS has to be told first
template <typename K>
int allow_dyn_lds(K kernel, size_t lds) {
  if (lds > 65536)
    HCTR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  return HCTR_OK;
}

struct Strides {  // of a row (s, b) of x and of y, in elements
  size_t xs, xb, ys, yb;
};
Strides strides(size_t batch, int seq, int vec, int hidden, int batch_first) {
  if (batch_first) return {(size_t)vec, (size_t)seq * vec, (size_t)hidden, (size_t)seq * hidden};
  return {batch * vec, (size_t)vec, batch * hidden, (size_t)hidden};
}

template <typename T>
bool rows_aligned(const void* p, size_t a, size_t b) {
  constexpr size_t VE = Geo<T>::kVec;
  return aligned16(p) && a % VE == 0 && b % VE == 0;
}

int fwd(size_t batch, int seq, int vec, int hidden, int batch_first, const void* x, const void* w,
        void* y, void* reserve, int dtype, hctr_stream_t stream) {
  HCTR_TRY(gru_check(batch, seq, vec, hidden, dtype));
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(x && w && y, "null pointer");
  const Strides st = strides(batch, seq, vec, hidden, batch_first);
  const int V = vec, H = hidden, B = (int)batch;
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using G = Geo<T>;
    const bool res = resident<T>(V, H);
    const size_t lds = fwd_lds<T>(V, H, res);
    int rc = HCTR_OK;
    with_bool(res, [&](auto r) {
      with_bool(small_shape<T>(V, H), [&](auto sm) {
        auto kernel = gru_fwd_kernel<T, decltype(r)::value, decltype(sm)::value>;
        if ((rc = allow_dyn_lds(kernel, lds)) != HCTR_OK) return;
        hipLaunchKernelGGL(kernel, dim3(grid_for(batch, G::kRows, kTileGrid)), dim3(kThreads), lds,
                           as_stream(stream), B, seq, V, H, (const T*)x, st.xs, st.xb, (const T*)w,
                           (T*)y, st.ys, st.yb, (float*)reserve, rows_aligned<T>(x, st.xs, st.xb),
                           rows_aligned<T>(w, V, 0), rows_aligned<T>(w, H, (size_t)3 * H * V));
      });
    });
    return rc;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int bwd(size_t batch, int seq, int vec, int hidden, int batch_first, const void* x, const void* w,
        const void* y, const void* reserve, const void* dy, void* dx, void* dweight, void* scratch,
        int dtype, hctr_stream_t stream) {
  HCTR_TRY(gru_check(batch, seq, vec, hidden, dtype));
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(x && w && y && reserve && dy && dx && dweight && scratch, "null pointer");
  const Strides st = strides(batch, seq, vec, hidden, batch_first);
  const int V = vec, H = hidden, B = (int)batch;
  const size_t rows = (size_t)seq * batch;
  const WgPlan plan = wg_plan(rows, V, H);
  float* dgates = (float*)scratch;
  float* part = dgates + rows * 4 * H;
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using G = Geo<T>;
    const bool res = resident<T>(V, H);
    const size_t lds = bwd_lds<T>(V, H, res);
    int rc = HCTR_OK;
    with_bool(res, [&](auto r) {
      with_bool(small_shape<T>(V, H), [&](auto sm) {
        auto kernel = gru_bwd_kernel<T, decltype(r)::value, decltype(sm)::value>;
        if ((rc = allow_dyn_lds(kernel, lds)) != HCTR_OK) return;
        hipLaunchKernelGGL(kernel, dim3(grid_for(batch, G::kRows, kTileGrid)), dim3(kThreads), lds, s,
                           B, seq, V, H, (const T*)w, (const T*)y, st.ys, st.yb,
                           (const float*)reserve, (const T*)dy, (T*)dx, st.xs, st.xb, dgates,
                           rows_aligned<T>(w, V, 0), rows_aligned<T>(w, H, (size_t)3 * H * V));
      });
    });
    HCTR_TRY(rc);
    const size_t items = (size_t)plan.ctiles * (plan.nt0 + plan.nt1) * plan.slabs;
    hipLaunchKernelGGL(gru_wgrad_kernel<T>, dim3(grid_for(items, 1, kWgGrid)), dim3(kThreads), 0, s,
                       B, rows, V, H, (const T*)x, st.xs, st.xb, (const T*)y, st.ys, st.yb,
                       (const float*)dgates, part, plan);
    hipLaunchKernelGGL(gru_wgrad_finish_kernel<T>,
                       dim3(grid_for((size_t)3 * H * (V + H + 1), kThreads)), dim3(kThreads), 0, s, V,
                       H, plan.slabs, (const float*)part, (T*)dweight);
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace
}  // namespace gru
}  // namespace hctr

extern "C" {

int hctr_gru_workspace(size_t batch, int seq, int vec, int hidden, size_t* reserve_bytes,
                       size_t* scratch_bytes) {
  HCTR_TRY(hctr::gru::gru_check(batch, seq, vec, hidden, HCTR_EMB_F32));
  HCTR_REQUIRE(reserve_bytes && scratch_bytes, "null pointer");
  *reserve_bytes = hctr::gru::reserve_bytes(batch, seq, hidden);
  *scratch_bytes = hctr::gru::scratch_bytes(batch, seq, vec, hidden);
  return HCTR_OK;
}

int hctr_gru_fwd(size_t batch, int seq, int vec, int hidden, int batch_first, const void* x,
                 const void* weight, void* y, void* reserve, int dtype, hctr_stream_t stream) {
  return hctr::gru::fwd(batch, seq, vec, hidden, batch_first, x, weight, y, reserve, dtype, stream);
}

int hctr_gru_bwd(size_t batch, int seq, int vec, int hidden, int batch_first, const void* x,
                 const void* weight, const void* y, const void* reserve, const void* dy, void* dx,
                 void* dweight, void* scratch, int dtype, hctr_stream_t stream) {
  return hctr::gru::bwd(batch, seq, vec, hidden, batch_first, x, weight, y, reserve, dy, dx, dweight,
                        scratch, dtype, stream);
}

}  // extern "C"
