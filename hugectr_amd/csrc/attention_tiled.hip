// attention_tiled.hip -- the second kernel family of multi-head attention: any seq_from, seq_to up to
// 4096 and size_per_head up to 128.  Taken into attention.hip (inside hctr::mha's unnamed namespace,
// after the first family, whose operand and softmax helpers it shares); hctr_mha_tiled_fwd /
// hctr_mha_tiled_bwd.
//
// A workgroup of four wavefronts owns a block of 128 rows of one (sample, head); a wavefront owns 32
// of them and keeps them in REGISTERS as the B-operand fragments of v_mfma_f32_32x32x16 (lane
// (r, h) holds elements 16 t + 8 h .. + 7 of row r), read from HBM once.  The other side streams
// through LDS in tiles of 64 rows, two tensors at a time, double buffered: the next tile's 16-byte
// loads are issued before the current tile's MFMAs and land in LDS after them, one barrier a tile.
// A tile is [64][32 DT + 8] of 16 bits (DT = ceil(d / 32); the + 8 spreads the rows over the
// banks); fp16 / bf16 bits go in as they are, an fp32 value is split into its (hi, lo) bf16 pair
// when the tile is filled and lives in two such planes -- three MFMAs per product, as in the first
// family.  Nothing in LDS or registers depends on seq_from / seq_to.
//
// Two products, two ways to read a tile:
//   * by rows (mma_rows): acc[i][j] = sum_k tile[i][k] b[j][k], A = one 16-byte LDS read.  With the
//     tile as A and the wavefront's own rows as B the result is TRANSPOSED: lane (r, h) holds the 16
//     values of its own row r against tile rows tile_row(reg, h).  Scale, mask, exp, the running
//     max / sum / smallest penalty and every rescaling are then lane-local, with one lane ^ 32
//     exchange per reduction;
//   * transposed (mma_tr): acc[c][j] += sum_i tile[i][c] p[j][i] with p taken straight from those
//     registers (registers 8 t .. 8 t + 7 ARE a B fragment, for the k order i = 16 t + 8 (e >> 2) +
//     4 h + (e & 3)) and A read with ds_read_b64_tr_b16 in the same order (HCTR_LDS_READ_TR16_B64).
//     P and dS never go through LDS, and the result is again per own row: lane (r, h) holds columns
//     32 ct + tile_row(reg, h) of row r, which leave as 8- or 16-byte stores.
//
// Forward, per block of 128 query rows: K and V tiles stream; online softmax per 32 keys:
//   r' = min(r, tile's smallest penalty); the running max moves by r - r' (with 0 / 1 masks that is
//   10000 or nothing, so what was accumulated under the larger penalty is scaled by exp(-10000) = 0);
//   s = q.k / sqrt(d) - (penalty - r'); max' = max(max, s); O, sum *= exp(max - max'); O += P V.
//   The 1e-6 joins the final sum once.  Optionally (max, 1 / (sum + 1e-6), r, -) leave as fp32
//   [B][H][m][4] for the backward.
// Backward, no atomics, two sweeps that both recompute S and dP = dO V^T from the inputs:
//   dq sweep, per block of 128 query rows over K / V tiles: delta = rowsum(dO o O) (fp32, from the
//     fragments as they are loaded; stored in the statistics' fourth slot), dS = P o (dP - delta),
//     dQ += dS K (K tile read transposed);
//   dkv sweep, per block of 128 keys over Q / dO tiles (+ their statistics): K and V rows in
//     registers, dV += P^T dO and dK += dS^T Q with the dO / Q tiles read transposed.
//
// The mask as two lengths (LEN; hctr_mha_tiled_len_fwd / _bwd): the same three bodies.  A workgroup
// reads its sample's two floats (LenBounds: nv valid keys, rows from first_plain on are plain).  A
// row's keys end at nv or, for a plain row, at n; past that end a key is what a key >= n is, and
// the smallest penalty is 0, so nothing is carried for it.  What is skipped:
//   forward, dq sweep: a block streams tiles only up to the largest end among its live rows
//     (ceil(nv / 64) tiles when all of them are valid), a wavefront leaves a tile's 32-key sub-tile
//     that lies past every one of its own rows (KeyEnds);
//   dkv sweep: a block of keys at or past nv is reached by plain rows only and starts at the query
//     tile that holds first_plain; without a plain row it stores zeros and streams nothing.
// Trip counts and barriers depend on the lengths, blockIdx and the shape only; the wavefront's
// skip holds no barrier and no LDS store.

constexpr int kTiledMaxSeq = 4096;
constexpr int kTiledMaxHead = 128;
constexpr int kTiledWaves = 4;
constexpr int kBlockRows = 32 * kTiledWaves;  // rows a workgroup owns
constexpr int kTileRows = 64;                 // rows of a streamed tile
constexpr int kTiledThreads = 64 * kTiledWaves;
typedef unsigned short u16;

// eight 16-bit values down a tile's column, in the k order of mma_tr: rows kr + 8 a + (0 .. 3) for
// a = 0, 1.  tr0: the address this lane supplies to the transposed read of the first four rows,
// e0: the element it receives from row kr
__device__ __forceinline__ u32x4 tr8(const u16* t, int tr0, int e0, int ld) {
  const hctr_u32x2 a = HCTR_LDS_READ_TR16_B64(t, tr0, e0, e0 + ld, e0 + 2 * ld, e0 + 3 * ld);
  const hctr_u32x2 b = HCTR_LDS_READ_TR16_B64(t, tr0 + 8 * ld, e0 + 8 * ld, e0 + 9 * ld,
                                              e0 + 10 * ld, e0 + 11 * ld);
  return (u32x4){a[0], a[1], b[0], b[1]};
}

// Tl<T>: eight elements of T on their way from HBM (raw) into a fragment or a tile, and a tile's
// reads.  fp16 / bf16: the bits as they are, one plane
template <typename T>
struct Tl {
  using frag = typename Op<T>::frag;
  using vec8 = decltype(frag::v);
  static constexpr int kPlanes = 1;
  struct raw {
    u32x4 v;
  };
  __device__ __forceinline__ static raw load8(const T* g) {
    raw r;
    r.v = *reinterpret_cast<const u32x4*>(g);
    return r;
  }
  __device__ __forceinline__ static raw zero8() {
    raw r;
    r.v = (u32x4){0u, 0u, 0u, 0u};
    return r;
  }
  __device__ __forceinline__ static void to_f32(const raw& r, float (&x)[8]) {
    const T* e = reinterpret_cast<const T*>(&r.v);
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = hctr::to_f32<T>(e[i]);
  }
  __device__ __forceinline__ static frag to_frag(const raw& r) {
    frag f;
    f.v = *reinterpret_cast<const vec8*>(&r.v);
    return f;
  }
  __device__ __forceinline__ static void put(u16* t, int plane, int off, const raw& r) {
    *reinterpret_cast<u32x4*>(t + off) = r.v;
  }
  __device__ __forceinline__ static frag get(const u16* t, int plane, int off) {
    raw r;
    r.v = *reinterpret_cast<const u32x4*>(t + off);
    return to_frag(r);
  }
  __device__ __forceinline__ static frag get_tr(const u16* t, int plane, int tr0, int e0, int ld) {
    raw r;
    r.v = tr8(t, tr0, e0, ld);
    return to_frag(r);
  }
};
// fp32: split once into (hi, lo) bf16, a plane each
template <>
struct Tl<float> {
  using frag = Op<float>::frag;
  static constexpr int kPlanes = 2;
  struct raw {
    u32x4 a, b;
  };
  __device__ __forceinline__ static raw load8(const float* g) {
    raw r;
    r.a = *reinterpret_cast<const u32x4*>(g);
    r.b = *reinterpret_cast<const u32x4*>(g + 4);
    return r;
  }
  __device__ __forceinline__ static raw zero8() {
    raw r;
    r.a = r.b = (u32x4){0u, 0u, 0u, 0u};
    return r;
  }
  __device__ __forceinline__ static void to_f32(const raw& r, float (&x)[8]) {
    const float* lo = reinterpret_cast<const float*>(&r.a);
    const float* hi = reinterpret_cast<const float*>(&r.b);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      x[i] = lo[i];
      x[4 + i] = hi[i];
    }
  }
  __device__ __forceinline__ static frag to_frag(const raw& r) {
    float x[8];
    to_f32(r, x);
    return Op<float>::make(x);
  }
  __device__ __forceinline__ static void put(u16* t, int plane, int off, const raw& r) {
    const frag f = to_frag(r);
    *reinterpret_cast<bf16x8*>(t + off) = f.hi;
    *reinterpret_cast<bf16x8*>(t + plane + off) = f.lo;
  }
  __device__ __forceinline__ static frag get(const u16* t, int plane, int off) {
    frag f;
    f.hi = *reinterpret_cast<const bf16x8*>(t + off);
    f.lo = *reinterpret_cast<const bf16x8*>(t + plane + off);
    return f;
  }
  __device__ __forceinline__ static frag get_tr(const u16* t, int plane, int tr0, int e0, int ld) {
    const u32x4 hi = tr8(t, tr0, e0, ld), lo = tr8(t + plane, tr0, e0, ld);
    frag f;
    f.hi = *reinterpret_cast<const bf16x8*>(&hi);
    f.lo = *reinterpret_cast<const bf16x8*>(&lo);
    return f;
  }
};

// the geometry of the tiles for DT 32-wide column tiles of the head (elements of 16 bits)
template <typename T, int DT>
struct TileGeo {
  static constexpr int ld = 32 * DT + 8;                 // row stride
  static constexpr int plane = kTileRows * ld;           // one plane of one tensor's tile
  static constexpr int tile = Tl<T>::kPlanes * plane;    // one tensor's tile
  static constexpr int stage = 2 * tile;                 // the two tensors that stream together
  static constexpr int cpr = 4 * DT;                     // 8-element chunks of a row
  static constexpr int per = kTileRows * cpr / kTiledThreads;  // chunks per thread and tensor
  static constexpr size_t lds_bytes = 2 * stage * sizeof(u16);  // double buffered
};

// the next tile of two tensors x, y (the same rows of both) on its way through registers: rows past
// rows_end and columns past d become the zeros that pad the MFMA's k
template <typename T, int DT>
struct Stage {
  using G = TileGeo<T, DT>;
  typename Tl<T>::raw x[G::per], y[G::per];
  __device__ __forceinline__ void load(const T* __restrict__ gx, const T* __restrict__ gy,
                                       size_t stride, int row0, int rows_end, int d, int tid) {
#pragma unroll
    for (int i = 0; i < G::per; i++) {
      const int idx = tid + kTiledThreads * i, row = row0 + idx / G::cpr, c = (idx % G::cpr) * 8;
      const bool ok = row < rows_end && c < d;
      x[i] = ok ? Tl<T>::load8(gx + row * stride + c) : Tl<T>::zero8();
      y[i] = ok ? Tl<T>::load8(gy + row * stride + c) : Tl<T>::zero8();
    }
  }
  __device__ __forceinline__ void store(u16* stage, int tid) const {
#pragma unroll
    for (int i = 0; i < G::per; i++) {
      const int idx = tid + kTiledThreads * i, off = (idx / G::cpr) * G::ld + (idx % G::cpr) * 8;
      Tl<T>::put(stage, G::plane, off, x[i]);
      Tl<T>::put(stage + G::tile, G::plane, off, y[i]);
    }
  }
};

// the lane's own row as B fragments: f[t] = elements 16 t + 8 h .. + 7 of g (nullptr: a row that
// does not exist, zeros)
template <typename T, int DT>
__device__ __forceinline__ void load_frags(typename Tl<T>::frag (&f)[2 * DT], const T* g, int d,
                                           int h) {
#pragma unroll
  for (int t = 0; t < 2 * DT; t++) {
    const int c = 16 * t + 8 * h;
    f[t] = Tl<T>::to_frag((g && c < d) ? Tl<T>::load8(g + c) : Tl<T>::zero8());
  }
}

// acc[i][j] = sum_k tile[row0 + i][k] b[j][k], k < 16 ksd: lane (r, h) receives its own row j = r
// against tile rows row0 + tile_row(reg, h)
template <typename T, int DT>
__device__ __forceinline__ f32x16 mma_rows(const u16* tile, int row0,
                                           const typename Tl<T>::frag (&b)[2 * DT], int ksd,
                                           int lane) {
  using G = TileGeo<T, DT>;
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2 * DT; t++) {
    if (t < ksd)
      acc = Op<T>::mma(Tl<T>::get(tile, G::plane, (row0 + r) * G::ld + 16 * t + 8 * h), b[t], acc);
  }
  return acc;
}
// acc[ct][c][j] += sum_i tile[row0 + i][32 ct + c] p[j][i], i < 32: p is the lane's own row j = r
// against tile rows row0 + tile_row(reg, h), as mma_rows leaves it; lane (r, h) receives columns
// 32 ct + tile_row(reg, h) of its own row
template <typename T, int DT>
__device__ __forceinline__ void mma_tr(f32x16 (&acc)[DT], const u16* tile, int row0,
                                       const f32x16& p, int lane) {
  using G = TileGeo<T, DT>;
  const int r = lane & 31, h = lane >> 5;
  const int tq = (lane >> 2) & 3, tp = lane & 3, tj = (lane >> 4) & 1;
#pragma unroll
  for (int t = 0; t < 2; t++) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; e++) x[e] = p[8 * t + e];
    const typename Tl<T>::frag pf = Op<T>::make(x);
    const int kr = row0 + 16 * t + 4 * h;
#pragma unroll
    for (int ct = 0; ct < DT; ct++)
      acc[ct] = Op<T>::mma(Tl<T>::get_tr(tile, G::plane, (kr + tq) * G::ld + 32 * ct + 16 * tj + 4 * tp,
                                         kr * G::ld + 32 * ct + r, G::ld),
                           pf, acc[ct]);
  }
}
// g[32 ct + tile_row(reg, h)] <- acc[ct][reg] * scale, columns < d: four consecutive columns a store
// (g: the lane's own row, nullptr for a row that does not exist)
template <typename T, int DT>
__device__ __forceinline__ void store_own_row(T* g, const f32x16 (&acc)[DT], float scale, int d,
                                              int h) {
  if (!g) return;
#pragma unroll
  for (int ct = 0; ct < DT; ct++) {
#pragma unroll
    for (int grp = 0; grp < 4; grp++) {
      const int c = 32 * ct + 8 * grp + 4 * h;
      if (c < d)
        hctr::st4_from_f32<T>(g + c, make_float4(acc[ct][4 * grp] * scale, acc[ct][4 * grp + 1] * scale,
                                                 acc[ct][4 * grp + 2] * scale,
                                                 acc[ct][4 * grp + 3] * scale));
    }
  }
}

// which (sample, head, block of rows) a workgroup owns; blocks of one head are neighbours, so the
// tiles they all stream stay in L2
struct TiledBlock {
  size_t b;   // sample
  int hd;     // head
  int row0;   // first row of the block
  size_t bh;  // b * heads + hd
  __device__ __forceinline__ TiledBlock(int heads, int rows) {
    const int nb = (rows + kBlockRows - 1) / kBlockRows;
    row0 = (int)(blockIdx.x % nb) * kBlockRows;
    bh = blockIdx.x / nb;
    b = bh / heads;
    hd = (int)(bh % heads);
  }
};
// where head hd of sample b starts in a [B, seq, H d] tensor
__device__ __forceinline__ size_t tiled_head_offset(size_t b, int hd, int seq, int heads, int d) {
  return (b * seq * heads + hd) * (size_t)d;
}

__device__ __forceinline__ f32x16 zero_tile() {
  return (f32x16){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// Where the keys end in a block of query rows (forward, dq sweep).  A dense mask: at n, for all.
// LEN: `row` for this lane's own row (LenBounds::key_end), `wave` the largest among the live rows of
// its wavefront, `block` the largest among the block's.  block depends on the sample's two lengths,
// blockIdx and the shape only, so every trip count and barrier taken from it is the same for the
// whole workgroup; wave is the same for the 64 lanes of a wavefront (tid >> 6) and bounds only
// code without a barrier or an LDS store.
template <bool LEN>
struct KeyEnds {
  int row, wave, block;
  __device__ __forceinline__ KeyEnds(const float* len_from, const float* len_to,
                                     const TiledBlock& blk, int m, int n, int tid) {
    row = wave = block = n;
    if (LEN) {
      const LenBounds lb(len_from, len_to, blk.b, m, n);
      const int w0 = blk.row0 + (tid >> 6) * 32;
      row = lb.key_end(w0 + (tid & 31));
      wave = lb.key_end_upto(w0 + 32 < m ? w0 + 32 : m);
      block = lb.key_end_upto(blk.row0 + kBlockRows < m ? blk.row0 + kBlockRows : m);
    }
  }
};

// ================================================================================================
// Forward
// ================================================================================================
// LEN (all three kernels): the mask comes from len_from / len_to (fp32 [B]) and `dense` is not read;
// otherwise from `dense` (or no mask) and the lengths are not read
template <typename T, int DT, bool LEN>
__global__ void __launch_bounds__(kTiledThreads)
    mha_tiled_fwd_kernel(int heads, int m, int n, int d, const T* __restrict__ q,
                         const T* __restrict__ k, const T* __restrict__ v,
                         const T* __restrict__ dense, const float* __restrict__ len_from,
                         const float* __restrict__ len_to, T* __restrict__ out,
                         float* __restrict__ stats, float scale) {
  const T* mask = LEN ? nullptr : dense;
  using G = TileGeo<T, DT>;
  HCTR_DYN_LDS16(u16, tsmem);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const TiledBlock blk(heads, m);
  const size_t stride = (size_t)heads * d;
  const int ksd = (d + 15) / 16;
  const int qrow = blk.row0 + (tid >> 6) * 32 + r;
  const bool live = qrow < m;
  const size_t off_m = tiled_head_offset(blk.b, blk.hd, m, heads, d) + qrow * stride;
  const T* kg = k + tiled_head_offset(blk.b, blk.hd, n, heads, d);
  const T* vg = v + tiled_head_offset(blk.b, blk.hd, n, heads, d);
  const T* mrow = (mask && live) ? mask + (blk.b * m + qrow) * (size_t)n : nullptr;
  const KeyEnds<LEN> ke(len_from, len_to, blk, m, n, tid);

  typename Tl<T>::frag qf[2 * DT];
  load_frags<T, DT>(qf, live ? q + off_m : nullptr, d, h);
  f32x16 o[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ct++) o[ct] = zero_tile();
  float rmax = -INFINITY, rsum = 0.f, rmin = mask ? INFINITY : 0.f;  // (rsum: this lane's half)

  Stage<T, DT> st;
  // tiles up to the block's last key (workgroup-uniform: KeyEnds), keys past it are not loaded
  const int nt = (ke.block + kTileRows - 1) / kTileRows;
  st.load(kg, vg, stride, 0, ke.block, d, tid);
  st.store(tsmem, tid);
  __syncthreads();
  for (int it = 0; it < nt; it++) {
    const u16* kt = tsmem + (it & 1) * G::stage;
    const u16* vt = kt + G::tile;
    if (it + 1 < nt) st.load(kg, vg, stride, (it + 1) * kTileRows, ke.block, d, tid);
    for (int sub = 0; sub < kTileRows; sub += 32) {
      const int key0 = it * kTileRows + sub;
      if (key0 >= ke.wave) break;  // past every row of this wavefront (the first sub-tile never is)
      f32x16 s = mma_rows<T, DT>(kt, sub, qf, ksd, lane);
      float pen[16];
#pragma unroll
      for (int reg = 0; reg < 16; reg++) pen[reg] = 0.f;
      if (mask) {
        float tmin = INFINITY;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int key = key0 + tile_row(reg, h);
          if (key < n) {
            pen[reg] = penalty(mrow, key);
            tmin = fminf(tmin, pen[reg]);
          }
        }
        tmin = fminf(tmin, __shfl_xor(tmin, 32));
        if (tmin < rmin) {  // what is accumulated was taken relative to the larger penalty
          rmax -= rmin - tmin;
          rmin = tmin;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int key = key0 + tile_row(reg, h);
        s[reg] = key < ke.row ? s[reg] * scale - (pen[reg] - rmin) : -INFINITY;
        mx = fmaxf(mx, s[reg]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(rmax, mx);  // finite: key 0 < ke.row
      const float alpha = __expf(rmax - mnew);
      float sum = 0.f;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        s[reg] = __expf(s[reg] - mnew);
        sum += s[reg];
      }
      rsum = rsum * alpha + sum;
      rmax = mnew;
#pragma unroll
      for (int ct = 0; ct < DT; ct++) {
#pragma unroll
        for (int reg = 0; reg < 16; reg++) o[ct][reg] *= alpha;
      }
      mma_tr<T, DT>(o, vt, sub, s, lane);
    }
    if (it + 1 < nt) st.store(tsmem + ((it + 1) & 1) * G::stage, tid);
    __syncthreads();
  }
  rsum += __shfl_xor(rsum, 32);
  const float rinv = 1.f / (rsum + kSoftmaxEps);
  store_own_row<T, DT>(live ? out + off_m : nullptr, o, rinv, d, h);
  if (stats && live && h == 0)
    *reinterpret_cast<f32x4*>(stats + (blk.bh * m + qrow) * 4) = (f32x4){rmax, rinv, rmin, 0.f};
}

// ================================================================================================
// Backward: the dq sweep
// ================================================================================================
template <typename T, int DT, bool LEN>
__global__ void __launch_bounds__(kTiledThreads)
    mha_tiled_dq_kernel(int heads, int m, int n, int d, const T* __restrict__ q,
                        const T* __restrict__ k, const T* __restrict__ v,
                        const T* __restrict__ dense, const float* __restrict__ len_from,
                        const float* __restrict__ len_to, const T* __restrict__ out,
                        const T* __restrict__ top, float* __restrict__ stats, T* __restrict__ dq,
                        float scale) {
  const T* mask = LEN ? nullptr : dense;
  using G = TileGeo<T, DT>;
  HCTR_DYN_LDS16(u16, tsmem);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const TiledBlock blk(heads, m);
  const size_t stride = (size_t)heads * d;
  const int ksd = (d + 15) / 16;
  const int qrow = blk.row0 + (tid >> 6) * 32 + r;
  const bool live = qrow < m;
  const size_t off_m = tiled_head_offset(blk.b, blk.hd, m, heads, d) + qrow * stride;
  const T* kg = k + tiled_head_offset(blk.b, blk.hd, n, heads, d);
  const T* vg = v + tiled_head_offset(blk.b, blk.hd, n, heads, d);
  const T* mrow = (mask && live) ? mask + (blk.b * m + qrow) * (size_t)n : nullptr;
  const KeyEnds<LEN> ke(len_from, len_to, blk, m, n, tid);

  typename Tl<T>::frag qf[2 * DT], gf[2 * DT];  // the lane's rows of Q and dO
  load_frags<T, DT>(qf, live ? q + off_m : nullptr, d, h);
  float delta = 0.f;  // rowsum(dO o O)
#pragma unroll
  for (int t = 0; t < 2 * DT; t++) {
    const int c = 16 * t + 8 * h;
    const bool ok = live && c < d;
    const typename Tl<T>::raw g8 = ok ? Tl<T>::load8(top + off_m + c) : Tl<T>::zero8();
    const typename Tl<T>::raw o8 = ok ? Tl<T>::load8(out + off_m + c) : Tl<T>::zero8();
    float gx[8], ox[8];
    Tl<T>::to_f32(g8, gx);
    Tl<T>::to_f32(o8, ox);
#pragma unroll
    for (int e = 0; e < 8; e++) delta += gx[e] * ox[e];
    gf[t] = Tl<T>::to_frag(g8);
  }
  delta += __shfl_xor(delta, 32);
  // a row that does not exist: 1 / (sum + eps) = 0 makes its P and dS zero
  float* srow = stats + (blk.bh * m + qrow) * 4;
  const f32x4 sv = live ? *reinterpret_cast<const f32x4*>(srow) : (f32x4){0.f, 0.f, 0.f, 0.f};
  const float rmax = sv[0], rinv = sv[1], rmin = sv[2];
  if (live && h == 0) srow[3] = delta;  // for the dkv sweep
  f32x16 g[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ct++) g[ct] = zero_tile();

  Stage<T, DT> st;
  // tiles up to the block's last key (workgroup-uniform: KeyEnds), keys past it are not loaded
  const int nt = (ke.block + kTileRows - 1) / kTileRows;
  st.load(kg, vg, stride, 0, ke.block, d, tid);
  st.store(tsmem, tid);
  __syncthreads();
  for (int it = 0; it < nt; it++) {
    const u16* kt = tsmem + (it & 1) * G::stage;
    const u16* vt = kt + G::tile;
    if (it + 1 < nt) st.load(kg, vg, stride, (it + 1) * kTileRows, ke.block, d, tid);
    for (int sub = 0; sub < kTileRows; sub += 32) {
      const int key0 = it * kTileRows + sub;
      if (key0 >= ke.wave) break;  // past every row of this wavefront (the first sub-tile never is)
      f32x16 s = mma_rows<T, DT>(kt, sub, qf, ksd, lane);
      const f32x16 dp = mma_rows<T, DT>(vt, sub, gf, ksd, lane);
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int key = key0 + tile_row(reg, h);
        const float p = __expf(logit(s[reg], scale, mrow, rmin, key, ke.row) - rmax) * rinv;
        s[reg] = p * (dp[reg] - delta);
      }
      mma_tr<T, DT>(g, kt, sub, s, lane);
    }
    if (it + 1 < nt) st.store(tsmem + ((it + 1) & 1) * G::stage, tid);
    __syncthreads();
  }
  store_own_row<T, DT>(live ? dq + off_m : nullptr, g, scale, d, h);
}

// ================================================================================================
// Backward: the dkv sweep
// ================================================================================================
template <typename T, int DT, bool LEN>
__global__ void __launch_bounds__(kTiledThreads)
    mha_tiled_dkv_kernel(int heads, int m, int n, int d, const T* __restrict__ q,
                         const T* __restrict__ k, const T* __restrict__ v,
                         const T* __restrict__ dense, const float* __restrict__ len_from,
                         const float* __restrict__ len_to, const T* __restrict__ top,
                         const float* __restrict__ stats, T* __restrict__ dk, T* __restrict__ dv,
                         float scale) {
  const T* mask = LEN ? nullptr : dense;
  using G = TileGeo<T, DT>;
  HCTR_DYN_LDS16(u16, tsmem);
  // the statistics of a tile's 64 query rows, double buffered like the tiles, in front of them
  f32x4* stt = reinterpret_cast<f32x4*>(tsmem);
  u16* tiles = tsmem + 2 * kTileRows * 8;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const TiledBlock blk(heads, n);
  const size_t stride = (size_t)heads * d;
  const int ksd = (d + 15) / 16;
  const int key = blk.row0 + (tid >> 6) * 32 + r;
  const bool live = key < n;
  const size_t off_n = tiled_head_offset(blk.b, blk.hd, n, heads, d) + key * stride;
  const T* qg = q + tiled_head_offset(blk.b, blk.hd, m, heads, d);
  const T* gg = top + tiled_head_offset(blk.b, blk.hd, m, heads, d);
  const float* sg = stats + blk.bh * m * 4;
  const T* mcol = (mask && live) ? mask + blk.b * m * (size_t)n + key : nullptr;

  typename Tl<T>::frag kf[2 * DT], vf[2 * DT];  // the lane's rows of K and V
  load_frags<T, DT>(kf, live ? k + off_n : nullptr, d, h);
  load_frags<T, DT>(vf, live ? v + off_n : nullptr, d, h);
  f32x16 gk[DT], gv[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ct++) gk[ct] = gv[ct] = zero_tile();

  Stage<T, DT> st;
  f32x4 sst = {0.f, 0.f, 0.f, 0.f};  // thread tid < 64: the statistics of the next tile's row tid
  const int nt = (m + kTileRows - 1) / kTileRows;
  auto load_stats = [&](int row0) {
    if (tid < kTileRows)
      sst = row0 + tid < m ? *reinterpret_cast<const f32x4*>(sg + (size_t)(row0 + tid) * 4)
                           : (f32x4){0.f, 0.f, 0.f, 0.f};  // 1 / (sum + eps) = 0: P = dS = 0
  };
  // LEN: a row below first_plain reaches the keys below nv only, every other row all of them.  A
  // block whose keys all lie at or past nv is reached by the plain rows alone: it starts at the
  // tile that holds first_plain, and with no plain row (first_plain == m) streams nothing and
  // stores the zeros.  it0 depends on the sample's two lengths, blockIdx and the shape only, so the
  // trip count and the barriers are the same for the whole workgroup
  int it0 = 0, first_plain = 0;
  bool key_valid = true;
  if (LEN) {
    const LenBounds lb(len_from, len_to, blk.b, m, n);
    first_plain = lb.first_plain;
    key_valid = key < lb.nv;
    if (blk.row0 >= lb.nv) it0 = first_plain == m ? nt : first_plain / kTileRows;
  }
  st.load(qg, gg, stride, it0 * kTileRows, m, d, tid);  // (rows past m: zeros, nothing is read)
  load_stats(it0 * kTileRows);
  st.store(tiles + (it0 & 1) * G::stage, tid);
  if (tid < kTileRows) stt[(it0 & 1) * kTileRows + tid] = sst;
  __syncthreads();
  for (int it = it0; it < nt; it++) {
    const u16* qt = tiles + (it & 1) * G::stage;
    const u16* gt = qt + G::tile;
    const f32x4* sv = stt + (it & 1) * kTileRows;
    if (it + 1 < nt) {
      st.load(qg, gg, stride, (it + 1) * kTileRows, m, d, tid);
      load_stats((it + 1) * kTileRows);
    }
    for (int sub = 0; sub < kTileRows; sub += 32) {
      const int q0 = it * kTileRows + sub;
      if (q0 >= m) break;
      f32x16 p = mma_rows<T, DT>(qt, sub, kf, ksd, lane);   // q.k of (query tile_row(reg, h), key)
      f32x16 ds = mma_rows<T, DT>(gt, sub, vf, ksd, lane);  // dP
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int ql = sub + tile_row(reg, h), qi = it * kTileRows + ql;
        const f32x4 row = sv[ql];  // max, 1 / (sum + eps), smallest penalty, delta
        const T* mrow = (mcol && qi < m) ? mcol + (size_t)qi * n : nullptr;
        const bool reached = live && (!LEN || key_valid || qi >= first_plain);
        const float lg = reached ? p[reg] * scale - (penalty(mrow, 0) - row[2]) : -INFINITY;
        p[reg] = __expf(lg - row[0]) * row[1];
        ds[reg] = p[reg] * (ds[reg] - row[3]);
      }
      mma_tr<T, DT>(gv, gt, sub, p, lane);
      mma_tr<T, DT>(gk, qt, sub, ds, lane);
    }
    if (it + 1 < nt) {
      st.store(tiles + ((it + 1) & 1) * G::stage, tid);
      if (tid < kTileRows) stt[((it + 1) & 1) * kTileRows + tid] = sst;
    }
    __syncthreads();
  }
  store_own_row<T, DT>(live ? dv + off_n : nullptr, gv, 1.f, d, h);
  store_own_row<T, DT>(live ? dk + off_n : nullptr, gk, scale, d, h);
}

// ================================================================================================
// Host side
// ================================================================================================
// what both tiled entry points refuse, by name, before anything else
int tiled_check(int heads, int seq_from, int seq_to, int size_per_head, int dtype) {
  HCTR_REQUIRE(heads >= 1, "mha_tiled: heads >= 1");
  HCTR_REQUIRE(seq_from >= 1 && seq_from <= kTiledMaxSeq, "mha_tiled: seq_from 1 .. 4096");
  HCTR_REQUIRE(seq_to >= 1 && seq_to <= kTiledMaxSeq, "mha_tiled: seq_to 1 .. 4096");
  HCTR_REQUIRE(size_per_head >= 8 && size_per_head % 8 == 0 && size_per_head <= kTiledMaxHead,
               "mha_tiled: size_per_head a multiple of 8, 8 .. 128");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               "mha_tiled: dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}
// one workgroup per (sample, head, block of 128 rows): the grid is not capped
int tiled_grid(size_t batch, int heads, int rows, unsigned* grid) {
  const size_t g = batch * (size_t)heads * (size_t)((rows + kBlockRows - 1) / kBlockRows);
  HCTR_REQUIRE(g <= 0x7fffffffull, "mha_tiled: batch * heads * blocks of 128 rows below 2^31");
  *grid = (unsigned)g;
  return HCTR_OK;
}
// f(the element type, DT): DT 32-wide column tiles hold the head
template <typename F>
int with_tiled_types(int dtype, int size_per_head, F&& f) {
  return with_dtype(dtype, [&](auto* t) -> int {
    switch ((size_per_head + 31) / 32) {
      case 1: return f(t, std::integral_constant<int, 1>{});
      case 2: return f(t, std::integral_constant<int, 2>{});
      case 3: return f(t, std::integral_constant<int, 3>{});
      default: return f(t, std::integral_constant<int, 4>{});
    }
  });
}

int tiled_fwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head, const void* q,
              const void* k, const void* v, const MaskSrc& ms, void* out, void* stats, int dtype,
              hctr_stream_t stream) {
  HCTR_TRY(tiled_check(heads, seq_from, seq_to, size_per_head, dtype));
  HCTR_REQUIRE(aligned16(q, k, v, ms.dense, out, stats), "mha_tiled: 16-byte aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(q && k && v && out && ms.complete(), "null pointer");
  unsigned grid;
  HCTR_TRY(tiled_grid(batch, heads, seq_from, &grid));
  const float scale = 1.f / sqrtf((float)size_per_head);
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_tiled_types(dtype, size_per_head, [&](auto* t, auto dt) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    constexpr int DT = decltype(dt)::value;
    return with_mask_src(ms, [&](auto len) -> int {
      auto kernel = mha_tiled_fwd_kernel<T, DT, decltype(len)::value>;
      const size_t lds = TileGeo<T, DT>::lds_bytes;
      HCTR_TRY(allow_dyn_lds(kernel, lds));
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTiledThreads), lds, s, heads, seq_from, seq_to,
                         size_per_head, (const T*)q, (const T*)k, (const T*)v, (const T*)ms.dense,
                         ms.len_from, ms.len_to, (T*)out, (float*)stats, scale);
      return HCTR_OK;
    });
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int tiled_bwd(size_t batch, int heads, int seq_from, int seq_to, int size_per_head, const void* q,
              const void* k, const void* v, const MaskSrc& ms, const void* out, void* stats,
              const void* top_grad, void* dq, void* dk, void* dv, int dtype, hctr_stream_t stream) {
  HCTR_TRY(tiled_check(heads, seq_from, seq_to, size_per_head, dtype));
  HCTR_REQUIRE(aligned16(q, k, v, ms.dense, out, stats, top_grad, dq, dk, dv),
               "mha_tiled: 16-byte aligned buffers");
  if (batch == 0) return HCTR_OK;
  HCTR_REQUIRE(q && k && v && top_grad && dq && dk && dv && ms.complete(), "null pointer");
  HCTR_REQUIRE(out && stats, "mha_tiled_bwd: out and stats of the forward");
  unsigned grid_q, grid_k;
  HCTR_TRY(tiled_grid(batch, heads, seq_from, &grid_q));
  HCTR_TRY(tiled_grid(batch, heads, seq_to, &grid_k));
  const float scale = 1.f / sqrtf((float)size_per_head);
  hipStream_t s = as_stream(stream);
  HCTR_TRY(with_tiled_types(dtype, size_per_head, [&](auto* t, auto dt) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    constexpr int DT = decltype(dt)::value;
    return with_mask_src(ms, [&](auto len) -> int {
      auto dq_kernel = mha_tiled_dq_kernel<T, DT, decltype(len)::value>;
      auto dkv_kernel = mha_tiled_dkv_kernel<T, DT, decltype(len)::value>;
      const size_t lds = TileGeo<T, DT>::lds_bytes;
      const size_t lds_kv = lds + 2 * kTileRows * sizeof(f32x4);
      HCTR_TRY(allow_dyn_lds(dq_kernel, lds));
      HCTR_TRY(allow_dyn_lds(dkv_kernel, lds_kv));
      hipLaunchKernelGGL(dq_kernel, dim3(grid_q), dim3(kTiledThreads), lds, s, heads, seq_from,
                         seq_to, size_per_head, (const T*)q, (const T*)k, (const T*)v,
                         (const T*)ms.dense, ms.len_from, ms.len_to, (const T*)out,
                         (const T*)top_grad, (float*)stats, (T*)dq, scale);
      hipLaunchKernelGGL(dkv_kernel, dim3(grid_k), dim3(kTiledThreads), lds_kv, s, heads, seq_from,
                         seq_to, size_per_head, (const T*)q, (const T*)k, (const T*)v,
                         (const T*)ms.dense, ms.len_from, ms.len_to, (const T*)top_grad,
                         (const float*)stats, (T*)dk, (T*)dv, scale);
      return HCTR_OK;
    });
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}
