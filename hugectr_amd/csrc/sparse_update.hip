// sparse_update.hip -- fused embedding backward + sparse optimizer update on gfx950.
//
// Replaces backward_sum/backward_mean (R/HugeCTR/src/embeddings/backward_functor.cu:26-104) and
// EmbeddingOptimizer::update (R/HugeCTR/src/optimizers/sparse_optimizer.cu:622-864).
// Reference pipeline: wgrad copy -> sample-id expand -> radix sort (row index -> bucket id) ->
// run flags -> scan -> BLOCKING D2H of the run count -> one block per unique row.
// Here: no wgrad tensor (the top gradient is read in place, the mean scale 1/n is applied while
// accumulating), the run count stays on the device (persistent grid-stride over runs), and a
// "group" of D/4 lanes owns a row with 16-byte accesses.  Gradient accumulation per row is in
// ascending bucket id, exactly the reference's order (stable sort), then / scaler.
//
// This unit: SparseUpdater, where a batch goes (update_typed), the (row, bucket) pairs and their
// sort, the hot / cold path of one-hot batches with its host state, and the small kernels -- any-D
// update, atomic SGD, global sweeps, wgrad.  The segmented family, the one that needs the
// row-offset type at compile time, is a unit of its own (su_units.h).
//
// A test tree from before that unit existed (commit cc146d1: its tests/emu/Makefile compiles
// this file three times, -DHCTR_SU_PART=0/1/2, and knows no su_*.hip) must still get a complete
// interpreter library: a non-hipcc build that does not announce the unit (HCTR_EMU_SU_UNITS)
// takes it in at the end of part 0, and parts 1 and 2 are empty.  The next split removes this.
#if !defined(__HIPCC__) && !defined(HCTR_EMU_SU_UNITS)
#define HCTR_SU_ONE_UNIT
#endif
#if !(defined(HCTR_SU_ONE_UNIT) && HCTR_SU_PART != 0)
#include "su_device.h"
#include "radix_sort.h"

#include <cstdlib>
#include <cstring>

#include "block_prims.h"

namespace hctr {
namespace {

constexpr int kTile = 1024;

// ---- step 1: (row index, bucket id) pairs (sample_id_expand_kernel :189-200) ------------------
template <typename OffT>
__global__ void __launch_bounds__(kBlock)
    expand_pairs_kernel(size_t buckets, size_t n_sort, const OffT* __restrict__ row_offset,
                        const uint64_t* __restrict__ value_index, uint32_t* __restrict__ keys,
                        uint32_t* __restrict__ vals, uint32_t* __restrict__ span_count,
                        uint32_t map_inner, uint32_t map_outer,
                        const uint32_t* __restrict__ skip_flag) {
  const size_t nnz = (size_t)row_offset[buckets];
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid == 0 && blockIdx.y == 0)  // long-run lists of seg_reduce / seg_combine
    span_count[0] = span_count[1] = span_count[2] = span_count[3] = 0u;
  // one-hot batch: the sort's first pass takes rows and payloads from where they lie (RsFirst)
  if (skip_flag != nullptr && *skip_flag != 0u) return;
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  // key-parallel (block_prims.h): the payload is the gradient row of the key's bucket
  // (SparseUpdater::map_inner)
  for_each_key_wave(buckets, row_offset, [&](size_t u, size_t j) {
    if (j >= n_sort) return;
    keys[j] = (uint32_t)value_index[j];
    vals[j] = map_inner ? ((uint32_t)u % map_inner) * map_outer + (uint32_t)u / map_inner
                        : (uint32_t)u;
  });
  // padding (host upper bound > live nnz): sorts to the end, never forms a counted run
  if (blockIdx.y != 0) return;
  for (size_t j = nnz + tid; j < n_sort; j += nthreads) {
    keys[j] = ~0u;
    vals[j] = 0xFFFFFFFFu;
  }
}

// ---- step 2: run starts ------------------------------------------------------------------------
__device__ __forceinline__ bool is_run_start(const uint32_t* k, size_t i, size_t nnz) {
  if (i >= nnz) return false;
  return i == 0 || k[i] != k[i - 1];
}

template <typename OffT>
__global__ void __launch_bounds__(kBlock)
    run_count_kernel(const uint32_t* __restrict__ keys, const OffT* __restrict__ row_offset,
                     size_t buckets, size_t n_tiles, uint32_t* __restrict__ tile_sums) {
  __shared__ uint32_t smem[kBlock / 64 + 1];
  const size_t nnz = (size_t)row_offset[buckets];
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kTile / kBlock; r++) {
      size_t i = tile * kTile + r * kBlock + threadIdx.x;
      c += is_run_start(keys, i, nnz) ? 1u : 0u;
    }
    uint32_t tot = block_reduce_sum<uint32_t, kBlock>(c, smem);
    if (threadIdx.x == 0) tile_sums[tile] = tot;
  }
}

__global__ void __launch_bounds__(1024)
    scan_tiles_u32_kernel(uint32_t* sums, size_t m, uint64_t* d_total) {
  __shared__ uint32_t smem[1024 / 64 + 1];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t base = 0; base < m; base += 1024) {
    size_t i = base + threadIdx.x;
    uint32_t v = (i < m) ? sums[i] : 0u;
    uint32_t tot;
    uint32_t ex = block_exclusive_scan<uint32_t, 1024>(v, smem, &tot);
    uint64_t c = carry;
    if (i < m) sums[i] = (uint32_t)(c + ex);
    __syncthreads();
    if (threadIdx.x == 0) carry = c + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *d_total = carry;
}

template <typename OffT>
__global__ void __launch_bounds__(kBlock)
    run_write_kernel(const uint32_t* __restrict__ keys, const OffT* __restrict__ row_offset,
                     size_t buckets, size_t n_tiles, const uint32_t* __restrict__ tile_sums,
                     const uint64_t* __restrict__ d_num_runs, uint32_t* __restrict__ run_start) {
  __shared__ uint32_t smem[kBlock / 64 + 1];
  const size_t nnz = (size_t)row_offset[buckets];
  if (blockIdx.x == 0 && threadIdx.x == 0) run_start[*d_num_runs] = (uint32_t)nnz;
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint32_t run = tile_sums[tile];
#pragma unroll
    for (int r = 0; r < kTile / kBlock; r++) {
      size_t i = tile * kTile + r * kBlock + threadIdx.x;
      bool f = is_run_start(keys, i, nnz);
      uint32_t tot;
      uint32_t ex = block_exclusive_scan<uint32_t, kBlock>(f ? 1u : 0u, smem, &tot);
      if (f) run_start[run + ex] = (uint32_t)i;
      run += tot;
    }
  }
}

// ---- hot rows of a one-hot batch ----------------------------------------------------------------
// Power-law batches are bimodal: a few thousand rows -- the rows of the tiny tables and the heads
// of the big ones, which the table handed out first and which therefore carry the LOWEST row
// numbers -- take two thirds of a batch's positions (Criteo-1TB shape, alpha 1.1: rows < 8192 take
// 71 % of the 1.7 M positions).  Sending those positions through a global radix sort only to cut
// the result into tiles again is what made the update latency-bound.  For a batch with one key per
// bucket (device flag of the index stage) the hot positions never enter the sort:
//   * position p belongs to stream p % G (G = slots per sample of a sample-major batch: all
//     positions of a stream come from ONE table, so its hot rows recur inside the stream; G = 1:
//     the positions as they lie) and a chunk is kHotChunk consecutive positions of one stream;
//   * hot_sort_kernel, one workgroup per chunk: the chunk's positions whose row is < H are sorted
//     by row inside LDS (two stable 7-bit passes, ascending position inside a row) and cut into
//     tiles of 32 like the global list is;
//   * hot_reduce_kernel, one lane group per tile (all chunks' tiles in one flat list): every run
//     (= one row's gradients inside the chunk) is summed in ascending position order; the pieces
//     of runs that cross tile borders are added in tile order by hot_join_kernel.  A chunk's
//     partial sums land in a pool (the far end of gsum, which the sorted list cannot reach: cold
//     pairs + hot partials <= nnz) and loc[row][chunk] says where;
//   * hot_apply_kernel, one lane group per hot row: partials in ascending chunk order, then the
//     optimizer -- a fixed association, so the result does not depend on scheduling;
//   * the positions of rows >= H go to the cold rows' chain (counted per row, below), which runs
//     on a side stream next to the hot rows' kernels.
// A batch that is not one-hot (flag 0) makes these kernels exit and the cold chain takes every
// position.
// Measured (MI355X, Criteo-1TB shape, round 4): one workgroup doing sort AND reduce of its chunk
// (8 tiles per lane group, one after the other) took 132 us for 310 MB -- a latency chain on 3
// waves per SIMD; hence the flat tile list.
constexpr int kHotChunk = 4096;
constexpr int kHotBlock = 512;
constexpr int kHotWaves = kHotBlock / 64;
constexpr int kHotRounds = kHotChunk / kHotBlock;  // entries per thread
constexpr int kHotBits = 7;                        // digit of one LDS pass; two passes
constexpr int kHotBins = 1 << kHotBits;
constexpr int kHotMaxRows = 1 << (2 * kHotBits);   // 16384
constexpr int kHotTile = 32;
constexpr int kHotTiles = kHotChunk / kHotTile;    // 128
constexpr int kHotPosBits = 12;                    // entry = row << 12 | position inside the chunk
static_assert((1 << kHotPosBits) == kHotChunk, "entry layout");
constexpr uint32_t kHotNone = 0xFFFFu;             // loc[][]: the row has no partial in this chunk
constexpr uint32_t kHotMaxStreams = 64;            // more slots per sample: the plain path

struct HotGeom {
  uint32_t n;          // positions (= buckets: one key each)
  uint32_t G;          // streams
  uint32_t cpg;        // chunks per stream
  uint32_t rows;       // H
  uint32_t map_inner, map_outer;  // gradient row of bucket u (SparseUpdater::map_inner)
  uint32_t loc_stride;  // chunks the loc table has room for, per row
};

// lanes of this wavefront whose digit equals mine (valid lanes only)
__device__ __forceinline__ unsigned long long hot_match(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < kHotBits; bit++) {
    const bool one = ((d >> bit) & 1u) != 0u;
    const unsigned long long bal = __ballot(one);
    m &= one ? bal : ~bal;
  }
  return valid ? m : 0ull;
}

// One stable LDS split of the workgroup's entries by the digit (e >> shift) & 127.  "Wavefront,
// then round, then lane" is the input order (wavefront w holds entries [w * 512, (w + 1) * 512) of
// it), and ranks are handed out in that nesting.  Returns the number of valid entries.
__device__ __forceinline__ uint32_t hot_lds_pass(const uint32_t (&e)[kHotRounds], uint32_t vmask,
                                                 int shift, uint32_t* __restrict__ dst,
                                                 uint32_t (*wh)[kHotBins], uint32_t* scan_smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kHotWaves * kHotBins; i += kHotBlock) (&wh[0][0])[i] = 0u;
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t info[kHotRounds];  // rank inside the match group | group size << 8
#pragma unroll
  for (int r = 0; r < kHotRounds; r++) {
    const bool valid = ((vmask >> r) & 1u) != 0u;
    const uint32_t d = (e[r] >> shift) & (kHotBins - 1);
    const unsigned long long m = hot_match(d, valid);
    const uint32_t rank = (uint32_t)__popcll(m & lt), cnt = (uint32_t)__popcll(m);
    info[r] = rank | (cnt << 8);
    if (valid && rank == 0u) atomicAdd(&wh[wave][d], cnt);
  }
  __syncthreads();
  uint32_t c = 0u;
  if (threadIdx.x < kHotBins) {
#pragma unroll
    for (int w = 0; w < kHotWaves; w++) c += wh[w][threadIdx.x];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan<uint32_t, kHotBlock>(c, scan_smem, &total);
  if (threadIdx.x < kHotBins) {
#pragma unroll
    for (int w = 0; w < kHotWaves; w++) {
      const uint32_t cw = wh[w][threadIdx.x];
      wh[w][threadIdx.x] = run;
      run += cw;
    }
  }
  __syncthreads();
  volatile uint32_t* cur = wh[wave];
#pragma unroll
  for (int r = 0; r < kHotRounds; r++) {
    const bool valid = ((vmask >> r) & 1u) != 0u;
    const uint32_t d = (e[r] >> shift) & (kHotBins - 1);
    uint32_t first = 0u;
    if (valid) first = cur[d];                        // every lane of the match group reads ...
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      const uint32_t rank = info[r] & 0xFFu;
      if (rank == 0u) cur[d] = first + (info[r] >> 8);  // ... before its leader advances
      dst[first + rank] = e[r];
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  return total;
}

// per-chunk results of hot_sort_kernel
struct HotBufs {
  uint32_t* S;       // [chunks][kHotChunk] the chunk's hot entries, sorted by row
  uint32_t* meta;    // [chunks][2] entries, first pool slot
  uint32_t* tpref;   // [chunks][kHotTiles + 1] run starts in front of a tile
  uint32_t* items;   // tiles that hold entries: chunk * kHotTiles + tile (any order)
  uint32_t* loc_blk;  // [hot rows] bit b: some chunk in [32 b, 32 b + 32) holds a partial
  uint32_t* joins;   // [.][3] runs that cross tile borders: chunk << 14 | first tile << 7 | last
                     //        tile, partial number, row
  uint32_t* counts;  // this update's counters: [0] pool slots taken, [1] items, [2] joins
  uint32_t* counts_next;  // the next update's (the other parity): zeroed by hot_sort_kernel
  uint16_t* loc;     // [hot rows][loc_stride] partial number of (row, chunk), kHotNone = none
  float* head;       // [chunks * kHotTiles][D] partial of the run that enters a tile
  float* tail;       // [chunks * kHotTiles][D] partial of the run that leaves a tile (its owner's)
};

// one workgroup per chunk: the chunk's hot entries sorted by row (LDS), run starts per tile, a
// block of pool slots for its partials, the work lists of hot_reduce_kernel / hot_join_kernel
__global__ void __launch_bounds__(kHotBlock)
    hot_sort_kernel(HotGeom hg, const uint32_t* __restrict__ one_hot,
                    const uint64_t* __restrict__ value_index, HotBufs hb) {
  // (before the flag is looked at: the counters alternate between two sets, and a batch that is not
  //  one-hot must leave the next one a clean set too)
  if (blockIdx.x == 0 && threadIdx.x == 0)
    hb.counts_next[0] = hb.counts_next[1] = hb.counts_next[2] = 0u;
  if (*one_hot == 0u) return;
  __shared__ uint32_t list[2][kHotChunk];
  __shared__ uint32_t wh[kHotWaves][kHotBins];
  __shared__ uint32_t scan_smem[kHotWaves + 1];
  __shared__ uint32_t tile_pref[kHotTiles + 2];  // run starts in front of a tile
  __shared__ uint32_t sh_ibase, sh_jbase;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.x;
  const uint32_t g = chunk / hg.cpg, c = chunk % hg.cpg;
  const uint32_t len_g = hg.n > g ? (hg.n - g + hg.G - 1u) / hg.G : 0u;  // positions of my stream
  const uint32_t c0 = c * (uint32_t)kHotChunk;
  // ---- the chunk's hot entries, sorted by row (stable: ascending position inside a row) -------
  uint32_t e[kHotRounds], vmask = 0u;
#pragma unroll
  for (int r = 0; r < kHotRounds; r++) {
    const uint32_t i = (uint32_t)(wave * (64 * kHotRounds) + r * 64 + lane);
    e[r] = 0u;
    if (c0 + i < len_g) {
      const uint64_t row = value_index[(size_t)(c0 + i) * hg.G + g];
      if (row < (uint64_t)hg.rows) {
        e[r] = ((uint32_t)row << kHotPosBits) | i;
        vmask |= 1u << r;
      }
    }
  }
  const uint32_t nh = hot_lds_pass(e, vmask, kHotPosBits, list[0], wh, scan_smem);
  if (threadIdx.x == 0) hb.meta[2 * chunk] = nh;
  if (nh == 0u) return;  // (uniform: every thread holds the block total)
  vmask = 0u;
#pragma unroll
  for (int r = 0; r < kHotRounds; r++) {
    const uint32_t j = (uint32_t)(wave * (64 * kHotRounds) + r * 64 + lane);
    e[r] = j < nh ? list[0][j] : 0u;
    if (j < nh) vmask |= 1u << r;
  }
  hot_lds_pass(e, vmask, kHotPosBits + kHotBits, list[1], wh, scan_smem);
  const uint32_t* S = list[1];
  const uint32_t nt = (nh + kHotTile - 1) / kHotTile;
  // ---- run starts per tile -> the run number of every tile's first entry ----------------------
#pragma unroll
  for (int r = 0; r < kHotRounds; r++) {
    const uint32_t j = (uint32_t)(wave * (64 * kHotRounds) + r * 64 + lane);
    const bool st = j < nh && (j == 0u || (S[j] >> kHotPosBits) != (S[j - 1] >> kHotPosBits));
    // (every run of the chunk becomes one partial of its row: hot_apply_kernel looks at the
    //  blocks of 32 chunks marked here only)
    if (st) atomicOr(hb.loc_blk + (S[j] >> kHotPosBits), 1u << (chunk >> 5));
    const unsigned long long bal = __ballot(st);
    if (lane == 0) {
      tile_pref[j / kHotTile] = (uint32_t)__popcll(bal & 0xFFFFFFFFull);
      tile_pref[j / kHotTile + 1] = (uint32_t)__popcll(bal >> 32);
    }
    if (j < nh) hb.S[(size_t)chunk * kHotChunk + j] = S[j];
  }
  __syncthreads();
  // a run that leaves tile t and began in it (or exactly at its start) is pieced together by
  // hot_join_kernel: tail of t + the heads of the tiles after it, through the last one it reaches
  uint32_t t2 = 0u, jrow = 0u;
  bool owner = false;
  if (threadIdx.x + 1u < nt) {
    const uint32_t t = threadIdx.x, base = t * kHotTile;
    jrow = S[base + kHotTile - 1u] >> kHotPosBits;
    owner = (S[base + kHotTile] >> kHotPosBits) == jrow &&
            !((S[base] >> kHotPosBits) == jrow && t > 0u && (S[base - 1u] >> kHotPosBits) == jrow);
    if (owner) {  // last entry of the run: the list is sorted by row
      uint32_t lo = base + kHotTile, hi = nh;  // S[lo] belongs to the run, S[hi] (if any) does not
      while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((S[mid] >> kHotPosBits) == jrow) lo = mid;
        else hi = mid;
      }
      t2 = lo / kHotTile;
    }
  }
  {
    const uint32_t cnt = threadIdx.x < kHotTiles ? tile_pref[threadIdx.x] : 0u;
    uint32_t nr, nj;
    const uint32_t ex = block_exclusive_scan<uint32_t, kHotBlock>(cnt, scan_smem, &nr);
    const uint32_t jx = block_exclusive_scan<uint32_t, kHotBlock>(owner ? 1u : 0u, scan_smem, &nj);
    if (threadIdx.x == 0) {
      // (which block of slots / list entries the chunk gets does not matter)  One 64-bit add
      // takes both: pool slots in the low word, work items in the high word
      const unsigned long long old =
          atomicAdd(reinterpret_cast<unsigned long long*>(hb.counts),
                    ((unsigned long long)nt << 32) | (unsigned long long)nr);
      hb.meta[2 * chunk + 1] = (uint32_t)old;
      sh_ibase = (uint32_t)(old >> 32);
      sh_jbase = nj > 0u ? atomicAdd(hb.counts + 2, nj) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < kHotTiles) {
      hb.tpref[(size_t)chunk * (kHotTiles + 1) + threadIdx.x] = ex;
      if (threadIdx.x < nt) hb.items[sh_ibase + threadIdx.x] = chunk * kHotTiles + threadIdx.x;
      if (owner) {
        uint32_t* jp = hb.joins + 3 * (size_t)(sh_jbase + jx);
        jp[0] = (chunk << 14) | (threadIdx.x << 7) | t2;
        // number of the last run that starts at or before the end of the tile
        jp[1] = ex + cnt - 1u;
        jp[2] = jrow;
      }
    }
    if (threadIdx.x == 0) hb.tpref[(size_t)chunk * (kHotTiles + 1) + kHotTiles] = nr;
  }
}

// one lane group per tile of 32 sorted entries (any chunk): runs summed in ascending position order;
// a run inside the tile is a finished partial of its (row, chunk), the piece of a run that enters
// / leaves the tile goes to head / tail
template <int LPR, typename GradT>
__global__ void __launch_bounds__(kBlock, 5)  // (<= 102 VGPRs: leaves room for the other chain)
    hot_reduce_kernel(HotGeom hg, const uint32_t* __restrict__ one_hot,
                      const GradT* __restrict__ grad, float* __restrict__ pool_end, HotBufs hb) {
  typedef typename Load4<GradT>::raw Raw;
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  // raw fragments in flight per lane: half a tile, 32 VGPRs.  Measured and dropped (round 4): the
  // whole tile in one batch at 4 waves per SIMD, and one 40-word record per tile written by
  // hot_sort_kernel (one fetch instead of item -> entries / counts): both 79 -> 90 us
  constexpr int QB = sizeof(Raw) == 8 ? 16 : 8;
  static_assert(kHotTile % QB == 0, "batches tile the tile");
  if (*one_hot == 0u) return;
  // the tile's entries + the one in front + the one behind, per lane group
  __shared__ uint32_t ent[GPB][kHotTile + 2];
  const int gq = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const uint32_t n_items = hb.counts[1];
  constexpr uint32_t kNoneRow = 0xFFFFFFFFu;
  for (uint32_t it = blockIdx.x * GPB + gq; it < n_items; it += gridDim.x * GPB) {
    const uint32_t item = hb.items[it];
    const uint32_t chunk = item / kHotTiles, t = item % kHotTiles;
    const uint32_t nh = hb.meta[2 * chunk], pbase = hb.meta[2 * chunk + 1];
    const uint32_t g = chunk / hg.cpg, c0 = (chunk % hg.cpg) * (uint32_t)kHotChunk;
    const uint32_t base = t * kHotTile;
    const uint32_t cnt = nh - base < (uint32_t)kHotTile ? nh - base : (uint32_t)kHotTile;
    const uint32_t* Sg = hb.S + (size_t)chunk * kHotChunk;
    __builtin_amdgcn_wave_barrier();  // (the previous item's reads of ent are done)
    for (int q = l; q < kHotTile + 2; q += LPR) {
      // ent[q] = entry base - 1 + q; outside the chunk's list: no row
      const bool in = (q > 0 || base > 0u) && base + (uint32_t)q < nh + 1u;
      ent[gq][q] = in ? Sg[base + (uint32_t)q - 1u] : kNoneRow;
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t* E = ent[gq] + 1;  // E[q]: entry q of the tile
    const uint32_t prev_row = base > 0u ? E[-1] >> kHotPosBits : kNoneRow;
    const uint32_t next_row = base + cnt < nh ? E[cnt] >> kHotPosBits : kNoneRow;
    uint32_t cur = E[0] >> kHotPosBits;
    bool from_prev = cur == prev_row;
    uint32_t ri = hb.tpref[(size_t)chunk * (kHotTiles + 1) + t] - (from_prev ? 1u : 0u);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t slot = (size_t)chunk * kHotTiles + t;
    auto emit_partial = [&](uint32_t row, uint32_t rix, const float4& a) {
      *reinterpret_cast<float4*>(pool_end - ((size_t)(pbase + rix) + 1u) * D + l * 4) = a;
      if (l == 0) hb.loc[(size_t)row * hg.loc_stride + chunk] = (uint16_t)rix;
    };
#pragma unroll
    for (int qb = 0; qb < kHotTile; qb += QB) {
      if ((uint32_t)qb >= cnt) break;
      Raw v[QB];
#pragma unroll
      for (int k = 0; k < QB; k++) {
        const uint32_t q = (uint32_t)(qb + k) < cnt ? (uint32_t)(qb + k) : cnt - 1u;
        const uint32_t u = (c0 + (E[q] & (uint32_t)(kHotChunk - 1))) * hg.G + g;
        const uint32_t b = hg.map_inner ? (u % hg.map_inner) * hg.map_outer + u / hg.map_inner : u;
        v[k] = Load4<GradT>::ld_raw(grad + (size_t)b * D + l * 4);
      }
#pragma unroll
      for (int k = 0; k < QB; k++) {
        const uint32_t q = (uint32_t)(qb + k);
        if (q < cnt) {
          const uint32_t row = E[q] >> kHotPosBits;
          if (row != cur) {  // the run in hand ends here (it may have begun in an earlier tile)
            if (from_prev) *reinterpret_cast<float4*>(hb.head + slot * D + l * 4) = acc;
            else emit_partial(cur, ri, acc);
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            cur = row;
            from_prev = false;
            ri++;
          }
          const float4 f = Load4<GradT>::cvt(v[k]);
          acc.x += f.x;
          acc.y += f.y;
          acc.z += f.z;
          acc.w += f.w;
        }
      }
    }
    const bool to_next = cur == next_row;
    if (from_prev) *reinterpret_cast<float4*>(hb.head + slot * D + l * 4) = acc;
    else if (to_next) *reinterpret_cast<float4*>(hb.tail + slot * D + l * 4) = acc;
    else emit_partial(cur, ri, acc);
  }
}

// runs that cross tile borders inside a chunk: tail of the tile they start in + the heads after it
template <int LPR>
__global__ void __launch_bounds__(kBlock)
    hot_join_kernel(HotGeom hg, const uint32_t* __restrict__ one_hot, float* __restrict__ pool_end,
                    HotBufs hb) {
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  constexpr int CU = 16;
  if (*one_hot == 0u) return;
  const int gq = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const uint32_t n_joins = hb.counts[2];
  for (uint32_t it = blockIdx.x * GPB + gq; it < n_joins; it += gridDim.x * GPB) {
    const uint32_t w = hb.joins[3 * (size_t)it], ri = hb.joins[3 * (size_t)it + 1];
    const uint32_t row = hb.joins[3 * (size_t)it + 2];
    const uint32_t chunk = w >> 14, t = (w >> 7) & 127u, t2 = w & 127u;
    const size_t slot0 = (size_t)chunk * kHotTiles;
    float4 acc = *reinterpret_cast<const float4*>(hb.tail + (slot0 + t) * D + l * 4);
    for (uint32_t i = t + 1u; i <= t2; i += CU) {
      float4 h[CU];
#pragma unroll
      for (int k = 0; k < CU; k++) {
        const uint32_t tt = i + (uint32_t)k <= t2 ? i + (uint32_t)k : i;
        h[k] = *reinterpret_cast<const float4*>(hb.head + (slot0 + tt) * D + l * 4);
      }
#pragma unroll
      for (int k = 0; k < CU; k++) {
        if (i + (uint32_t)k <= t2) {
          acc.x += h[k].x;
          acc.y += h[k].y;
          acc.z += h[k].z;
          acc.w += h[k].w;
        }
      }
    }
    const uint32_t pbase = hb.meta[2 * chunk + 1];
    *reinterpret_cast<float4*>(pool_end - ((size_t)(pbase + ri) + 1u) * D + l * 4) = acc;
    if (l == 0) hb.loc[(size_t)row * hg.loc_stride + chunk] = (uint16_t)ri;
  }
}

// one lane group per hot row: its partials in ascending chunk order, then the optimizer
constexpr int kHotApplyChunks = 1024;  // first pool slots of the chunks, staged in LDS
template <int LPR>
__global__ void __launch_bounds__(kBlock)
    hot_apply_kernel(HotGeom hg, uint32_t n_chunks, const uint32_t* __restrict__ one_hot,
                     OptConst o, float* __restrict__ table, float* __restrict__ state0,
                     float* __restrict__ state1, unsigned long long* __restrict__ prev_time,
                     const float* __restrict__ pool_end, HotBufs hb) {
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  constexpr int CU = 8;
  constexpr int LU = 4;  // loc words per lane per trip
  constexpr unsigned long long kGroupMask = LPR >= 64 ? ~0ull : ((1ull << LPR) - 1ull);
  if (*one_hot == 0u) return;
  __shared__ uint32_t cbase[kHotApplyChunks];
  for (uint32_t i = threadIdx.x; i < n_chunks; i += kBlock) cbase[i] = hb.meta[2 * i + 1];
  __syncthreads();
  const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const int gshift = ((threadIdx.x & 63) / LPR) * LPR;
  for (uint32_t row = blockIdx.x * GPB + g; row < hg.rows; row += gridDim.x * GPB) {
    // blocks of 32 chunks that hold a partial of this row (a row of one stream: one or two)
    uint32_t blk = hb.loc_blk[row];
    __builtin_amdgcn_wave_barrier();  // (every lane of the group has read the word ...)
    if (blk == 0u) continue;
    if (l == 0) hb.loc_blk[row] = 0u;  // (... before it is cleaned for the next update)
    uint16_t* lrow = hb.loc + (size_t)row * hg.loc_stride;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    while (blk != 0u) {
      const uint32_t b32 = (uint32_t)__ffs((int)blk) - 1u;
      blk &= blk - 1u;
      for (uint32_t cb = b32 * 32u; cb < b32 * 32u + 32u && cb < n_chunks; cb += LPR * LU) {
        uint32_t v[LU];
#pragma unroll
        for (int u = 0; u < LU; u++) {
          const uint32_t cc = cb + (uint32_t)(u * LPR + l);
          v[u] = (cc < n_chunks && cc < b32 * 32u + 32u) ? (uint32_t)lrow[cc] : kHotNone;
        }
#pragma unroll
        for (int u = 0; u < LU; u++) {
          const uint32_t cc = cb + (uint32_t)(u * LPR + l);
          unsigned long long m = (__ballot(v[u] != kHotNone) >> gshift) & kGroupMask;
          uint32_t myslot = 0u;
          if (v[u] != kHotNone) {
            lrow[cc] = (uint16_t)kHotNone;  // clean for the next update
            myslot = cbase[cc] + v[u];
          }
          while (m != 0ull) {
            uint32_t slot[CU];
            int nk = 0;
#pragma unroll
            for (int k = 0; k < CU; k++) {
              int bit = 0;
              if (m != 0ull) {
                bit = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                nk = k + 1;
              }
              slot[k] = (uint32_t)__shfl((int)myslot, gshift + bit, 64);
            }
            float4 h[CU];
#pragma unroll
            for (int k = 0; k < CU; k++) {
              if (k < nk)
                h[k] = *reinterpret_cast<const float4*>(pool_end - ((size_t)slot[k] + 1u) * D + l * 4);
            }
#pragma unroll
            for (int k = 0; k < CU; k++) {
              if (k < nk) {
                acc.x += h[k].x;
                acc.y += h[k].y;
                acc.z += h[k].z;
                acc.w += h[k].w;
              }
            }
            any = true;
          }
        }
      }
    }
    if (any) apply_row_vec4<LPR>(o, (uint64_t)row, l, acc, table, state0, state1, prev_time);
  }
}

// ---- cold rows of a one-key-per-position batch: counted per row, never sorted ---------------------
// The positions the hot-row kernels leave (rows >= H; all of them when the batch's flag says the
// offsets were ragged) used to go through a global radix sort whose only job was to put the
// gradients of a row side by side: 70 us of latency-bound passes for 490 k pairs of which a third
// are alone in their row (Criteo-1TB shape, alpha 1.1: 221 k cold rows, 167 k of them met once,
// 53 k met 2 .. 32 times, 1.2 k more often).  Here the rows are COUNTED instead:
//   * cold_count_kernel, one thread per position: rank = atomicAdd(cnt[row], 1) -- the order of
//     arrival, whatever it is; the position that arrives first announces the row (dlist);
//   * cold_base_kernel, one thread per announced row: a row met once goes to the list of singles
//     with its position; a row met c > 1 times gets c consecutive entries of plist (handed out in
//     any order) and cnt[row] = base | kColdBased; runs of more than short_max go to their own list;
//   * cold_scatter_kernel, one thread per position: plist[base + rank] = position;
//   * cold_reduce_kernel: singles -- gradient row and table row of several rows in flight per lane
//     group, no list at all; short runs -- a lane group sorts the run's positions ASCENDING (LDS
//     rank count: the arrival order never reaches the arithmetic) and adds the gradients in that
//     order, the reference's order (stable sort by row, sparse_optimizer.cu:657-676); long runs -- a
//     workgroup sorts the positions (LDS bitonic up to kColdLds; beyond that it re-derives them in
//     order by scanning the batch's rows), lane groups sum pieces of 32 consecutive entries, the
//     pieces are added in order.  Every association is a function of the run alone, so the result
//     does not depend on scheduling.  The kernel leaves cnt[] zero again.
// The gradient row of position p: the bucket p itself (through the gradient map) when the batch's
// flag says one key per bucket, else the bucket found by a search of the offsets (bkt[]).
constexpr uint32_t kColdBased = 0x80000000u;
constexpr uint32_t kColdNone = 0xFFFFFFFFu;
constexpr int kColdPer = 8;      // positions per thread (count / scatter)
constexpr int kColdLds = 2048;   // longest run sorted inside LDS
constexpr int kColdPiece = 32;   // entries of a long run summed by one lane group at a time

struct ColdGeom {
  uint32_t n;          // positions
  uint32_t hot_rows;   // H (rows below it belong to the hot kernels while the flag is set)
  uint32_t max_vocab;
  uint32_t map_inner, map_outer;
  uint32_t short_max;  // longest run a lane group sorts (cold_reduce_kernel<LPR>: kShortMax)
  int off_is_u32, combiner;
  size_t buckets;
};

struct ColdBufs {
  uint32_t* cnt;      // [max_vocab] zero between updates
  uint32_t* rank;     // [max_nnz] order of arrival of a position inside its row
  uint32_t* plist;    // [max_nnz] positions of the rows met more than once, row by row
  uint32_t* bkt;      // [max_nnz] bucket of a position (ragged batches only)
  uint2* dlist;       // [max_nnz] (row, first position to arrive)
  uint2* singles;     // [max_nnz] (row, position)
  uint4* segs;        // [max_nnz / 2] short runs: row, base, length
  uint4* longs;       // long runs: row, base, length
  // this update's counters, 128 bytes apart (same-word device-scope atomics cost ~11 ns each and
  // words of one line share that queue): [kCcRows] rows announced; [kCcPl] 64 bits: plist entries
  // handed out | long runs << 32; [kCcSs] 64 bits: short runs | singles << 32
  uint32_t* counts;
  uint32_t* counts_next;
};
constexpr int kCcRows = 0, kCcPl = 32, kCcSs = 64, kCcWords = 96;
constexpr int kColdBlock = 1024;  // count / base / scatter: few, large workgroups = few counter atomics
constexpr int kColdBasePer = 4;   // announced rows per thread of cold_base_kernel

// bucket of key position j: the last u with offset[u] <= j (empty buckets skipped)
__device__ __forceinline__ uint32_t cold_bucket_of(const void* ro_v, bool u32, size_t buckets,
                                                   uint32_t j) {
  size_t lo = 0, hi = buckets;  // offset[lo] <= j < offset[hi]
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    const unsigned long long v = u32 ? (unsigned long long)((const uint32_t*)ro_v)[mid]
                                     : (unsigned long long)((const long long*)ro_v)[mid];
    if (v <= (unsigned long long)j) lo = mid;
    else hi = mid;
  }
  return (uint32_t)lo;
}

__global__ void __launch_bounds__(kColdBlock)
    cold_count_kernel(ColdGeom cg, const uint32_t* __restrict__ one_hot,
                      const void* __restrict__ row_offset, const uint64_t* __restrict__ value_index,
                      ColdBufs cb) {
  __shared__ uint32_t smem[kColdBlock / 64 + 1];
  __shared__ uint32_t sh_base;
  if (blockIdx.x == 0 && threadIdx.x < kCcWords) cb.counts_next[threadIdx.x] = 0u;
  const bool oh = *one_hot != 0u;
  const uint64_t H = oh ? (uint64_t)cg.hot_rows : 0ull;
  const uint32_t p0 = blockIdx.x * (uint32_t)(kColdBlock * kColdPer) + threadIdx.x;
  uint32_t row[kColdPer], rk[kColdPer];
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    const uint32_t p = p0 + (uint32_t)(r * kColdBlock);
    row[r] = kColdNone;
    if (p < cg.n) {
      const uint64_t v = value_index[p];
      if (v >= H && v < (uint64_t)cg.max_vocab) row[r] = (uint32_t)v;
    }
  }
#pragma unroll
  for (int r = 0; r < kColdPer; r++)
    rk[r] = row[r] != kColdNone ? atomicAdd(cb.cnt + row[r], 1u) : 1u;
  uint32_t nlead = 0u;
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    const uint32_t p = p0 + (uint32_t)(r * kColdBlock);
    if (row[r] != kColdNone) {
      cb.rank[p] = rk[r];
      if (!oh) cb.bkt[p] = cold_bucket_of(row_offset, cg.off_is_u32 != 0, cg.buckets, p);
      nlead += rk[r] == 0u ? 1u : 0u;
    }
  }
  uint32_t tot;
  uint32_t ex = block_exclusive_scan<uint32_t, kColdBlock>(nlead, smem, &tot);
  if (threadIdx.x == 0) sh_base = tot > 0u ? atomicAdd(cb.counts + kCcRows, tot) : 0u;
  __syncthreads();
  ex += sh_base;
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    if (row[r] != kColdNone && rk[r] == 0u)
      cb.dlist[ex++] = make_uint2(row[r], p0 + (uint32_t)(r * kColdBlock));
  }
}

__global__ void __launch_bounds__(kColdBlock) cold_base_kernel(ColdGeom cg, ColdBufs cb) {
  __shared__ unsigned long long smem64[kColdBlock / 64 + 1];
  __shared__ unsigned long long smem64b[kColdBlock / 64 + 1];
  __shared__ unsigned long long sh[2];
  constexpr uint32_t kTrip = (uint32_t)(kColdBlock * kColdBasePer);
  const uint32_t nd = cb.counts[kCcRows];
  for (uint32_t i0 = blockIdx.x * kTrip; i0 < nd; i0 += gridDim.x * kTrip) {
    // thread t takes kColdBasePer CONSECUTIVE rows of the trip (one scan covers them)
    uint2 e[kColdBasePer];
    uint32_t c[kColdBasePer];
#pragma unroll
    for (int k = 0; k < kColdBasePer; k++) {
      const uint32_t i = i0 + threadIdx.x * (uint32_t)kColdBasePer + (uint32_t)k;
      e[k] = make_uint2(0u, 0u);
      if (i < nd) e[k] = cb.dlist[i];
    }
#pragma unroll
    for (int k = 0; k < kColdBasePer; k++) {
      const uint32_t i = i0 + threadIdx.x * (uint32_t)kColdBasePer + (uint32_t)k;
      c[k] = i < nd ? cb.cnt[e[k].x] : 0u;
    }
    // two 64-bit scans: plist entries | long runs << 32, and short runs | singles << 32
    unsigned long long a = 0ull, b = 0ull;
#pragma unroll
    for (int k = 0; k < kColdBasePer; k++) {
      if (c[k] > cg.short_max) a += (unsigned long long)c[k] | (1ull << 32);
      else if (c[k] > 1u) {
        a += (unsigned long long)c[k];
        b += 1ull;
      } else if (c[k] == 1u) b += 1ull << 32;
    }
    unsigned long long ta, tb;
    unsigned long long xa = block_exclusive_scan<unsigned long long, kColdBlock>(a, smem64, &ta);
    unsigned long long xb = block_exclusive_scan<unsigned long long, kColdBlock>(b, smem64b, &tb);
    if (threadIdx.x == 0) {
      sh[0] = ta != 0ull ? atomicAdd(reinterpret_cast<unsigned long long*>(cb.counts + kCcPl), ta) : 0ull;
      sh[1] = tb != 0ull ? atomicAdd(reinterpret_cast<unsigned long long*>(cb.counts + kCcSs), tb) : 0ull;
    }
    __syncthreads();
    xa += sh[0];
    xb += sh[1];
#pragma unroll
    for (int k = 0; k < kColdBasePer; k++) {
      if (c[k] == 1u) {
        cb.singles[(uint32_t)(xb >> 32)] = e[k];
        xb += 1ull << 32;
      } else if (c[k] > 1u) {
        const uint32_t base = (uint32_t)xa;
        cb.cnt[e[k].x] = base | kColdBased;
        const uint4 seg = make_uint4(e[k].x, base, c[k], 0u);
        if (c[k] > cg.short_max) {
          cb.longs[(uint32_t)(xa >> 32)] = seg;
          xa += (unsigned long long)c[k] | (1ull << 32);
        } else {
          cb.segs[(uint32_t)xb] = seg;
          xa += (unsigned long long)c[k];
          xb += 1ull;
        }
      }
    }
    __syncthreads();  // (sh is rewritten by the next trip)
  }
}

__global__ void __launch_bounds__(kColdBlock)
    cold_scatter_kernel(ColdGeom cg, const uint32_t* __restrict__ one_hot,
                        const uint64_t* __restrict__ value_index, ColdBufs cb) {
  const uint64_t H = *one_hot != 0u ? (uint64_t)cg.hot_rows : 0ull;
  const uint32_t p0 = blockIdx.x * (uint32_t)(kColdBlock * kColdPer) + threadIdx.x;
  uint32_t row[kColdPer], w[kColdPer], rk[kColdPer];
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    const uint32_t p = p0 + (uint32_t)(r * kColdBlock);
    row[r] = kColdNone;
    if (p < cg.n) {
      const uint64_t v = value_index[p];
      if (v >= H && v < (uint64_t)cg.max_vocab) row[r] = (uint32_t)v;
    }
  }
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    w[r] = row[r] != kColdNone ? cb.cnt[row[r]] : 0u;
    rk[r] = row[r] != kColdNone ? cb.rank[p0 + (uint32_t)(r * kColdBlock)] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kColdPer; r++) {
    if ((w[r] & kColdBased) != 0u)
      cb.plist[(w[r] & ~kColdBased) + rk[r]] = p0 + (uint32_t)(r * kColdBlock);
  }
}

template <int LPR>
struct ColdShape {
  // LDS per workgroup: three arrays of GPB x kEMax words = 24 KB whatever LPR is
  static constexpr int kEMax = 8 * LPR < 256 ? 8 * LPR : 256;   // entries of a slab of short runs
  static constexpr int kShortMax = kEMax < 32 ? kEMax : 32;     // longest short run
  static constexpr int kNS = kEMax / 32 > 0 ? kEMax / 32 : 1;   // short runs per slab
};

template <int LPR, typename GradT, bool kSgd>
__global__ void __launch_bounds__(kBlock)
    cold_reduce_kernel(ColdGeom cg, const uint32_t* __restrict__ one_hot,
                       const void* __restrict__ row_offset,
                       const uint64_t* __restrict__ value_index, const GradT* __restrict__ grad,
                       OptConst o, float* __restrict__ table, float* __restrict__ state0,
                       float* __restrict__ state1, unsigned long long* __restrict__ prev_time,
                       float* __restrict__ gsum, ColdBufs cb) {
  typedef typename Load4<GradT>::raw Raw;
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  constexpr int EMAX = ColdShape<LPR>::kEMax;
  constexpr int NSS = ColdShape<LPR>::kNS;
  constexpr int QB = sizeof(Raw) == 8 ? 16 : 8;
  constexpr int NS1 = kSgd ? 8 : 4;  // singles in flight per lane group
  static_assert(GPB * EMAX * 3 <= 6144 && kColdLds <= 6144, "LDS budget");
  __shared__ uint32_t lds[6144];
  __shared__ uint32_t scan_smem[kBlock / 64 + 1];
  const bool oh = *one_hot != 0u;
  const bool mean = cg.combiner == 1 && !oh;  // (one key per bucket: the mean is the sum)
  const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
  auto grad_row = [&](uint32_t p) -> uint32_t {
    if (!oh) return cb.bkt[p];
    return cg.map_inner ? (p % cg.map_inner) * cg.map_outer + p / cg.map_inner : p;
  };
  auto cvt = [&](const Raw& r, uint32_t b) -> float4 {
    return scaled_grad<GradT>(r, mean ? 1 : 0,
                              mean ? bucket_len(row_offset, cg.off_is_u32 != 0, b) : 1);
  };
  auto add = [](float4& a, const float4& f) {
    a.x += f.x;
    a.y += f.y;
    a.z += f.z;
    a.w += f.w;
  };
  // plain SGD: the row of a finished run is completed when the next one finishes (its read
  // travels meanwhile), as in seg_reduce_kernel
  uint32_t pend_row = kColdNone;
  float4 pend_w = make_float4(0.f, 0.f, 0.f, 0.f), pend_d = pend_w;
  auto pend_flush = [&]() {
    if (pend_row != kColdNone) {
      add(pend_w, pend_d);
      *reinterpret_cast<float4*>(table + (size_t)pend_row * D + l * 4) = pend_w;
      pend_row = kColdNone;
    }
  };
  auto emit = [&](uint32_t row, const float4& a) {
    if constexpr (kSgd) {
      pend_flush();
      pend_d.x = -o.lr * (a.x / o.scaler);
      pend_d.y = -o.lr * (a.y / o.scaler);
      pend_d.z = -o.lr * (a.z / o.scaler);
      pend_d.w = -o.lr * (a.w / o.scaler);
      pend_row = row;
      pend_w = *reinterpret_cast<const float4*>(table + (size_t)row * D + l * 4);
    } else {
      apply_row_vec4<LPR>(o, (uint64_t)row, l, a, table, state0, state1, prev_time);
    }
    if (l == 0) cb.cnt[row] = 0u;  // clean for the next update
  };

  // ---- long runs: one workgroup each --------------------------------------------------------------
  const uint32_t n3 = cb.counts[kCcPl + 1];
  for (uint32_t ir = blockIdx.x; ir < n3; ir += gridDim.x) {
    const uint4 e = cb.longs[ir];
    const uint32_t row = e.x, base = e.y, c = e.z;
    __syncthreads();  // (LDS of the part above / of the previous run is no longer read)
    const uint32_t* sp;  // the run's positions, ascending
    if (c <= 512u) {
      // one pass: an entry's place = the number of entries below it (positions are distinct)
      for (uint32_t q = threadIdx.x; q < c; q += (uint32_t)kBlock) lds[2048 + q] = cb.plist[base + q];
      __syncthreads();
      for (uint32_t q = threadIdx.x; q < c; q += (uint32_t)kBlock) {
        const uint32_t mine = lds[2048 + q];
        uint32_t rnk = 0u;
        for (uint32_t t = 0u; t < c; t++) rnk += lds[2048 + t] < mine ? 1u : 0u;
        lds[rnk] = mine;
      }
      __syncthreads();
      sp = lds;
    } else if (c <= (uint32_t)kColdLds) {
      uint32_t N = 1024u;
      while (N < c) N <<= 1;
      for (uint32_t q = threadIdx.x; q < N; q += (uint32_t)kBlock)
        lds[q] = q < c ? cb.plist[base + q] : kColdNone;
      __syncthreads();
      for (uint32_t k = 2u; k <= N; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
          for (uint32_t t = threadIdx.x; t < (N >> 1); t += (uint32_t)kBlock) {
            const uint32_t lo = ((t / j) * (j << 1)) + (t % j), hi = lo + j;
            const bool up = (lo & k) == 0u;
            const uint32_t a = lds[lo], b = lds[hi];
            if ((a > b) == up) {
              lds[lo] = b;
              lds[hi] = a;
            }
          }
          __syncthreads();
        }
      }
      sp = lds;
    } else {
      // longer than the LDS list: the batch's rows are walked in order and the positions of this
      // row written back over the run's (unordered) entries as they come
      uint32_t filled = 0u;
      for (uint32_t q0 = 0u; q0 < cg.n; q0 += (uint32_t)(kBlock * 4)) {
        const uint32_t p = q0 + threadIdx.x * 4u;
        uint32_t m = 0u;
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (p + (uint32_t)r < cg.n && value_index[p + (uint32_t)r] == (uint64_t)row) m |= 1u << r;
        uint32_t tot;
        uint32_t ex = block_exclusive_scan<uint32_t, kBlock>((uint32_t)__popc(m), scan_smem, &tot);
#pragma unroll
        for (int r = 0; r < 4; r++)
          if ((m >> r) & 1u) cb.plist[base + filled + ex++] = p + (uint32_t)r;
        filled += tot;
      }
      __syncthreads();
      sp = cb.plist + base;
    }
    // pieces of kColdPiece entries, lane group by lane group; the sums wait in gsum[base + first
    // entry] (rows of gsum the hot rows' pool cannot reach: cold entries + hot partials <= n)
    const uint32_t np = (c + (uint32_t)kColdPiece - 1u) / (uint32_t)kColdPiece;
    for (uint32_t k = (uint32_t)g; k < np; k += (uint32_t)GPB) {
      const uint32_t q0 = k * (uint32_t)kColdPiece;
      const uint32_t cntp = c - q0 < (uint32_t)kColdPiece ? c - q0 : (uint32_t)kColdPiece;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int qb = 0; qb < kColdPiece; qb += QB) {
        if ((uint32_t)qb >= cntp) break;
        Raw v[QB];
        uint32_t bb[QB];
#pragma unroll
        for (int t = 0; t < QB; t++) {
          const uint32_t q = (uint32_t)(qb + t) < cntp ? (uint32_t)(qb + t) : cntp - 1u;
          bb[t] = grad_row(sp[q0 + q]);
        }
#pragma unroll
        for (int t = 0; t < QB; t++) v[t] = Load4<GradT>::ld_raw(grad + (size_t)bb[t] * D + l * 4);
#pragma unroll
        for (int t = 0; t < QB; t++)
          if ((uint32_t)(qb + t) < cntp) add(acc, cvt(v[t], bb[t]));
      }
      *reinterpret_cast<float4*>(gsum + (size_t)(base + q0) * D + l * 4) = acc;
    }
    __syncthreads();
    if (g == 0) {
      float4 tot = *reinterpret_cast<const float4*>(gsum + (size_t)base * D + l * 4);
      constexpr int CU = 8;
      for (uint32_t k = 1u; k < np; k += (uint32_t)CU) {
        float4 h[CU];
#pragma unroll
        for (int t = 0; t < CU; t++) {
          const uint32_t kk = k + (uint32_t)t < np ? k + (uint32_t)t : k;
          h[t] = *reinterpret_cast<const float4*>(
              gsum + (size_t)(base + kk * (uint32_t)kColdPiece) * D + l * 4);
        }
#pragma unroll
        for (int t = 0; t < CU; t++)
          if (k + (uint32_t)t < np) add(tot, h[t]);
      }
      apply_row_vec4<LPR>(o, (uint64_t)row, l, tot, table, state0, state1, prev_time);
      if (l == 0) cb.cnt[row] = 0u;
    }
  }
  __syncthreads();  // (the long runs' LDS lists are no longer read)

  // ---- rows met once ---------------------------------------------------------------------------
  const uint32_t n1 = cb.counts[kCcSs + 1];
  for (uint32_t i0 = (blockIdx.x * (uint32_t)GPB + (uint32_t)g) * (uint32_t)NS1; i0 < n1;
       i0 += gridDim.x * (uint32_t)(GPB * NS1)) {
    uint32_t row[NS1], b[NS1];
    Raw v[NS1];
    float4 w[NS1];
#pragma unroll
    for (int k = 0; k < NS1; k++) {
      const uint32_t i = i0 + (uint32_t)k < n1 ? i0 + (uint32_t)k : n1 - 1u;
      const uint2 e = cb.singles[i];
      row[k] = e.x;
      b[k] = grad_row(e.y);
    }
#pragma unroll
    for (int k = 0; k < NS1; k++) {
      v[k] = Load4<GradT>::ld_raw(grad + (size_t)b[k] * D + l * 4);
      if constexpr (kSgd) w[k] = *reinterpret_cast<const float4*>(table + (size_t)row[k] * D + l * 4);
    }
#pragma unroll
    for (int k = 0; k < NS1; k++) {
      if (i0 + (uint32_t)k < n1) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        add(a, cvt(v[k], b[k]));
        if constexpr (kSgd) {
          w[k].x += -o.lr * (a.x / o.scaler);
          w[k].y += -o.lr * (a.y / o.scaler);
          w[k].z += -o.lr * (a.z / o.scaler);
          w[k].w += -o.lr * (a.w / o.scaler);
          *reinterpret_cast<float4*>(table + (size_t)row[k] * D + l * 4) = w[k];
        } else {
          apply_row_vec4<LPR>(o, (uint64_t)row[k], l, a, table, state0, state1, prev_time);
        }
        if (l == 0) cb.cnt[row[k]] = 0u;
      }
    }
  }

  // ---- short runs: NSS of them per lane group and trip ------------------------------------------
  {
    uint32_t* raw = lds + (size_t)g * (3 * EMAX);
    uint32_t* srt = raw + EMAX;
    uint32_t* erow = srt + EMAX;
    const uint32_t n2 = cb.counts[kCcSs];
    for (uint32_t i0 = (blockIdx.x * (uint32_t)GPB + (uint32_t)g) * (uint32_t)NSS; i0 < n2;
         i0 += gridDim.x * (uint32_t)(GPB * NSS)) {
      uint32_t srow[NSS], sbase[NSS], soff[NSS + 1];
      soff[0] = 0u;
#pragma unroll
      for (int j = 0; j < NSS; j++) {
        srow[j] = kColdNone;
        sbase[j] = 0u;
        soff[j + 1] = soff[j];
        if (i0 + (uint32_t)j < n2) {
          const uint4 e = cb.segs[i0 + (uint32_t)j];
          srow[j] = e.x;
          sbase[j] = e.y;
          soff[j + 1] = soff[j] + e.z;
        }
      }
      const uint32_t E = soff[NSS];
      __builtin_amdgcn_wave_barrier();  // (the previous trip's reads of the lists are done)
      for (uint32_t q = (uint32_t)l; q < E; q += (uint32_t)LPR) {
        uint32_t bs = sbase[0], of = 0u, rw = srow[0];
#pragma unroll
        for (int j = 1; j < NSS; j++) {
          if (q >= soff[j]) {
            bs = sbase[j];
            of = soff[j];
            rw = srow[j];
          }
        }
        raw[q] = cb.plist[bs + (q - of)];
        erow[q] = rw;
      }
      __builtin_amdgcn_wave_barrier();
      // the run's positions in ascending order: rank = entries of the run below mine
      for (uint32_t q = (uint32_t)l; q < E; q += (uint32_t)LPR) {
        uint32_t s0 = 0u, s1 = soff[1];
#pragma unroll
        for (int j = 1; j < NSS; j++) {
          if (q >= soff[j]) {
            s0 = soff[j];
            s1 = soff[j + 1];
          }
        }
        const uint32_t mine = raw[q];
        uint32_t rnk = 0u;
        for (uint32_t t = s0; t < s1; t++) rnk += raw[t] < mine ? 1u : 0u;
        srt[s0 + rnk] = mine;
      }
      __builtin_amdgcn_wave_barrier();
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      uint32_t cur = erow[0];
#pragma unroll 1
      for (uint32_t qb = 0; qb < E; qb += (uint32_t)QB) {
        Raw v[QB];
        uint32_t bb[QB];
#pragma unroll
        for (int k = 0; k < QB; k++) {
          const uint32_t q = qb + (uint32_t)k < E ? qb + (uint32_t)k : E - 1u;
          bb[k] = grad_row(srt[q]);
        }
#pragma unroll
        for (int k = 0; k < QB; k++) v[k] = Load4<GradT>::ld_raw(grad + (size_t)bb[k] * D + l * 4);
#pragma unroll
        for (int k = 0; k < QB; k++) {
          const uint32_t q = qb + (uint32_t)k;
          if (q < E) {
            const uint32_t rw = erow[q];
            if (rw != cur) {
              emit(cur, acc);
              acc = make_float4(0.f, 0.f, 0.f, 0.f);
              cur = rw;
            }
            add(acc, cvt(v[k], bb[k]));
          }
        }
      }
      emit(cur, acc);
    }
    if constexpr (kSgd) pend_flush();
  }

}

__global__ void __launch_bounds__(kBlock) cold_clear_kernel(ColdBufs cb) {
  const uint32_t nd = cb.counts[kCcRows];
  for (uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x; i < nd;
       i += gridDim.x * (uint32_t)kBlock)
    cb.cnt[cb.dlist[i].x] = 0u;
}

// chunks the per-chunk tables have room for
inline uint32_t hot_chunks_max(const SparseUpdater& u) {
  return (uint32_t)(ceil_div<size_t>(u.max_nnz, (size_t)kHotChunk) + kHotMaxStreams);
}

}  // namespace

// What the hot / cold path keeps between calls.  The buffers are the structs the kernels take; the
// plan is what the kernels of one batch share (geometry, this batch's counter sets), built once per
// batch -- by SparseUpdater::prework() right after the index stage (the grouping work needs the
// rows only, not the gradients: hot_sort_kernel and the cold rows' count / base / scatter then run
// on side streams under the dense tower) or by the update itself.
struct HotColdState {
  std::vector<void*> owned;       // the device buffers below, as hot_buffers() allocated them
  hipStream_t cold_s = nullptr;   // the cold pairs' chain (default priority)
  HotBufs hb = {};                // (hb.loc != nullptr <=> the set is complete)
  ColdBufs cb = {};
  uint32_t* hot_counts = nullptr;   // two alternating sets {pool slots, items, joins, -}
  uint32_t* cold_counts = nullptr;  // two alternating sets of kCcWords
  uint32_t parity = 0;              // set the next batch takes
  // ---- the batch in hand --------------------------------------------------------------------
  bool valid = false;  // the grouping kernels of (vi, n, buckets) are enqueued; the reduces are not
  const uint64_t* vi = nullptr;
  size_t n = 0, buckets = 0;
  size_t n_chunks = 0;
  int lpr = 0;
  HotGeom hg = {};
  ColdGeom cg = {};
  hipEvent_t ev_hot = nullptr, ev_cold = nullptr;
};

namespace {

// everything the path asks of a batch except what only the update knows (gradient alignment,
// store-only mode)
bool plan_possible(const SparseUpdater& u, size_t buckets, size_t nnz) {
  const uint32_t G = u.hot_streams;
  if (!(u.hot_rows > 0 && u.one_hot_flag != nullptr && G > 0 && G <= kHotMaxStreams &&
        nnz == buckets && nnz >= u.hot_min_n && nnz < 0x7FFFFFF0ull && lpr_supported(u.D) &&
        u.scale_row_offset == nullptr))
    return false;
  // (a gradient map -- the embedding_collection's transposed read -- is applied by the cold chain
  //  for one-hot batches only, cold_reduce_kernel's grad_row(); a ragged batch with nnz == buckets
  //  would read unmapped rows there: the sorting path, which maps in every case, takes those)
  if (u.map_inner != 0u) return false;
  const size_t per_g = ceil_div<size_t>(nnz, (size_t)G);
  const size_t n_chunks = (size_t)G * ceil_div<size_t>(per_g, (size_t)kHotChunk);
  return n_chunks <= (size_t)hot_chunks_max(u) && n_chunks <= (size_t)kHotApplyChunks;
}

inline void plan_build(SparseUpdater& u, HotColdState& hc, size_t buckets, size_t nnz, int combiner,
                       bool off_is_u32, const uint64_t* vi) {
  const uint32_t G = u.hot_streams;
  const size_t per_g = ceil_div<size_t>(nnz, (size_t)G);
  const size_t cpg = ceil_div<size_t>(per_g, (size_t)kHotChunk);
  hc.vi = vi;
  hc.n = nnz;
  hc.buckets = buckets;
  hc.n_chunks = (size_t)G * cpg;
  hc.lpr = u.D / 4;
  hc.hg.n = (uint32_t)nnz;
  hc.hg.G = G;
  hc.hg.cpg = (uint32_t)cpg;
  hc.hg.rows = u.hot_rows;
  hc.hg.map_inner = u.map_inner;
  hc.hg.map_outer = u.map_outer;
  hc.hg.loc_stride = hot_chunks_max(u);
  hc.cg.n = (uint32_t)nnz;
  hc.cg.hot_rows = u.hot_rows;
  hc.cg.max_vocab = (uint32_t)u.max_vocab;
  hc.cg.map_inner = u.map_inner;
  hc.cg.map_outer = u.map_outer;
  hc.cg.short_max =
      (uint32_t)with_lpr(hc.lpr, [](auto L) { return ColdShape<decltype(L)::value>::kShortMax; });
  hc.cg.off_is_u32 = off_is_u32 ? 1 : 0;
  hc.cg.combiner = combiner;
  hc.cg.buckets = buckets;
  // counter sets alternate: hot [0..3] / [4..7], cold [0..kCcWords) / [kCcWords..)
  hc.hb.counts = hc.hot_counts + 4 * (hc.parity & 1u);
  hc.hb.counts_next = hc.hot_counts + 4 * ((hc.parity + 1u) & 1u);
  hc.cb.counts = hc.cold_counts + kCcWords * (hc.parity & 1u);
  hc.cb.counts_next = hc.cold_counts + kCcWords * ((hc.parity + 1u) & 1u);
  hc.parity++;
}

// the grouping kernels of a planned batch: the hot rows' chunk sort on hs, the cold rows' count /
// base / scatter on cs
inline int plan_launch_grouping(SparseUpdater& u, HotColdState& hc, const void* ro, hipStream_t hs,
                                hipStream_t cs) {
  hipLaunchKernelGGL(hot_sort_kernel, dim3((unsigned)hc.n_chunks), dim3(kHotBlock), 0, hs, hc.hg,
                     u.one_hot_flag, hc.vi, hc.hb);
  HCTR_LAUNCH_CHECK();
  const unsigned pgrid = (unsigned)ceil_div<size_t>(hc.n, (size_t)(kColdBlock * kColdPer));
  const unsigned bgrid = (unsigned)grid_for(hc.n, kColdBlock * kColdBasePer, 256);
  hipLaunchKernelGGL(cold_count_kernel, dim3(pgrid), dim3(kColdBlock), 0, cs, hc.cg,
                     u.one_hot_flag, ro, hc.vi, hc.cb);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cold_base_kernel, dim3(bgrid), dim3(kColdBlock), 0, cs, hc.cg, hc.cb);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cold_scatter_kernel, dim3(pgrid), dim3(kColdBlock), 0, cs, hc.cg,
                     u.one_hot_flag, hc.vi, hc.cb);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// a batch whose grouping kernels ran ahead but whose update takes another path (or never comes):
// the per-row words go back to zero.  Nothing grouped ahead: a no-op
int plan_discard(SparseUpdater& u, hipStream_t s) {
  HotColdState* hc = u.hot_cold;
  if (hc == nullptr || !hc->valid) return HCTR_OK;
  HCTR_HIP(hipStreamWaitEvent(s, hc->ev_hot, 0));
  HCTR_HIP(hipStreamWaitEvent(s, hc->ev_cold, 0));
  hipLaunchKernelGGL(cold_clear_kernel, dim3(grid_for(hc->n, kBlock, 1024)), dim3(kBlock), 0, s,
                     hc->cb);
  HCTR_LAUNCH_CHECK();
  hc->valid = false;
  return HCTR_OK;
}

// any D: one wavefront per run, lanes stride over the vector
template <typename OffT, typename GradT>
__global__ void __launch_bounds__(kBlock)
    update_rows_generic_kernel(const uint64_t* __restrict__ d_num_runs,
                               const uint32_t* __restrict__ run_start,
                               const uint32_t* __restrict__ sorted_rows,
                               const uint32_t* __restrict__ sorted_buckets,
                               const OffT* __restrict__ scale_ro, int combiner, int D,
                               const GradT* __restrict__ grad, OptConst o,
                               float* __restrict__ table, float* __restrict__ state0,
                               float* __restrict__ state1,
                               unsigned long long* __restrict__ prev_time) {
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const size_t nwaves = ((size_t)gridDim.x * kBlock) >> 6;
  const size_t num_runs = (size_t)*d_num_runs;
  for (size_t r = wave; r < num_runs; r += nwaves) {
    const uint32_t off = run_start[r];
    const uint32_t cnt = run_start[r + 1] - off;
    const uint64_t row = (uint64_t)sorted_rows[off];
    if (row == kNoRow) continue;
    auto grad_of = [&](uint32_t k, int v) -> float {
      const uint32_t b = sorted_buckets[off + k];
      float gv = Load4<GradT>::ld1(grad + (size_t)b * D + v);
      if (combiner == 1) {
        long long n = (long long)scale_ro[b + 1] - (long long)scale_ro[b];
        if (n > 1) {
          const float sc = 1.0f / (float)n;  // even sizes: align2 rule (16-bit scaler)
          gv = Load4<GradT>::rnd(gv * (D % 2 == 0 ? Load4<GradT>::rnd(sc) : sc));
        }
      }
      return gv;
    };
    // A LONG run of a short vector (the wide tables of Wide & Deep: D = 1, a hot row met tens of
    // thousands of times): with one lane per element the wavefront would walk the run with 1 .. 32
    // lanes, two dependent loads per entry (measured: 1.75 ms per step for three D = 1 tables at
    // batch 16384).  Instead 64 / L lane groups (L = D rounded up to a power of two) take every
    // (64 / L)-th entry each, in ascending order, and their partial sums are combined by a fixed
    // butterfly -- an association that depends on the run's length only.  Runs of up to 64 entries
    // keep the plain ascending sum.
    if (D <= 32 && cnt > 64u) {
      int L = 1;
      while (L < D) L <<= 1;
      const int G = 64 / L, g = lane / L, v = lane % L;
      float part = 0.0f;
      if (v < D)
        for (uint32_t k = (uint32_t)g; k < cnt; k += (uint32_t)G) part += grad_of(k, v);
      for (int ofs = 32; ofs >= L; ofs >>= 1) part += __shfl_xor(part, ofs, 64);
      if (g == 0 && v < D) {
        const float gi = part / o.scaler;
        const size_t f = row * (uint64_t)D + v;
        float w = table[f];
        float s0 = needs_s0(o) ? ld_state1(state0, f, o.state_half) : 0.f;
        float s1 = needs_s1(o) ? ld_state1(state1, f, o.state_half) : 0.f;
        unsigned long long pt = needs_pt(o) ? prev_time[f] : 1ull;
        apply_opt(o, gi, w, &s0, &s1, &pt);
        table[f] = w;
        if (needs_s0(o)) st_state1(state0, f, o.state_half, s0);
        if (needs_s1(o)) st_state1(state1, f, o.state_half, s1);
        if (needs_pt(o)) prev_time[f] = pt;
      }
      continue;
    }
    for (int v = lane; v < D; v += 64) {
      float gi = 0.0f;
      for (uint32_t k = 0; k < cnt; k++) gi += grad_of(k, v);
      gi /= o.scaler;
      const size_t f = row * (uint64_t)D + v;
      float w = table[f];
      float s0 = needs_s0(o) ? ld_state1(state0, f, o.state_half) : 0.f;
      float s1 = needs_s1(o) ? ld_state1(state1, f, o.state_half) : 0.f;
      unsigned long long pt = needs_pt(o) ? prev_time[f] : 1ull;
      apply_opt(o, gi, w, &s0, &s1, &pt);
      table[f] = w;
      if (needs_s0(o)) st_state1(state0, f, o.state_half, s0);
      if (needs_s1(o)) st_state1(state1, f, o.state_half, s1);
      if (needs_pt(o)) prev_time[f] = pt;
    }
  }
}

// SGD with atomic_update (opt_sgd_atomic_kernel :564-582): w[idx] += -(lr/scaler) * wgrad[bucket]
template <typename OffT, typename GradT>
__global__ void __launch_bounds__(kBlock)
    sgd_atomic_kernel(size_t buckets, int D, int combiner, const OffT* __restrict__ row_offset,
                      const uint64_t* __restrict__ value_index, const GradT* __restrict__ grad,
                      float lr_scale, float* __restrict__ table,
                      const OffT* __restrict__ scale_ro) {
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const size_t nwaves = ((size_t)gridDim.x * kBlock) >> 6;
  for (size_t u = wave; u < buckets; u += nwaves) {
    const long long off = (long long)row_offset[u];
    const int n = (int)((long long)row_offset[u + 1] - off);
    // (the scaling CSR is read for the mean combiner only)
    const int ns = combiner == 1 ? (int)((long long)scale_ro[u + 1] - (long long)scale_ro[u]) : 1;
    float sc = (combiner == 1 && ns > 1) ? 1.0f / (float)ns : 1.0f;
    if (D % 2 == 0) sc = Load4<GradT>::rnd(sc);  // align2 rule (backward_functor.cu:83-104)
    for (int v = lane; v < D; v += 64) {
      float gv = Load4<GradT>::ld1(grad + u * (size_t)D + v);
      if (combiner == 1) gv = Load4<GradT>::rnd(gv * sc);
      const float dw = -lr_scale * gv;
      for (int j = 0; j < n; j++) {
        const uint64_t idx = value_index[off + j];
        if (idx != kInvalidIndex) unsafeAtomicAdd(table + idx * (uint64_t)D + v, dw);
      }
    }
  }
}

// ---- global (whole-table) sweeps ----------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
    adam_global_sweep_kernel(size_t n, float beta1, float beta2, float eps, float alpha_t,
                             int state_half, float* __restrict__ m, float* __restrict__ v,
                             float* __restrict__ w) {
  // adam_update_kernel_global :269-288
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kBlock) {
    float mi = beta1 * ld_state1(m, i, state_half);
    float vi = beta2 * ld_state1(v, i, state_half);
    st_state1(m, i, state_half, state_store(state_half, mi));
    st_state1(v, i, state_half, state_store(state_half, vi));
    w[i] += -alpha_t * mi / (sqrtf(vi) + eps);
  }
}

__global__ void __launch_bounds__(kBlock)
    momentum_global_sweep_kernel(size_t n, float factor, int state_half, float* __restrict__ mo,
                                 float* __restrict__ w) {
  // momentum_sgd_update_kernel_global :316-329
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kBlock) {
    float m = ld_state1(mo, i, state_half);
    m *= factor;
    w[i] += m;
    st_state1(mo, i, state_half, state_store(state_half, m));
  }
}

__global__ void __launch_bounds__(kBlock)
    nesterov_global_sweep_kernel(size_t n, float mu, int state_half, float* __restrict__ accm,
                                 float* __restrict__ w) {
  // nesterov_global_update_kernel_global :333-347
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kBlock) {
    float a = ld_state1(accm, i, state_half);
    a *= mu;
    st_state1(accm, i, state_half, state_store(state_half, a));
    w[i] += a * mu;
  }
}

// ---- wgrad materialisation (tests / get_wgrad) --------------------------------------------------
template <typename OffT, typename GradT>
__global__ void __launch_bounds__(kBlock)
    wgrad_kernel(size_t buckets, int D, int combiner, const OffT* __restrict__ row_offset,
                 const GradT* __restrict__ top, GradT* __restrict__ wgrad) {
  const size_t total = buckets * (size_t)D;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const size_t u = i / D;
    float g = Load4<GradT>::ld1(top + i);
    if (combiner == 1) {
      long long n = (long long)row_offset[u + 1] - (long long)row_offset[u];
      if (n > 1) {
        const float sc = 1.0f / (float)n;
        g = g * (D % 2 == 0 ? Load4<GradT>::rnd(sc) : sc);
        // the product first, THEN the conversion: without the barrier the compiler folds
        // convert * scaler -> convert into one mixed-precision fma(g, sc, +0), and -0 + +0 is
        // +0: a gradient of -0.0 came back as +0.0 (the reference's __hmul2 keeps the sign)
        asm volatile("" : "+v"(g));
      }
    }
    if constexpr (std::is_same<GradT, float>::value) wgrad[i] = g;
    else if constexpr (std::is_same<GradT, __half>::value) wgrad[i] = __float2half_rn(g);
    else wgrad[i] = __float2bfloat16(g);
  }
}

// (row, bucket) pairs -> stable radix sort by row (sparse_optimizer.cu:657-676); stage 2 of the
// profiler brackets the sort
template <typename OffT>
int sort_stage(SparseUpdater& u, size_t buckets, size_t n, const OffT* ro, const uint64_t* vi,
               hipStream_t s) {
  // wavefronts per 64-bucket chunk = the average bucket length (for_each_key_wave): one for
  // one-hot input, 8 for the MLPerf multi-hot shape whose 100-hot table would otherwise be the tail
  const size_t avg = buckets > 0 ? (n + buckets - 1) / buckets : 1;
  const unsigned parts = (unsigned)(avg < 1 ? 1 : (avg > 16 ? 16 : avg));
  // one key per bucket on the host's count AND on the device's word (the index stage checked the
  // offsets): rows and payloads are read in place by the sort's first pass
  const RsFirst first = {vi, u.one_hot_flag, u.map_inner, u.map_outer};
  const bool in_place = u.one_hot_flag != nullptr && n == buckets;
  hipLaunchKernelGGL((expand_pairs_kernel<OffT>), dim3(grid_for(buckets, kBlock), parts),
                     dim3(kBlock), 0, s, buckets, n, ro, vi, u.sort_keys_in, u.sort_vals_in,
                     u.span_count, u.map_inner, u.map_outer, in_place ? u.one_hot_flag : nullptr);
  HCTR_LAUNCH_CHECK();
  // end_bit = log2(max_vocab)+1 (sparse_optimizer.cu:663).  The padding key and the key of a
  // position without a row are all ones: inside end_bit bits they are 2^end_bit - 1, above every
  // live row (rows < top <= 2^end_bit - 1), so they sort last without a bit of their own
  int end_bit = 1;
  // (row_bound: the caller may know that only the first row_bound rows of the table exist yet)
  const size_t top = (u.row_bound > 0 && u.row_bound < u.max_vocab) ? u.row_bound : u.max_vocab;
  while (end_bit < 32 && ((size_t)1 << end_bit) <= top) end_bit++;
  if (u.prof) u.prof->begin(2, s);
  HCTR_TRY(radix_sort_pairs_u32(u.sort_temp, u.sort_temp_bytes, u.sort_keys_in, u.sort_keys_out,
                                u.sort_vals_in, u.sort_vals_out, n, end_bit, s,
                                in_place ? &first : nullptr));
  if (u.prof) u.prof->end(2, s);
  return HCTR_OK;
}

// Global update types sweep the table (sparse_optimizer.cu:269-347 run over all
// max_vocabulary_size_per_gpu rows).  A row that was never handed out has zero state,
// and zero state is a fixed point of every sweep (m = v = 0 stay 0, w += -alpha * 0 / (0 + eps)
// leaves w's bits alone): sweeping the rows handed out so far -- row_bound, the same upper bound
// the sort's key width uses -- gives the identical table for a fraction of the traffic while a
// table fills up (DeepFM / Criteo-Kaggle, 33.7 M rows x 16: 12.9 GB per step down to the live rows).
inline size_t swept_elems(const SparseUpdater& u) {
  const size_t live_rows = (u.row_bound > 0 && u.row_bound < u.max_vocab) ? u.row_bound : u.max_vocab;
  return live_rows * (size_t)u.D;
}

// the sweep that runs before the rows of the batch are updated (Nesterov)
inline int global_sweep_before(const SparseUpdater& u, const OptState& opt, float* table,
                               float* state0, hipStream_t s) {
  if (!(opt.optimizer == HCTR_OPT_NESTEROV && opt.update_type == HCTR_UPDATE_GLOBAL))
    return HCTR_OK;
  const size_t n = swept_elems(u);
  hipLaunchKernelGGL(nesterov_global_sweep_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s,
                     n, opt.momentum_factor, opt.state_half, state0, table);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// the sweep that runs after them (Adam, momentum SGD)
inline int global_sweep_after(const SparseUpdater& u, const OptState& opt, const OptConst& o,
                              float* table, float* state0, float* state1, hipStream_t s) {
  if (opt.update_type != HCTR_UPDATE_GLOBAL) return HCTR_OK;
  const size_t n = swept_elems(u);
  if (opt.optimizer == HCTR_OPT_ADAM) {
    hipLaunchKernelGGL(adam_global_sweep_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, n,
                       opt.beta1, opt.beta2, opt.epsilon, o.alpha_t, opt.state_half, state0,
                       state1, table);
    HCTR_LAUNCH_CHECK();
  } else if (opt.optimizer == HCTR_OPT_MOMENTUM_SGD) {
    hipLaunchKernelGGL(momentum_global_sweep_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s,
                       n, opt.momentum_factor, opt.state_half, state0, table);
    HCTR_LAUNCH_CHECK();
  }
  return HCTR_OK;
}

// SGD with atomic_update: every (bucket, key) adds its scaled gradient to its row, nothing sorted
template <typename OffT, typename GradT>
int update_sgd_atomic(const SparseUpdater& u, size_t buckets, int combiner, const OffT* ro,
                      const OffT* sro, const uint64_t* vi, const GradT* grad, const OptState& opt,
                      float* table, hipStream_t s) {
  const float lr_scale = opt.lr / opt.scaler;
  hipLaunchKernelGGL((sgd_atomic_kernel<OffT, GradT>), dim3(grid_for(buckets * 64, kBlock)),
                     dim3(kBlock), 0, s, buckets, u.D, combiner, ro, vi, grad, lr_scale, table,
                     sro);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

inline int pairs_source(SparseUpdater& u, size_t buckets, size_t nnz, const uint64_t* vi,
                        hipStream_t s, SortedPairs& p) {
  p = {u.sort_keys_out, u.sort_vals_out, nnz, false};
  if (u.ext_rows != nullptr) {
    // presorted by the caller: only the long-run counters need a reset
    p.rows = u.ext_rows;
    p.buckets = u.ext_buckets;
    HCTR_HIP(hipMemsetAsync(u.span_count, 0, 4 * sizeof(uint32_t), s));
  } else if (u.early_n >= nnz && u.early_vi == vi && u.early_buckets == buckets) {
    // (row, bucket) pairs of this batch were sorted on the side stream right after the index
    // stage (SparseUpdater::presort); padding keys sit behind the live ones
    HCTR_HIP(hipStreamWaitEvent(s, u.ev_sorted, 0));
    p.n = u.early_n;
  } else {
    p.need_sort = true;
  }
  u.early_n = 0;
  return HCTR_OK;
}

// Hot rows of a one-hot batch (see hot_sort_kernel) on s, the cold rows' chain (see
// cold_count_kernel) on the side stream; they touch disjoint rows.  pre: prework() enqueued the
// grouping kernels of this batch already.  Stage 2 of the profiler = fork .. join, all of the
// update.
template <typename GradT>
int update_hot_cold(SparseUpdater& u, HotColdState& hc, bool pre, size_t buckets, size_t nnz,
                          int combiner, const void* ro, bool off_is_u32, const uint64_t* vi,
                          const GradT* grad, const OptConst& o, float* table, float* state0,
                          float* state1, uint64_t* prev_time, hipStream_t s) {
  if (!pre) plan_build(u, hc, buckets, nnz, combiner, off_is_u32, vi);
  hipStream_t cs = hc.cold_s;  // the cold chain's stream
  if (u.prof) u.prof->begin(2, s);
  HCTR_HIP(hipEventRecord(u.ev_fork, s));
  HCTR_HIP(hipStreamWaitEvent(cs, u.ev_fork, 0));
  if (pre) {  // grouped ahead (prework): the reduces wait for their chain's kernels only
    HCTR_HIP(hipStreamWaitEvent(s, hc.ev_hot, 0));
    HCTR_HIP(hipStreamWaitEvent(cs, hc.ev_cold, 0));
    hc.valid = false;
  } else {
    HCTR_TRY(plan_launch_grouping(u, hc, ro, s, cs));
  }
  float* pool_end = u.gsum + u.max_nnz * (size_t)u.D;
  const size_t items_max = nnz / kHotTile + hc.n_chunks;
  // the hot rows' reduce is a grid-stride loop over a bounded number of workgroups: a kernel
  // that queues one workgroup per tile fills every wave slot of the device and the other
  // chain only trickles in (measured, round 4: its scatter 21 -> 96 us; 768 workgroups: 60)
  constexpr int kColdGrid = 2048, kHotGrid = 768;
  HCTR_TRY(with_lpr(hc.lpr, [&](auto L) -> int {
    constexpr int LPR = decltype(L)::value;
    constexpr int GPB = kBlock / LPR;
    with_bool(o.optimizer == HCTR_OPT_SGD, [&](auto sgd) {
      hipLaunchKernelGGL((cold_reduce_kernel<LPR, GradT, decltype(sgd)::value>), dim3(kColdGrid),
                         dim3(kBlock), 0, cs, hc.cg, u.one_hot_flag, ro, vi, grad, o, table, state0,
                         state1, (unsigned long long*)prev_time, u.gsum, hc.cb);
    });
    HCTR_LAUNCH_CHECK();
    hipLaunchKernelGGL((hot_reduce_kernel<LPR, GradT>), dim3(grid_for(items_max, GPB, kHotGrid)),
                       dim3(kBlock), 0, s, hc.hg, u.one_hot_flag, grad, pool_end, hc.hb);
    HCTR_LAUNCH_CHECK();
    hipLaunchKernelGGL((hot_join_kernel<LPR>), dim3(grid_for(items_max / 8 + 1, GPB, 2048)),
                       dim3(kBlock), 0, s, hc.hg, u.one_hot_flag, pool_end, hc.hb);
    HCTR_LAUNCH_CHECK();
    hipLaunchKernelGGL((hot_apply_kernel<LPR>), dim3(grid_for(u.hot_rows, GPB)), dim3(kBlock), 0,
                       s, hc.hg, (uint32_t)hc.n_chunks, u.one_hot_flag, o, table, state0, state1,
                       (unsigned long long*)prev_time, (const float*)pool_end, hc.hb);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }));
  // join: the cold chain's end is ordered before whatever follows on s
  HCTR_HIP(hipEventRecord(u.ev_sorted, cs));
  HCTR_HIP(hipStreamWaitEvent(s, u.ev_sorted, 0));
  if (u.prof) u.prof->end(2, s);
  return HCTR_OK;
}

// any other embedding_vec_size: run detection + one wavefront per unique row
template <typename OffT, typename GradT>
int update_generic(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner,
                   const OffT* ro, const OffT* sro, const GradT* grad, const OptConst& o,
                   float* table, float* state0, float* state1, uint64_t* prev_time,
                   hipStream_t s) {
  const size_t n_tiles = ceil_div<size_t>(p.n, kTile);
  const int tgrid = (int)(n_tiles < (size_t)kMaxGrid ? n_tiles : (size_t)kMaxGrid);
  hipLaunchKernelGGL((run_count_kernel<OffT>), dim3(tgrid), dim3(kBlock), 0, s, p.rows, ro,
                     buckets, n_tiles, u.tile_sums);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_tiles_u32_kernel, dim3(1), dim3(1024), 0, s, u.tile_sums, n_tiles,
                     u.d_num_runs);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL((run_write_kernel<OffT>), dim3(tgrid), dim3(kBlock), 0, s, p.rows, ro,
                     buckets, n_tiles, u.tile_sums, u.d_num_runs, u.run_start);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL((update_rows_generic_kernel<OffT, GradT>), dim3(grid_for(p.n * 64, kBlock)),
                     dim3(kBlock), 0, s, u.d_num_runs, u.run_start, p.rows, p.buckets, sro,
                     combiner, u.D, grad, o, table, state0, state1, (unsigned long long*)prev_time);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int update_typed(SparseUpdater& u, size_t buckets, size_t nnz, int combiner, const void* ro,
                 int key_type, const uint64_t* vi, const void* grad, int grad_dtype,
                 const OptState& opt, float* table, float* state0, float* state1,
                 uint64_t* prev_time, hipStream_t s) {
  const void* sro = u.scale_row_offset ? u.scale_row_offset : ro;
  const OptConst o = opt_const(opt);
  if (u.map_inner != 0u) {
    if (combiner != 0 || u.ext_rows != nullptr || (opt.optimizer == HCTR_OPT_SGD && opt.atomic_update) ||
        (size_t)u.map_inner * u.map_outer != buckets) {
      set_error("gradient map: sum combiner, sorted update, samples * lookups == buckets only");
      return HCTR_ERR_INVALID_ARG;
    }
  }
  const bool u32 = key_type == HCTR_KEY_U32;
  if (opt.optimizer == HCTR_OPT_SGD && opt.atomic_update)
    return with_types(key_type, grad_dtype, [&](auto* off, auto* g) -> int {
      return update_sgd_atomic(u, buckets, combiner, (decltype(off))ro, (decltype(off))sro, vi,
                               (decltype(g))grad, opt, table, s);
    });
  HCTR_TRY(global_sweep_before(u, opt, table, state0, s));
  if (nnz > 0) {
    SortedPairs p;
    HCTR_TRY(pairs_source(u, buckets, nnz, vi, s, p));
    const bool a16 = reinterpret_cast<uintptr_t>(grad) % 16 == 0;
    float* direct = (opt.optimizer == kOptStoreSum && opt.scaler == 1.0f) ? table : nullptr;
    const HotColdState* hc = u.hot_cold;
    const bool hot = p.need_sort && a16 && direct == nullptr && plan_possible(u, buckets, nnz);
    const bool pre = hot && hc != nullptr && hc->valid && hc->vi == vi && hc->n == nnz &&
                     hc->buckets == buckets;
    if (!pre) HCTR_TRY(plan_discard(u, s));
    if (hot) {
      HCTR_TRY(u.hot_buffers(s));
      HCTR_TRY(with_dtype(grad_dtype, [&](auto* g) -> int {
        return update_hot_cold(u, *u.hot_cold, pre, buckets, nnz, combiner, ro, u32, vi,
                               (decltype(g))grad, o, table, state0, state1, prev_time, s);
      }));
    } else {
      if (p.need_sort)
        HCTR_TRY(u32 ? sort_stage(u, buckets, nnz, (const uint32_t*)ro, vi, s)
                     : sort_stage(u, buckets, nnz, (const long long*)ro, vi, s));
      if (u.prof) u.prof->begin(3, s);
      if (a16 && lpr_supported(u.D))
        HCTR_TRY((u32 ? update_segmented_u32 : update_segmented_i64)(
            u, p, buckets, combiner, ro, sro, grad, grad_dtype, opt, direct, table, state0, state1,
            prev_time, s));
      else
        HCTR_TRY(with_types(key_type, grad_dtype, [&](auto* off, auto* g) -> int {
          return update_generic(u, p, buckets, combiner, (decltype(off))ro, (decltype(off))sro,
                                (decltype(g))grad, o, table, state0, state1, prev_time, s);
        }));
      if (u.prof) u.prof->end(3, s);
    }
  }
  return global_sweep_after(u, opt, o, table, state0, state1, s);
}

void free_hot_cold(SparseUpdater& u) {
  HotColdState* hc = u.hot_cold;
  if (hc == nullptr) return;
  for (void* p : hc->owned) (void)hipFree(p);
  if (hc->ev_hot) (void)hipEventDestroy(hc->ev_hot);
  if (hc->ev_cold) (void)hipEventDestroy(hc->ev_cold);
  if (hc->cold_s) {
    (void)hipStreamSynchronize(hc->cold_s);
    (void)hipStreamDestroy(hc->cold_s);
  }
  delete hc;
  u.hot_cold = nullptr;
}

}  // namespace

int SparseUpdater::create(size_t max_nnz_, size_t max_vocab_, int D_, bool eager_hot) {
  max_nnz = max_nnz_ > 0 ? max_nnz_ : 1;
  max_vocab = max_vocab_;
  D = D_;
  // row indices are sorted as 32-bit keys
  if (max_vocab >= 0xFFFFFFF0ull) {
    set_error("more than 2^32 - 16 rows per GPU are not supported by the sparse update");
    return HCTR_ERR_UNSUPPORTED;
  }
  HCTR_TRY(dev_alloc(owned, sort_keys_in, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(owned, sort_keys_out, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(owned, sort_vals_in, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(owned, sort_vals_out, max_nnz * sizeof(uint32_t)));
  sort_temp_bytes = radix_sort_temp_bytes(max_nnz);
  HCTR_TRY(dev_alloc(owned, sort_temp, sort_temp_bytes));
  HCTR_TRY(dev_alloc(owned, tile_sums, (ceil_div<size_t>(max_nnz, kTile) + 1) * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(owned, run_start, (max_nnz + 2) * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(owned, d_num_runs, sizeof(uint64_t)));
  HCTR_HIP(hipMemset(d_num_runs, 0, sizeof(uint64_t)));
  {
    int lo = 0, hi = 0;  // hi = numerically lowest = most urgent
    HCTR_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HCTR_HIP(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, hi));
    HCTR_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HCTR_HIP(hipEventCreateWithFlags(&ev_sorted, hipEventDisableTiming));
  }
  const size_t seg_tiles = ceil_div<size_t>(max_nnz, (size_t)kSegTile) + 1;
  HCTR_TRY(dev_alloc(owned, seg_head, seg_tiles * (size_t)D * sizeof(float)));
  HCTR_TRY(dev_alloc(owned, seg_tail, seg_tiles * (size_t)D * sizeof(float)));
  HCTR_TRY(dev_alloc(owned, gsum, max_nnz * (size_t)D * sizeof(float)));
  HCTR_TRY(dev_alloc(owned, span_list, seg_tiles * sizeof(uint32_t)));
  // [0] long runs, [1] unused, [2..3] one 64-bit counter: big runs (upper half) / their chunks
  HCTR_TRY(dev_alloc(owned, span_count, 4 * sizeof(uint32_t)));
  HCTR_HIP(hipMemset(span_count, 0, 4 * sizeof(uint32_t)));
  // per big run: start tile, length in tile partials, first chunk number, finished-chunk counter
  // (the counters start at zero and every update leaves them at zero)
  big_stride = seg_tiles;
  HCTR_TRY(dev_alloc(owned, big_list, 4 * seg_tiles * sizeof(uint32_t)));
  HCTR_HIP(hipMemset(big_list, 0, 4 * seg_tiles * sizeof(uint32_t)));
  // hot rows of one-hot batches.  HCTR_HOT_ROWS: rows below it are hot (0 = off);
  // HCTR_HOT_MIN: batches with fewer positions keep the plain path (a small batch is launch-bound:
  // two more kernels and a stream fork cost more than its sort)
  {
    const char* hr = getenv("HCTR_HOT_ROWS");
    long rows = hr ? atol(hr) : 8192;
    if (rows < 0) rows = 0;
    if (rows > kHotMaxRows) rows = kHotMaxRows;
    const char* hm = getenv("HCTR_HOT_MIN");
    hot_min_n = hm ? (size_t)atoll(hm) : (size_t)262144;
    hot_rows = 0;
    // (the tables themselves: here for an owner that announces one-hot batches (eager_hot), else by
    //  the first update that takes the path -- hot_buffers(); see sparse_update.h)
    if (rows > 0 && max_nnz >= hot_min_n && lpr_supported(D)) {
      hot_rows = (uint32_t)rows;
      if (eager_hot) {
        HCTR_TRY(hot_buffers(nullptr));
        HCTR_HIP(hipDeviceSynchronize());  // (the clears above ran on the null stream)
      }
    }
  }
  return HCTR_OK;
}

int SparseUpdater::hot_buffers(hipStream_t s) {
  if (hot_cold != nullptr && hot_cold->hb.loc != nullptr) return HCTR_OK;
  free_hot_cold(*this);  // (what an earlier, failed attempt left)
  HotColdState& hc = *(hot_cold = new HotColdState());
  HotBufs& hb = hc.hb;
  ColdBufs& cb = hc.cb;
  HCTR_HIP(hipStreamCreateWithPriority(&hc.cold_s, hipStreamNonBlocking, 0));  // default priority
  const size_t C = hot_chunks_max(*this);
  HCTR_TRY(dev_alloc(hc.owned, hb.S, C * kHotChunk * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, hb.loc_blk, (size_t)hot_rows * sizeof(uint32_t)));
  HCTR_HIP(hipMemsetAsync(hb.loc_blk, 0, (size_t)hot_rows * sizeof(uint32_t), s));
  HCTR_TRY(dev_alloc(hc.owned, hb.meta, C * 2 * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, hb.tpref, C * (kHotTiles + 1) * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, hb.items, (max_nnz / kHotTile + C + 1) * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, hb.joins, 3 * C * kHotTiles * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, hc.hot_counts, 8 * sizeof(uint32_t)));
  HCTR_HIP(hipMemsetAsync(hc.hot_counts, 0, 8 * sizeof(uint32_t), s));
  const size_t part = C * kHotTiles * (size_t)D * sizeof(float);
  HCTR_TRY(dev_alloc(hc.owned, hb.head, part));
  HCTR_TRY(dev_alloc(hc.owned, hb.tail, part));
  HCTR_TRY(dev_alloc(hc.owned, cb.cnt, max_vocab * sizeof(uint32_t)));
  HCTR_HIP(hipMemsetAsync(cb.cnt, 0, max_vocab * sizeof(uint32_t), s));
  HCTR_TRY(dev_alloc(hc.owned, cb.rank, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, cb.plist, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, cb.bkt, max_nnz * sizeof(uint32_t)));
  HCTR_TRY(dev_alloc(hc.owned, cb.dlist, max_nnz * sizeof(uint2)));
  HCTR_TRY(dev_alloc(hc.owned, cb.singles, max_nnz * sizeof(uint2)));
  HCTR_TRY(dev_alloc(hc.owned, cb.segs, (max_nnz / 2 + 1) * sizeof(uint4)));
  HCTR_TRY(dev_alloc(hc.owned, cb.longs, (max_nnz / 2 + 1) * sizeof(uint4)));
  HCTR_TRY(dev_alloc(hc.owned, hc.cold_counts, 2 * kCcWords * sizeof(uint32_t)));
  HCTR_HIP(hipMemsetAsync(hc.cold_counts, 0, 2 * kCcWords * sizeof(uint32_t), s));
  HCTR_HIP(hipEventCreateWithFlags(&hc.ev_hot, hipEventDisableTiming));
  HCTR_HIP(hipEventCreateWithFlags(&hc.ev_cold, hipEventDisableTiming));
  // (last: its presence is what marks the set complete)
  const size_t loc_bytes = (size_t)hot_rows * C * sizeof(uint16_t);
  HCTR_TRY(dev_alloc(hc.owned, hb.loc, loc_bytes));
  // kHotNone everywhere; hot_apply keeps it so.  (On the caller's stream: the kernels that follow
  // on it, and on the side stream behind its fork event, see the tables initialised)
  HCTR_HIP(hipMemsetAsync(hb.loc, 0xFF, loc_bytes, s));
  return HCTR_OK;
}

int SparseUpdater::destroy() {
  for (void* p : owned) (void)hipFree(p);
  free_hot_cold(*this);
  if (side) {
    (void)hipStreamSynchronize(side);
    (void)hipStreamDestroy(side);
    (void)hipEventDestroy(ev_fork);
    (void)hipEventDestroy(ev_sorted);
  }
  *this = SparseUpdater();
  return HCTR_OK;
}

int SparseUpdater::presort(size_t buckets, size_t n, const void* row_offset, int key_type,
                           const uint64_t* value_index, hipStream_t s) {
  early_n = 0;
  if (buckets == 0 || n == 0 || n > max_nnz || buckets > 0xFFFFFFF0ull || !side) return HCTR_OK;
  HCTR_HIP(hipEventRecord(ev_fork, s));
  HCTR_HIP(hipStreamWaitEvent(side, ev_fork, 0));
  int rc;
  if (key_type == HCTR_KEY_U32)
    rc = sort_stage<uint32_t>(*this, buckets, n, (const uint32_t*)row_offset, value_index, side);
  else
    rc = sort_stage<long long>(*this, buckets, n, (const long long*)row_offset, value_index, side);
  if (rc != HCTR_OK) return rc;
  HCTR_HIP(hipEventRecord(ev_sorted, side));
  early_n = n;
  early_vi = value_index;
  early_buckets = buckets;
  return HCTR_OK;
}

int SparseUpdater::prework(size_t buckets, size_t nnz, int combiner, const void* row_offset,
                           int key_type, const uint64_t* value_index, hipStream_t s) {
  HotColdState* hc = hot_cold;
  if (hc == nullptr || hc->hb.loc == nullptr || !side) return HCTR_OK;
  HCTR_TRY(plan_discard(*this, s));  // (a batch that was never updated)
  if (buckets == 0 || nnz == 0 || nnz > max_nnz || !plan_possible(*this, buckets, nnz))
    return HCTR_OK;
  plan_build(*this, *hc, buckets, nnz, combiner, key_type == HCTR_KEY_U32, value_index);
  // both chains behind what s has enqueued so far (the index stage), next to what follows on it
  HCTR_HIP(hipEventRecord(ev_fork, s));
  HCTR_HIP(hipStreamWaitEvent(side, ev_fork, 0));
  HCTR_HIP(hipStreamWaitEvent(hc->cold_s, ev_fork, 0));
  HCTR_TRY(plan_launch_grouping(*this, *hc, row_offset, side, hc->cold_s));
  HCTR_HIP(hipEventRecord(hc->ev_hot, side));
  HCTR_HIP(hipEventRecord(hc->ev_cold, hc->cold_s));
  hc->valid = true;
  return HCTR_OK;
}

int SparseUpdater::update(size_t buckets, size_t nnz, int combiner, const void* row_offset,
                          int key_type, const uint64_t* value_index, const void* top_grad,
                          int grad_dtype, const OptState& opt, float* table, float* state0,
                          float* state1, uint64_t* prev_time, hipStream_t s) {
  if (buckets == 0) return HCTR_OK;
  if (nnz > max_nnz) {
    set_error("update: nnz exceeds the workspace (batch_size * max_feature_num)");
    return HCTR_ERR_INVALID_ARG;
  }
  if (buckets > 0xFFFFFFF0ull) {
    set_error("update: more than 2^32 buckets");
    return HCTR_ERR_UNSUPPORTED;
  }
  switch (opt.optimizer) {
    case HCTR_OPT_SGD:
    case HCTR_OPT_ADAM:
    case HCTR_OPT_ADAGRAD:
    case HCTR_OPT_MOMENTUM_SGD:
    case HCTR_OPT_NESTEROV:
    case kOptStoreSum: break;
    case HCTR_OPT_FTRL:
      if (allow_ftrl) break;
      [[fallthrough]];
    default:
      // Ftrl / RMSProp are not implemented by the reference's GPU update either
      set_error("sparse optimizer not supported (reference: sparse_optimizer.cu:821-826)");
      return HCTR_ERR_UNSUPPORTED;
  }
  if (opt.update_type == HCTR_UPDATE_LAZY_GLOBAL && opt.optimizer != HCTR_OPT_ADAM) {
    set_error("lazy global update is only implemented for Adam (sparse_optimizer.cu:829-850)");
    return HCTR_ERR_UNSUPPORTED;
  }
  if (key_type != HCTR_KEY_U32 && key_type != HCTR_KEY_I64) {
    set_error("key_type");
    return HCTR_ERR_INVALID_ARG;
  }
  if (grad_dtype != HCTR_EMB_F32 && grad_dtype != HCTR_EMB_F16 && grad_dtype != HCTR_EMB_BF16) {
    set_error("grad dtype");
    return HCTR_ERR_INVALID_ARG;
  }
  return update_typed(*this, buckets, nnz, combiner, row_offset, key_type, value_index, top_grad,
                      grad_dtype, opt, table, state0, state1, prev_time, s);
}

int materialize_wgrad(size_t buckets, int D, int combiner, const void* ro, int key_type,
                      const void* top, void* wgrad, int dtype, hipStream_t s) {
  if (buckets == 0) return HCTR_OK;
  const int grid = grid_for(buckets * (size_t)D, kBlock);
  HCTR_TRY(with_types(key_type, dtype, [&](auto* off, auto* g) -> int {
    hipLaunchKernelGGL((wgrad_kernel<std::remove_pointer_t<decltype(off)>,
                                     std::remove_pointer_t<decltype(g)>>),
                       dim3(grid), dim3(kBlock), 0, s, buckets, D, combiner, (decltype(off))ro,
                       (decltype(g))top, (decltype(g))wgrad);
    return HCTR_OK;
  }));
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // namespace hctr
#ifdef HCTR_SU_ONE_UNIT
#include "su_segmented.hip"
#endif
#endif
