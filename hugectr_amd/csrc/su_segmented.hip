// su_segmented.hip -- the sorted (row, bucket) list of a batch whose D is a supported multiple of 4:
// tile-based segmented reduce + optimizer (a unit of the sparse update, su_units.h).  The one kernel
// family that needs the row-offset type at compile time.
#include "su_device.h"

namespace hctr {
namespace {

// Tile-based segmented reduce + optimizer.  The sorted (row, bucket) list is cut into tiles of
// kSegTile positions; a group of LPR lanes walks one tile in order, so every group performs about
// the same number of gradient-row reads no matter how skewed the key distribution is (the
// reference gives one block to each unique row, sparse_optimizer.cu:223-237 -- a power-law head
// row with 20k duplicates is then one serial 20k-iteration loop).
//   * A run (= all gradients of one row) that starts in tile t is OWNED by tile t's group.  The
//     owner follows it up to one tile past its own tile end; the next tile's group skips those
//     leading positions.  So every run that ends before the end of tile t+1 is reduced by one group
//     in ascending bucket order (the reference's order, stable sort) and applied at once.
//   * A run that reaches beyond tile t+1 is "long": the owner stores the sum of its own part in
//     tail[t] and appends t to span_list; every later tile the run touches stores its part in
//     head[t'].  seg_combine_kernel adds tail + heads in a fixed order (deterministic).

// Phase A: segmented sums.  Pure load/accumulate/store -- no read-modify-write of table rows
// inside the walk.  The kernel is bound by DEPENDENT memory round trips per tile, not by bytes, so
// everything a tile may need is fetched in as few trips as possible:
//   trip 1: the tile's 32 (row, bucket) pairs, one per lane (coalesced), the NEXT tile's pairs
//           (for the run that overhangs the tile end) and the four neighbour rows that decide
//           ownership -- run starts / overhang length become 32-bit ballot masks;
//   trips 2..: the 32 gradient rows of the tile plus the first kSegAhead rows of the overhang,
//           issued back to back in batches of QB raw (unconverted) fragments, clamped to a row the
//           batch reads anyway where a position is not needed.
// The only sequential part is the fp32 add chain, which is what fixes the summation order.
// The sum of a run its owner finishes goes to gsum[start position]; seg_apply_kernel picks it up.
constexpr int kSegAhead = 8;

// row id of tile position q (0..31): the metadata lane that holds it broadcasts it to the group
template <int NPL, int ML>
__device__ __forceinline__ uint32_t seg_row_at(const uint32_t (&mrow)[NPL], int q, int gshift) {
  uint32_t src = mrow[0];
#pragma unroll
  for (int j = 1; j < NPL; j++) src = (q / ML == j) ? mrow[j] : src;
  return (uint32_t)__shfl((int)src, gshift + (q % ML), 64);
}

constexpr int kFuseNone = 0, kFuseSgd = 1, kFuseAdaGrad = 2;

template <int LPR, typename OffT, typename GradT, int kFuse>
__global__ void __launch_bounds__(kBlock)
    seg_reduce_kernel(size_t buckets, const OffT* __restrict__ row_offset,
                      const uint32_t* __restrict__ sorted_rows,
                      const uint32_t* __restrict__ sorted_buckets, int combiner,
                      const GradT* __restrict__ grad, float* __restrict__ gsum,
                      float* __restrict__ head, float* __restrict__ tail,
                      uint32_t* __restrict__ span_list, uint32_t* __restrict__ span_count,
                      float* __restrict__ direct_out, const OffT* __restrict__ scale_ro,
                      OptConst fuse_o, float* __restrict__ fuse_state0) {
  // kFuse (kFuseSgd / kFuseAdaGrad): the optimizer applied where a run's sum is complete --
  // e.g. table[row] += -lr * (sum / scaler) -- right here (direct_out = the table) instead of
  // parking the sum in gsum for seg_apply.  Every row is one run owned by one lane group, so
  // nobody else touches it; the arithmetic is seg_apply's (apply_opt), bit for bit, without the
  // gsum round trip (2 x D x 4 bytes per unique row).  Optimizers with two state vectors or
  // time stamps keep the two-pass form (their row registers would cost the gather its occupancy).
  // Measured (MI355X): one-hot Criteo-1TB update 231 -> 209 us, embedding_collection one-hot
  // backward+update 365 -> 295 us, multi-hot MLPerf shape 2.15 -> 1.84 ms.  (No-return fp32
  // atomic adds in place of the read-modify-write were 2x SLOWER: 496 us / 4.2 ms.)
  // scale_ro: the CSR whose bucket lengths divide a mean gradient.  The distributed embedding
  // divides by the bucket's key count over ALL GPUs (backward() with the all-reduced row offsets,
  // distributed_slot_sparse_embedding_hash.hpp:216-221), not by this rank's filtered count.
  // direct_out != nullptr (hctr_updater_reduce_presorted): the sum of a finished run goes to
  // direct_out[row] instead of gsum[run start] -- no apply pass is needed afterwards
  typedef typename Load4<GradT>::raw Raw;
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  constexpr int T = kSegTile;
  constexpr int LA = kSegAhead;
  constexpr int ML = LPR < T ? LPR : T;  // lanes of a group that carry tile metadata
  constexpr int NPL = T / ML;            // metadata entries per such lane
  constexpr int QB = sizeof(Raw) == 8 ? 20 : 10;  // fragments in flight per lane: 40 VGPRs
  constexpr bool kOff32 = sizeof(OffT) == 4;
  static_assert(T == 32 && (T + LA) % QB == 0, "masks are 32-bit; batches tile T + LA");
  const int g = threadIdx.x / LPR;
  const int l = threadIdx.x % LPR;
  const int gshift = ((threadIdx.x & 63) / LPR) * LPR;  // first lane of my group in the wave
  constexpr unsigned long long kGroupMask = ML >= 64 ? ~0ull : ((1ull << ML) - 1ull);
  const size_t nnz = (size_t)row_offset[buckets];
  const size_t n_tiles = (nnz + T - 1) / T;
  // kFuse: the row update of a finished run is completed when the NEXT run finishes -- its row
  // (and accumulator) read travels while the next run's gradients are added, instead of stalling
  // the lane group (one-hot update 205 -> 195 us, multi-hot backward + update 1.73 -> 1.59 ms)
  uint32_t pend_row = 0xFFFFFFFFu;
  float4 pend_w = make_float4(0.f, 0.f, 0.f, 0.f), pend_d = pend_w;
  RowRegs pend_rr;  // kFuseAdaGrad: row + accumulator in flight, pend_d = the run's gradient sum
  auto pend_flush = [&]() {
    if (pend_row != 0xFFFFFFFFu) {
      if constexpr (kFuse == kFuseAdaGrad) {
        OptConst oo = fuse_o;
        oo.optimizer = HCTR_OPT_ADAGRAD;  // (compile-time: the state loads / stores fold)
        row_compute(oo, pend_d, pend_rr);
        row_store<LPR>(oo, (uint64_t)pend_row, l, pend_rr, direct_out, fuse_state0, nullptr, nullptr);
      } else {
        pend_w.x += pend_d.x;
        pend_w.y += pend_d.y;
        pend_w.z += pend_d.z;
        pend_w.w += pend_d.w;
        *reinterpret_cast<float4*>(direct_out + (size_t)pend_row * D + l * 4) = pend_w;
      }
    }
  };
  for (size_t tile = (size_t)blockIdx.x * GPB + g; tile < n_tiles;
       tile += (size_t)gridDim.x * GPB) {
    const size_t base = tile * T;
    const size_t end = (base + T < nnz) ? base + T : nnz;
    const size_t limit = (end + T < nnz) ? end + T : nnz;
    const int nvalid = (int)(end - base);
    // ---- trip 1: all metadata --------------------------------------------------------------
    uint32_t mrow[NPL], mbkt[NPL], prow[NPL], nrow[NPL], nbkt[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) {
      const size_t pos = base + (size_t)j * ML + l;
      const bool valid = l < ML && pos < end;
      mrow[j] = valid ? (uint32_t)sorted_rows[pos] : 0xFFFFFFFFu;
      mbkt[j] = valid ? sorted_buckets[pos] : 0u;
      prow[j] = (valid && pos > 0) ? (uint32_t)sorted_rows[pos - 1] : 0xFFFFFFFFu;
      const size_t np = end + (size_t)j * ML + l;
      const bool nval = l < ML && np < limit;
      nrow[j] = nval ? (uint32_t)sorted_rows[np] : 0xFFFFFFFFu;
      nbkt[j] = nval ? sorted_buckets[np] : 0u;
    }
    // rows at base-T, base-T-1 (who owns a run that enters this tile) and at limit (does the
    // overhanging run reach beyond tile+1); 0xFFFFFFFF never equals a live row
    const uint32_t row_pt = base >= (size_t)T ? (uint32_t)sorted_rows[base - T] : 0xFFFFFFFFu;
    const uint32_t row_pt1 = base > (size_t)T ? (uint32_t)sorted_rows[base - T - 1] : 0xFFFFFFFFu;
    const uint32_t row_lim = limit < nnz ? (uint32_t)sorted_rows[limit] : 0xFFFFFFFFu;

    uint32_t startmask = 0u;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
      const size_t pos = base + (size_t)j * ML + l;
      const bool valid = l < ML && pos < end;
      const bool is_start = valid && (pos == 0 || prow[j] != mrow[j]);
      const unsigned long long bal = __ballot(is_start);
      startmask |= (uint32_t)((bal >> gshift) & kGroupMask) << (j * ML);
    }
    const uint32_t row0 = (uint32_t)__shfl((int)mrow[0], gshift, 64);
    const uint32_t cur_row =
        (uint32_t)__shfl((int)mrow[(nvalid - 1) / ML], gshift + ((nvalid - 1) % ML), 64);
    const uint32_t next_row0 = (uint32_t)__shfl((int)nrow[0], gshift, 64);
#define HCTR_RUN_DST(q_)                                                                        \
  ((direct_out != nullptr && seg_row_at<NPL, ML>(mrow, (q_), gshift) != 0xFFFFFFFFu)             \
       ? direct_out + (size_t)seg_row_at<NPL, ML>(mrow, (q_), gshift) * D                       \
       : gsum + (base + (size_t)(q_)) * D) /* a run of keys without a row has no output row */
    auto emit_run = [&](int q_run, const float4& a) {
      if constexpr (kFuse == kFuseSgd) {
        const uint32_t r = seg_row_at<NPL, ML>(mrow, q_run, gshift);
        if (r != 0xFFFFFFFFu) {
          pend_flush();
          pend_d.x = -fuse_o.lr * (a.x / fuse_o.scaler);
          pend_d.y = -fuse_o.lr * (a.y / fuse_o.scaler);
          pend_d.z = -fuse_o.lr * (a.z / fuse_o.scaler);
          pend_d.w = -fuse_o.lr * (a.w / fuse_o.scaler);
          pend_row = r;
          pend_w = *reinterpret_cast<const float4*>(direct_out + (size_t)r * D + l * 4);
        }
      } else if constexpr (kFuse == kFuseAdaGrad) {
        const uint32_t r = seg_row_at<NPL, ML>(mrow, q_run, gshift);
        if (r != 0xFFFFFFFFu) {
          pend_flush();
          OptConst oo = fuse_o;
          oo.optimizer = HCTR_OPT_ADAGRAD;
          pend_d = a;
          pend_row = r;
          row_load<LPR>(oo, (uint64_t)r, l, pend_rr, direct_out, fuse_state0, nullptr, nullptr);
        }
      } else {
        *reinterpret_cast<float4*>(HCTR_RUN_DST(q_run) + l * 4) = a;
      }
    };
    const bool ends_at_tile_end = end == nnz || next_row0 != cur_row;
    int q0 = 0;
    bool head_mode = false;
    if (base > 0 && (startmask & 1u) == 0u) {
      // the tile starts inside a run begun earlier: owned by the previous tile AND ending inside
      // this tile -> its owner reduces it, skip it; otherwise it is (part of) a long run.
      const bool owner_prev = row_pt != row0 || base == (size_t)T || row_pt1 != row0;
      const bool whole_tile = startmask == 0u;
      const bool ends_inside = !whole_tile || ends_at_tile_end;
      if (owner_prev && ends_inside) q0 = whole_tile ? nvalid : __ffs((int)startmask) - 1;
      else head_mode = true;
    }
    if (q0 >= nvalid) continue;  // the whole tile belonged to the previous tile's run
    // overhang: leading positions of the next tile that continue this tile's last run
    uint32_t matchmask = 0u;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
      const unsigned long long bal = __ballot(nrow[j] == cur_row);
      matchmask |= (uint32_t)((bal >> gshift) & kGroupMask) << (j * ML);
    }
    const bool whole_head = head_mode && startmask == 0u;  // one earlier run covers the tile
    int cnt = (~matchmask == 0u) ? T : __ffs((int)~matchmask) - 1;  // leading ones
    if (ends_at_tile_end || whole_head) cnt = 0;
    const int cnt_la = cnt < LA ? cnt : LA;

    // ---- trips 2..: gradient rows, QB fragments in flight ---------------------------------
    int run_start = q0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 own_part = acc;
    const uint32_t b_q0 = (uint32_t)__shfl((int)mbkt[q0 / ML], gshift + (q0 % ML), 64);
#pragma unroll
    for (int qb = 0; qb < T + LA; qb += QB) {
      Raw v[QB];
      int nb[QB];
#pragma unroll
      for (int k = 0; k < QB; k++) {
        const int q = qb + k;
        uint32_t bsel;
        if (q < T) {
          const uint32_t bq = (uint32_t)__shfl((int)mbkt[q / ML], gshift + (q % ML), 64);
          bsel = (q >= q0 && q < nvalid) ? bq : b_q0;
        } else {
          const uint32_t bq =
              (uint32_t)__shfl((int)nbkt[(q - T) / ML], gshift + ((q - T) % ML), 64);
          bsel = (q - T) < cnt_la ? bq : b_q0;
        }
        v[k] = Load4<GradT>::ld_raw(grad + (size_t)bsel * D + l * 4);
        nb[k] = combiner == 1 ? bucket_len(scale_ro, kOff32, bsel) : 1;
      }
#pragma unroll
      for (int k = 0; k < QB; k++) {
        const int q = qb + k;
        if (q == T) own_part = acc;
        if (q < T) {
          if (q >= q0 && q < nvalid) {
            if (((startmask >> q) & 1u) != 0u && q != q0) {
              if (head_mode) *reinterpret_cast<float4*>(head + tile * D + l * 4) = acc;
              else emit_run(run_start, acc);
              acc = make_float4(0.f, 0.f, 0.f, 0.f);
              run_start = q;
              head_mode = false;
            }
            const float4 f = scaled_grad<GradT>(v[k], combiner, nb[k]);
            acc.x += f.x;
            acc.y += f.y;
            acc.z += f.z;
            acc.w += f.w;
          }
        } else if ((q - T) < cnt_la) {
          const float4 f = scaled_grad<GradT>(v[k], combiner, nb[k]);
          acc.x += f.x;
          acc.y += f.y;
          acc.z += f.z;
          acc.w += f.w;
        }
      }
    }
    if (head_mode) {  // one run covers the whole tile
      *reinterpret_cast<float4*>(head + tile * D + l * 4) = acc;
      continue;
    }
    if (cnt == 0) {  // the last run ends with the tile
      emit_run(run_start, acc);
      continue;
    }
    // the last run of this tile continues: this group owns it and follows it through tile+1
    if (cnt > LA) {
      constexpr int QC = 8;
#pragma unroll 1
      for (int qb = LA; qb < cnt; qb += QC) {
        Raw v[QC];
        int nb[QC];
#pragma unroll
        for (int k = 0; k < QC; k++) {
          const int q = (qb + k) < cnt ? qb + k : cnt - 1;
          // NPL > 1: the register index is dynamic here -> select with a small unrolled scan
          uint32_t src = nbkt[0];
#pragma unroll
          for (int j = 1; j < NPL; j++) src = (q / ML == j) ? nbkt[j] : src;
          const uint32_t bsel = (uint32_t)__shfl((int)src, gshift + (q % ML), 64);
          v[k] = Load4<GradT>::ld_raw(grad + (size_t)bsel * D + l * 4);
          nb[k] = combiner == 1 ? bucket_len(scale_ro, kOff32, bsel) : 1;
        }
#pragma unroll
        for (int k = 0; k < QC; k++) {
          if (qb + k < cnt) {
            const float4 f = scaled_grad<GradT>(v[k], combiner, nb[k]);
            acc.x += f.x;
            acc.y += f.y;
            acc.z += f.z;
            acc.w += f.w;
          }
        }
      }
    }
    // long <=> the run reaches beyond the end of tile+1
    const bool runs_on = cnt == T && limit < nnz && row_lim == cur_row;
    if (!runs_on) {
      emit_run(run_start, acc);
    } else {
      *reinterpret_cast<float4*>(tail + tile * D + l * 4) = own_part;
      if (l == 0) span_list[atomicAdd(span_count, 1u)] = (uint32_t)tile;
    }
  }
  if constexpr (kFuse != kFuseNone) pend_flush();
}
#undef HCTR_RUN_DST

// Phase B: one lane inspects one sorted position; run starts of runs that are not "long" are
// compacted with a wave ballot and handed to lane groups, which read the run's gradient sum from
// gsum[position] and apply the optimizer to the row (one coalesced D*4-byte RMW per row).
// kSgd: plain SGD known at compile time -- one float4 of state per row instead of the generic
// RowRegs (w, two state vectors, four time stamps: 148 VGPRs, 3 waves per SIMD), 8 rows per lane
// group in flight instead of 4 (93 VGPRs).  Same arithmetic, same bits; seg_apply 98 -> 70 us at
// the bench shape.
template <int LPR, typename OffT, bool kSgd>
__global__ void __launch_bounds__(kBlock)
    seg_apply_kernel(size_t buckets, const OffT* __restrict__ row_offset,
                     const uint32_t* __restrict__ sorted_rows, const float* __restrict__ gsum,
                     OptConst o, float* __restrict__ table, float* __restrict__ state0,
                     float* __restrict__ state1, unsigned long long* __restrict__ prev_time) {
  constexpr int D = LPR * 4;
  constexpr int G = 64 / LPR;  // groups per wavefront
  constexpr int T = kSegTile;
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR;
  const int l = lane % LPR;
  const size_t nnz = (size_t)row_offset[buckets];
  const size_t wave = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const size_t nwaves = ((size_t)gridDim.x * kBlock) >> 6;
  for (size_t c0 = wave * 64; c0 < nnz; c0 += nwaves * 64) {
    const size_t p = c0 + lane;
    uint32_t row = 0;
    bool active = false;
    if (p < nnz) {
      row = sorted_rows[p];
      const bool is_start = p == 0 || sorted_rows[p - 1] != row;
      if (is_start) {
        const size_t e2 = (p / T + 2) * T;  // first position after the tile following p's tile
        const bool is_long = e2 < nnz && sorted_rows[e2] == row;
        active = !is_long && (uint64_t)row != kNoRow;
      }
    }
    unsigned long long mask = __ballot(active);
    // R rows per group per step: all gsum / table / state reads of a step are issued before the
    // first optimizer evaluation
    constexpr int R = kSgd ? 8 : 4;
    while (mask != 0ull) {
      int src[R];
#pragma unroll
      for (int k = 0; k < R; k++) {
        src[k] = -1;
#pragma unroll
        for (int q = 0; q < G; q++) {
          if (mask != 0ull) {
            const int bit = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            if (q == g) src[k] = bit;
          }
        }
      }
      uint32_t r2[R];
      float4 gi[R];
      if constexpr (kSgd) {
        float4 w[R];
#pragma unroll
        for (int k = 0; k < R; k++) {
          r2[k] = (uint32_t)__shfl((int)row, src[k] < 0 ? 0 : src[k], 64);
          if (src[k] >= 0) {
            gi[k] = *reinterpret_cast<const float4*>(gsum + (c0 + src[k]) * D + l * 4);
            w[k] = *reinterpret_cast<const float4*>(table + (uint64_t)r2[k] * D + l * 4);
          }
        }
#pragma unroll
        for (int k = 0; k < R; k++) {
          if (src[k] >= 0) {  // row_compute + apply_opt(HCTR_OPT_SGD): w += -lr * (g / scaler)
            w[k].x += -o.lr * (gi[k].x / o.scaler);
            w[k].y += -o.lr * (gi[k].y / o.scaler);
            w[k].z += -o.lr * (gi[k].z / o.scaler);
            w[k].w += -o.lr * (gi[k].w / o.scaler);
            *reinterpret_cast<float4*>(table + (uint64_t)r2[k] * D + l * 4) = w[k];
          }
        }
      } else {
        RowRegs rr[R];
#pragma unroll
        for (int k = 0; k < R; k++) {
          r2[k] = (uint32_t)__shfl((int)row, src[k] < 0 ? 0 : src[k], 64);
          if (src[k] >= 0) {
            gi[k] = *reinterpret_cast<const float4*>(gsum + (c0 + src[k]) * D + l * 4);
            row_load<LPR>(o, (uint64_t)r2[k], l, rr[k], table, state0, state1, prev_time);
          }
        }
#pragma unroll
        for (int k = 0; k < R; k++) {
          if (src[k] >= 0) {
            row_compute(o, gi[k], rr[k]);
            row_store<LPR>(o, (uint64_t)r2[k], l, rr[k], table, state0, state1, prev_time);
          }
        }
      }
    }
  }
}

// Long runs (listed in span_list by the tile they start in): tail[t0] + head[t0+1] + head[t0+2] ...
// With power-law keys most long runs are a few tiles long while a handful (the rows of 3- or
// 10-row tables) span hundreds of tiles.  seg_combine_kernel gives one lane group to each run: it
// measures the run (how many following tiles begin with the same row) and adds the head partials
// in order, 8 reads in flight; runs of more than kCombBigTiles tiles are parked in big_list and
// taken by seg_combine_big_kernel, one 1024-thread workgroup per run: group q adds heads q,
// q+GPB, ...; the GPB sums are added in the fixed order q = 0..GPB-1.  Both orders are fixed, so
// the result does not depend on scheduling.
constexpr int kCombBigTiles = 64;
constexpr int kCombBlock = 1024;
constexpr int kCombBigChunk = 2048;  // tile partials one workgroup of the big kernel adds

template <int LPR, typename OffT>
__global__ void __launch_bounds__(kBlock)
    seg_combine_kernel(size_t buckets, const OffT* __restrict__ row_offset,
                       const uint32_t* __restrict__ sorted_rows, OptConst o,
                       float* __restrict__ table, float* __restrict__ state0,
                       float* __restrict__ state1, unsigned long long* __restrict__ prev_time,
                       const float* __restrict__ head, const float* __restrict__ tail,
                       const uint32_t* __restrict__ span_list, uint32_t* __restrict__ span_count,
                       uint32_t* __restrict__ big_list, size_t big_stride) {
  constexpr int D = LPR * 4;
  constexpr int GPB = kBlock / LPR;
  constexpr int CU = 8;
  constexpr unsigned long long kGroupMask = LPR >= 64 ? ~0ull : ((1ull << LPR) - 1ull);
  const int g = threadIdx.x / LPR;
  const int l = threadIdx.x % LPR;
  const int gshift = ((threadIdx.x & 63) / LPR) * LPR;
  const size_t nnz = (size_t)row_offset[buckets];
  const size_t n_tiles = (nnz + kSegTile - 1) / kSegTile;
  const uint32_t n_span = span_count[0];
  for (size_t si = (size_t)blockIdx.x * GPB + g; si < n_span; si += (size_t)gridDim.x * GPB) {
    const size_t t0 = span_list[si];
    const uint32_t row = sorted_rows[(t0 + 1) * kSegTile - 1];
    float4 acc = *reinterpret_cast<const float4*>(tail + t0 * D + l * 4);
    size_t n_heads = 0;
    bool parked = false;
    for (;;) {
      const size_t tt = t0 + 1 + n_heads + l;
      const bool match = tt < n_tiles && sorted_rows[tt * kSegTile] == row;
      const unsigned long long gm = (__ballot(match) >> gshift) & kGroupMask;
      const int ld = gm == kGroupMask ? LPR : __ffsll((long long)~gm) - 1;
      n_heads += (size_t)ld;
      if (ld < LPR) break;
      if (n_heads > (size_t)kCombBigTiles) {
        parked = true;
        break;
      }
    }
    if (parked) {
      // a big run: measure it to the end (LPR evenly spaced probes per round; tiles < lo begin
      // with `row`, tile hi does not) and register its chunks of kCombBigChunk tile partials --
      // seg_combine_big_kernel gives every chunk a workgroup of its own
      size_t lo = t0 + 1 + n_heads, hi = n_tiles;
      while (lo < hi) {
        const size_t step = (hi - lo + LPR - 1) / LPR;
        const size_t probe = lo + (size_t)l * step;
        const bool match = probe < hi && sorted_rows[probe * kSegTile] == row;
        const unsigned long long gm = (__ballot(match) >> gshift) & kGroupMask;
        const int m = gm == kGroupMask ? LPR : __ffsll((long long)~gm) - 1;
        if (m == 0) {
          hi = lo;
        } else {
          const size_t first_miss = lo + (size_t)m * step;
          lo = lo + (size_t)(m - 1) * step + 1;
          if (first_miss < hi) hi = first_miss;
        }
      }
      if (l == 0) {
        const size_t n = lo - (t0 + 1);
        const unsigned long long nch = (n + kCombBigChunk - 1) / kCombBigChunk;
        // one 64-bit counter: runs in the upper half, chunks in the lower -- the chunk bases
        // then ascend with the slot numbers (binary search in the big kernel)
        const unsigned long long old = atomicAdd(
            reinterpret_cast<unsigned long long*>(span_count + 2), (1ull << 32) | nch);
        const size_t slot = (size_t)(old >> 32);
        big_list[slot] = (uint32_t)t0;
        big_list[big_stride + slot] = (uint32_t)n;
        big_list[2 * big_stride + slot] = (uint32_t)(old & 0xFFFFFFFFull);
      }
      continue;
    }
    for (size_t i = 0; i < n_heads; i += CU) {
      float4 h[CU];
#pragma unroll
      for (int c = 0; c < CU; c++) {
        const size_t tt = t0 + 1 + (i + c < n_heads ? i + c : i);  // clamp: always a legal read
        h[c] = *reinterpret_cast<const float4*>(head + tt * D + l * 4);
      }
#pragma unroll
      for (int c = 0; c < CU; c++) {
        if (i + c < n_heads) {
          acc.x += h[c].x;
          acc.y += h[c].y;
          acc.z += h[c].z;
          acc.w += h[c].w;
        }
      }
    }
    apply_row_vec4<LPR>(o, (uint64_t)row, l, acc, table, state0, state1, prev_time);
  }
}

template <int LPR, typename OffT>
__global__ void __launch_bounds__(kCombBlock)
    seg_combine_big_kernel(size_t buckets, const OffT* __restrict__ row_offset,
                           const uint32_t* __restrict__ sorted_rows, OptConst o,
                           float* __restrict__ table, float* __restrict__ state0,
                           float* __restrict__ state1, unsigned long long* __restrict__ prev_time,
                           float* head, const float* __restrict__ tail, uint32_t* big_list,
                           size_t big_stride, const uint32_t* __restrict__ span_count) {
  // Work item = one chunk (kCombBigChunk tile partials) of one big run.  A row with a million
  // gradients is 30 000 partials: one workgroup adding them all was the tail of the whole update
  // (a single CU's bandwidth); now its chunks run side by side.  Every chunk sum has a fixed order
  // (group q adds partials q, q + GPB, ...; the GPB group sums are added q = 0..GPB-1), a chunk's
  // sum is parked in the slot of its own first partial, and the workgroup that finishes LAST (a
  // counter per run) adds tail + chunk sums in chunk order and applies the optimizer: the result
  // does not depend on which workgroup that is.
  constexpr int D = LPR * 4;
  constexpr int GPB = kCombBlock / LPR;
  constexpr int CU = 8;
  __shared__ float4 part[kCombBlock];
  __shared__ int is_last;
  const int g = threadIdx.x / LPR;
  const int l = threadIdx.x % LPR;
  const unsigned long long ctr = *reinterpret_cast<const unsigned long long*>(span_count + 2);
  const uint32_t n_big = (uint32_t)(ctr >> 32);
  const uint32_t total = (uint32_t)(ctr & 0xFFFFFFFFull);
  const uint32_t* big_t0 = big_list;
  const uint32_t* big_len = big_list + big_stride;
  const uint32_t* big_base = big_list + 2 * big_stride;
  uint32_t* big_done = big_list + 3 * big_stride;
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    uint32_t lo = 0, hi = n_big;  // the run whose chunks include w: last slot with base <= w
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (big_base[mid] <= w) lo = mid;
      else hi = mid;
    }
    const uint32_t slot = lo;
    const size_t t0 = big_t0[slot];
    const size_t n_heads = big_len[slot];
    const uint32_t c = w - big_base[slot];
    const uint32_t nch = (uint32_t)((n_heads + kCombBigChunk - 1) / kCombBigChunk);
    const uint32_t row = sorted_rows[(t0 + 1) * kSegTile - 1];
    const size_t h0 = (size_t)c * kCombBigChunk;
    const size_t h1 = h0 + kCombBigChunk < n_heads ? h0 + kCombBigChunk : n_heads;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = h0 + (size_t)g; i < h1; i += (size_t)GPB * CU) {
      float4 h[CU];
#pragma unroll
      for (int k = 0; k < CU; k++) {
        const size_t ii = i + (size_t)k * GPB;
        const size_t tt = t0 + 1 + (ii < h1 ? ii : i);
        h[k] = *reinterpret_cast<const float4*>(head + tt * D + l * 4);
      }
#pragma unroll
      for (int k = 0; k < CU; k++) {
        if (i + (size_t)k * GPB < h1) {
          acc.x += h[k].x;
          acc.y += h[k].y;
          acc.z += h[k].z;
          acc.w += h[k].w;
        }
      }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0) {
      float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nch == 1u) tot = *reinterpret_cast<const float4*>(tail + t0 * D + l * 4);
#pragma unroll 8
      for (int q = 0; q < GPB; q++) {
        const float4 pq = part[q * LPR + l];
        tot.x += pq.x;
        tot.y += pq.y;
        tot.z += pq.z;
        tot.w += pq.w;
      }
      if (nch == 1u) {
        apply_row_vec4<LPR>(o, (uint64_t)row, l, tot, table, state0, state1, prev_time);
      } else {  // every partial of this chunk has been read (the barrier above): reuse slot h0
        *reinterpret_cast<float4*>(head + (t0 + 1 + h0) * D + l * 4) = tot;
        __threadfence();
      }
    }
    __syncthreads();
    if (nch > 1u) {
      if (threadIdx.x == 0) is_last = atomicAdd(big_done + slot, 1u) == nch - 1u ? 1 : 0;
      __syncthreads();
      if (is_last != 0) {
        if (g == 0) {
          __threadfence();
          float4 tot = *reinterpret_cast<const float4*>(tail + t0 * D + l * 4);
          for (uint32_t c2 = 0; c2 < nch; c2++) {
            float* p = head + (t0 + 1 + (size_t)c2 * kCombBigChunk) * D + l * 4;
            // (sums other workgroups parked: read past this CU's vector cache)
            tot.x += __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tot.y += __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tot.z += __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tot.w += __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          apply_row_vec4<LPR>(o, (uint64_t)row, l, tot, table, state0, state1, prev_time);
        }
        if (threadIdx.x == 0) big_done[slot] = 0u;  // clean for the next update
      }
      __syncthreads();
    }
  }
}

template <typename OffT, typename GradT>
int update_segmented_typed(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner,
                           const OffT* ro, const OffT* sro, const GradT* grad, const OptConst& o,
                           float* direct, float* table, float* state0, float* state1,
                           uint64_t* prev_time, hipStream_t s) {
  // plain SGD: the apply pass folds into the reduce (seg_reduce_kernel<.., kFuseSgd>);
  // HCTR_SGD_FUSED=0 keeps the two-pass form (measurements, the bit-equality test)
  const char* fuse_env = getenv("HCTR_SGD_FUSED");  // (read per call: tests flip it in-process)
  int fuse = kFuseNone;
  if (!(fuse_env && fuse_env[0] == '0') && direct == nullptr) {
    if (o.optimizer == HCTR_OPT_SGD) fuse = kFuseSgd;
    if (o.optimizer == HCTR_OPT_ADAGRAD) fuse = kFuseAdaGrad;
  }
  const size_t nnz = p.n;
  const size_t seg_tiles = ceil_div<size_t>(nnz, (size_t)kSegTile);
  return with_lpr(u.D / 4, [&](auto L) -> int {
    constexpr int LPR = decltype(L)::value;
    constexpr int GPB = kBlock / LPR;
    auto reduce = [&](auto F, float* out) {
      hipLaunchKernelGGL((seg_reduce_kernel<LPR, OffT, GradT, decltype(F)::value>),
                         dim3(grid_for(seg_tiles, GPB, 1 << 20)), dim3(kBlock), 0, s, buckets, ro,
                         p.rows, p.buckets, combiner, grad, u.gsum, u.seg_head, u.seg_tail,
                         u.span_list, u.span_count, out, sro, o, state0);
    };
    if (fuse == kFuseSgd) reduce(std::integral_constant<int, kFuseSgd>{}, table);
    else if (fuse == kFuseAdaGrad) reduce(std::integral_constant<int, kFuseAdaGrad>{}, table);
    else reduce(std::integral_constant<int, kFuseNone>{}, direct);
    HCTR_LAUNCH_CHECK();
    if (direct == nullptr && fuse == kFuseNone) {
      with_bool(o.optimizer == HCTR_OPT_SGD, [&](auto sgd) {
        hipLaunchKernelGGL((seg_apply_kernel<LPR, OffT, decltype(sgd)::value>),
                           dim3(grid_for(nnz, kBlock, 256 * 8)), dim3(kBlock), 0, s, buckets, ro,
                           p.rows, u.gsum, o, table, state0, state1,
                           (unsigned long long*)prev_time);
      });
      HCTR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((seg_combine_kernel<LPR, OffT>), dim3(grid_for(seg_tiles, GPB * 4, 1024)),
                       dim3(kBlock), 0, s, buckets, ro, p.rows, o, table, state0, state1,
                       (unsigned long long*)prev_time, u.seg_head, u.seg_tail, u.span_list,
                       u.span_count, u.big_list, u.big_stride);
    HCTR_LAUNCH_CHECK();
    hipLaunchKernelGGL((seg_combine_big_kernel<LPR, OffT>), dim3(256), dim3(kCombBlock), 0, s,
                       buckets, ro, p.rows, o, table, state0, state1,
                       (unsigned long long*)prev_time, u.seg_head, u.seg_tail, u.big_list,
                       u.big_stride, u.span_count);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  });
}

template <typename OffT>
int update_segmented(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner,
                     const void* ro, const void* sro, const void* grad, int grad_dtype,
                     const OptState& opt, float* direct, float* table, float* state0, float* state1,
                     uint64_t* prev_time, hipStream_t s) {
  const OptConst o = opt_const(opt);
  return with_dtype(grad_dtype, [&](auto* g) -> int {
    return update_segmented_typed(u, p, buckets, combiner, (const OffT*)ro, (const OffT*)sro,
                                  (decltype(g))grad, o, direct, table, state0, state1, prev_time, s);
  });
}

}  // namespace

// The unit's kernels hang off these two functions, one per row-offset type.  HCTR_SEG_OFF (32 / 64,
// the Makefile) picks one: the two halves build side by side as two objects -- the one place where
// one source feeds two.  Undefined: both.
#define HCTR_SEG_ENTRY(name, OffT)                                                               \
  int name(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner, const void* ro, \
           const void* sro, const void* grad, int grad_dtype, const OptState& opt, float* direct, \
           float* table, float* state0, float* state1, uint64_t* prev_time, hipStream_t s) {     \
    return update_segmented<OffT>(u, p, buckets, combiner, ro, sro, grad, grad_dtype, opt, direct, \
                                  table, state0, state1, prev_time, s);                          \
  }
#if !defined(HCTR_SEG_OFF) || HCTR_SEG_OFF == 32
HCTR_SEG_ENTRY(update_segmented_u32, uint32_t)
#endif
#if !defined(HCTR_SEG_OFF) || HCTR_SEG_OFF == 64
HCTR_SEG_ENTRY(update_segmented_i64, long long)
#endif
#undef HCTR_SEG_ENTRY

}  // namespace hctr
