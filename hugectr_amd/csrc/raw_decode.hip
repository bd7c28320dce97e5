// raw_decode.hip -- one launch splits one batch of Raw records (gfx950, wave64).
//
// The Raw format keeps fixed-size samples, every field 4 bytes: label[L] dense[Dn] keys[sum of
// hotness].  The reference stages the records of its asynchronous reader in pinned memory, copies
// them up and splits them with split_feat_major_kernel
// (R/HugeCTR/src/data_readers/multi_hot/split_batch.cu:42-84): one thread per word, a scattered
// 8-byte store per key.  Here:
//
//   * a workgroup takes a TILE of consecutive samples times all columns -- one contiguous range of
//     the record buffer -- reads it with 16-byte loads and parks it in LDS;
//   * a device-resident plan (hctr_raw_segment table + one addend per column, built once by the
//     reader) says where every column range of every sample range goes.  For each segment the
//     tile's output is ONE contiguous range (sample-major [sample][column of the segment]; a
//     collection group is one segment per lookup, so its feature-major layout is the same thing),
//     written from LDS with consecutive lanes on consecutive elements;
//   * records wider than kRdMaxCols columns are taken in column passes; a segment cut by a pass
//     writes rows of its part, still coalesced inside a row.
//
// Plain vector stores, every position written once, no atomics.  The LDS tile keeps the records'
// own layout (row stride = columns of the pass): a column range narrower than a row is read with a
// bank conflict of up to 8 ways at even strides, which at 4 bytes in / 8 bytes out per word stays
// far below what HBM allows (DESIGN.md "Raw reader").
// Compiled as part of embedding_kernels.hip's unit (included at its end, like dense_lookup.hip).
#include "common.h"

namespace hctr {
namespace {

constexpr int kRdBlock = 256;
constexpr uint32_t kRdLdsWords = 8192;  // 32 KiB tile: four workgroups fit the LDS of a CU
constexpr uint32_t kRdMaxCols = 256;    // columns of one pass
constexpr uint32_t kRdMaxTile = 256;    // samples of one tile, a multiple of 32 (16-byte loads)

inline uint32_t rd_pass_cols(size_t width) {
  return width < kRdMaxCols ? (uint32_t)width : kRdMaxCols;
}
// width 3 -> 256, 40 -> 192, 228 -> 32, >= 256 -> 32
inline uint32_t rd_tile_samples(size_t width) {
  uint32_t ts = kRdLdsWords / rd_pass_cols(width);
  if (ts > kRdMaxTile) ts = kRdMaxTile;
  return ts & ~31u;
}

template <int KIND>
__device__ __forceinline__ void rd_store(char* __restrict__ dst, size_t i, uint32_t w,
                                         long long add) {
  if constexpr (KIND == HCTR_RAW_BITS) {
    reinterpret_cast<uint32_t*>(dst)[i] = w;
  } else if constexpr (KIND == HCTR_RAW_I2F) {
    reinterpret_cast<float*>(dst)[i] = (float)(int32_t)w;
  } else if constexpr (KIND == HCTR_RAW_LOG1P) {
    // the reference's logf(x + 1.f) with the logarithm taken in fp64 and rounded once: logf as
    // it is lowered for gfx950 lands up to 2 floats from the correctly rounded value (measured),
    // this form at most 1, and a batch has few dense words
    reinterpret_cast<float*>(dst)[i] = (float)log((double)((float)(int32_t)w + 1.f));
  } else if constexpr (KIND == HCTR_RAW_KEY_I64) {
    reinterpret_cast<long long*>(dst)[i] = (long long)((unsigned long long)w +
                                                       (unsigned long long)add);
  } else if constexpr (KIND == HCTR_RAW_KEY_I32) {
    reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)((unsigned long long)w +
                                                     (unsigned long long)add);
  } else {
    reinterpret_cast<long long*>(dst)[i] = (long long)(unsigned long long)w;
  }
}

// the part of one segment that lies in the staged tile: rows [row0, row0 + rows) of the tile,
// columns [tc0, tc0 + m) of the pass (row stride nc) -> dst[(drow0 + r) * seg_cols + dcol0 + j]
template <int KIND>
__device__ __forceinline__ void rd_write(const uint32_t* __restrict__ tile,
                                         const long long* __restrict__ add, uint32_t nc,
                                         uint32_t row0, uint32_t rows, uint32_t tc0, uint32_t m,
                                         char* __restrict__ dst, size_t drow0, uint32_t dcol0,
                                         uint32_t seg_cols) {
  const uint32_t total = rows * m;
  for (uint32_t e = threadIdx.x; e < total; e += kRdBlock) {
    const uint32_t r = e / m;
    const uint32_t j = e - r * m;
    const uint32_t w = tile[(row0 + r) * nc + tc0 + j];
    rd_store<KIND>(dst, (drow0 + r) * (size_t)seg_cols + dcol0 + j, w, add[tc0 + j]);
  }
}

__global__ void __launch_bounds__(kRdBlock)
    raw_decode_kernel(const uint32_t* __restrict__ raw, size_t batch, uint32_t width,
                      const hctr_raw_segment* __restrict__ segs, int n_segments,
                      const long long* __restrict__ addend, char* __restrict__ out, uint32_t ts,
                      uint32_t cw) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kRdLdsWords];
  __shared__ long long add[kRdMaxCols];
  const size_t n_tiles = (batch + ts - 1) / ts;
  for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const size_t s_lo = t * ts;
    const uint32_t ns = batch - s_lo < (size_t)ts ? (uint32_t)(batch - s_lo) : ts;
    for (uint32_t c_lo = 0; c_lo < width; c_lo += cw) {
      const uint32_t nc = width - c_lo < cw ? width - c_lo : cw;
      const uint32_t n = ns * nc;  // <= kRdLdsWords
      if (nc == width) {
        // whole records: one contiguous range, 16-byte aligned (ts is a multiple of 32 samples)
        const uint32_t* src = raw + s_lo * width;
        const uint32_t n4 = n >> 2;
        for (uint32_t i = threadIdx.x; i < n4; i += kRdBlock)
          reinterpret_cast<uint4*>(tile)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (uint32_t i = (n4 << 2) + threadIdx.x; i < n; i += kRdBlock) tile[i] = src[i];
      } else {
        for (uint32_t e = threadIdx.x; e < n; e += kRdBlock) {
          const uint32_t r = e / nc;
          tile[e] = raw[(s_lo + r) * width + c_lo + (e - r * nc)];
        }
      }
      for (uint32_t c = threadIdx.x; c < nc; c += kRdBlock) add[c] = addend[c_lo + c];
      __syncthreads();
      for (int g = 0; g < n_segments; g++) {
        const hctr_raw_segment sg = segs[g];
        const uint32_t sc1 = sg.col0 + sg.ncols;
        const uint32_t c0 = sg.col0 > c_lo ? sg.col0 : c_lo;
        const uint32_t c1 = sc1 < c_lo + nc ? sc1 : c_lo + nc;
        const size_t r0 = sg.sample0 > s_lo ? (size_t)sg.sample0 : s_lo;
        const size_t r1 = sg.sample1 < s_lo + ns ? (size_t)sg.sample1 : s_lo + ns;
        if (c0 >= c1 || r0 >= r1) continue;
        char* dst = out + sg.dst_offset;
        const uint32_t row0 = (uint32_t)(r0 - s_lo), rows = (uint32_t)(r1 - r0);
        const uint32_t tc0 = c0 - c_lo, m = c1 - c0, dcol0 = c0 - sg.col0;
        const size_t drow0 = r0 - (size_t)sg.sample0;
        switch (sg.kind) {
          case HCTR_RAW_BITS:
            rd_write<HCTR_RAW_BITS>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0, sg.ncols);
            break;
          case HCTR_RAW_I2F:
            rd_write<HCTR_RAW_I2F>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0, sg.ncols);
            break;
          case HCTR_RAW_LOG1P:
            rd_write<HCTR_RAW_LOG1P>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0,
                                     sg.ncols);
            break;
          case HCTR_RAW_KEY_I64:
            rd_write<HCTR_RAW_KEY_I64>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0,
                                       sg.ncols);
            break;
          case HCTR_RAW_KEY_I32:
            rd_write<HCTR_RAW_KEY_I32>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0,
                                       sg.ncols);
            break;
          case HCTR_RAW_RAWKEY_I64:
            rd_write<HCTR_RAW_RAWKEY_I64>(tile, add, nc, row0, rows, tc0, m, dst, drow0, dcol0,
                                          sg.ncols);
            break;
          default:
            break;  // (an unknown kind writes nothing)
        }
      }
      __syncthreads();  // the tile is overwritten by the next pass
    }
  }
}

}  // namespace
}  // namespace hctr

extern "C" {

size_t hctr_raw_decode_tile(size_t width) {
  return width == 0 ? 0 : (size_t)hctr::rd_tile_samples(width);
}

int hctr_raw_decode(const uint32_t* raw, size_t batch, size_t width, const void* plan,
                    int n_segments, void* out_base, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(raw && plan && out_base, "hctr_raw_decode: null pointer");
  HCTR_REQUIRE(batch >= 1 && batch < (1ull << 31), "hctr_raw_decode: batch must be 1..2^31-1");
  HCTR_REQUIRE(width >= 1 && width < (1ull << 24), "hctr_raw_decode: width must be 1..2^24-1");
  HCTR_REQUIRE(n_segments >= 1 && n_segments <= HCTR_RAW_DECODE_MAX_SEGMENTS,
               "hctr_raw_decode: n_segments must be 1..4096");
  HCTR_REQUIRE(((uintptr_t)raw & 15) == 0, "hctr_raw_decode: raw must be 16-byte aligned");
  HCTR_REQUIRE(((uintptr_t)plan & 7) == 0 && ((uintptr_t)out_base & 7) == 0,
               "hctr_raw_decode: plan and out_base must be 8-byte aligned");
  const uint32_t ts = rd_tile_samples(width), cw = rd_pass_cols(width);
  const size_t tiles = ceil_div<size_t>(batch, (size_t)ts);
  const int grid = (int)(tiles < (size_t)HCTR_RAW_DECODE_MAX_BLOCKS
                             ? tiles : (size_t)HCTR_RAW_DECODE_MAX_BLOCKS);
  const hctr_raw_segment* segs = (const hctr_raw_segment*)plan;
  const long long* addend = (const long long*)(segs + n_segments);
  hipLaunchKernelGGL(raw_decode_kernel, dim3(grid), dim3(kRdBlock), 0, as_stream(stream), raw,
                     batch, (uint32_t)width, segs, n_segments, addend, (char*)out_base, ts, cw);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
