// parquet_decode.hip -- one launch turns the resident columns of a Parquet file into one batch
// (gfx950, wave64).
//
// The reference reads a file into device columns and converts them with three kinds of launches and
// a scan: dense_data_converter_kernel__, offset_kernel__, value_kernel_without_shared_mem__ /
// value_kernel__ (R/HugeCTR/src/data_readers/parquet_data_converter.cu:55-260).  Arrow's list
// offsets ARE prefix sums, so with the offsets of a whole file rebased to off[0] = 0 by the staging
// thread (hugectr_amd/data.py) every output position has a closed form (include/hugectr_amd.h) and
// ONE launch writes label, dense, every param's (row offsets, keys) and every collection's
// (keys, bucket range).  A device-resident plan (hctr_parquet_segment table, built once per reader)
// lists the work; a workgroup takes work items grid-strided and finds an item's segment by binary
// search over item0:
//
//   * TILE   (label, dense, params whose slots are all scalar): column-major -> row-major.  A tile
//     of up to 32 columns x 64 .. 1024 samples (about 2048 elements: fewer columns, more samples)
//     is read with the lanes of a wave along the samples of ONE column (coalesced), converted,
//     parked in LDS as 8-byte words [column][samples + 1], and written with consecutive lanes on
//     consecutive output elements (coalesced); the cast or the addend is applied on the way in,
//     so LDS holds output bits.
//   * RAGGED (a param with a list slot): a group of lanes per sample (the plan chooses 1..64 from
//     the mean keys per sample).  The group sums off_s[a+b] - off_s[a] over the slots (the
//     sample's base), runs an exclusive prefix over the slots' lengths with shuffles and writes
//     the S row offsets of the sample with consecutive lanes, then walks the slots with its lanes
//     on consecutive keys.
//   * GROUP  (one lookup of a collection): a contiguous range of values widened to int64, and the
//     lookup's bucket range; the lookup's base is the sum of the counts of the lookups before it.
//
// Plain vector stores, every output element written exactly once, no atomics, no scratch; results
// do not depend on which workgroup takes which item.
// Compiled as part of embedding_kernels.hip's unit (included at its end, like raw_decode.hip).
#include "common.h"

namespace hctr {
namespace {

constexpr int kPqBlock = 256;
constexpr uint32_t kPqTs = HCTR_PQ_TILE_SAMPLES;  // one wave along the samples of a column
constexpr uint32_t kPqTc = HCTR_PQ_TILE_COLS;
constexpr uint32_t kPqLdsWords = kPqTc * (kPqTs + 1);  // 8-byte words of the tile

// samples of a TILE item: 64 at 32 columns and more, 64 * (32 / columns) below, at most 1024;
// columns * (samples + 1) <= kPqLdsWords
__device__ __forceinline__ uint32_t pq_tile_samples(uint32_t ncols) {
  const uint32_t nc = ncols < kPqTc ? ncols : kPqTc;
  const uint32_t k = kPqTc / nc;
  return kPqTs * (k < 16 ? k : 16);
}

struct PqCol {
  const char* values;
  const long long* offsets;  // nullptr: off[i] = i
  uint32_t ptype;
};

__device__ __forceinline__ PqCol pq_col(const char* __restrict__ slot,
                                        const hctr_parquet_column* __restrict__ cols, uint32_t c) {
  const hctr_parquet_column d = cols[c];
  PqCol r;
  r.values = slot + d.values;
  r.offsets = d.offsets == HCTR_PQ_NO_OFFSETS
                  ? nullptr : reinterpret_cast<const long long*>(slot + d.offsets);
  r.ptype = d.ptype;
  return r;
}
__device__ __forceinline__ long long pq_off(const PqCol& c, size_t i) {
  return c.offsets ? c.offsets[i] : (long long)i;
}
// element i of a column as a key: int32 is sign-extended (numpy's astype(np.int64))
__device__ __forceinline__ long long pq_key(const PqCol& c, size_t i) {
  return c.ptype == HCTR_PQ_I64 ? reinterpret_cast<const long long*>(c.values)[i]
                                : (long long)reinterpret_cast<const int32_t*>(c.values)[i];
}
// element i of a column as fp32, round to nearest even; via_f64: through fp64 first, as numpy does
// for columns it stacked into a float64 array (only an int64 beyond 2^53 can tell the difference)
__device__ __forceinline__ float pq_f32(const PqCol& c, size_t i, bool via_f64) {
  switch (c.ptype) {
    case HCTR_PQ_F32: return reinterpret_cast<const float*>(c.values)[i];
    case HCTR_PQ_F64: return (float)reinterpret_cast<const double*>(c.values)[i];
    case HCTR_PQ_I32: return (float)reinterpret_cast<const int32_t*>(c.values)[i];
    default: {
      const long long v = reinterpret_cast<const long long*>(c.values)[i];
      return via_f64 ? (float)(double)v : (float)v;
    }
  }
}

__device__ __forceinline__ void pq_tile(const hctr_parquet_segment& sg, uint32_t item,
                                        const char* __restrict__ slot,
                                        const hctr_parquet_column* __restrict__ cols,
                                        const long long* __restrict__ addend,
                                        const uint32_t* __restrict__ list, size_t a,
                                        char* __restrict__ out,
                                        const uint64_t* __restrict__ out_offsets,
                                        unsigned long long* __restrict__ tile) {
  if (sg.ncols == 0) return;
  const uint32_t col_chunks = (sg.ncols + kPqTc - 1) / kPqTc;
  const uint32_t TS = pq_tile_samples(sg.ncols), stride = TS + 1;
  const uint32_t ts = item / col_chunks, cc = item - ts * col_chunks;
  if (ts > (sg.sample1 - sg.sample0) / TS) return;  // (uniform over the workgroup)
  const uint32_t s_lo = sg.sample0 + ts * TS;
  const uint32_t c_lo = cc * kPqTc;
  if (s_lo >= sg.sample1 || c_lo >= sg.ncols) return;  // (uniform over the workgroup)
  const uint32_t ns = sg.sample1 - s_lo < TS ? sg.sample1 - s_lo : TS;
  const uint32_t nc = sg.ncols - c_lo < kPqTc ? sg.ncols - c_lo : kPqTc;
  const bool f32 = sg.out_kind == HCTR_PQ_OUT_F32 || sg.out_kind == HCTR_PQ_OUT_F32_VIA_F64;
  const bool via = sg.out_kind == HCTR_PQ_OUT_F32_VIA_F64;
  // in: a wave reads 64 consecutive samples of one column
  for (uint32_t e = threadIdx.x; e < nc * TS; e += kPqBlock) {
    const uint32_t j = e / TS, r = e - j * TS;
    if (r >= ns) continue;
    const uint32_t li = sg.list0 + c_lo + j;
    const PqCol c = pq_col(slot, cols, list[li]);
    const size_t row = a + s_lo + r;
    unsigned long long w;
    if (f32) w = (unsigned long long)__float_as_uint(pq_f32(c, row, via));
    else w = (unsigned long long)pq_key(c, row) + (unsigned long long)addend[li];
    tile[j * stride + r] = w;
  }
  __syncthreads();
  // out: rows [s_lo - sample0, ..) of a [samples][ncols] array, columns [c_lo, c_lo + nc)
  char* dst = out + out_offsets[sg.out0];
  const size_t drow0 = s_lo - sg.sample0;
  const bool wide = sg.out_kind == HCTR_PQ_OUT_KEY_I64;
  for (uint32_t e = threadIdx.x; e < ns * nc; e += kPqBlock) {
    const uint32_t r = e / nc, j = e - r * nc;
    const unsigned long long w = tile[j * stride + r];
    const size_t i = (drow0 + r) * (size_t)sg.ncols + c_lo + j;
    if (wide) reinterpret_cast<unsigned long long*>(dst)[i] = w;
    else reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)w;
  }
  __syncthreads();  // the tile is overwritten by the workgroup's next item
}

template <typename T>
__device__ __forceinline__ void pq_ragged(const hctr_parquet_segment& sg, uint32_t item,
                                          const char* __restrict__ slot,
                                          const hctr_parquet_column* __restrict__ cols,
                                          const long long* __restrict__ addend,
                                          const uint32_t* __restrict__ list, size_t a, size_t B,
                                          char* __restrict__ out,
                                          const uint64_t* __restrict__ out_offsets) {
  const uint32_t G = sg.group, S = sg.ncols;
  const uint32_t per_block = kPqBlock / G;
  const uint32_t g = threadIdx.x % G;
  const size_t b = (size_t)item * per_block + threadIdx.x / G;
  const bool live = b < B;  // (idle groups still take part in the shuffles)
  const size_t row = live ? a + b : a;
  T* ro = sg.out0 == HCTR_PQ_NO_OUTPUT ? nullptr
                                       : reinterpret_cast<T*>(out + out_offsets[sg.out0]);
  T* keys = reinterpret_cast<T*>(out + out_offsets[sg.out1]);
  // base of the sample: everything the samples before it hold, over all slots
  long long base = 0;
  for (uint32_t s = g; s < S; s += G) {
    const PqCol c = pq_col(slot, cols, list[sg.list0 + s]);
    base += pq_off(c, row) - pq_off(c, a);
  }
  for (uint32_t d = 1; d < G; d <<= 1) base += __shfl_xor(base, (int)d, (int)G);
  // exclusive prefix of the slots' lengths, G slots at a time: lane g writes slot s0 + g
  long long carry = base;
  for (uint32_t s0 = 0; s0 < S; s0 += G) {
    const uint32_t s = s0 + g;
    long long len = 0;
    if (s < S) {
      const PqCol c = pq_col(slot, cols, list[sg.list0 + s]);
      len = pq_off(c, row + 1) - pq_off(c, row);
    }
    long long incl = len;
    for (uint32_t d = 1; d < G; d <<= 1) {
      const long long t = __shfl_up(incl, d, (int)G);
      if (g >= d) incl += t;
    }
    if (live && ro && s < S) ro[b * S + s] = (T)(carry + incl - len);
    carry += __shfl(incl, (int)(G - 1), (int)G);
  }
  if (!live) return;
  if (ro && b == B - 1 && g == 0) ro[B * S] = (T)carry;  // = sum over the slots of off[a+B] - off[a]
  // keys: the slots one after another, the group's lanes on consecutive keys
  long long pos = base;
  for (uint32_t s = 0; s < S; s++) {
    const uint32_t li = sg.list0 + s;
    const PqCol c = pq_col(slot, cols, list[li]);
    const long long src = pq_off(c, row), len = pq_off(c, row + 1) - src;
    const unsigned long long add = (unsigned long long)addend[li];
    for (long long j = g; j < len; j += G)
      keys[pos + j] = (T)((unsigned long long)pq_key(c, (size_t)(src + j)) + add);
    pos += len;
  }
}

__device__ __forceinline__ void pq_group(const hctr_parquet_segment& sg, uint32_t item,
                                         const char* __restrict__ slot,
                                         const hctr_parquet_column* __restrict__ cols,
                                         const uint32_t* __restrict__ list, size_t a, size_t B,
                                         char* __restrict__ out,
                                         const uint64_t* __restrict__ out_offsets) {
  // keys of the lookups before this one (uniform over the workgroup), and of all of them
  long long kbase = 0, total = 0;
  for (uint32_t l = 0; l < sg.ncols; l++) {
    const PqCol c = pq_col(slot, cols, list[sg.list0 + l]);
    const long long n = pq_off(c, a + B) - pq_off(c, a);
    if (l < sg.lookup) kbase += n;
    total += n;
  }
  const PqCol c = pq_col(slot, cols, list[sg.list0 + sg.lookup]);
  const long long src0 = pq_off(c, a), cnt = pq_off(c, a + B) - src0;
  if (sg.out0 != HCTR_PQ_NO_OUTPUT) {
    long long* br = reinterpret_cast<long long*>(out + out_offsets[sg.out0]);
    const size_t b = (size_t)item * kPqBlock + threadIdx.x;
    if (b < B) br[(size_t)sg.lookup * B + b] = kbase + pq_off(c, a + b) - src0;
    if (sg.lookup + 1 == sg.ncols && b == B - 1) br[(size_t)sg.ncols * B] = total;
  }
  long long* keys = reinterpret_cast<long long*>(out + out_offsets[sg.out1]) + kbase;
  const long long step = (long long)sg.n_items * kPqBlock;
  for (long long i = (long long)item * kPqBlock + threadIdx.x; i < cnt; i += step)
    keys[i] = pq_key(c, (size_t)(src0 + i));
}

__global__ void __launch_bounds__(kPqBlock)
    parquet_decode_kernel(const char* __restrict__ slot,
                          const hctr_parquet_column* __restrict__ cols,
                          const hctr_parquet_segment* __restrict__ segs, int n_segments,
                          const long long* __restrict__ addend, const uint32_t* __restrict__ list,
                          uint32_t n_items, size_t a, size_t B, char* __restrict__ out,
                          const uint64_t* __restrict__ out_offsets) {
  __shared__ unsigned long long tile[kPqLdsWords];
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    // the last segment with item0 <= it (item0 is non-decreasing; uniform over the workgroup)
    int lo = 0, hi = n_segments - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].item0 <= it) lo = mid;
      else hi = mid - 1;
    }
    const hctr_parquet_segment sg = segs[lo];
    const uint32_t item = it - sg.item0;
    if (it < sg.item0 || item >= sg.n_items) continue;
    switch (sg.kind) {
      case HCTR_PQ_SEG_TILE:
        pq_tile(sg, item, slot, cols, addend, list, a, out, out_offsets, tile);
        break;
      case HCTR_PQ_SEG_RAGGED:
        if (sg.out_kind == HCTR_PQ_OUT_KEY_I64)
          pq_ragged<long long>(sg, item, slot, cols, addend, list, a, B, out, out_offsets);
        else
          pq_ragged<int32_t>(sg, item, slot, cols, addend, list, a, B, out, out_offsets);
        break;
      case HCTR_PQ_SEG_GROUP:
        pq_group(sg, item, slot, cols, list, a, B, out, out_offsets);
        break;
      default:
        break;  // (an unknown kind writes nothing)
    }
  }
}

}  // namespace
}  // namespace hctr

extern "C" {

int hctr_parquet_decode(const void* slot, const void* columns, int n_columns, const void* plan,
                        int n_segments, int n_list, size_t n_items, size_t rows, size_t first_row,
                        size_t batch, void* out_base, const uint64_t* out_offsets, int n_outputs,
                        hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(slot && columns && plan && out_base && out_offsets,
               "hctr_parquet_decode: null pointer");
  HCTR_REQUIRE(batch >= 1 && batch < (1ull << 31), "hctr_parquet_decode: batch must be 1..2^31-1");
  HCTR_REQUIRE(rows < (1ull << 40) && first_row <= rows && batch <= rows - first_row,
               "hctr_parquet_decode: rows [first_row, first_row + batch) must lie inside the file");
  HCTR_REQUIRE(n_columns >= 1 && n_columns < (1 << 24),
               "hctr_parquet_decode: n_columns must be 1..2^24-1");
  HCTR_REQUIRE(n_segments >= 1 && n_segments <= HCTR_PQ_DECODE_MAX_SEGMENTS,
               "hctr_parquet_decode: n_segments must be 1..4096");
  HCTR_REQUIRE(n_list >= 1 && n_list < (1 << 24), "hctr_parquet_decode: n_list must be 1..2^24-1");
  HCTR_REQUIRE(n_items >= 1 && n_items < (1ull << 31),
               "hctr_parquet_decode: n_items must be 1..2^31-1");
  HCTR_REQUIRE(n_outputs >= 1, "hctr_parquet_decode: n_outputs must be positive");
  HCTR_REQUIRE(((uintptr_t)slot & 7) == 0 && ((uintptr_t)columns & 7) == 0 &&
                   ((uintptr_t)plan & 7) == 0 && ((uintptr_t)out_base & 7) == 0 &&
                   ((uintptr_t)out_offsets & 7) == 0,
               "hctr_parquet_decode: slot, columns, plan, out_base and out_offsets must be 8-byte "
               "aligned");
  const hctr_parquet_segment* segs = (const hctr_parquet_segment*)plan;
  const long long* addend = (const long long*)(segs + n_segments);
  const uint32_t* list = (const uint32_t*)(addend + n_list);
  const int grid = (int)(n_items < (size_t)HCTR_PQ_DECODE_MAX_BLOCKS
                             ? n_items : (size_t)HCTR_PQ_DECODE_MAX_BLOCKS);
  hipLaunchKernelGGL(parquet_decode_kernel, dim3(grid), dim3(kPqBlock), 0, as_stream(stream),
                     (const char*)slot, (const hctr_parquet_column*)columns, segs, n_segments,
                     addend, list, (uint32_t)n_items, first_row, batch, (char*)out_base,
                     out_offsets);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
