// dense_lookup.hip -- the two kernels behind SOK's dense lookups (sok.all2all_dense_embedding,
// sok.group_lookup): a stable partition of keys by owner GPU and a batched indexed row copy.
// Compiled as part of embedding_kernels.hip.
//
// hctr_dist_select replaces the DistSelect op
// (R/sparse_operation_kit/kit_src/lookup/impl/select_kernel.cu:22-170, kernels/select.cc:41-70).
// The reference appends to each split through shared-memory atomics, so the order inside a split
// is the arrival order of that run.  Here the order is positional: every wavefront owns one
// contiguous chunk of the keys; (1) it counts its keys per owner in its own LDS row, (2) one
// exclusive scan runs over the counts laid out [owner][chunk], which is exactly the order of the
// output, (3) it walks its chunk again 64 keys at a time and gives each key the slot
// base[owner] + (number of lower lanes with the same owner), the lanes with the same owner found
// with one ballot per owner bit.  Chunks ascend with position, steps ascend inside a chunk, lanes
// ascend inside a step: a stable partition.
//
// hctr_indexed_row_copy replaces FusedLookupKernel (kit_src/lookup/impl/group_lookup.cu:24-42),
// reorderKernel and gatherExKernel (impl/reorder_kernel.cu:24-48): all three are "row i of the
// output is row f(i) of the input", for several (input, output) pairs at once in the first.  The
// reference gives a row to a warp (group lookup) or to a thread block (reorder / gatherEx) and
// copies element by element; here a group of min(64, dim/4) lanes owns 4 rows at a time, each lane
// moving 16 bytes of each, all four loads issued before the first store (the row fetch is bound by
// its round trip, not by bytes: DESIGN.md section 8, items 3 and 11).
#include "block_prims.h"
#include "common.h"
#include "cvt16.h"
#include "scan.h"

namespace hctr {
namespace {

// ---- dist_select --------------------------------------------------------------------------------
constexpr int kDsBlock = 256;
constexpr int kDsWaves = kDsBlock / kWave;
constexpr int kDsMaxSplits = 256;
constexpr size_t kDsMaxChunks = 1024;  // HCTR_DIST_SELECT_WS_BYTES counts on it
constexpr size_t kDsMinChunk = 256;    // keys: fewer are not worth a wavefront of their own

struct DsPlan {
  uint32_t chunks;  // wavefronts that have keys
  uint64_t per;     // keys per chunk, a multiple of 64
};

inline DsPlan ds_plan(size_t n) {
  size_t chunks = ceil_div<size_t>(n, kDsMinChunk);
  if (chunks > kDsMaxChunks) chunks = kDsMaxChunks;
  if (chunks < 1) chunks = 1;
  const size_t per = ceil_div<size_t>(ceil_div<size_t>(n, chunks), (size_t)kWave) * kWave;
  DsPlan p;
  p.per = per;
  p.chunks = (uint32_t)ceil_div<size_t>(n, per);
  return p;
}

// key mod N, the non-negative remainder
__device__ __forceinline__ uint32_t ds_owner(uint32_t key, uint32_t N) { return key % N; }
__device__ __forceinline__ uint32_t ds_owner(long long key, uint32_t N) {
  long long r = key % (long long)N;
  if (r < 0) r += (long long)N;
  return (uint32_t)r;
}

// the valid lanes of this wavefront whose owner equals mine (0 for a lane that is not valid).
// Called by whole wavefronts; bits = number of bits of N - 1.
__device__ __forceinline__ unsigned long long ds_peers(uint32_t owner, bool valid, int bits) {
  unsigned long long m = __ballot(valid);
  for (int b = 0; b < bits; b++) {
    const bool one = ((owner >> b) & 1u) != 0u;
    const unsigned long long s = __ballot(one);
    m &= one ? s : ~s;
  }
  return valid ? m : 0ull;
}

// 1/3: cnt[owner * chunks + chunk] = keys of that owner in that chunk.  A wavefront's LDS row is
// its own (the wave barrier orders its lanes' accesses; the row is read through a volatile pointer
// because other lanes write it).
template <typename K>
__global__ void __launch_bounds__(kDsBlock)
    ds_count_kernel(const K* __restrict__ keys, uint64_t n, uint32_t N, int bits, uint32_t chunks,
                    uint64_t per, unsigned long long* __restrict__ cnt) {
  __shared__ uint32_t s_cnt[kDsWaves][kDsMaxSplits];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t c = blockIdx.x * kDsWaves + w;  // wave-uniform
  if (c >= chunks) return;
  volatile uint32_t* mine = s_cnt[w];
  for (uint32_t o = lane; o < N; o += kWave) mine[o] = 0u;
  __builtin_amdgcn_wave_barrier();
  const uint64_t begin = (uint64_t)c * per;
  const uint64_t end = begin + per < n ? begin + per : n;
  for (uint64_t p0 = begin; p0 < end; p0 += kWave) {
    const uint64_t p = p0 + (unsigned)lane;
    const bool valid = p < end;
    const uint32_t owner = valid ? ds_owner(keys[p], N) : 0u;
    const unsigned long long m = ds_peers(owner, valid, bits);
    // the lowest lane of every owner present adds that owner's count: distinct addresses
    if (valid && (m & ((1ull << lane) - 1ull)) == 0ull)
      mine[owner] = mine[owner] + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  for (uint32_t o = lane; o < N; o += kWave) cnt[(size_t)o * chunks + c] = mine[o];
}

// 3/3: off = the exclusive scan of cnt (off[N * chunks] = n).  Block 0 also writes the splits.
template <typename K>
__global__ void __launch_bounds__(kDsBlock)
    ds_scatter_kernel(const K* __restrict__ keys, uint64_t n, uint32_t N, int bits, uint32_t chunks,
                      uint64_t per, const unsigned long long* __restrict__ off,
                      K* __restrict__ out_keys, int32_t* __restrict__ order,
                      int32_t* __restrict__ splits) {
  __shared__ uint32_t s_base[kDsWaves][kDsMaxSplits];
  if (blockIdx.x == 0)
    for (uint32_t o = threadIdx.x; o < N; o += kDsBlock)
      splits[o] = (int32_t)(off[(size_t)(o + 1) * chunks] - off[(size_t)o * chunks]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t c = blockIdx.x * kDsWaves + w;
  if (c >= chunks) return;
  volatile uint32_t* mine = s_base[w];
  for (uint32_t o = lane; o < N; o += kWave) mine[o] = (uint32_t)off[(size_t)o * chunks + c];
  __builtin_amdgcn_wave_barrier();
  const uint64_t begin = (uint64_t)c * per;
  const uint64_t end = begin + per < n ? begin + per : n;
  for (uint64_t p0 = begin; p0 < end; p0 += kWave) {
    const uint64_t p = p0 + (unsigned)lane;
    const bool valid = p < end;
    K key = 0;
    if (valid) key = keys[p];
    const uint32_t owner = valid ? ds_owner(key, N) : 0u;
    const unsigned long long m = ds_peers(owner, valid, bits);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    const uint32_t base = valid ? mine[owner] : 0u;
    __builtin_amdgcn_wave_barrier();  // every lane has read its base before a leader moves it
    if (valid) {
      const uint64_t j = (uint64_t)base + rank;
      if (j < n) {  // (always: the counts come from the same keys)
        out_keys[j] = key;
        order[j] = (int32_t)p;
      }
      if (rank == 0u) mine[owner] = base + (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

template <typename K>
int ds_run(const K* keys, size_t n, int num_splits, K* out_keys, int32_t* order, int32_t* splits,
           unsigned long long* ws, hipStream_t s) {
  const DsPlan p = ds_plan(n);
  const uint32_t N = (uint32_t)num_splits;
  int bits = 0;
  while ((1u << bits) < N) bits++;
  const size_t m = (size_t)N * p.chunks;
  const int grid = (int)ceil_div<size_t>(p.chunks, (size_t)kDsWaves);
  hipLaunchKernelGGL(ds_count_kernel<K>, dim3(grid), dim3(kDsBlock), 0, s, keys, (uint64_t)n, N,
                     bits, p.chunks, p.per, ws);
  HCTR_LAUNCH_CHECK();
  // in place; the total (= n) lands behind the last count, where the splits read it
  hipLaunchKernelGGL(scan_detail::scan_tiles_u64_kernel, dim3(1), dim3(1024), 0, s, ws, m, ws + m);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ds_scatter_kernel<K>, dim3(grid), dim3(kDsBlock), 0, s, keys, (uint64_t)n, N,
                     bits, p.chunks, p.per, ws, out_keys, order, splits);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// ---- indexed row copy ---------------------------------------------------------------------------
constexpr int kRcBlock = 256;
constexpr int kRcRows = 4;  // rows a lane group has in flight
constexpr int kRcMaxTasks = HCTR_ROW_COPY_MAX_TASKS;

// one task as the kernel sees it (the descriptors travel as kernel arguments)
struct RcTask {
  const void* src;
  const void* index;
  void* dst;
  const int32_t* dst_pos;
  uint64_t src_rows;  // 0: no upper bound
  uint64_t n;
  uint64_t dst_rows;
  uint32_t chunk0;     // first chunk of this task in the flattened (task, row) space
  uint32_t dim;
  uint32_t index_div;
  uint32_t flags;      // bit 0: int64 index; bit 1: 4-element path; bits 8..: log2(lanes per row)
};
struct RcArgs {
  RcTask t[kRcMaxTasks];
};

template <typename T, int W>
struct RcIo;
template <>
struct RcIo<float, 4> {
  __device__ __forceinline__ static float4 ld(const float* p) {
    return *reinterpret_cast<const float4*>(p);
  }
};
template <>
struct RcIo<__half, 4> {
  __device__ __forceinline__ static float4 ld(const __half* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    const __half2 a = *reinterpret_cast<const __half2*>(&u.x);
    const __half2 b = *reinterpret_cast<const __half2*>(&u.y);
    const float2 fa = __half22float2(a), fb = __half22float2(b);
    return make_float4(fa.x, fa.y, fb.x, fb.y);
  }
};
template <>
struct RcIo<float, 1> {
  __device__ __forceinline__ static float4 ld(const float* p) {
    return make_float4(*p, 0.f, 0.f, 0.f);
  }
};
template <>
struct RcIo<__half, 1> {
  __device__ __forceinline__ static float4 ld(const __half* p) {
    return make_float4(__half2float(*p), 0.f, 0.f, 0.f);
  }
};

// one chunk (kRcRows rows per lane group) of task T, W elements per lane and load.  Every load is
// unconditional on a clamped address (a load under a branch would wait for the ones before it):
// a row that is out of range reads row 0 and stores zeros, a position behind n reads position n - 1
// and stores nothing.
template <typename S, typename D, int W>
__device__ __forceinline__ void rc_chunk(const RcTask& T, uint64_t chunk) {
  const int gs = (int)(T.flags >> 8);
  const int gl = 1 << gs;
  const int rpp = kRcBlock >> gs;  // rows per pass of the workgroup
  const uint64_t g = threadIdx.x >> gs;
  const int l = (int)(threadIdx.x & (unsigned)(gl - 1));
  const uint64_t dim = T.dim;
  const int units = (int)(T.dim / (unsigned)W);
  const S* src = static_cast<const S*>(T.src);
  D* dst = static_cast<D*>(T.dst);
  const uint64_t base = chunk * (uint64_t)(rpp * kRcRows);
  uint64_t r[kRcRows], d[kRcRows];
  bool live[kRcRows], put[kRcRows];
#pragma unroll
  for (int u = 0; u < kRcRows; u++) {
    const uint64_t i = base + (uint64_t)(u * rpp) + g;
    const bool ok = i < T.n;
    const uint64_t ic = ok ? i : T.n - 1;
    uint64_t row = ic;
    bool lv = true;
    if (T.index != nullptr) {
      if (T.flags & 1u) {
        const long long k = static_cast<const long long*>(T.index)[ic];
        lv = k >= 0;  // (INVALID = -1: no row)
        row = (uint64_t)k;
      } else {
        row = static_cast<const uint32_t*>(T.index)[ic];
      }
      if (T.index_div != 1u) row /= (uint64_t)T.index_div;
    }
    lv = lv && (T.src_rows == 0ull || row < T.src_rows);
    long long dr = (long long)ic;
    if (T.dst_pos != nullptr) dr = T.dst_pos[ic];
    live[u] = lv;
    r[u] = lv ? row : 0ull;
    put[u] = ok && dr >= 0 && (uint64_t)dr < T.dst_rows;
    d[u] = (uint64_t)dr;
  }
  for (int vb = 0; vb < units; vb += gl) {
    const int v = vb + l;
    const bool vok = v < units;
    const uint64_t e = (uint64_t)(vok ? v : 0) * W;
    float4 x[kRcRows];
#pragma unroll
    for (int u = 0; u < kRcRows; u++) x[u] = RcIo<S, W>::ld(src + r[u] * dim + e);
#pragma unroll
    for (int u = 0; u < kRcRows; u++) {
      if (!(put[u] && vok)) continue;
      const float4 y = live[u] ? x[u] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (W == 4)
        st4_from_f32<D>(dst + d[u] * dim + e, y);
      else
        st_from_f32<D>(dst + d[u] * dim + e, y.x);
    }
  }
}

// grid-stride over the chunks of all tasks; a chunk lies inside one task, so the descriptor fields
// are wave-uniform (scalar loads from the kernel arguments)
template <typename S, typename D>
__global__ void __launch_bounds__(kRcBlock)
    rc_indexed_row_copy_kernel(RcArgs a, int num_tasks, uint32_t total_chunks) {
  for (uint32_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    int t = 0;  // the last task whose first chunk is <= c (tasks without rows have no chunk)
    for (int k = 1; k < num_tasks; k++) t += a.t[k].chunk0 <= c ? 1 : 0;
    const RcTask& T = a.t[t];
    if (T.flags & 2u)
      rc_chunk<S, D, 4>(T, (uint64_t)(c - T.chunk0));
    else
      rc_chunk<S, D, 1>(T, (uint64_t)(c - T.chunk0));
  }
}

template <typename S, typename D>
int rc_launch(const RcArgs& a, int num_tasks, uint32_t total_chunks, hipStream_t s) {
  const int grid = (int)(total_chunks < (uint32_t)kMaxGrid ? total_chunks : (uint32_t)kMaxGrid);
  hipLaunchKernelGGL((rc_indexed_row_copy_kernel<S, D>), dim3(grid), dim3(kRcBlock), 0, s, a,
                     num_tasks, total_chunks);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

inline bool rc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace hctr

using namespace hctr;

extern "C" {

int hctr_dist_select(const void* keys, int key_type, size_t n, int num_splits, void* out_keys,
                     int32_t* order, int32_t* splits, void* workspace, size_t workspace_bytes,
                     hctr_stream_t stream) {
  HCTR_REQUIRE(num_splits >= 1 && num_splits <= kDsMaxSplits, "num_splits must be in [1, 256]");
  HCTR_REQUIRE(key_type == HCTR_KEY_U32 || key_type == HCTR_KEY_I64,
               "key_type must be HCTR_KEY_U32 or HCTR_KEY_I64");
  HCTR_REQUIRE(n < ((size_t)1 << 31), "n must be below 2^31 (order is int32)");
  HCTR_REQUIRE(splits, "splits is null");
  HCTR_REQUIRE(n == 0 || (keys && out_keys && order), "keys / out_keys / order are null");
  HCTR_REQUIRE(n == 0 || workspace, "workspace is null");
  HCTR_REQUIRE(n == 0 || workspace_bytes >= HCTR_DIST_SELECT_WS_BYTES(num_splits),
               "workspace_bytes is below HCTR_DIST_SELECT_WS_BYTES(num_splits)");
  HCTR_REQUIRE(n == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
               "workspace must be 8-byte aligned");
  const hipStream_t s = as_stream(stream);
  if (n == 0) {
    HCTR_HIP(hipMemsetAsync(splits, 0, sizeof(int32_t) * (size_t)num_splits, s));
    return HCTR_OK;
  }
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  if (key_type == HCTR_KEY_I64)
    return ds_run<long long>(static_cast<const long long*>(keys), n, num_splits,
                             static_cast<long long*>(out_keys), order, splits, ws, s);
  return ds_run<uint32_t>(static_cast<const uint32_t*>(keys), n, num_splits,
                          static_cast<uint32_t*>(out_keys), order, splits, ws, s);
}

int hctr_indexed_row_copy(const hctr_row_copy_task* tasks, int num_tasks, int src_dtype,
                          int dst_dtype, hctr_stream_t stream) {
  HCTR_REQUIRE(tasks, "tasks is null");
  HCTR_REQUIRE(num_tasks >= 1 && num_tasks <= kRcMaxTasks,
               "num_tasks must be in [1, HCTR_ROW_COPY_MAX_TASKS]");
  HCTR_REQUIRE(src_dtype == HCTR_EMB_F32 || src_dtype == HCTR_EMB_F16,
               "src_dtype must be HCTR_EMB_F32 or HCTR_EMB_F16");
  HCTR_REQUIRE(dst_dtype == HCTR_EMB_F32 || dst_dtype == HCTR_EMB_F16,
               "dst_dtype must be HCTR_EMB_F32 or HCTR_EMB_F16");
  RcArgs a{};
  uint64_t chunks = 0;
  for (int k = 0; k < num_tasks; k++) {
    const hctr_row_copy_task& in = tasks[k];
    const std::string at = "task " + std::to_string(k) + ": ";
    HCTR_REQUIRE(in.dim >= 1, at + "dim must be positive");
    HCTR_REQUIRE(in.index_div >= 1 && in.index_div < (1ull << 32),
                 at + "index_div must be in [1, 2^32)");
    HCTR_REQUIRE(!in.index || in.index_type == HCTR_KEY_U32 || in.index_type == HCTR_KEY_I64,
                 at + "index_type must be HCTR_KEY_U32 or HCTR_KEY_I64");
    HCTR_REQUIRE(in.n == 0 || (in.src && in.dst), at + "src / dst are null");
    HCTR_REQUIRE(!in.dst_pos || in.n < ((size_t)1 << 31), at + "n must be below 2^31 with dst_pos");
    HCTR_REQUIRE(in.dst_pos || in.dst_rows >= in.n, at + "dst_rows is below n");
    const bool vec = in.dim % 4 == 0 && rc_aligned16(in.src) && rc_aligned16(in.dst);
    const int units = vec ? in.dim / 4 : in.dim;
    int gs = 0;
    while ((1 << gs) < units && (1 << gs) < kWave) gs++;
    const uint64_t rows_per_chunk = (uint64_t)(kRcBlock >> gs) * kRcRows;
    RcTask& t = a.t[k];
    t.src = in.src;
    t.index = in.index;
    t.dst = in.dst;
    t.dst_pos = in.dst_pos;
    t.src_rows = in.src_rows;
    t.n = in.n;
    t.dst_rows = in.dst_rows;
    t.chunk0 = (uint32_t)chunks;
    t.dim = (uint32_t)in.dim;
    t.index_div = (uint32_t)in.index_div;
    t.flags = (in.index && in.index_type == HCTR_KEY_I64 ? 1u : 0u) | (vec ? 2u : 0u) |
              ((uint32_t)gs << 8);
    chunks += ceil_div<uint64_t>(in.n, rows_per_chunk);
    HCTR_REQUIRE(chunks < (1ull << 31), at + "too many rows in one call");
  }
  if (chunks == 0) return HCTR_OK;
  const hipStream_t s = as_stream(stream);
  const uint32_t total = (uint32_t)chunks;
  if (src_dtype == HCTR_EMB_F32 && dst_dtype == HCTR_EMB_F32)
    return rc_launch<float, float>(a, num_tasks, total, s);
  if (src_dtype == HCTR_EMB_F32) return rc_launch<float, __half>(a, num_tasks, total, s);
  if (dst_dtype == HCTR_EMB_F32) return rc_launch<__half, float>(a, num_tasks, total, s);
  return rc_launch<__half, __half>(a, num_tasks, total, s);
}

}  // extern "C"
