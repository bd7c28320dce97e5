// ebc_unique.hip -- CompressionStrategy.Unique for embedding_collection on several GPUs (compiled
// inside ebc.hip, which provides the includes, kBlock, ld_as_f32 / st_from_f32 and hctr_updater).
//
// The reference's second model-parallel operator (R/HugeCTR/embedding/
// dense_model_parallel_embedding.cpp, key side data_distributor/
// dense_data_distribution_op_impl.cu): instead of one pooled vector per (lookup, sample) the owner
// ships every DISTINCT row once per destination GPU, the receiver pools, per-row gradient SUMS
// travel back.  Restated here with two deliberate differences:
//   * de-duplication happens on the OWNER, per destination, over the routed CSR it builds anyway
//     (the reference hashes on the sender before the key exchange, partition_and_unique_on_dp_input);
//   * every sum is ordered and fp32, rounded once (the reference's receiver adds with
//     one_to_one_atomic in arrival order, network_forward.cu:525-528, and for a 16-bit output
//     accumulates in the 16-bit type).  Two runs give identical bits; no float atomics anywhere.
//
// Owner:    routed CSR, buckets [peer][local lookup][b_local] (a peer's keys are one range)
//           hctr_ebc_uniq_plan: stable sort by row, one stable pass by peer -> per peer the
//           distinct rows ascending (urow, peer_off) and ridx[j] = index of key j's row in its
//           peer's list; hctr_ebc_uniq_gather_rows fills the send buffer.
// Receiver: hctr_ebc_uniq_network_forward gathers and pools out of the compact row buffer;
//           hctr_ebc_uniq_network_backward groups the key positions by received row (stable sort)
//           and sums the buckets' gradients per row in ascending position order (the segmented
//           reduce of the sparse update, hctr_updater_reduce_presorted: 32-position tiles, a run
//           that spans tiles is summed by several lane groups and its partials added in tile order).

namespace hctr {
namespace {

constexpr uint64_t kUniqMaxRow = 0xFFFFFFEFull;  // the sparse updater's row bound (2^32 - 16 rows)

__device__ __forceinline__ int uniq_peer_of(unsigned long long j, int world, size_t bpp,
                                            const long long* __restrict__ bucket_range) {
  // last peer p with key_off[p] <= j, key_off[p] = bucket_range[p * bpp]; j >= key_off[world]
  // (padding behind the live keys) -> world
  int lo = 0, hi = world + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned long long)bucket_range[(size_t)mid * bpp] <= j) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__global__ void __launch_bounds__(kBlock)
    uniq_plan_init_kernel(size_t n, size_t nb, const long long* __restrict__ bucket_range,
                          const uint64_t* __restrict__ rows, uint32_t* __restrict__ r32,
                          uint32_t* __restrict__ iota) {
  const size_t live = (size_t)bucket_range[nb];
  for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < n;
       j += (size_t)gridDim.x * kBlock) {
    // (a row number above the bound is the dynamic table's "no row" of a key that an evaluation
    //  lookup did not find: it stays one distinct entry, which the gather fills with zeros)
    r32[j] = j < live ? (rows[j] > kUniqMaxRow ? 0xFFFFFFFFu : (uint32_t)rows[j]) : 0u;
    iota[j] = (uint32_t)j;
  }
}

__global__ void __launch_bounds__(kBlock)
    uniq_plan_peer_kernel(size_t n, int world, size_t bpp,
                          const long long* __restrict__ bucket_range,
                          const uint32_t* __restrict__ pos_s, uint32_t* __restrict__ peer) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kBlock)
    peer[i] = (uint32_t)uniq_peer_of(pos_s[i], world, bpp, bucket_range);
}

// after the pass by peer: position q holds (peer_s[q], row r_s[idx_s[q]]), rows ascending inside a
// peer; a run head is the first position of a (peer, row)
__global__ void __launch_bounds__(kBlock)
    uniq_plan_flags_kernel(size_t n, int world, const uint32_t* __restrict__ peer_s,
                           const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ r_s,
                           uint32_t* __restrict__ flags) {
  for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n;
       q += (size_t)gridDim.x * kBlock) {
    const uint32_t p = peer_s[q];
    uint32_t f = 0u;
    if (p < (uint32_t)world)
      f = (q == 0 || peer_s[q - 1] != p || r_s[idx_s[q - 1]] != r_s[idx_s[q]]) ? 1u : 0u;
    flags[q] = f;
  }
}

// gid = exclusive scan of flags (n + 1 entries, gid[n] = distinct rows over all peers); peer p's
// sorted segment is [key_off[p], key_off[p + 1]) because the pass by peer is stable and complete
__global__ void __launch_bounds__(kBlock)
    uniq_plan_emit_kernel(size_t n, int world, size_t bpp,
                          const long long* __restrict__ bucket_range,
                          const uint32_t* __restrict__ peer_s, const uint32_t* __restrict__ idx_s,
                          const uint32_t* __restrict__ r_s, const uint32_t* __restrict__ pos_s,
                          const uint32_t* __restrict__ flags, const uint32_t* __restrict__ gid,
                          uint64_t* __restrict__ urow, long long* __restrict__ peer_off,
                          uint32_t* __restrict__ ridx) {
  for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n;
       q += (size_t)gridDim.x * kBlock) {
    if (q <= (size_t)world) peer_off[q] = (long long)gid[(size_t)bucket_range[q * bpp]];
    const uint32_t p = peer_s[q];
    if (p >= (uint32_t)world) continue;
    const uint32_t f = flags[q];
    const uint32_t g = gid[q] + f - 1u;
    const uint32_t first = gid[(size_t)bucket_range[(size_t)p * bpp]];
    const uint32_t i = idx_s[q];
    ridx[pos_s[i]] = g - first;
    if (f) urow[g] = r_s[i] == 0xFFFFFFFFu ? ~0ull : (uint64_t)r_s[i];
  }
}

// owner: distinct rows of the fp32 table -> send buffer in the vector type; a row number at or
// above row_bound ("no row") sends zeros
template <typename T>
__global__ void __launch_bounds__(kBlock)
    uniq_gather_bounded_kernel(size_t n, int ev, const uint64_t* __restrict__ urow,
                               const float* __restrict__ table, uint64_t row_bound,
                               T* __restrict__ out) {
  const size_t total = n * (size_t)ev;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const size_t r = i / ev;
    const uint64_t row = urow[r];
    st_from_f32<T>(out + i, row < row_bound ? table[row * (uint64_t)ev + (i - r * ev)] : 0.f);
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
    uniq_gather_bounded_vec_kernel(size_t n, int ev, const uint64_t* __restrict__ urow,
                                   const float* __restrict__ table, uint64_t row_bound,
                                   T* __restrict__ out) {
  const int d4 = ev / 4;
  const size_t total = n * (size_t)d4;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const size_t r = i / d4;
    const int c = (int)(i - r * d4);
    const uint64_t row = urow[r];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < row_bound) v = *reinterpret_cast<const float4*>(table + row * (uint64_t)ev + c * 4);
    T* o = out + r * (size_t)ev + c * 4;
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<float4*>(o) = v;
    } else {
      alignas(8) T t[4];
      st_from_f32<T>(t, v.x);
      st_from_f32<T>(t + 1, v.y);
      st_from_f32<T>(t + 2, v.z);
      st_from_f32<T>(t + 3, v.w);
      *reinterpret_cast<uint2*>(o) = *reinterpret_cast<uint2*>(t);
    }
  }
}

// (n == 0 or fewer positions than peers: the offsets alone)
__global__ void __launch_bounds__(kBlock)
    uniq_plan_offsets_kernel(size_t n, int world, size_t bpp,
                             const long long* __restrict__ bucket_range,
                             const uint32_t* __restrict__ gid, long long* __restrict__ peer_off) {
  for (int p = threadIdx.x; p <= world; p += kBlock)
    peer_off[p] = n == 0 ? 0ll : (long long)gid[(size_t)bucket_range[(size_t)p * bpp]];
}

struct UniqPlanWs {
  uint32_t *r32, *iota, *r_s, *pos_s, *peer, *peer_s, *idx_s, *flags, *gid;
  unsigned long long *tile_sums, *d_total;
  void* sort_temp;
  size_t sort_bytes, total;
};

inline UniqPlanWs uniq_plan_ws(void* base, size_t n) {
  const size_t m = n > 0 ? n : 1;
  const size_t a = ((m + 1) * sizeof(uint32_t) + 15) / 16 * 16;  // one u32 array, 16-byte steps
  char* p = (char*)base;
  UniqPlanWs w;
  uint32_t** arrs[] = {&w.r32, &w.iota, &w.r_s, &w.pos_s, &w.peer, &w.peer_s, &w.idx_s, &w.flags,
                       &w.gid};
  for (uint32_t** q : arrs) {
    *q = (uint32_t*)p;
    p += a;
  }
  w.tile_sums = (unsigned long long*)p;
  p += (m / 1024 + 2) * 8;
  w.d_total = (unsigned long long*)p;
  p += 16;
  w.sort_temp = p;
  w.sort_bytes = radix_sort_temp_bytes(m);
  p += w.sort_bytes;
  w.total = (size_t)(p - (char*)base) + 64;
  return w;
}

inline int bit_length(uint64_t v) {
  int b = 1;
  while (b < 64 && (v >> b) != 0) b++;
  return b;
}

// ---- receiver, forward: out[l][b] = (sum over shards s of (sum over the keys of bucket
//      (block(l, s), b) of rows[r_off[src] + ridx[q]])) / count, fp32, rounded once
template <typename T>
__global__ void __launch_bounds__(kBlock)
    uniq_fwd_vec_kernel(size_t bpg, int num_lookup, int row16, int max_shards,
                        const int* __restrict__ src_blocks, const int* __restrict__ combiner,
                        const long long* __restrict__ bucket_counts, int batch_major,
                        const long long* __restrict__ recv_range,
                        const uint32_t* __restrict__ ridx, const long long* __restrict__ r_off,
                        const int* __restrict__ blk_src, const uint32_t* __restrict__ one_hot,
                        const uint4* __restrict__ rows, uint4* __restrict__ out) {
  constexpr int N = Vec16<T>::N;
  constexpr int U = 4;  // rows in flight per lane
  // every received bucket holds exactly its own key: no offsets are read
  const bool flat = one_hot != nullptr && *one_hot != 0u;
  const size_t total = (size_t)num_lookup * bpg * row16;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const size_t lb = i / (uint32_t)row16;
    const uint32_t c = (uint32_t)(i - lb * (uint32_t)row16);
    const uint32_t l = (uint32_t)(lb / bpg);
    const size_t b = lb - (size_t)l * bpg;
    float div = 1.0f;
    if (combiner[l] == 1) {
      const long long cnt = bucket_counts[(size_t)l * bpg + b];
      if (cnt > 0) div = (float)cnt;
    }
    const int* blocks = src_blocks + (size_t)l * max_shards;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; k++) acc[k] = 0.f;
    for (int s = 0; s < max_shards; s++) {
      const int blk = blocks[s];
      if (blk < 0) continue;
      const size_t bucket = (size_t)blk * bpg + b;
      const size_t q0 = flat ? bucket : (size_t)recv_range[bucket];
      const size_t q1 = flat ? bucket + 1 : (size_t)recv_range[bucket + 1];
      const size_t base = (size_t)r_off[blk_src[blk]];
      float part[N];
#pragma unroll
      for (int k = 0; k < N; k++) part[k] = 0.f;
      for (size_t q = q0; q < q1; q += U) {
        uint4 v[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
          const size_t qq = q + k < q1 ? q + k : q1 - 1;
          v[k] = rows[(base + ridx[qq]) * (size_t)row16 + c];
        }
#pragma unroll
        for (int k = 0; k < U; k++) {
          if (q + k < q1) {
            const T* rt = reinterpret_cast<const T*>(&v[k]);
#pragma unroll
            for (int e = 0; e < N; e++) part[e] += ld_as_f32<T>(rt + e);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < N; k++) acc[k] += part[k];
    }
    uint4 o;
    T* ot = reinterpret_cast<T*>(&o);
#pragma unroll
    for (int k = 0; k < N; k++) st_from_f32<T>(ot + k, acc[k] / div);
    out[(batch_major ? (b * (size_t)num_lookup + l) : ((size_t)l * bpg + b)) * row16 + c] = o;
  }
}

// any other vector size: one thread per element
template <typename T>
__global__ void __launch_bounds__(kBlock)
    uniq_fwd_kernel(size_t bpg, int num_lookup, int ev, int max_shards,
                    const int* __restrict__ src_blocks, const int* __restrict__ combiner,
                    const long long* __restrict__ bucket_counts, int batch_major,
                    const long long* __restrict__ recv_range, const uint32_t* __restrict__ ridx,
                    const long long* __restrict__ r_off, const int* __restrict__ blk_src,
                    const T* __restrict__ rows, T* __restrict__ out) {
  const size_t total = (size_t)num_lookup * bpg * ev;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const int e = (int)(i % ev);
    const size_t lb = i / ev;
    const size_t b = lb % bpg;
    const int l = (int)(lb / bpg);
    float div = 1.0f;
    if (combiner[l] == 1) {
      const long long cnt = bucket_counts[(size_t)l * bpg + b];
      if (cnt > 0) div = (float)cnt;
    }
    float acc = 0.f;
    for (int s = 0; s < max_shards; s++) {
      const int blk = src_blocks[l * max_shards + s];
      if (blk < 0) continue;
      const size_t bucket = (size_t)blk * bpg + b;
      const size_t base = (size_t)r_off[blk_src[blk]];
      float part = 0.f;
      for (size_t q = (size_t)recv_range[bucket]; q < (size_t)recv_range[bucket + 1]; q++)
        part += ld_as_f32<T>(rows + (base + ridx[q]) * (size_t)ev + e);
      acc += part;
    }
    const size_t dense_idx = batch_major ? (b * (size_t)num_lookup + l) * ev + e
                                         : ((size_t)l * bpg + b) * ev + e;
    st_from_f32<T>(out + dense_idx, acc / div);
  }
}

// ---- receiver, backward ---------------------------------------------------------------------------
// gradient of every bucket divided by its key count (Average lookups), kept fp32
template <typename T>
__global__ void __launch_bounds__(kBlock)
    uniq_scale_grad_kernel(size_t bpg, int num_lookup, int ev, const int* __restrict__ combiner,
                           const long long* __restrict__ bucket_counts, int batch_major,
                           const T* __restrict__ grad, float* __restrict__ out) {
  const size_t total = (size_t)num_lookup * bpg * ev;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (size_t)gridDim.x * kBlock) {
    const size_t v = i / ev;  // gradient row, in the output's own layout
    const size_t b = batch_major ? v / num_lookup : v % bpg;
    const int l = (int)(batch_major ? v % num_lookup : v / bpg);
    float div = 1.0f;
    if (combiner[l] == 1) {
      const long long cnt = bucket_counts[(size_t)l * bpg + b];
      if (cnt > 0) div = (float)cnt;
    }
    out[i] = ld_as_f32<T>(grad + i) / div;
  }
}

// key position q of received bucket (block, b) -> (row of the received buffer, gradient row)
__global__ void __launch_bounds__(kBlock)
    uniq_bwd_expand_kernel(size_t nbk, size_t bpg, int num_lookup, int batch_major,
                           const long long* __restrict__ recv_range,
                           const uint32_t* __restrict__ ridx, const long long* __restrict__ r_off,
                           const int* __restrict__ blk_src, const int* __restrict__ blk_lookup,
                           uint32_t* __restrict__ grow, uint32_t* __restrict__ pos_bucket,
                           uint32_t* __restrict__ iota) {
  for_each_key_wave(nbk, recv_range, [&](size_t bucket, size_t q) {
    const size_t blk = bucket / bpg, b = bucket - blk * bpg;
    const uint32_t l = (uint32_t)blk_lookup[blk];
    grow[q] = (uint32_t)r_off[blk_src[blk]] + ridx[q];
    pos_bucket[q] = batch_major ? (uint32_t)(b * (size_t)num_lookup + l)
                                : (uint32_t)((size_t)l * bpg + b);
    iota[q] = (uint32_t)q;
  });
}

__global__ void __launch_bounds__(kBlock)
    uniq_bwd_buckets_kernel(size_t n, size_t out_buckets, const uint32_t* __restrict__ pos_s,
                            const uint32_t* __restrict__ pos_bucket,
                            uint32_t* __restrict__ sorted_bucket, long long* __restrict__ live) {
  // live[out_buckets] = n: the position count the segmented reduce reads on the device
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n || i <= out_buckets;
       i += (size_t)gridDim.x * kBlock) {
    if (i < n) sorted_bucket[i] = pos_bucket[pos_s[i]];
    if (i <= out_buckets) live[i] = i == out_buckets ? (long long)n : 0ll;
  }
}

struct UniqBwdWs {
  uint32_t *grow, *iota, *pos_bucket, *rows_s, *pos_s, *bucket_s;
  long long* live;
  float* scaled;
  void* sort_temp;
  size_t sort_bytes, total;
};

inline UniqBwdWs uniq_bwd_ws(void* base, size_t n, size_t out_buckets, int ev) {
  const size_t m = n > 0 ? n : 1;
  const size_t a = (m * sizeof(uint32_t) + 15) / 16 * 16;
  char* p = (char*)base;
  UniqBwdWs w;
  uint32_t** arrs[] = {&w.grow, &w.iota, &w.pos_bucket, &w.rows_s, &w.pos_s, &w.bucket_s};
  for (uint32_t** q : arrs) {
    *q = (uint32_t*)p;
    p += a;
  }
  w.live = (long long*)p;
  p += ((out_buckets + 1) * 8 + 15) / 16 * 16;
  w.scaled = (float*)p;
  p += (out_buckets * (size_t)ev * sizeof(float) + 15) / 16 * 16;
  w.sort_temp = p;
  w.sort_bytes = radix_sort_temp_bytes(m);
  p += w.sort_bytes;
  w.total = (size_t)(p - (char*)base) + 64;
  return w;
}

}  // namespace
}  // namespace hctr

extern "C" {

size_t hctr_ebc_uniq_plan_workspace_bytes(size_t max_positions) {
  return hctr::uniq_plan_ws(nullptr, max_positions).total;
}

int hctr_ebc_uniq_plan(size_t positions, int world, size_t buckets_per_peer,
                       const int64_t* bucket_range, const uint64_t* rows, uint64_t max_row,
                       uint64_t* urow, int64_t* peer_off, uint32_t* ridx, void* workspace,
                       size_t workspace_bytes, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(world >= 1 && world <= 1024, "world");
  HCTR_REQUIRE(positions < 0xFFFFFFF0ull, "positions");
  HCTR_REQUIRE(max_row <= kUniqMaxRow, "row numbers must stay below 2^32 - 16");
  HCTR_REQUIRE(bucket_range && peer_off, "null pointer");
  HCTR_REQUIRE(positions == 0 || (rows && urow && ridx && workspace), "null pointer");
  const UniqPlanWs w = uniq_plan_ws(workspace, positions);
  HCTR_REQUIRE(positions == 0 || workspace_bytes >= w.total, "workspace too small");
  hipStream_t s = as_stream(stream);
  const size_t n = positions, bpp = buckets_per_peer;
  const long long* br = (const long long*)bucket_range;
  if (n == 0) {
    hipLaunchKernelGGL(uniq_plan_offsets_kernel, dim3(1), dim3(kBlock), 0, s, n, world, bpp, br,
                       (const uint32_t*)nullptr, (long long*)peer_off);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }
  const int grid = grid_for(n, kBlock, 4096);
  hipLaunchKernelGGL(uniq_plan_init_kernel, dim3(grid), dim3(kBlock), 0, s, n,
                     (size_t)world * bpp, br, rows, w.r32, w.iota);
  HCTR_LAUNCH_CHECK();
  // (a 32-bit key cannot hold (peer, row) for rows up to 2^32 - 16: rows first, then one stable
  //  pass by peer)
  HCTR_TRY(radix_sort_pairs_u32(w.sort_temp, w.sort_bytes, w.r32, w.r_s, w.iota, w.pos_s, n,
                                bit_length(max_row) > 32 ? 32 : bit_length(max_row), s));
  hipLaunchKernelGGL(uniq_plan_peer_kernel, dim3(grid), dim3(kBlock), 0, s, n, world, bpp, br,
                     w.pos_s, w.peer);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(radix_sort_pairs_u32(w.sort_temp, w.sort_bytes, w.peer, w.peer_s, w.iota, w.idx_s, n,
                                bit_length((uint64_t)world), s));
  hipLaunchKernelGGL(uniq_plan_flags_kernel, dim3(grid), dim3(kBlock), 0, s, n, world, w.peer_s,
                     w.idx_s, w.r_s, w.flags);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(exclusive_scan_to_offsets<uint32_t>(w.flags, n, w.tile_sums, w.d_total, w.gid, s));
  hipLaunchKernelGGL(uniq_plan_emit_kernel, dim3(grid), dim3(kBlock), 0, s, n, world, bpp, br,
                     w.peer_s, w.idx_s, w.r_s, w.pos_s, w.flags, w.gid, urow,
                     (long long*)peer_off, ridx);
  HCTR_LAUNCH_CHECK();
  if (n <= (size_t)world) {  // fewer positions than peers: the emit pass did not reach every offset
    hipLaunchKernelGGL(uniq_plan_offsets_kernel, dim3(1), dim3(kBlock), 0, s, n, world, bpp, br,
                       w.gid, (long long*)peer_off);
    HCTR_LAUNCH_CHECK();
  }
  return HCTR_OK;
}

int hctr_ebc_uniq_gather_rows(size_t n_rows, int ev_size, const uint64_t* urow, const float* table,
                              uint64_t row_bound, void* out, int out_dtype, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(ev_size > 0, "ev_size");
  HCTR_REQUIRE(out_dtype == HCTR_EMB_F32 || out_dtype == HCTR_EMB_F16 || out_dtype == HCTR_EMB_BF16,
               "out_dtype");
  if (n_rows == 0) return HCTR_OK;
  HCTR_REQUIRE(urow && table && out, "null pointer");
  hipStream_t s = as_stream(stream);
  const bool vec = ev_size % 4 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0;
#define HCTR_UGATHER(T)                                                                          \
  if (vec)                                                                                       \
    hipLaunchKernelGGL((uniq_gather_bounded_vec_kernel<T>),                                      \
                       dim3(grid_for(n_rows * (size_t)(ev_size / 4), kBlock, 8192)), dim3(kBlock), \
                       0, s, n_rows, ev_size, urow, table, row_bound, (T*)out);                  \
  else                                                                                           \
    hipLaunchKernelGGL((uniq_gather_bounded_kernel<T>),                                          \
                       dim3(grid_for(n_rows * (size_t)ev_size, kBlock, 8192)), dim3(kBlock), 0, s, \
                       n_rows, ev_size, urow, table, row_bound, (T*)out);
  if (out_dtype == HCTR_EMB_F32) {
    HCTR_UGATHER(float)
  } else if (out_dtype == HCTR_EMB_F16) {
    HCTR_UGATHER(__half)
  } else {
    HCTR_UGATHER(__hip_bfloat16)
  }
#undef HCTR_UGATHER
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_ebc_uniq_network_forward(size_t batch_per_gpu, int num_lookup, int ev_size, int max_shards,
                                  const int32_t* d_src_blocks, const int32_t* d_combiner,
                                  const int64_t* d_bucket_counts, int batch_major,
                                  const int64_t* recv_range, const uint32_t* ridx,
                                  const int64_t* r_off, const int32_t* d_block_source,
                                  const uint32_t* d_one_hot, const void* rows, void* out, int dtype,
                                  hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(num_lookup >= 0 && ev_size > 0 && max_shards >= 1, "num_lookup / ev_size / max_shards");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16, "dtype");
  const size_t total = (size_t)num_lookup * batch_per_gpu * ev_size;
  if (total == 0) return HCTR_OK;
  HCTR_REQUIRE(d_src_blocks && d_combiner && d_bucket_counts && recv_range && r_off &&
                   d_block_source && out,
               "null pointer");
  // (rows / ridx may be null only when no key arrived at all; the ranges then are all empty)
  hipStream_t s = as_stream(stream);
  const size_t esz = dtype == HCTR_EMB_F32 ? 4 : 2;
  const bool vec = ((size_t)ev_size * esz) % 16 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0;
#define HCTR_UFWD(T)                                                                             \
  if (vec) {                                                                                     \
    const int row16 = (int)((size_t)ev_size * sizeof(T) / 16);                                   \
    hipLaunchKernelGGL((uniq_fwd_vec_kernel<T>),                                                 \
                       dim3(grid_for((size_t)num_lookup * batch_per_gpu * row16, kBlock, 8192)), \
                       dim3(kBlock), 0, s, batch_per_gpu, num_lookup, row16, max_shards,         \
                       d_src_blocks, d_combiner, (const long long*)d_bucket_counts, batch_major, \
                       (const long long*)recv_range, ridx, (const long long*)r_off,              \
                       d_block_source, d_one_hot, (const uint4*)rows, (uint4*)out);              \
  } else {                                                                                       \
    hipLaunchKernelGGL((uniq_fwd_kernel<T>), dim3(grid_for(total, kBlock, 8192)), dim3(kBlock),  \
                       0, s, batch_per_gpu, num_lookup, ev_size, max_shards, d_src_blocks,       \
                       d_combiner, (const long long*)d_bucket_counts, batch_major,               \
                       (const long long*)recv_range, ridx, (const long long*)r_off,              \
                       d_block_source, (const T*)rows, (T*)out);                                 \
  }
  if (dtype == HCTR_EMB_F32) {
    HCTR_UFWD(float)
  } else if (dtype == HCTR_EMB_F16) {
    HCTR_UFWD(__half)
  } else {
    HCTR_UFWD(__hip_bfloat16)
  }
#undef HCTR_UFWD
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_ebc_uniq_backward_workspace_bytes(size_t max_positions, size_t batch_per_gpu,
                                              int num_lookup, int ev_size) {
  return hctr::uniq_bwd_ws(nullptr, max_positions, batch_per_gpu * (size_t)(num_lookup > 0 ? num_lookup : 0),
                           ev_size > 0 ? ev_size : 1).total;
}

int hctr_ebc_uniq_network_backward(hctr_updater* u, size_t batch_per_gpu, int num_lookup,
                                   int ev_size, int num_blocks, const int32_t* d_block_lookup,
                                   const int32_t* d_block_source, const int32_t* d_combiner,
                                   const int64_t* d_bucket_counts, int batch_major, int any_average,
                                   const int64_t* recv_range, const uint32_t* ridx,
                                   const int64_t* r_off, size_t positions, size_t n_rows,
                                   const void* grad, int grad_dtype, float* out_sum,
                                   void* workspace, size_t workspace_bytes, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(u, "null handle");
  HCTR_REQUIRE(num_lookup >= 0 && num_blocks >= 0 && ev_size > 0, "num_lookup / num_blocks / ev_size");
  HCTR_REQUIRE(ev_size == u->impl.D, "ev_size differs from the updater's vector size");
  HCTR_REQUIRE(grad_dtype == HCTR_EMB_F32 || grad_dtype == HCTR_EMB_F16 ||
                   grad_dtype == HCTR_EMB_BF16,
               "grad_dtype");
  HCTR_REQUIRE(positions < 0xFFFFFFF0ull && n_rows <= positions, "positions / n_rows");
  if (n_rows == 0) return HCTR_OK;
  const size_t out_buckets = batch_per_gpu * (size_t)num_lookup;
  const size_t nbk = batch_per_gpu * (size_t)num_blocks;
  HCTR_REQUIRE(out_buckets > 0 && out_buckets < 0xFFFFFFF0ull && nbk > 0, "no buckets");
  HCTR_REQUIRE(d_block_lookup && d_block_source && d_combiner && d_bucket_counts && recv_range &&
                   ridx && r_off && grad && out_sum && workspace,
               "null pointer");
  const UniqBwdWs w = uniq_bwd_ws(workspace, positions, out_buckets, ev_size);
  HCTR_REQUIRE(workspace_bytes >= w.total, "workspace too small");
  hipStream_t s = as_stream(stream);
  const void* g = grad;
  int gdt = grad_dtype;
  if (any_average) {
    const size_t total = out_buckets * (size_t)ev_size;
    const int sgrid = grid_for(total, kBlock, 8192);
#define HCTR_USCALE(T)                                                                          \
  hipLaunchKernelGGL((uniq_scale_grad_kernel<T>), dim3(sgrid), dim3(kBlock), 0, s, batch_per_gpu, \
                     num_lookup, ev_size, d_combiner, (const long long*)d_bucket_counts,        \
                     batch_major, (const T*)grad, w.scaled)
    if (grad_dtype == HCTR_EMB_F32) HCTR_USCALE(float);
    else if (grad_dtype == HCTR_EMB_F16) HCTR_USCALE(__half);
    else HCTR_USCALE(__hip_bfloat16);
#undef HCTR_USCALE
    HCTR_LAUNCH_CHECK();
    g = w.scaled;
    gdt = HCTR_EMB_F32;
  }
  hipLaunchKernelGGL(uniq_bwd_expand_kernel, dim3(grid_for(nbk, kBlock)), dim3(kBlock), 0, s, nbk,
                     batch_per_gpu, num_lookup, batch_major, (const long long*)recv_range, ridx,
                     (const long long*)r_off, d_block_source, d_block_lookup, w.grow, w.pos_bucket,
                     w.iota);
  HCTR_LAUNCH_CHECK();
  // stable: the positions of one row keep their ascending order, so its sum is reproducible
  HCTR_TRY(radix_sort_pairs_u32(w.sort_temp, w.sort_bytes, w.grow, w.rows_s, w.iota, w.pos_s,
                                positions, bit_length((uint64_t)n_rows), s));
  hipLaunchKernelGGL(uniq_bwd_buckets_kernel,
                     dim3(grid_for(positions > out_buckets ? positions : out_buckets + 1, kBlock, 4096)),
                     dim3(kBlock), 0, s, positions, out_buckets, w.pos_s, w.pos_bucket, w.bucket_s,
                     w.live);
  HCTR_LAUNCH_CHECK();
  return hctr_updater_reduce_presorted(u, positions, out_buckets, (const int64_t*)w.live, w.rows_s,
                                       w.bucket_s, g, gdt, n_rows, out_sum, stream);
}

}  // extern "C"
