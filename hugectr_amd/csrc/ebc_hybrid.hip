// ebc_hybrid.hip -- embedding_collection on hybrid tables (storage="hybrid": one bounded LRU table,
// hctr_lru_*, per local table shard; included by ebc.hip).
//
// The routed keys of a step lie in [peer][local lookup][b_local] bucket order, one (peer, lookup)
// SEGMENT after the other, and several lookups may share a table.  A hybrid table counts its LRU
// time in inserting calls, so a table's keys of one step must reach it in ONE call: the three
// kernels below move between the routed order and the order grouped by table,
// [table][peer][lookup], without a host loop over world x lookups slices:
//   (a) ebc_group_segments_kernel   routed keys -> grouped keys
//   (b) ebc_hybrid_row_ptrs_kernel  grouped row numbers -> per-key row address in ROUTED order (what
//                                   hctr_forward_pool_ptrs reads) + the routed -> grouped positions
//   (c) ebc_hybrid_key_grads_kernel gradient of every bucket -> one fp32 row per key in GROUPED
//                                   order (what hctr_lru_apply_update reads), any gradient dtype,
//                                   the batch-major read address of the one-GPU output included
// A segment is described by its first key (the routed bucket offsets, every seg_stride-th entry)
// and by seg_dst, its first position in the grouped order, which the host computes from the
// offsets it reads once per step anyway.  One lane per key; the key's segment is found by binary
// search (a few thousand segments at most: a dozen probes of an L2-resident array).  Plain vector
// stores, every position written once: no atomics.
namespace hctr {
namespace {

constexpr int kHybBlock = 256;

// the segment of routed position i: the LAST one that starts at or before i (empty segments share
// their start with the next one)
__device__ __forceinline__ size_t hyb_segment_of(const long long* __restrict__ seg_offsets,
                                                 size_t n_seg, size_t stride, long long i) {
  size_t lo = 0, hi = n_seg;  // first segment in (lo, hi] ... that starts after i
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (seg_offsets[mid * stride] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kHybBlock)
    ebc_group_segments_kernel(size_t n_seg, size_t stride, const long long* __restrict__ seg_offsets,
                              const long long* __restrict__ seg_dst,
                              const long long* __restrict__ keys, size_t nnz,
                              long long* __restrict__ out_keys) {
  for (size_t i = (size_t)blockIdx.x * kHybBlock + threadIdx.x; i < nnz;
       i += (size_t)gridDim.x * kHybBlock) {
    const size_t s = hyb_segment_of(seg_offsets, n_seg, stride, (long long)i);
    const unsigned long long g =
        (unsigned long long)(seg_dst[s] + ((long long)i - seg_offsets[s * stride]));
    if (g < nnz) out_keys[g] = keys[i];  // (a descriptor that points outside writes nothing)
  }
}

__global__ void __launch_bounds__(kHybBlock)
    ebc_hybrid_row_ptrs_kernel(size_t n_seg, size_t stride, const long long* __restrict__ seg_offsets,
                               const long long* __restrict__ seg_dst,
                               const int* __restrict__ seg_table, int n_tables,
                               const unsigned long long* __restrict__ table_desc, int ev_size,
                               const unsigned long long* __restrict__ rows, size_t nnz,
                               const float** __restrict__ out_ptrs, uint32_t* __restrict__ out_perm) {
  for (size_t i = (size_t)blockIdx.x * kHybBlock + threadIdx.x; i < nnz;
       i += (size_t)gridDim.x * kHybBlock) {
    const size_t s = hyb_segment_of(seg_offsets, n_seg, stride, (long long)i);
    const unsigned long long g =
        (unsigned long long)(seg_dst[s] + ((long long)i - seg_offsets[s * stride]));
    const int t = seg_table[s];
    const float* p = nullptr;
    uint32_t pos = 0xFFFFFFFFu;
    if (g < nnz) {
      pos = (uint32_t)g;
      if (t >= 0 && t < n_tables) {
        const unsigned long long r = rows[g];
        const float* base = reinterpret_cast<const float*>(table_desc[2 * t]);
        if (base && r < table_desc[2 * t + 1]) p = base + (size_t)r * (size_t)ev_size;
      }
    }
    out_ptrs[i] = p;
    out_perm[i] = pos;
  }
}

template <typename T>
__device__ __forceinline__ float4 ld4_row(const T* p) { return ld4_as_f32<T>(p); }
template <>
__device__ __forceinline__ float4 ld4_row<float>(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}

// G (a power of two <= 64) lanes per bucket: the bucket's gradient row is copied, as fp32, to the
// grouped position of each of its keys.  VEC (ev_size % 4 == 0, rows 16-byte aligned): four
// elements per lane and access, D counts float4 words
template <typename T, bool VEC>
__global__ void __launch_bounds__(kHybBlock)
    ebc_hybrid_key_grads_kernel(size_t buckets, int D, int G,
                                const long long* __restrict__ bucket_range,
                                const uint32_t* __restrict__ perm, size_t nnz,
                                const T* __restrict__ grad, size_t samples, size_t lookups,
                                float* __restrict__ key_grads) {
  const size_t tid = (size_t)blockIdx.x * kHybBlock + threadIdx.x;
  const int sub = (int)(tid & (size_t)(G - 1));
  const size_t step = ((size_t)gridDim.x * kHybBlock) / (size_t)G;
  const size_t row = VEC ? (size_t)D * 4 : (size_t)D;  // elements per row
  for (size_t u = tid / (size_t)G; u < buckets; u += step) {
    // bucket u = lookup * samples + sample lies in gradient row sample * lookups + lookup of the
    // batch-major output (hctr_forward_pool_mapped's store address)
    const size_t gu = samples ? (u % samples) * lookups + u / samples : u;
    const T* src = grad + gu * row;
    const long long b = bucket_range[u], e = bucket_range[u + 1];
    for (long long j = b; j < e; ++j) {
      if ((unsigned long long)j >= nnz) break;
      const uint32_t p = perm[j];
      if (p >= nnz) continue;
      float* dst = key_grads + (size_t)p * row;
      if (VEC) {
        for (int c = sub; c < D; c += G)
          reinterpret_cast<float4*>(dst)[c] = ld4_row<T>(src + 4 * c);
      } else {
        for (int c = sub; c < D; c += G) dst[c] = ld_as_f32<T>(src + c);
      }
    }
  }
}

inline int hyb_lanes_per_row(int D) {
  int g = 1;
  while (g < 64 && g < D) g <<= 1;
  return g;
}

}  // namespace
}  // namespace hctr

extern "C" {

int hctr_ebc_group_segments(size_t n_seg, size_t seg_stride, const int64_t* seg_offsets,
                            const int64_t* seg_dst, const int64_t* keys, size_t nnz,
                            int64_t* out_keys, hctr_stream_t stream) {
  HCTR_REQUIRE(nnz < 0xFFFFFFF0ull, "nnz must be below 2^32");
  if (nnz == 0) return HCTR_OK;
  HCTR_REQUIRE(n_seg >= 1 && seg_stride >= 1, "keys without a segment");
  HCTR_REQUIRE(seg_offsets && seg_dst && keys && out_keys, "null pointer");
  HCTR_REQUIRE(keys != out_keys, "the grouping is not done in place");
  hipLaunchKernelGGL(ebc_group_segments_kernel, dim3(grid_for(nnz, kHybBlock)), dim3(kHybBlock), 0,
                     as_stream(stream), n_seg, seg_stride, (const long long*)seg_offsets,
                     (const long long*)seg_dst, (const long long*)keys, nnz, (long long*)out_keys);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_ebc_hybrid_row_ptrs(size_t n_seg, size_t seg_stride, const int64_t* seg_offsets,
                             const int64_t* seg_dst, const int32_t* seg_table, int n_tables,
                             const uint64_t* table_desc, int ev_size, const uint64_t* rows,
                             size_t nnz, const float** out_ptrs, uint32_t* out_perm,
                             hctr_stream_t stream) {
  HCTR_REQUIRE(nnz < 0xFFFFFFF0ull, "nnz must be below 2^32");
  HCTR_REQUIRE(ev_size >= 1 && n_tables >= 0, "ev_size / n_tables");
  if (nnz == 0) return HCTR_OK;
  HCTR_REQUIRE(n_seg >= 1 && seg_stride >= 1 && n_tables >= 1, "keys without a segment or a table");
  HCTR_REQUIRE(seg_offsets && seg_dst && seg_table && table_desc && rows && out_ptrs && out_perm,
               "null pointer");
  hipLaunchKernelGGL(ebc_hybrid_row_ptrs_kernel, dim3(grid_for(nnz, kHybBlock)), dim3(kHybBlock), 0,
                     as_stream(stream), n_seg, seg_stride, (const long long*)seg_offsets,
                     (const long long*)seg_dst, (const int*)seg_table, n_tables,
                     (const unsigned long long*)table_desc, ev_size,
                     (const unsigned long long*)rows, nnz, out_ptrs, out_perm);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_ebc_hybrid_key_grads(size_t buckets, int ev_size, const int64_t* bucket_range,
                              const uint32_t* perm, size_t nnz, const void* grad, int grad_dtype,
                              size_t samples, size_t lookups, float* key_grads,
                              hctr_stream_t stream) {
  HCTR_REQUIRE(nnz < 0xFFFFFFF0ull, "nnz must be below 2^32");
  HCTR_REQUIRE(ev_size >= 1, "ev_size");
  HCTR_REQUIRE((samples == 0 && lookups == 0) || samples * lookups == buckets,
               "gradient map: samples * lookups must equal the bucket count");
  HCTR_REQUIRE(grad_dtype == HCTR_EMB_F32 || grad_dtype == HCTR_EMB_F16 ||
                   grad_dtype == HCTR_EMB_BF16, "grad_dtype");
  if (nnz == 0 || buckets == 0) return HCTR_OK;
  HCTR_REQUIRE(bucket_range && perm && grad && key_grads, "null pointer");
  hipStream_t s = as_stream(stream);
  const long long* br = (const long long*)bucket_range;
  // four elements per access when the rows allow it (fp32: 16-byte, 16-bit: 8-byte source rows)
  const size_t src_align = grad_dtype == HCTR_EMB_F32 ? 16 : 8;
  const bool vec = ev_size % 4 == 0 && (uintptr_t)grad % src_align == 0 &&
                   (uintptr_t)key_grads % 16 == 0;
  const int W = vec ? ev_size / 4 : ev_size;
  const int G = hyb_lanes_per_row(W);
  const dim3 grid(grid_for(buckets * (size_t)G, kHybBlock)), block(kHybBlock);
#define HCTR_HYB_KG(T, VEC)                                                                       \
  hipLaunchKernelGGL((ebc_hybrid_key_grads_kernel<T, VEC>), grid, block, 0, s, buckets, W, G, br, \
                     perm, nnz, (const T*)grad, samples, lookups, key_grads)
  if (grad_dtype == HCTR_EMB_F32) {
    if (vec) HCTR_HYB_KG(float, true); else HCTR_HYB_KG(float, false);
  } else if (grad_dtype == HCTR_EMB_F16) {
    if (vec) HCTR_HYB_KG(__half, true); else HCTR_HYB_KG(__half, false);
  } else {
    if (vec) HCTR_HYB_KG(__hip_bfloat16, true); else HCTR_HYB_KG(__hip_bfloat16, false);
  }
#undef HCTR_HYB_KG
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

}  // extern "C"
