// ebc_io.hip -- device side of Model.embedding_load / embedding_dump for embedding_collection
// tables (hugectr_amd/embedding_io.py holds the file format; included by ebc.hip).
//
// The reference's loader reads a table's whole key and weight file into host memory, filters the
// keys a GPU owns (key % num_shards == shard_id) with a host loop and hands the survivors to the
// table (EmbeddingParameterIO::load_embedding_weight, R/HugeCTR/embedding_storage/weight_io/
// parameter_IO.cpp:473-541; RaggedStaticEmbeddingTable::load_by_id / DynamicEmbeddingTable::
// load_by_id, dynamic_embedding.cu:432-472).  Here the files are streamed through two pinned,
// device-mapped host chunks (as hctr_tiered_* allocates its host table): Python fills one from the
// files while the kernels below read the other one STRAIGHT over the host link -- no staging copy,
// the filter runs where the rows land:
//   (a) io_check_kernel          keys only: owned / foreign / out-of-range counts
//   (b) io_import_static_kernel  owned key -> row row_start + key / num_shards of the flat shard
//                                table and of its optimizer state arrays; foreign keys write nothing
//   (c) io_select_*              stable compaction of the owned keys / rows into device buffers for
//                                the dynamic table's insert + scatter_update
// Export of a static shard is contiguous: plain asynchronous copies into the chunk, the keys an
// arithmetic sequence written by the host (no kernel where a copy does the job).
namespace hctr {
namespace {

constexpr int kIoBlock = 256;

// 0 = owned by (num_shards, shard_id), 1 = foreign, 2 = outside [0, vocab); *q = key / num_shards
template <typename K>
__device__ __forceinline__ int io_classify(K key, uint32_t ns, uint32_t sid, uint64_t vocab,
                                           uint64_t* q) {
  const uint64_t u = (uint64_t)key;  // (a negative int64 key becomes >= 2^63 >= vocab)
  if (u >= vocab) return 2;
  *q = u / ns;
  return (u % ns == sid) ? 0 : 1;
}

template <typename K>
__global__ void __launch_bounds__(kIoBlock)
    io_check_kernel(const K* __restrict__ keys, size_t n, uint32_t ns, uint32_t sid, uint64_t vocab,
                    unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long smem[kIoBlock / 64 + 1];
  unsigned long long own = 0, foreign = 0, bad = 0;
  for (size_t i = (size_t)blockIdx.x * kIoBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kIoBlock) {
    uint64_t q;
    const int c = io_classify(keys[i], ns, sid, vocab, &q);
    own += c == 0;
    foreign += c == 1;
    bad += c == 2;
  }
  own = block_reduce_sum<unsigned long long, kIoBlock>(own, smem);
  foreign = block_reduce_sum<unsigned long long, kIoBlock>(foreign, smem);
  bad = block_reduce_sum<unsigned long long, kIoBlock>(bad, smem);
  if (threadIdx.x == 0) {
    if (own) atomicAdd(&counts[0], own);
    if (foreign) atomicAdd(&counts[1], foreign);
    if (bad) atomicAdd(&counts[2], bad);
  }
}

// one row's W words (float4 when VEC: ev_size % 4 == 0, 16-byte accesses; else float) copied by
// the G lanes of its group, lane `sub` taking words sub, sub + G, ...
template <bool VEC>
__device__ __forceinline__ void io_copy_row(const float* __restrict__ src, float* __restrict__ dst,
                                            int W, int G, int sub) {
  if (VEC) {
    const float4* s = reinterpret_cast<const float4*>(src);
    float4* d = reinterpret_cast<float4*>(dst);
    for (int c = sub; c < W; c += G) d[c] = s[c];
  } else {
    for (int c = sub; c < W; c += G) dst[c] = src[c];
  }
}

// G (a power of two <= 64) lanes per row; rows, state0, state1: the chunk in pinned host memory
template <typename K, bool VEC>
__global__ void __launch_bounds__(kIoBlock)
    io_import_static_kernel(const K* __restrict__ keys, const float* __restrict__ rows,
                            const float* __restrict__ s0, const float* __restrict__ s1, size_t n,
                            int D, int G, uint32_t ns, uint32_t sid, uint64_t vocab,
                            uint64_t row_start, float* __restrict__ table, float* __restrict__ d0,
                            float* __restrict__ d1) {
  const size_t tid = (size_t)blockIdx.x * kIoBlock + threadIdx.x;
  const int sub = (int)(tid & (size_t)(G - 1));
  const size_t stride = ((size_t)gridDim.x * kIoBlock) / (size_t)G;
  const int W = VEC ? D / 4 : D;
  for (size_t r = tid / (size_t)G; r < n; r += stride) {
    uint64_t q;
    if (io_classify(keys[r], ns, sid, vocab, &q) != 0) continue;  // foreign: nothing is written
    const size_t dst = (size_t)(row_start + q) * (size_t)D, src = r * (size_t)D;
    io_copy_row<VEC>(rows + src, table + dst, W, G, sub);
    if (d0) io_copy_row<VEC>(s0 + src, d0 + dst, W, G, sub);
    if (d1) io_copy_row<VEC>(s1 + src, d1 + dst, W, G, sub);
  }
}

// dst[row_index[i]][:] = src[i][:] for row_index[i] < row_bound (state rows of a dynamic table)
template <bool VEC>
__global__ void __launch_bounds__(kIoBlock)
    io_scatter_rows_kernel(const uint64_t* __restrict__ row_index, const float* __restrict__ src,
                           size_t n, int D, int G, uint64_t row_bound, float* __restrict__ dst) {
  const size_t tid = (size_t)blockIdx.x * kIoBlock + threadIdx.x;
  const int sub = (int)(tid & (size_t)(G - 1));
  const size_t stride = ((size_t)gridDim.x * kIoBlock) / (size_t)G;
  const int W = VEC ? D / 4 : D;
  for (size_t r = tid / (size_t)G; r < n; r += stride) {
    const uint64_t row = row_index[r];
    if (row >= row_bound) continue;
    io_copy_row<VEC>(src + r * (size_t)D, dst + (size_t)row * (size_t)D, W, G, sub);
  }
}

// stable compaction, tile = kIoBlock consecutive keys: owned keys per tile ...
template <typename K>
__global__ void __launch_bounds__(kIoBlock)
    io_select_count_kernel(const K* __restrict__ keys, size_t n, size_t n_tiles, uint32_t ns,
                           uint32_t sid, uint64_t vocab, unsigned long long* __restrict__ tile_cnt) {
  __shared__ unsigned long long smem[kIoBlock / 64 + 1];
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const size_t i = tile * kIoBlock + threadIdx.x;
    uint64_t q;
    const unsigned long long own = (i < n && io_classify(keys[i], ns, sid, vocab, &q) == 0) ? 1 : 0;
    const unsigned long long tot = block_reduce_sum<unsigned long long, kIoBlock>(own, smem);
    if (threadIdx.x == 0) tile_cnt[tile] = tot;
  }
}

// ... and, behind the exclusive scan of those counts, every tile's owned keys in their order at
// tile_off[tile]; their rows (and state rows) are then copied by the whole workgroup
template <typename K, bool VEC>
__global__ void __launch_bounds__(kIoBlock)
    io_select_scatter_kernel(const K* __restrict__ keys, const float* __restrict__ rows,
                             const float* __restrict__ s0, const float* __restrict__ s1, size_t n,
                             size_t n_tiles, int D, uint32_t ns, uint32_t sid, uint64_t vocab,
                             const unsigned long long* __restrict__ tile_off,
                             long long* __restrict__ out_keys, float* __restrict__ out_rows,
                             float* __restrict__ o0, float* __restrict__ o1) {
  __shared__ unsigned long long smem[kIoBlock / 64 + 1];
  __shared__ uint32_t s_src[kIoBlock];
  const size_t W = VEC ? (size_t)D / 4 : (size_t)D;
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const size_t i = tile * kIoBlock + threadIdx.x;
    uint64_t q;
    const bool own = i < n && io_classify(keys[i], ns, sid, vocab, &q) == 0;
    unsigned long long tot;
    const unsigned long long pos =
        block_exclusive_scan<unsigned long long, kIoBlock>(own ? 1ull : 0ull, smem, &tot);
    const size_t base = (size_t)tile_off[tile];
    if (own) {
      s_src[pos] = threadIdx.x;
      out_keys[base + pos] = (long long)keys[i];
    }
    __syncthreads();
    for (size_t e = threadIdx.x; e < (size_t)tot * W; e += kIoBlock) {
      const size_t j = e / W, c = e - j * W;
      const size_t src = (tile * kIoBlock + s_src[j]) * W + c, dst = (base + j) * W + c;
      if (VEC) {
        reinterpret_cast<float4*>(out_rows)[dst] = reinterpret_cast<const float4*>(rows)[src];
        if (o0) reinterpret_cast<float4*>(o0)[dst] = reinterpret_cast<const float4*>(s0)[src];
        if (o1) reinterpret_cast<float4*>(o1)[dst] = reinterpret_cast<const float4*>(s1)[src];
      } else {
        out_rows[dst] = rows[src];
        if (o0) o0[dst] = s0[src];
        if (o1) o1[dst] = s1[src];
      }
    }
    __syncthreads();
  }
}

static inline int io_lanes_per_row(int words) {
  int g = 1;
  while (g < words && g < 64) g *= 2;
  return g;
}

static inline size_t io_align(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace
}  // namespace hctr

struct hctr_ebc_io {
  size_t R = 0;  // rows per chunk
  int D = 0, key_type = 0;
  size_t off_rows = 0, off_s0 = 0, off_s1 = 0, bytes = 0;
  char* host[2] = {nullptr, nullptr};  // pinned, device-mapped
  char* dev[2] = {nullptr, nullptr};   // the same memory as the device addresses it
  hipEvent_t ev[2] = {nullptr, nullptr};  // the device work issued on a chunk so far
  unsigned long long *tile_cnt = nullptr, *tile_off = nullptr, *tile_sums = nullptr,
                     *d_total = nullptr, *h_word = nullptr;
  size_t key_bytes() const { return key_type == HCTR_KEY_I64 ? 8 : 4; }
};

extern "C" {

int hctr_ebc_io_destroy(hctr_ebc_io* io) {
  if (!io) return HCTR_OK;
  (void)hipDeviceSynchronize();
  for (int w = 0; w < 2; w++) {
    if (io->ev[w]) (void)hipEventDestroy(io->ev[w]);
    if (io->host[w]) (void)hipHostFree(io->host[w]);
  }
  for (void* q : {(void*)io->tile_cnt, (void*)io->tile_off, (void*)io->tile_sums, (void*)io->d_total})
    if (q) (void)hipFree(q);
  if (io->h_word) (void)hipHostFree(io->h_word);
  delete io;
  return HCTR_OK;
}

int hctr_ebc_io_create(size_t chunk_rows, int ev_size, int key_type, hctr_ebc_io** out) {
  using namespace hctr;
  HCTR_REQUIRE(out, "null pointer");
  HCTR_REQUIRE(chunk_rows > 0 && chunk_rows < ((size_t)1 << 31), "chunk_rows");
  HCTR_REQUIRE(ev_size > 0 && ev_size <= 16384, "ev_size");
  HCTR_REQUIRE(key_type == HCTR_KEY_U32 || key_type == HCTR_KEY_I64, "key_type");
  hctr_ebc_io* io = new hctr_ebc_io();
  io->R = chunk_rows;
  io->D = ev_size;
  io->key_type = key_type;
  const size_t row_bytes = io_align(chunk_rows * (size_t)ev_size * sizeof(float));
  io->off_rows = io_align(chunk_rows * 8);
  io->off_s0 = io->off_rows + row_bytes;
  io->off_s1 = io->off_s0 + row_bytes;
  io->bytes = io->off_s1 + row_bytes;
  const size_t n_tiles = ceil_div<size_t>(chunk_rows, (size_t)kIoBlock);
  bool ok = true;
  for (int w = 0; ok && w < 2; w++) {
    ok = hipHostMalloc((void**)&io->host[w], io->bytes,
                       hipHostMallocMapped | hipHostMallocPortable) == hipSuccess &&
         hipHostGetDevicePointer((void**)&io->dev[w], io->host[w], 0) == hipSuccess &&
         hipEventCreateWithFlags(&io->ev[w], hipEventDisableTiming) == hipSuccess;
  }
  if (ok) ok = hipMalloc(&io->tile_cnt, n_tiles * 8) == hipSuccess &&
               hipMalloc(&io->tile_off, (n_tiles + 1) * 8) == hipSuccess &&
               hipMalloc(&io->tile_sums, (ceil_div<size_t>(n_tiles, 1024) + 1) * 8) == hipSuccess &&
               hipMalloc(&io->d_total, 8) == hipSuccess &&
               hipHostMalloc((void**)&io->h_word, 8, hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    set_error("hctr_ebc_io_create: host / device allocation failed");
    (void)hipGetLastError();
    hctr_ebc_io_destroy(io);
    return HCTR_ERR_HIP;
  }
  *out = io;
  return HCTR_OK;
}

int hctr_ebc_io_chunk(hctr_ebc_io* io, int which, void** keys, float** rows, float** state0,
                      float** state1) {
  HCTR_REQUIRE(io, "null handle");
  HCTR_REQUIRE(which == 0 || which == 1, "which");
  if (keys) *keys = io->host[which];
  if (rows) *rows = (float*)(io->host[which] + io->off_rows);
  if (state0) *state0 = (float*)(io->host[which] + io->off_s0);
  if (state1) *state1 = (float*)(io->host[which] + io->off_s1);
  return HCTR_OK;
}

int hctr_ebc_io_wait(hctr_ebc_io* io, int which) {
  HCTR_REQUIRE(io, "null handle");
  HCTR_REQUIRE(which == 0 || which == 1, "which");
  HCTR_HIP(hipEventSynchronize(io->ev[which]));
  return HCTR_OK;
}

#define HCTR_IO_ARGS(io, which, n, num_shards, shard_id)                                  \
  HCTR_REQUIRE(io, "null handle");                                                        \
  HCTR_REQUIRE(which == 0 || which == 1, "which");                                        \
  HCTR_REQUIRE(n <= io->R, "more keys than the chunk holds");                             \
  HCTR_REQUIRE(num_shards > 0 && shard_id >= 0 && shard_id < num_shards, "num_shards / shard_id")

int hctr_ebc_io_check(hctr_ebc_io* io, int which, size_t n, int num_shards, int shard_id,
                      uint64_t vocab, uint64_t* d_counts, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_IO_ARGS(io, which, n, num_shards, shard_id);
  HCTR_REQUIRE(d_counts, "null pointer");
  if (n == 0) return HCTR_OK;
  hipStream_t s = as_stream(stream);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(d_counts);
  const int grid = grid_for(n, kIoBlock);
  if (io->key_type == HCTR_KEY_I64)
    hipLaunchKernelGGL(io_check_kernel<long long>, dim3(grid), dim3(kIoBlock), 0, s,
                       (const long long*)io->dev[which], n, (uint32_t)num_shards,
                       (uint32_t)shard_id, vocab, c);
  else
    hipLaunchKernelGGL(io_check_kernel<uint32_t>, dim3(grid), dim3(kIoBlock), 0, s,
                       (const uint32_t*)io->dev[which], n, (uint32_t)num_shards, (uint32_t)shard_id,
                       vocab, c);
  HCTR_LAUNCH_CHECK();
  HCTR_HIP(hipEventRecord(io->ev[which], s));
  return HCTR_OK;
}

int hctr_ebc_io_import_static(hctr_ebc_io* io, int which, size_t n, int num_shards, int shard_id,
                              uint64_t vocab, uint64_t row_start, float* table, float* state0,
                              float* state1, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_IO_ARGS(io, which, n, num_shards, shard_id);
  HCTR_REQUIRE(table, "null pointer");
  HCTR_REQUIRE(state0 || !state1, "state1 without state0");
  if (n == 0) return HCTR_OK;
  hipStream_t s = as_stream(stream);
  const int D = io->D;
  const bool vec = D % 4 == 0;
  const int G = io_lanes_per_row(vec ? D / 4 : D);
  const int grid = grid_for(n * (size_t)G, kIoBlock);
  const char* b = io->dev[which];
  const float* rows = (const float*)(b + io->off_rows);
  const float* s0 = (const float*)(b + io->off_s0);
  const float* s1 = (const float*)(b + io->off_s1);
#define HCTR_IO_IMPORT(K, VEC)                                                                   \
  hipLaunchKernelGGL((io_import_static_kernel<K, VEC>), dim3(grid), dim3(kIoBlock), 0, s,        \
                     (const K*)b, rows, s0, s1, n, D, G, (uint32_t)num_shards, (uint32_t)shard_id, \
                     vocab, row_start, table, state0, state1)
  if (io->key_type == HCTR_KEY_I64) {
    if (vec) {
      HCTR_IO_IMPORT(long long, true);
    } else {
      HCTR_IO_IMPORT(long long, false);
    }
  } else {
    if (vec) {
      HCTR_IO_IMPORT(uint32_t, true);
    } else {
      HCTR_IO_IMPORT(uint32_t, false);
    }
  }
#undef HCTR_IO_IMPORT
  HCTR_LAUNCH_CHECK();
  HCTR_HIP(hipEventRecord(io->ev[which], s));
  return HCTR_OK;
}

int hctr_ebc_io_select(hctr_ebc_io* io, int which, size_t n, int num_shards, int shard_id,
                       uint64_t vocab, int64_t* out_keys, float* out_rows, float* out_state0,
                       float* out_state1, size_t* selected, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_IO_ARGS(io, which, n, num_shards, shard_id);
  HCTR_REQUIRE(out_keys && out_rows && selected, "null pointer");
  HCTR_REQUIRE(out_state0 || !out_state1, "state1 without state0");
  *selected = 0;
  if (n == 0) return HCTR_OK;
  hipStream_t s = as_stream(stream);
  const int D = io->D;
  const bool vec = D % 4 == 0;
  const size_t n_tiles = ceil_div<size_t>(n, (size_t)kIoBlock);
  const int grid = (int)(n_tiles < (size_t)kMaxGrid ? n_tiles : (size_t)kMaxGrid);
  const char* b = io->dev[which];
  const float* rows = (const float*)(b + io->off_rows);
  const float* s0 = (const float*)(b + io->off_s0);
  const float* s1 = (const float*)(b + io->off_s1);
  const uint32_t ns = (uint32_t)num_shards, sid = (uint32_t)shard_id;
  if (io->key_type == HCTR_KEY_I64)
    hipLaunchKernelGGL(io_select_count_kernel<long long>, dim3(grid), dim3(kIoBlock), 0, s,
                       (const long long*)b, n, n_tiles, ns, sid, vocab, io->tile_cnt);
  else
    hipLaunchKernelGGL(io_select_count_kernel<uint32_t>, dim3(grid), dim3(kIoBlock), 0, s,
                       (const uint32_t*)b, n, n_tiles, ns, sid, vocab, io->tile_cnt);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(exclusive_scan_to_offsets<unsigned long long>(io->tile_cnt, n_tiles, io->tile_sums,
                                                         io->d_total, io->tile_off, s));
#define HCTR_IO_SELECT(K, VEC)                                                                    \
  hipLaunchKernelGGL((io_select_scatter_kernel<K, VEC>), dim3(grid), dim3(kIoBlock), 0, s,        \
                     (const K*)b, rows, s0, s1, n, n_tiles, D, ns, sid, vocab, io->tile_off,       \
                     (long long*)out_keys, out_rows, out_state0, out_state1)
  if (io->key_type == HCTR_KEY_I64) {
    if (vec) {
      HCTR_IO_SELECT(long long, true);
    } else {
      HCTR_IO_SELECT(long long, false);
    }
  } else {
    if (vec) {
      HCTR_IO_SELECT(uint32_t, true);
    } else {
      HCTR_IO_SELECT(uint32_t, false);
    }
  }
#undef HCTR_IO_SELECT
  HCTR_LAUNCH_CHECK();
  HCTR_HIP(hipEventRecord(io->ev[which], s));
  HCTR_HIP(hipMemcpyAsync(io->h_word, io->d_total, 8, hipMemcpyDeviceToHost, s));
  HCTR_HIP(hipStreamSynchronize(s));
  *selected = (size_t)*io->h_word;
  return HCTR_OK;
}

int hctr_ebc_io_scatter_rows(size_t n, int ev_size, const uint64_t* row_index, const float* src,
                             float* dst, uint64_t row_bound, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(ev_size > 0, "ev_size");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(row_index && src && dst, "null pointer");
  const bool vec = ev_size % 4 == 0;
  const int G = io_lanes_per_row(vec ? ev_size / 4 : ev_size);
  const int grid = grid_for(n * (size_t)G, kIoBlock);
  if (vec)
    hipLaunchKernelGGL(io_scatter_rows_kernel<true>, dim3(grid), dim3(kIoBlock), 0,
                       as_stream(stream), row_index, src, n, ev_size, G, row_bound, dst);
  else
    hipLaunchKernelGGL(io_scatter_rows_kernel<false>, dim3(grid), dim3(kIoBlock), 0,
                       as_stream(stream), row_index, src, n, ev_size, G, row_bound, dst);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_ebc_io_export_static(hctr_ebc_io* io, int which, size_t n, uint64_t first_key,
                              uint64_t key_step, const float* table_rows, const float* state0,
                              const float* state1, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(io, "null handle");
  HCTR_REQUIRE(which == 0 || which == 1, "which");
  HCTR_REQUIRE(n <= io->R, "more rows than the chunk holds");
  if (n == 0) return HCTR_OK;
  HCTR_REQUIRE(table_rows, "null pointer");
  HCTR_REQUIRE(io->key_type == HCTR_KEY_I64 || first_key + (n - 1) * key_step <= 0xFFFFFFFFull,
               "keys beyond uint32");
  hipStream_t s = as_stream(stream);
  const size_t bytes = n * (size_t)io->D * sizeof(float);
  char* h = io->host[which];
  HCTR_HIP(hipMemcpyAsync(h + io->off_rows, table_rows, bytes, hipMemcpyDeviceToHost, s));
  if (state0) HCTR_HIP(hipMemcpyAsync(h + io->off_s0, state0, bytes, hipMemcpyDeviceToHost, s));
  if (state1) HCTR_HIP(hipMemcpyAsync(h + io->off_s1, state1, bytes, hipMemcpyDeviceToHost, s));
  HCTR_HIP(hipEventRecord(io->ev[which], s));
  // (the keys while the copies run; the caller waits on the chunk before it reads either)
  if (io->key_type == HCTR_KEY_I64) {
    long long* k = (long long*)h;
    for (size_t j = 0; j < n; j++) k[j] = (long long)(first_key + j * key_step);
  } else {
    uint32_t* k = (uint32_t*)h;
    for (size_t j = 0; j < n; j++) k[j] = (uint32_t)(first_key + j * key_step);
  }
  return HCTR_OK;
}

#undef HCTR_IO_ARGS

}  // extern "C"
