// metrics.hip -- evaluation metrics on the device (gfx950, wave64): AUC, NDCG, HitRate, SMAPE.
//
// The reference keeps them in R/HugeCTR/src/metrics.cu (AUC: a histogram-partitioned multi-GPU sort
// and a trapezoid sum in fp32; HitRate / SMAPE: one kernel with atomics per batch; NDCG: two library
// sorts).  Here one launch per evaluation batch files the scores away and updates the counters, and
// the finalise is our own radix sort plus one tie-aware pass in INTEGERS:
//
//   hctr_metric_accumulate   pred [n, C] (fp32 / fp16 / bf16), label [n, C] fp32 ->
//                            class-major store keys u32 [C][cap], labels f32 [C][cap] at `offset`,
//                            + counter block (labels that are not 0 / 1 per class, HitRate's
//                            checked / hits, SMAPE's sum and count)
//   hctr_metric_auc          one class: stable sort of (key, label bits), then 2U, P, N as u64
//   hctr_metric_ndcg         one class: DCG and ideal DCG as fp64
//
// The key of a score is the order-preserving u32 image of its exact fp32 value (sign bit flipped for
// non-negatives, all bits for negatives, -0.0 as +0.0, every NaN 0xFFFFFFFF): equal scores are equal
// keys, so a run of equal keys IS a tie group of the ROC curve.
//   2U = sum over runs of equal key: pos_run * (2 * neg_below_run + neg_run)
// is the Mann-Whitney statistic with ties counted one half (the reference's trapezoid rule) times
// two; AUC = 2U / (2 P N) is left to the host in fp64.  Integer words: no summation order, the same
// bits on every call.  There is no floating-point atomic in this unit; fp64 sums (SMAPE, DCG) are
// per-workgroup partials reduced in a fixed order.
// Compiled as part of radix_sort.hip's unit (included at its end, like hybrid_table.hip in det.hip):
// the finalise is that sort plus one pass.
#include "block_prims.h"
#include "common.h"
#include "cvt16.h"
#include "radix_sort.h"
#include "scan.h"

namespace hctr {
namespace {

constexpr int kMtBlock = 256;
constexpr int kMtPer = 8;                     // consecutive elements per thread (finalise)
constexpr int kMtTile = kMtBlock * kMtPer;    // 2048
constexpr int kMtAccGrid = 1024;              // accumulate: at most this many workgroups / partials
constexpr uint32_t kOneBits = 0x3F800000u;    // 1.0f
// counter block (u64 words)
constexpr int kCtChecked = 0, kCtHits = 1, kCtSmapeCnt = 2, kCtSmapeSum = 3, kCtTicket = 4,
              kCtBad = 8;

__device__ __forceinline__ uint32_t order_key(float f) {
  uint32_t b = __float_as_uint(f);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;  // NaN: all tie, all last
  if (b == 0x80000000u) b = 0u;                             // -0.0 == +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ double u64_as_double(unsigned long long u) {
  double d;
  memcpy(&d, &u, sizeof(d));
  return d;
}
__device__ __forceinline__ unsigned long long double_as_u64(double d) {
  unsigned long long u;
  memcpy(&u, &d, sizeof(u));
  return u;
}

// one evaluation batch: element e = row * C + c of pred / label -> store slot [c][offset + row]
template <typename T>
__global__ void __launch_bounds__(kMtBlock)
    metric_accumulate_kernel(const T* __restrict__ pred, const float* __restrict__ label, size_t n,
                             int C, uint32_t* __restrict__ keys, float* __restrict__ labels,
                             size_t cap, size_t offset, unsigned long long* __restrict__ counters,
                             double* __restrict__ partials) {
  __shared__ uint32_t bad[HCTR_METRIC_MAX_CLASSES];
  __shared__ unsigned long long red_u[kMtBlock / 64];
  __shared__ double red_d[kMtBlock / 64];
  __shared__ int is_last;
  for (int c = threadIdx.x; c < C; c += kMtBlock) bad[c] = 0u;
  __syncthreads();
  const size_t total = n * (size_t)C;
  unsigned long long checked = 0ull, hits = 0ull;
  double err = 0.0;
  for (size_t e = (size_t)blockIdx.x * kMtBlock + threadIdx.x; e < total;
       e += (size_t)gridDim.x * kMtBlock) {
    const size_t row = e / (size_t)C;
    const int c = (int)(e - row * (size_t)C);
    const float p = ld_as_f32<T>(pred + e);
    const float l = label[e];
    const size_t slot = (size_t)c * cap + offset + row;
    keys[slot] = order_key(p);
    labels[slot] = l;
    if (l != 0.0f && l != 1.0f) atomicAdd(&bad[c], 1u);
    const double pd = (double)p, ld = (double)l;
    if (pd > 0.8) {  // (the promotion `preds[i] > 0.8` performs in the reference)
      checked++;
      if (l == 1.0f) hits++;
    }
    const double sum = pd + ld;
    if (sum != 0.0) err += fabs(pd - ld) / (sum / 2.0);
  }
  checked = block_reduce_sum<unsigned long long, kMtBlock>(checked, red_u);
  hits = block_reduce_sum<unsigned long long, kMtBlock>(hits, red_u);
  err = block_reduce_sum<double, kMtBlock>(err, red_d);
  for (int c = threadIdx.x; c < C; c += kMtBlock) {
    if (bad[c] != 0u) atomicAdd(&counters[kCtBad + c], (unsigned long long)bad[c]);
  }
  if (threadIdx.x == 0) {
    if (checked != 0ull) atomicAdd(&counters[kCtChecked], checked);
    if (hits != 0ull) atomicAdd(&counters[kCtHits], hits);
    partials[blockIdx.x] = err;
    __threadfence();
    is_last = atomicAdd(&counters[kCtTicket], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0) return;
  // the last workgroup to arrive adds the partials up, always in workgroup order
  __threadfence();
  double s = 0.0;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += kMtBlock) {
    // (sums other workgroups parked: read past this CU's vector cache)
    s += u64_as_double(__hip_atomic_load(reinterpret_cast<unsigned long long*>(partials) + b,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  s = block_reduce_sum<double, kMtBlock>(s, red_d);
  if (threadIdx.x == 0) {
    counters[kCtSmapeSum] = double_as_u64(u64_as_double(counters[kCtSmapeSum]) + s);
    counters[kCtSmapeCnt] += (unsigned long long)total;
    counters[kCtTicket] = 0ull;  // clean for the next batch
  }
}

// ---- AUC ---------------------------------------------------------------------------------------------
// negatives (label != 1.0) per tile of the sorted list
__global__ void __launch_bounds__(kMtBlock)
    metric_auc_count_kernel(const uint32_t* __restrict__ lab, size_t n,
                            unsigned long long* __restrict__ tile_neg,
                            unsigned long long* __restrict__ out) {
  __shared__ uint32_t red[kMtBlock / 64];
  const size_t base = (size_t)blockIdx.x * kMtTile;
  uint32_t c = 0u;
#pragma unroll
  for (int k = 0; k < kMtPer; k++) {
    const size_t i = base + (size_t)k * kMtBlock + threadIdx.x;
    if (i < n && lab[i] != kOneBits) c++;
  }
  c = block_reduce_sum<uint32_t, kMtBlock>(c, red);
  if (threadIdx.x == 0) {
    tile_neg[blockIdx.x] = c;
    if (blockIdx.x == 0) out[0] = 0ull;
  }
}

// negatives in [0, x) of the sorted list: the tile prefix + a count inside x's tile (whole workgroup)
__device__ __forceinline__ unsigned long long neg_below(
    size_t x, size_t n, const uint32_t* __restrict__ lab,
    const unsigned long long* __restrict__ tile_base, unsigned long long all_neg, uint32_t* red) {
  if (x >= n) return all_neg;  // (uniform: x is the same in every thread)
  const size_t t = x / kMtTile, first = t * kMtTile;
  uint32_t c = 0u;
  for (size_t i = first + threadIdx.x; i < x; i += kMtBlock) c += lab[i] != kOneBits ? 1u : 0u;
  c = block_reduce_sum<uint32_t, kMtBlock>(c, red);
  return tile_base[t] + c;
}

// every positive adds neg_below(start of its run) + neg_below(end of its run).  A run that crosses
// a tile edge can only be the run of the tile's first or last key: those two ends are found by a
// binary search in the whole list, everything else inside the tile's LDS copy.
__global__ void __launch_bounds__(kMtBlock)
    metric_auc_run_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ lab,
                          size_t n, const unsigned long long* __restrict__ tile_base,
                          const unsigned long long* __restrict__ d_all_neg,
                          unsigned long long* __restrict__ out) {
  __shared__ uint32_t sk[kMtTile];
  __shared__ uint32_t ln[kMtTile + 1];  // negative flags, then their exclusive prefix
  __shared__ uint32_t scan_smem[kMtBlock / 64 + 1];
  __shared__ uint32_t red[kMtBlock / 64];
  __shared__ unsigned long long red64[kMtBlock / 64];
  __shared__ size_t edge[2];
  const size_t base = (size_t)blockIdx.x * kMtTile;
  const int tile_n = (int)(n - base < (size_t)kMtTile ? n - base : (size_t)kMtTile);
  const unsigned long long all_neg = *d_all_neg;
#pragma unroll
  for (int k = 0; k < kMtPer; k++) {
    const int j = k * kMtBlock + threadIdx.x;
    const bool valid = j < tile_n;
    sk[j] = valid ? key[base + j] : 0xFFFFFFFFu;
    ln[j] = (valid && lab[base + j] != kOneBits) ? 1u : 0u;
  }
  __syncthreads();
  uint32_t flag[kMtPer], mine = 0u;
#pragma unroll
  for (int q = 0; q < kMtPer; q++) {
    flag[q] = ln[threadIdx.x * kMtPer + q];
    mine += flag[q];
  }
  uint32_t tile_negs;
  uint32_t run = block_exclusive_scan<uint32_t, kMtBlock>(mine, scan_smem, &tile_negs);
#pragma unroll
  for (int q = 0; q < kMtPer; q++) {
    ln[threadIdx.x * kMtPer + q] = run;
    run += flag[q];
  }
  if (threadIdx.x == 0) {
    ln[kMtTile] = tile_negs;
    // the ends of the runs that may cross this tile's edges
    const uint32_t kf = sk[0], kl = sk[tile_n - 1];
    size_t x = base, y = base + (size_t)tile_n;
    if (base > 0 && key[base - 1] == kf) {  // first position of kf in [0, base)
      size_t lo = 0, hi = base - 1;
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key[mid] < kf) lo = mid + 1;
        else hi = mid;
      }
      x = lo;
    }
    if (y < n && key[y] == kl) {  // first position past kl in (y, n]
      size_t lo = y + 1, hi = n;
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key[mid] <= kl) lo = mid + 1;
        else hi = mid;
      }
      y = lo;
    }
    edge[0] = x;
    edge[1] = y;
  }
  __syncthreads();
  const unsigned long long here = tile_base[blockIdx.x];
  const unsigned long long g_lo = neg_below(edge[0], n, lab, tile_base, all_neg, red);
  const unsigned long long g_hi = neg_below(edge[1], n, lab, tile_base, all_neg, red);
  unsigned long long sum = 0ull;
  uint32_t seen = 0xFFFFFFFFu;
  unsigned long long both = 0ull;  // of the run of key `seen`
  bool have = false;
#pragma unroll
  for (int q = 0; q < kMtPer; q++) {
    const int j = threadIdx.x * kMtPer + q;
    if (j >= tile_n || flag[q] != 0u) continue;
    const uint32_t k = sk[j];
    if (!have || k != seen) {
      int lo = 0, hi = j;  // first position of k
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sk[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      const int ls = lo;
      lo = j + 1;
      hi = tile_n;  // first position past k
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sk[mid] <= k) lo = mid + 1;
        else hi = mid;
      }
      const int le = lo;
      both = (ls == 0 ? g_lo : here + ln[ls]) + (le == tile_n ? g_hi : here + ln[le]);
      seen = k;
      have = true;
    }
    sum += both;
  }
  sum = block_reduce_sum<unsigned long long, kMtBlock>(sum, red64);
  if (threadIdx.x == 0) {
    if (sum != 0ull) atomicAdd(&out[0], sum);
    if (blockIdx.x == 0) {
      out[1] = (unsigned long long)n - all_neg;
      out[2] = all_neg;
    }
  }
}

__global__ void metric_zero_kernel(unsigned long long* out, int words) {
  if ((int)threadIdx.x < words) out[threadIdx.x] = 0ull;
}

// ---- NDCG --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMtBlock)
    metric_label_key_kernel(const uint32_t* __restrict__ lab, size_t n, uint32_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * kMtBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kMtBlock)
    out[i] = order_key(__uint_as_float(lab[i]));
}

// partial[b] = sum over this workgroup's elements of label_i / log2(2 + (n - 1 - i))
__global__ void __launch_bounds__(kMtBlock)
    metric_dcg_kernel(const uint32_t* __restrict__ lab, size_t n, double* __restrict__ partial) {
  __shared__ double red[kMtBlock / 64];
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * kMtBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kMtBlock)
    s += (double)__uint_as_float(lab[i]) / log2(2.0 + (double)(n - 1 - i));
  s = block_reduce_sum<double, kMtBlock>(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kMtBlock)
    metric_sum_partials_kernel(const double* __restrict__ partial, int m, double* __restrict__ out) {
  __shared__ double red[kMtBlock / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < m; b += kMtBlock) s += partial[b];
  s = block_reduce_sum<double, kMtBlock>(s, red);
  if (threadIdx.x == 0) *out = s;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t mt_tiles(size_t n) { return ceil_div<size_t>(n > 0 ? n : 1, (size_t)kMtTile); }
constexpr size_t kMtMaxN = 0x7FFFFFFFull;  // n < 2^31 per class: 2U < 2^63

}  // namespace
}  // namespace hctr

extern "C" {

size_t hctr_metric_accumulate_temp_bytes(void) { return hctr::kMtAccGrid * sizeof(double); }

int hctr_metric_accumulate(const void* pred, int pred_dtype, const float* label, size_t n, int C,
                           uint32_t* keys, float* labels, size_t cap, size_t offset,
                           uint64_t* counters, void* temp, size_t temp_bytes,
                           hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(C >= 1 && C <= HCTR_METRIC_MAX_CLASSES, "hctr_metric_accumulate: C must be 1..256");
  HCTR_REQUIRE(n <= kMtMaxN && cap <= kMtMaxN, "hctr_metric_accumulate: n, cap must be < 2^31");
  HCTR_REQUIRE(offset <= cap && n <= cap - offset, "hctr_metric_accumulate: offset + n > cap");
  HCTR_REQUIRE(keys && labels && counters && temp, "hctr_metric_accumulate: null pointer");
  HCTR_REQUIRE(n == 0 || (pred && label), "hctr_metric_accumulate: null pointer");
  HCTR_REQUIRE(temp_bytes >= hctr_metric_accumulate_temp_bytes(),
               "hctr_metric_accumulate: workspace too small");
  HCTR_REQUIRE(pred_dtype == HCTR_EMB_F32 || pred_dtype == HCTR_EMB_F16 ||
                   pred_dtype == HCTR_EMB_BF16, "hctr_metric_accumulate: dtype");
  if (n == 0) return HCTR_OK;
  const int grid = grid_for(n * (size_t)C, kMtBlock, kMtAccGrid);
  return with_dtype(pred_dtype, [&](auto* tag) -> int {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(metric_accumulate_kernel<T>, dim3(grid), dim3(kMtBlock), 0,
                       as_stream(stream), (const T*)pred, label, n, C, keys, labels, cap, offset,
                       (unsigned long long*)counters, (double*)temp);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  });
}

size_t hctr_metric_auc_temp_bytes(size_t n) {
  using namespace hctr;
  return 2 * up256(n * sizeof(uint32_t)) + up256((mt_tiles(n) + 2) * sizeof(uint64_t)) +
         up256(radix_sort_temp_bytes(n));
}

int hctr_metric_auc(void* temp, size_t temp_bytes, const uint32_t* keys, const float* labels,
                    size_t n, uint64_t* out, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(n <= kMtMaxN, "hctr_metric_auc: n must be < 2^31");
  HCTR_REQUIRE(out && temp && (n == 0 || (keys && labels)), "hctr_metric_auc: null pointer");
  HCTR_REQUIRE(temp_bytes >= hctr_metric_auc_temp_bytes(n), "hctr_metric_auc: workspace too small");
  hipStream_t s = as_stream(stream);
  unsigned long long* o = (unsigned long long*)out;
  if (n == 0) {
    hipLaunchKernelGGL(metric_zero_kernel, dim3(1), dim3(64), 0, s, o, 3);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }
  char* p = (char*)temp;
  uint32_t* sk = (uint32_t*)p;
  p += up256(n * sizeof(uint32_t));
  uint32_t* sv = (uint32_t*)p;
  p += up256(n * sizeof(uint32_t));
  const size_t tiles = mt_tiles(n);
  unsigned long long* tile_neg = (unsigned long long*)p;
  unsigned long long* d_all = tile_neg + tiles + 1;
  p += up256((tiles + 2) * sizeof(uint64_t));
  HCTR_TRY(radix_sort_pairs_u32(p, radix_sort_temp_bytes(n), keys, sk, (const uint32_t*)labels, sv,
                                n, 32, s));
  hipLaunchKernelGGL(metric_auc_count_kernel, dim3((unsigned)tiles), dim3(kMtBlock), 0, s, sv, n,
                     tile_neg, o);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_detail::scan_tiles_u64_kernel, dim3(1), dim3(1024), 0, s, tile_neg,
                     tiles, d_all);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(metric_auc_run_kernel, dim3((unsigned)tiles), dim3(kMtBlock), 0, s, sk, sv, n,
                     tile_neg, d_all, o);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

size_t hctr_metric_ndcg_temp_bytes(size_t n) {
  using namespace hctr;
  return 4 * up256(n * sizeof(uint32_t)) + up256(kMaxGrid * sizeof(double)) +
         up256(radix_sort_temp_bytes(n));
}

int hctr_metric_ndcg(void* temp, size_t temp_bytes, const uint32_t* keys, const float* labels,
                     size_t n, double* out, hctr_stream_t stream) {
  using namespace hctr;
  HCTR_REQUIRE(n <= kMtMaxN, "hctr_metric_ndcg: n must be < 2^31");
  HCTR_REQUIRE(out && temp && (n == 0 || (keys && labels)), "hctr_metric_ndcg: null pointer");
  HCTR_REQUIRE(temp_bytes >= hctr_metric_ndcg_temp_bytes(n),
               "hctr_metric_ndcg: workspace too small");
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    hipLaunchKernelGGL(metric_zero_kernel, dim3(1), dim3(64), 0, s, (unsigned long long*)out, 2);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }
  char* p = (char*)temp;
  uint32_t* a = (uint32_t*)p;  // sorted score keys, later sorted label keys
  p += up256(n * sizeof(uint32_t));
  uint32_t* b = (uint32_t*)p;  // labels in score order
  p += up256(n * sizeof(uint32_t));
  uint32_t* c = (uint32_t*)p;  // the labels' own keys
  p += up256(n * sizeof(uint32_t));
  uint32_t* d = (uint32_t*)p;  // labels in their own order
  p += up256(n * sizeof(uint32_t));
  double* partial = (double*)p;
  p += up256(kMaxGrid * sizeof(double));
  const size_t rs_bytes = radix_sort_temp_bytes(n);
  const int grid = grid_for(n, kMtBlock);
  HCTR_TRY(radix_sort_pairs_u32(p, rs_bytes, keys, a, (const uint32_t*)labels, b, n, 32, s));
  hipLaunchKernelGGL(metric_dcg_kernel, dim3(grid), dim3(kMtBlock), 0, s, b, n, partial);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(metric_sum_partials_kernel, dim3(1), dim3(kMtBlock), 0, s, partial, grid, out);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(metric_label_key_kernel, dim3(grid), dim3(kMtBlock), 0, s, b, n, c);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(radix_sort_pairs_u32(p, rs_bytes, c, a, b, d, n, 32, s));
  hipLaunchKernelGGL(metric_dcg_kernel, dim3(grid), dim3(kMtBlock), 0, s, d, n, partial);
  HCTR_LAUNCH_CHECK();
  hipLaunchKernelGGL(metric_sum_partials_kernel, dim3(1), dim3(kMtBlock), 0, s, partial, grid,
                     out + 1);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}
}
