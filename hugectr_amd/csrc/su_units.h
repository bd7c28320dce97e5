// su_units.h -- what the units of the sparse update ask of each other (internal).
//   sparse_update.hip  SparseUpdater, where a batch goes (update_typed), pairs + sort, the hot /
//                      cold path of one-hot batches, the generic path, atomic SGD, sweeps, wgrad
//   su_segmented.hip   the sorted list of a D that is a supported multiple of 4: seg_* kernels
//   su_device.h        what the kernels of both units inline
// Every kernel is instantiated in exactly one object.
#pragma once
#include "sparse_update.h"

namespace hctr {

// hipMalloc whose result joins `owned`, the one list a destroy() frees: a buffer is named where it
// is allocated and nowhere else
template <typename T>
inline int dev_alloc(std::vector<void*>& owned, T*& p, size_t bytes) {
  HCTR_HIP(hipMalloc((void**)&p, bytes));
  owned.push_back(p);
  return HCTR_OK;
}

// f((OffT*)nullptr, (GradT*)nullptr) for the row-offset type of key_type (the caller has checked
// it) and the gradient type of grad_dtype
template <typename F>
int with_types(int key_type, int grad_dtype, F&& f) {
  return with_dtype(grad_dtype, [&](auto* g) -> int {
    int rc = HCTR_OK;
    with_bool(key_type == HCTR_KEY_U32, [&](auto u32) {
      rc = f((std::conditional_t<decltype(u32)::value, uint32_t, long long>*)nullptr, g);
    });
    return rc;
  });
}

// the (row, bucket) list the sorted paths walk: ascending rows, n entries (padding behind the live
// ones); need_sort: it still has to be made, into sort_keys_out / sort_vals_out (sort_stage)
struct SortedPairs {
  const uint32_t* rows;
  const uint32_t* buckets;
  size_t n;
  bool need_sort;
};

// ---- su_segmented.hip ---------------------------------------------------------------------------
// positions of the sorted list per tile; SparseUpdater::create sizes the tile partials with it
constexpr int kSegTile = 32;

// segmented reduce, the apply pass unless the optimizer folds into the reduce, then the runs that
// cross tile borders, for 32-bit / 64-bit row offsets (ro, sro).  direct != nullptr: store-only
// mode, finished runs are written straight to their output row
int update_segmented_u32(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner,
                         const void* ro, const void* sro, const void* grad, int grad_dtype,
                         const OptState& opt, float* direct, float* table, float* state0,
                         float* state1, uint64_t* prev_time, hipStream_t s);
int update_segmented_i64(SparseUpdater& u, const SortedPairs& p, size_t buckets, int combiner,
                         const void* ro, const void* sro, const void* grad, int grad_dtype,
                         const OptState& opt, float* direct, float* table, float* state0,
                         float* state1, uint64_t* prev_time, hipStream_t s);

}  // namespace hctr
