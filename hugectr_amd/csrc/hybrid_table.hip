// hybrid_table.hip -- bounded key -> vector table with LRU eviction (SOK DynamicVariable,
// var_type="hybrid").
//
// Plays the part of the reference's HKV-backed variable
// (R/sparse_operation_kit/kit_src/variable/impl/hkv_variable.cu:274-493): find_or_insert and
// lookup_with_evict on a table of fixed capacity whose least recently used entry makes room.  The
// semantics are this project's own (DESIGN.md "Hybrid table"), chosen so that every call is
// deterministic and checkable bit for bit against tests/lru_oracle.py:
//
//   C = capacity slots in C / S buckets of S slots; bucket = MurmurHash3_32(key) % (C / S).
//   Slot s holds a key (or kLruEmpty), a uint64 score (the number of the last inserting call that
//   touched it), a 1-byte digest (hash >> 24) and row s of the [C][D] fp32 store.
//   An inserting call t: (1) hits get score t; (2) the distinct missing keys of each bucket, in
//   ascending key order, take the lowest empty slot, else the slot with the smallest (score, slot)
//   among scores < t (its (key, row) is evicted), else are rejected; (3) new rows get the
//   initializer's value, a pure function of (seed, key, element), and zero optimizer state.
//
// Layout for MI355X: one 128-B digest line per bucket (S = 128) filters the probe to that line plus
// the matching key; the insert step gives every bucket to one wave, so slots are claimed without
// CAS and in a fixed order.  Rows after the slots are per-call rows: what a key that is not stored
// (a miss of a read-only lookup, a rejected key) reads in the current call, so the path's gather /
// pooling kernels run unchanged on the row numbers handed out here.
//
// Low-frequency filter (hctr_lru_lookup_index_filtered): in an inserting call a key that is not
// stored is admitted only if a hash of (seed, key, t) falls below the admission threshold; the
// others get the kLruFiltered row, touch nothing, and hctr_lru_compact drops them from the batch.
// hctr_lru_export_if exports the slots whose score is at least a given call number.
//
// Host-memory tier (hctr_lru_create_tiered): slots [0, H) keep their rows (and optimizer states) in
// HBM, slots [H, C) in pinned, device-mapped host memory, H a whole number of buckets.  Only where
// the bytes live changes.  The rows handed out are still HBM rows: an HBM-resident key gets its
// slot, every other position p gets the per-call row H + p, into which lru_stage_kernel copies the
// host slot's row (or the initializer's value).  hctr_lru_apply_update stages the distinct host
// slots of a step into rows H + u (u = rank in slot order), runs the sparse optimizer there and
// writes them back.
//
// Growth (hctr_lru_create_growing): the table starts with C0 slots, Cmax = C0 * 2^j.  An inserting
// call below Cmax first probes (find in kLruProbe mode, sort, count: nothing is written), reads
// occ and m = its distinct new keys back, and doubles C while C < Cmax and occ + m > L * C
// (lru_double: lru_split_kernel + lru_move_kernel per doubling); then it runs as on a fixed
// table.  hctr_lru_create(_tiered) are the case j = 0, which never takes that path.
//
// One table, one code path: hctr_lru holds the LruTbl the kernels take, and an untiered table is the
// case H = C of it (no host arrays, every slot an HBM slot).  Every host function serves both
// kinds; where they differ it is in which kernels a lookup launches:
//   untiered  a position that is not stored gets its per-call row, and the initializer's value in
//             it, from the find kernel (kLruRead) or from lru_insert_kernel<K, false> (a rejected
//             key): no launch beyond the find / insert ones;
//   tiered    the find / insert kernels hand out slots (kLruFind, lru_insert_kernel<K, true>, whose
//             Tier flag also makes lru_slot_row look at H), and lru_stage_kernel turns them into
//             rows.
// The Filter flag of lru_find_kernel is set by an inserting call whose threshold admits less than
// every key.  lru_slot_io_kernel (slot-addressed reads and writes, the export's rows) tests
// slot < H at run time and so needs no flag.
//
// Compiled as part of det.hip's unit (included at its end): the bounded sibling of the dynamic
// table, built into every library that carries the dynamic table.  Its internal names carry an
// lru prefix for that reason.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "common.h"
#include "radix_sort.h"
#include "scan.h"

namespace hctr {
namespace {

constexpr int kLruBlock = 256;
constexpr int kLruWavesPerBlock = kLruBlock / kWave;
constexpr uint64_t kLruEmpty = ~0ull;
// row index of a key the low-frequency filter did not admit (distinct from kInvalidIndex)
constexpr uint64_t kLruFiltered = ~0ull - 1;
constexpr uint64_t kLruAdmitAll = 1ull << 32;
constexpr int kLruMaxSlotsPerLane = 4;  // S <= 256

__device__ __forceinline__ uint64_t lru_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// constant, or uniform (0, 1] from 24 bits of a counter-based hash of (seed, key, element)
__device__ __forceinline__ float lru_init_value(int mode, float val, uint64_t seed, uint64_t key,
                                                uint32_t e) {
  if (mode == 0) return val;
  const uint64_t h = lru_splitmix64(seed ^ lru_splitmix64(key * 0x100000001B3ull + e));
  return ((float)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);
}

// admission draw of a key that is not stored, in inserting call t: 32 bits of a counter-based hash
// of (seed, key, t); the key is admitted iff the draw < admit_below (= ceil(p * 2^32))
__device__ __forceinline__ uint32_t lru_admit_draw(uint64_t seed, uint64_t key, uint64_t t) {
  return (uint32_t)(lru_splitmix64(seed ^ lru_splitmix64(key ^ lru_splitmix64(t))) >> 32);
}

template <typename K>
__device__ __forceinline__ uint64_t lru_key_u64(K k);
template <>
__device__ __forceinline__ uint64_t lru_key_u64<uint32_t>(uint32_t k) {
  return (uint64_t)k;
}
template <>
__device__ __forceinline__ uint64_t lru_key_u64<long long>(long long k) {
  return (uint64_t)k;
}

struct LruTbl {
  uint64_t* keys;     // [C]
  uint64_t* scores;   // [C]
  uint8_t* digests;   // [C]
  float* rows;        // [H + scratch][D]: the slots in HBM, then the per-call rows
  float* st[2];       // optimizer states: [C][D] (tiered: the rows' shape) or null
  // slots >= H live in the host arrays, row s at (s - H) * D.  H = C: untiered, no host arrays
  float* hrows;       // [C - H][D] host-mapped
  float* hst[2];      // [C - H][D] or null, with the state it belongs to
  uint64_t H;
  uint64_t nb;        // buckets
  int S, D;
  uint64_t C;
  int init_mode;
  float init_val;
  uint64_t seed;
};

// kLruProbe: kLruInsert's outputs without its side effects (no score, no filtered count): the pass
// by which a table below its largest capacity counts a call's new keys before it decides to grow
enum { kLruFind = 0, kLruRead = 1, kLruInsert = 2, kLruProbe = 3 };

// One thread per key: the bucket's digest line (S bytes, 16 B per load), then the key of every
// slot whose digest matches.  kLruFind: slot or kInvalidIndex.  kLruRead: slot, or a scratch row
// holding the initializer's value.  kLruInsert: hits get score t; misses are handed to the sort
// (bucket = nb marks a hit, which sorts behind every bucket).  Filter (kLruInsert only): a miss
// whose admission draw is >= admit_below gets kLruFiltered and sorts behind the buckets like a hit;
// such positions are counted in counters[2], one atomic per wave.
template <typename K, bool Filter>
__global__ void __launch_bounds__(kLruBlock)
    lru_find_kernel(LruTbl T, const K* __restrict__ in, size_t n, int mode, uint64_t t,
                    uint64_t* __restrict__ idx, uint32_t* __restrict__ sbkt,
                    uint32_t* __restrict__ slo, uint32_t* __restrict__ shi,
                    uint32_t* __restrict__ sval, uint64_t admit_below,
                    unsigned long long* __restrict__ counters) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (Filter) {
    // the whole wave reaches the ballot below (lanes past n take part as "not filtered")
    if (i - (threadIdx.x % kWave) >= n) return;
  } else if (i >= n) {
    return;
  }
  const bool live = i < n;
  const K kk = in[live ? i : 0];
  const uint64_t key = lru_key_u64<K>(kk);
  const uint32_t h = murmur3_key(kk);
  const uint64_t b = (uint64_t)h % T.nb;
  const uint32_t dg = h >> 24;
  const uint64_t base = b * (uint64_t)T.S;
  const uint32_t pat = dg * 0x01010101u;
  const uint4* line = reinterpret_cast<const uint4*>(T.digests + base);
  uint64_t slot = kInvalidIndex;
  // (the all-ones key is the empty marker: never stored, never found)
  for (int w = 0; w < T.S / 16 && slot == kInvalidIndex && key != kLruEmpty; w++) {
    const uint4 v = line[w];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    for (int q = 0; q < 4 && slot == kInvalidIndex; q++) {
      const uint32_t x = words[q] ^ pat;
      // every zero byte of x is flagged (bytes above one may be flagged falsely: the key decides)
      uint32_t m = (x - 0x01010101u) & ~x & 0x80808080u;
      while (m) {
        const int byte = __builtin_ctz(m) >> 3;
        const uint64_t s = base + (uint64_t)(w * 16 + q * 4 + byte);
        if (T.keys[s] == key) {
          slot = s;
          break;
        }
        m &= m - 1;
      }
    }
  }
  if (mode == kLruFind) {
    idx[i] = slot;
    return;
  }
  if (mode == kLruRead) {
    if (slot != kInvalidIndex) {
      idx[i] = slot;
      return;
    }
    const uint64_t r = T.C + (T.init_mode == 0 ? 0 : i);
    idx[i] = r;
    if (T.init_mode != 0)
      for (int e = 0; e < T.D; e++)
        T.rows[r * T.D + e] = lru_init_value(T.init_mode, T.init_val, T.seed, key, e);
    return;
  }
  bool filtered = false;
  if (Filter) {
    filtered = live && slot == kInvalidIndex && lru_admit_draw(T.seed, key, t) >= admit_below;
    const uint64_t fm = __ballot(filtered);
    if (fm && mode != kLruProbe && (threadIdx.x % kWave) == 0)
      atomicAdd(&counters[2], (unsigned long long)__popcll(fm));
    if (!live) return;
    if (filtered) slot = kLruFiltered;
  }
  // (every writer writes the same t)
  if (slot != kInvalidIndex && !filtered && mode != kLruProbe) T.scores[slot] = t;
  idx[i] = slot;
  sbkt[i] = slot != kInvalidIndex ? (uint32_t)T.nb : (uint32_t)b;
  slo[i] = (uint32_t)key;
  if (shi) shi[i] = (uint32_t)(key >> 32);
  sval[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kLruBlock)
    lru_permute_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ perm,
                       size_t n, uint32_t* __restrict__ out) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i < n) out[i] = src[perm[i]];
}

__device__ __forceinline__ uint32_t lru_lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// One wave per bucket: its run [lo, hi) in the sorted missing keys, and how many of its distinct
// keys will evict: min(max(distinct - empty, 0), slots with score < t).  miss (may be null) gathers
// the distinct keys of all buckets, one atomic per bucket that has some.
template <typename K>
__global__ void __launch_bounds__(kLruBlock)
    lru_count_kernel(LruTbl T, const K* __restrict__ in, const uint32_t* __restrict__ sbkt,
                     const uint32_t* __restrict__ perm, uint32_t n, uint64_t t,
                     uint32_t* __restrict__ rng, uint32_t* __restrict__ evict_cnt,
                     unsigned long long* __restrict__ miss) {
  const uint64_t b = blockIdx.x * (uint64_t)kLruWavesPerBlock + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (b >= T.nb) return;
  const uint32_t lo = lru_lower_bound_u32(sbkt, n, (uint32_t)b);
  const uint32_t hi = lru_lower_bound_u32(sbkt, n, (uint32_t)b + 1);
  if (lane == 0) {
    rng[2 * b] = lo;
    rng[2 * b + 1] = hi;
  }
  if (lo == hi) {
    if (lane == 0) evict_cnt[b] = 0;
    return;
  }
  uint32_t distinct = 0;
  for (uint32_t j0 = lo; j0 < hi; j0 += kWave) {
    const uint32_t j = j0 + lane;
    bool first = false;
    if (j < hi) {
      const uint64_t k = lru_key_u64<K>(in[perm[j]]);
      first = k != kLruEmpty && (j == lo || k != lru_key_u64<K>(in[perm[j - 1]]));
    }
    distinct += (uint32_t)__popcll(__ballot(first));
  }
  if (miss && lane == 0 && distinct) atomicAdd(miss, (unsigned long long)distinct);
  uint32_t empty = 0, elig = 0;
  const uint64_t base = b * (uint64_t)T.S;
  for (int j = 0; j < T.S / kWave; j++) {
    const uint64_t s = base + (uint64_t)(j * kWave + lane);
    const uint64_t k = T.keys[s];
    empty += (uint32_t)__popcll(__ballot(k == kLruEmpty));
    elig += (uint32_t)__popcll(__ballot(k != kLruEmpty && T.scores[s] < t));
  }
  if (lane == 0) {
    const uint32_t need = distinct > empty ? distinct - empty : 0;
    evict_cnt[b] = need < elig ? need : elig;
  }
}

__device__ __forceinline__ uint64_t lru_wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint64_t o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

// a slot's row in one of the table's arrays: HBM below H, host memory from H on (Tier only)
template <bool Tier>
__device__ __forceinline__ float* lru_slot_row(float* hbm, float* host, uint64_t H, uint64_t s,
                                               int D) {
  if (Tier && s >= H) return host + (s - H) * (uint64_t)D;
  return hbm + s * (uint64_t)D;
}

// One wave per bucket inserts the bucket's distinct missing keys in ascending key order.  Lane l
// keeps slots l, l + 64, ... (key, score) in registers; a victim is the wave-wide minimum of
// (score << 16 | slot) over slots with score < t.  Tier: rows and states of slots >= H are in host
// memory, and a rejected key gets kInvalidIndex (lru_stage_kernel gives it a per-call row).
template <typename K, bool Tier>
__global__ void __launch_bounds__(kLruBlock)
    lru_insert_kernel(LruTbl T, const K* __restrict__ in, const uint32_t* __restrict__ perm,
                      const uint32_t* __restrict__ rng, const uint32_t* __restrict__ evict_off,
                      uint64_t t, uint64_t* __restrict__ idx, void* __restrict__ ev_keys,
                      int key_bytes, float* __restrict__ ev_rows,
                      unsigned long long* __restrict__ counters) {
  const uint64_t b = blockIdx.x * (uint64_t)kLruWavesPerBlock + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (b >= T.nb) return;
  const uint32_t lo = rng[2 * b], hi = rng[2 * b + 1];
  if (lo == hi) return;
  const int spl = T.S / kWave;
  const uint64_t base = b * (uint64_t)T.S;
  uint64_t k[kLruMaxSlotsPerLane], sc[kLruMaxSlotsPerLane];
#pragma unroll
  for (int j = 0; j < kLruMaxSlotsPerLane; j++) {
    k[j] = j < spl ? T.keys[base + j * kWave + lane] : 0ull;
    sc[j] = j < spl ? T.scores[base + j * kWave + lane] : t;
  }
  uint32_t out_e = evict_off[b];
  unsigned long long filled = 0, rejected = 0;
  const int D = T.D;
  uint32_t j = lo;
  while (j < hi) {
    const K kk = in[perm[j]];
    const uint64_t key = lru_key_u64<K>(kk);
    uint32_t r = j + 1;
    while (r < hi && lru_key_u64<K>(in[perm[r]]) == key) r++;
    // lowest empty slot
    int sl = -1;
#pragma unroll
    for (int q = 0; q < kLruMaxSlotsPerLane; q++) {
      const uint64_t m = __ballot(q < spl && k[q] == kLruEmpty);
      if (sl < 0 && m) sl = q * kWave + __ffsll((long long)m) - 1;
    }
    if (key == kLruEmpty) sl = -2;  // the empty marker itself is rejected
    bool evict = false;
    if (sl == -1) {
      uint64_t best = ~0ull;
#pragma unroll
      for (int q = 0; q < kLruMaxSlotsPerLane; q++)
        if (q < spl && k[q] != kLruEmpty && sc[q] < t) {
          const uint64_t c = (sc[q] << 16) | (uint64_t)(q * kWave + lane);
          best = c < best ? c : best;
        }
      best = lru_wave_min_u64(best);
      if (best != ~0ull) {
        sl = (int)(best & 0xFFFF);
        evict = true;
      }
    }
    uint64_t res;
    if (sl >= 0) {
      const int q = sl / kWave, owner = sl % kWave;
      const uint64_t s = base + (uint64_t)sl;
      uint64_t kq = 0;
#pragma unroll
      for (int x = 0; x < kLruMaxSlotsPerLane; x++)
        if (x == q) kq = k[x];
      const uint64_t old = __shfl(kq, owner);
      if (evict && ev_keys) {
        if (lane == 0) {
          if (key_bytes == 8)
            static_cast<uint64_t*>(ev_keys)[out_e] = old;
          else
            static_cast<uint32_t*>(ev_keys)[out_e] = (uint32_t)old;
        }
        if (ev_rows) {
          const float* src = lru_slot_row<Tier>(T.rows, T.hrows, T.H, s, D);
          for (int e = lane; e < D; e += kWave)
            ev_rows[(uint64_t)out_e * D + e] = src[e];  // read before the overwrite
        }
      }
      if (evict) out_e++;
      if (lane == owner) {
#pragma unroll
        for (int x = 0; x < kLruMaxSlotsPerLane; x++)
          if (x == q) {
            k[x] = key;
            sc[x] = t;
          }
        T.keys[s] = key;
        T.scores[s] = t;
        T.digests[s] = (uint8_t)(murmur3_key(kk) >> 24);
      }
      // (the addresses stay inside the loop: three row pointers kept across it cost the untiered
      // instantiation two more spilled SGPRs)
      for (int e = lane; e < D; e += kWave) {
        lru_slot_row<Tier>(T.rows, T.hrows, T.H, s, D)[e] =
            lru_init_value(T.init_mode, T.init_val, T.seed, key, e);
        if (T.st[0]) lru_slot_row<Tier>(T.st[0], T.hst[0], T.H, s, D)[e] = 0.0f;
        if (T.st[1]) lru_slot_row<Tier>(T.st[1], T.hst[1], T.H, s, D)[e] = 0.0f;
      }
      if (!evict) filled++;
      res = s;
    } else {
      rejected++;
      res = kInvalidIndex;
    }
    for (uint32_t p = j; p < r; p++) {
      const uint32_t pos = perm[p];
      uint64_t row = res;
      if (!Tier && res == kInvalidIndex) {
        row = T.C + (T.init_mode == 0 ? 0 : pos);
        if (T.init_mode != 0)
          for (int e = lane; e < D; e += kWave)
            T.rows[row * D + e] = lru_init_value(T.init_mode, T.init_val, T.seed, key, e);
      }
      if (lane == 0) idx[pos] = row;
    }
    j = r;
  }
  if (lane == 0) {
    if (filled) atomicAdd(&counters[0], filled);
    if (rejected) atomicAdd(&counters[1], rejected);
  }
}

// a slot is exported iff it is occupied and its score >= min_score (0: every occupied slot)
__device__ __forceinline__ bool lru_exported(const uint64_t* keys, const uint64_t* scores, size_t i,
                                             uint64_t min_score) {
  return keys[i] != kLruEmpty && (min_score == 0 || scores[i] >= min_score);
}

__global__ void __launch_bounds__(kLruBlock)
    lru_occupied_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ scores,
                        size_t C, uint64_t min_score, uint32_t* __restrict__ flag) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i < C) flag[i] = lru_exported(keys, scores, i, min_score) ? 1u : 0u;
}

__global__ void __launch_bounds__(kLruBlock)
    lru_export_kernel(const uint64_t* __restrict__ keys, size_t C, const uint32_t* __restrict__ off,
                      const uint64_t* __restrict__ scores, uint64_t min_score, size_t max_out,
                      int key_bytes, void* __restrict__ out_keys, uint64_t* __restrict__ out_slots,
                      uint64_t* __restrict__ out_scores) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i >= C || !lru_exported(keys, scores, i, min_score)) return;
  const uint32_t o = off[i];
  if (o >= max_out) return;
  if (out_keys) {
    if (key_bytes == 8)
      static_cast<uint64_t*>(out_keys)[o] = keys[i];
    else
      static_cast<uint32_t*>(out_keys)[o] = (uint32_t)keys[i];
  }
  if (out_slots) out_slots[o] = i;
  if (out_scores) out_scores[o] = scores[i];
}

__global__ void lru_fill_kernel(float* p, size_t n, float v) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void __launch_bounds__(kLruBlock)
    lru_clear_kernel(uint64_t* keys, uint64_t* scores, size_t C) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i < C) {
    keys[i] = kLruEmpty;
    scores[i] = 0;
  }
}

// CSR compaction of a filtered lookup: keep[i] = 1 unless row i is kLruFiltered; an exclusive scan
// of keep gives every kept position its output position, so order is kept inside each sample and
// a sample's new offset is the scan at its old offset.
__global__ void __launch_bounds__(kLruBlock)
    lru_keep_kernel(const uint64_t* __restrict__ rows, size_t n, uint32_t* __restrict__ keep) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i < n) keep[i] = rows[i] != kLruFiltered ? 1u : 0u;
}

__global__ void __launch_bounds__(kLruBlock)
    lru_compact_kernel(size_t B, const long long* __restrict__ off, size_t n,
                       const uint64_t* __restrict__ rows, const void* __restrict__ keys,
                       int key_bytes, const float* __restrict__ w,
                       const uint32_t* __restrict__ pos, long long* __restrict__ out_off,
                       uint64_t* __restrict__ out_rows, void* __restrict__ out_keys,
                       float* __restrict__ out_w) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i <= B) out_off[i] = (long long)pos[off[i]];
  if (i >= n) return;
  const uint64_t r = rows[i];
  if (r == kLruFiltered) return;
  const uint32_t o = pos[i];
  out_rows[o] = r;
  if (key_bytes == 8)
    static_cast<uint64_t*>(out_keys)[o] = static_cast<const uint64_t*>(keys)[i];
  else
    static_cast<uint32_t*>(out_keys)[o] = static_cast<const uint32_t*>(keys)[i];
  if (w) out_w[o] = w[i];
}

// ---- host-memory tier ----------------------------------------------------------------------------
// The row kernels below give each position (key, slot, staged row) a group of gl lanes, gl = the
// power of two >= D capped at a wave, so rows of D = 16 fill a wave with four of them.  They read
// the positions' slots from one array and write the rows handed out to another.
inline int lru_group_lanes(int D) {
  int g = 1;
  while (g < D && g < kWave) g <<= 1;
  return g;
}

// after a lookup on a tiered table: slot[p] holds a slot, kInvalidIndex (a miss, a rejected key) or
// kLruFiltered.  A position whose slot is an HBM slot keeps it; every other one (but a filtered
// one) gets the per-call row H + p, holding the host slot's row or the initializer's value.
template <typename K>
__global__ void __launch_bounds__(kLruBlock)
    lru_stage_kernel(LruTbl T, const K* __restrict__ in, size_t n, int gl,
                     const uint64_t* __restrict__ slot, uint64_t* __restrict__ idx) {
  const size_t p = (blockIdx.x * (size_t)kLruBlock + threadIdx.x) / (size_t)gl;
  const int l = (int)(threadIdx.x % (unsigned)gl);
  if (p >= n) return;
  const uint64_t s = slot[p];
  if (s < T.H || s == kLruFiltered) {
    if (l == 0) idx[p] = s;
    return;
  }
  const uint64_t r = T.H + p;
  float* dst = T.rows + r * (uint64_t)T.D;
  if (s < T.C) {
    const float* src = T.hrows + (s - T.H) * (uint64_t)T.D;
    for (int e = l; e < T.D; e += gl) dst[e] = src[e];
  } else {
    const uint64_t key = lru_key_u64<K>(in[p]);
    for (int e = l; e < T.D; e += gl)
      dst[e] = lru_init_value(T.init_mode, T.init_val, T.seed, key, e);
  }
  if (l == 0) idx[p] = r;
}

// optimizer step on a tiered table, 1/3: sort key = the host slot's number above H (all ones for
// HBM slots and invalid ones: they sort last), value = position; rows[] starts as the slots
__global__ void __launch_bounds__(kLruBlock)
    lru_step_keys_kernel(const uint64_t* __restrict__ slots, size_t n, uint64_t H, uint64_t C,
                         uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                         uint64_t* __restrict__ rows) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = slots[i];
  key[i] = (s >= H && s < C) ? (uint32_t)(s - H) : 0xFFFFFFFFu;
  val[i] = (uint32_t)i;
  rows[i] = s;
}

// 2/3: first[j] = sorted position j starts a run of one host slot
__global__ void __launch_bounds__(kLruBlock)
    lru_step_first_kernel(const uint32_t* __restrict__ key, size_t n, uint32_t host_slots,
                          uint32_t* __restrict__ first) {
  const size_t j = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (j < n) first[j] = (key[j] < host_slots && (j == 0 || key[j] != key[j - 1])) ? 1u : 0u;
}

// 3/3, both directions.  u = the run's rank (off = exclusive scan of first).  in: every position of
// a host slot gets row H + u, the run's first copies the slot's row and states into that row.
// out (after the update): the run's first copies them back.
template <bool In>
__global__ void __launch_bounds__(kLruBlock)
    lru_step_stage_kernel(LruTbl T, const uint32_t* __restrict__ key,
                          const uint32_t* __restrict__ val, const uint32_t* __restrict__ first,
                          const uint32_t* __restrict__ off, size_t n, int gl,
                          uint64_t* __restrict__ rows) {
  const size_t j = (blockIdx.x * (size_t)kLruBlock + threadIdx.x) / (size_t)gl;
  const int l = (int)(threadIdx.x % (unsigned)gl);
  if (j >= n) return;
  const uint32_t k = key[j];
  if ((uint64_t)k >= T.C - T.H) return;
  const bool f = first[j] != 0u;
  const uint64_t r = T.H + (uint64_t)(f ? off[j] : off[j] - 1u);
  if (In && l == 0) rows[val[j]] = r;
  if (!f) return;
  const uint64_t D = (uint64_t)T.D;
  float* hbm[3] = {T.rows + r * D, T.st[0] ? T.st[0] + r * D : nullptr,
                   T.st[1] ? T.st[1] + r * D : nullptr};
  float* host[3] = {T.hrows + k * D, T.hst[0] ? T.hst[0] + k * D : nullptr,
                    T.hst[1] ? T.hst[1] + k * D : nullptr};
  for (int a = 0; a < 3; a++) {
    if (!hbm[a]) continue;
    for (int e = l; e < T.D; e += gl) {
      if (In)
        hbm[a][e] = host[a][e];
      else
        host[a][e] = hbm[a][e];
    }
  }
}

// slot-addressed I/O on one array (rows or a state), either table: a slot below H is in hbm, the
// others in host; a slot >= C is skipped.  dir 0: out = array[slot]; 1: array[slot] = v; 2: +=.
__global__ void __launch_bounds__(kLruBlock)
    lru_slot_io_kernel(float* hbm, float* host, uint64_t H, uint64_t C,
                       const uint64_t* __restrict__ slots, size_t n, int D, int dir,
                       float* __restrict__ buf) {
  const size_t i = blockIdx.x * (size_t)kLruBlock + threadIdx.x;
  if (i >= n * (size_t)D) return;
  const uint64_t s = slots[i / D];
  if (s >= C) return;
  float* p = (s < H ? hbm + s * (uint64_t)D : host + (s - H) * (uint64_t)D) + i % D;
  if (dir == 0)
    buf[i] = *p;
  else if (dir == 1)
    *p = buf[i];
  else
    *p = *p + buf[i];
}

// ---- growth: one doubling C -> 2C ------------------------------------------------------------------
// One wave per old bucket b (T.nb, T.C: the table before the doubling; its arrays already have room
// for 2C slots, the upper half empty).  A key whose hash % (2 nb) is b + nb moves: the movers of a
// bucket, in ascending slot order, take slots (b + nb) * S + 0, 1, ... with their score and digest,
// and leave an empty slot.  Lane l owns slots l, l + 64, ... as in lru_insert_kernel; a mover's rank
// is the movers of the earlier slot groups plus those on lower lanes of its own.  Every (source,
// destination) pair goes into `list` for lru_move_kernel; a bucket reserves its run of the list
// with one atomic, so the list's order varies and its contents do not.
template <typename K>
__global__ void __launch_bounds__(kLruBlock)
    lru_split_kernel(LruTbl T, uint32_t* __restrict__ list, unsigned long long* __restrict__ list_n) {
  const uint64_t b = blockIdx.x * (uint64_t)kLruWavesPerBlock + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (b >= T.nb) return;
  const int spl = T.S / kWave;
  const uint64_t base = b * (uint64_t)T.S, nbase = (b + T.nb) * (uint64_t)T.S;
  uint64_t k[kLruMaxSlotsPerLane], mv[kLruMaxSlotsPerLane];
  uint32_t total = 0;
#pragma unroll
  for (int q = 0; q < kLruMaxSlotsPerLane; q++) {
    k[q] = q < spl ? T.keys[base + q * kWave + lane] : kLruEmpty;
    const bool moves = k[q] != kLruEmpty && (uint64_t)murmur3_key((K)k[q]) % (2 * T.nb) != b;
    mv[q] = __ballot(moves);
    total += (uint32_t)__popcll(mv[q]);
  }
  if (total == 0) return;
  unsigned long long first = 0;
  if (lane == 0) first = atomicAdd(list_n, (unsigned long long)total);
  first = __shfl(first, 0);
  uint32_t before = 0;
#pragma unroll
  for (int q = 0; q < kLruMaxSlotsPerLane; q++) {
    if ((mv[q] >> lane) & 1ull) {
      const uint32_t rank = before + (uint32_t)__popcll(mv[q] & ((1ull << lane) - 1ull));
      const uint64_t src = base + (uint64_t)(q * kWave + lane), dst = nbase + rank;
      T.keys[dst] = k[q];
      T.scores[dst] = T.scores[src];
      T.digests[dst] = T.digests[src];
      T.keys[src] = kLruEmpty;
      T.scores[src] = 0;
      T.digests[src] = 0;
      list[2 * (first + rank)] = (uint32_t)src;
      list[2 * (first + rank) + 1] = (uint32_t)dst;
    }
    before += (uint32_t)__popcll(mv[q]);
  }
}

// the rows and every allocated state of the pairs lru_split_kernel listed, a group of gl lanes per
// pair; either end may be in either tier (slot < H at run time, as lru_slot_io_kernel).  Sources
// lie below the old capacity and destinations above it, so one pass has no hazards.  The grid covers
// max_n >= *list_n pairs (the occupied slots, which the host knows).
__global__ void __launch_bounds__(kLruBlock)
    lru_move_kernel(LruTbl T, const uint32_t* __restrict__ list,
                    const unsigned long long* __restrict__ list_n, size_t max_n, int gl) {
  const size_t p = (blockIdx.x * (size_t)kLruBlock + threadIdx.x) / (size_t)gl;
  const int l = (int)(threadIdx.x % (unsigned)gl);
  if (p >= max_n || p >= *list_n) return;
  const uint64_t src = list[2 * p], dst = list[2 * p + 1], D = (uint64_t)T.D;
  float* hbm[3] = {T.rows, T.st[0], T.st[1]};
  float* host[3] = {T.hrows, T.hst[0], T.hst[1]};
  for (int a = 0; a < 3; a++) {
    if (!hbm[a]) continue;
    const float* from = src < T.H ? hbm[a] + src * D : host[a] + (src - T.H) * D;
    float* to = dst < T.H ? hbm[a] + dst * D : host[a] + (dst - T.H) * D;
    for (int e = l; e < T.D; e += gl) to[e] = from[e];
  }
}

inline int lru_blocks(size_t n) { return (int)ceil_div<size_t>(n > 0 ? n : 1, (size_t)kLruBlock); }

}  // namespace
}  // namespace hctr

using namespace hctr;

struct hctr_lru {
  // what the kernels see, passed to them as it stands.  Slots [H, C) keep rows and states in
  // pinned, device-mapped host memory; the HBM arrays of rows (and, tiered, of states) hold H slots
  // plus `scratch` per-call rows.  H = C: untiered.  T.C is the capacity now: it doubles, up to
  // Cmax, when an inserting call would load the table beyond L (lru_double), and H = min(C, Hb).
  LruTbl T{};
  uint64_t Cmax = 0, Hb = 0;  // largest capacity; HBM budget in slots (>= Cmax: never tiered)
  double L = 0.5;             // max_load_factor
  uint64_t doublings = 0;
  int key_type = HCTR_KEY_I64;
  size_t scratch = 0;  // rows after the H slots
  void* host_alloc[3] = {nullptr, nullptr, nullptr};  // the pinned allocations behind hrows / hst
  uint64_t* ws_rows = nullptr;            // [ws_n] staged rows of a step (tiered)
  uint64_t t = 0;  // inserting calls so far
  // [0] occupied slots, [1] rejected keys, [2] filtered, [3] a growing call's distinct new keys
  unsigned long long* counters = nullptr;
  unsigned long long* h_word = nullptr;    // pinned host words (4)
  // per-call workspace (n keys)
  size_t ws_n = 0;
  uint32_t* ws = nullptr;  // 8 arrays of ws_n
  unsigned long long* ws_tiles = nullptr;  // scan tiles of ws_n + 1 elements (compaction)
  void* sort_temp = nullptr;
  size_t sort_temp_bytes = 0;
  // per-bucket workspace
  uint32_t* rng = nullptr;        // [2 nb]
  uint32_t* evict_cnt = nullptr;  // [nb]
  uint32_t* evict_off = nullptr;  // [nb + 1]
  unsigned long long* tile_sums = nullptr;
  unsigned long long* d_total = nullptr;

  bool tiered() const { return T.H < T.C; }
  bool tiers() const { return Hb < Cmax; }  // tiered now, or once it has grown past Hb
  int key_bytes() const { return key_type == HCTR_KEY_I64 ? 8 : 4; }
  size_t row_bytes() const { return (size_t)T.D * sizeof(float); }
};

namespace {

void lru_free(hctr_lru* h) {
  void* dev[] = {h->T.keys, h->T.scores, h->T.digests, h->T.rows, h->T.st[0], h->T.st[1],
                 h->counters, h->ws, h->ws_tiles, h->ws_rows, h->sort_temp, h->rng, h->evict_cnt,
                 h->evict_off, h->tile_sums, h->d_total};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  void* host[] = {h->host_alloc[0], h->host_alloc[1], h->host_alloc[2], h->h_word};
  for (void* p : host)
    if (p) (void)hipHostFree(p);
  delete h;
}

// f(const K* keys), K the table's key type: the key-type dispatch of every entry point
template <typename F>
int lru_with_keys(const hctr_lru* h, const void* keys, F f) {
  if (h->key_type == HCTR_KEY_I64) return f(static_cast<const long long*>(keys));
  return f(static_cast<const uint32_t*>(keys));
}

// one device word through the pinned host word: one host synchronisation
template <typename W>
int lru_read_word(hctr_lru* h, const unsigned long long* d, hipStream_t s, W* out) {
  HCTR_HIP(hipMemcpyAsync(h->h_word, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HCTR_HIP(hipStreamSynchronize(s));
  *out = (W)*h->h_word;
  return HCTR_OK;
}

// the HBM array *a moves to a store of `rows` rows; its H slots are kept
int lru_grow(hctr_lru* h, float** a, size_t rows, hipStream_t s) {
  float* nr = nullptr;
  HCTR_HIP(hipMalloc(&nr, rows * h->row_bytes()));
  if (h->T.H)
    HCTR_HIP(hipMemcpyAsync(nr, *a, h->T.H * h->row_bytes(), hipMemcpyDeviceToDevice, s));
  HCTR_HIP(hipStreamSynchronize(s));
  HCTR_HIP(hipFree(*a));
  *a = nr;
  return HCTR_OK;
}

// per-call workspace and per-call rows for n keys
int lru_reserve(hctr_lru* h, size_t n, hipStream_t s) {
  if (n > h->ws_n) {
    if (h->ws) HCTR_HIP(hipFree(h->ws));
    if (h->ws_tiles) HCTR_HIP(hipFree(h->ws_tiles));
    if (h->sort_temp) HCTR_HIP(hipFree(h->sort_temp));
    h->ws = nullptr;
    h->ws_tiles = nullptr;
    h->sort_temp = nullptr;
    h->ws_n = 0;
    const size_t cap = n < 4096 ? 4096 : n;
    HCTR_HIP(hipMalloc(&h->ws, cap * 8 * sizeof(uint32_t)));
    HCTR_HIP(hipMalloc(&h->ws_tiles, (cap / 1024 + 2) * sizeof(unsigned long long)));
    h->sort_temp_bytes = radix_sort_temp_bytes(cap);
    HCTR_HIP(hipMalloc(&h->sort_temp, h->sort_temp_bytes));
    if (h->tiers()) {
      if (h->ws_rows) HCTR_HIP(hipFree(h->ws_rows));
      h->ws_rows = nullptr;
      HCTR_HIP(hipMalloc(&h->ws_rows, cap * sizeof(uint64_t)));
    }
    h->ws_n = cap;
  }
  // Per-call rows, grown once per new largest call (the slots move with their array).  Tiered:
  // every position may need one, in the rows and in the states.  Untiered: only the rows, and only
  // a key-dependent initializer needs more than the one row a constant takes.
  if (n > h->scratch && (h->tiered() || h->T.init_mode != 0)) {
    HCTR_TRY(lru_grow(h, &h->T.rows, h->T.H + n, s));
    for (float*& st : h->T.st)
      if (st && h->tiered()) HCTR_TRY(lru_grow(h, &st, h->T.H + n, s));
    h->scratch = n;
  }
  return HCTR_OK;
}

// lru_find_kernel over n keys, idx[i] = kLruFind: slot or kInvalidIndex; kLruRead: row; kLruInsert
// (call h->t, through the filter when admit_below < kLruAdmitAll): slot, kInvalidIndex for the
// insert step or kLruFiltered, and the sort's inputs (bucket, key low / high word, position) in
// the first four arrays of ws; kLruProbe: the same for the call to come, h->t + 1
template <typename K>
int lru_launch_find(hctr_lru* h, const K* keys, size_t n, int mode, uint64_t admit_below,
                    uint64_t* idx, hipStream_t s) {
  uint32_t* w[4] = {nullptr, nullptr, nullptr, nullptr};
  if (mode >= kLruInsert)
    for (int a = 0; a < 4; a++) w[a] = h->ws + a * h->ws_n;
  if (sizeof(K) != 8) w[2] = nullptr;
  auto kernel = mode >= kLruInsert && admit_below < kLruAdmitAll ? lru_find_kernel<K, true>
                                                                  : lru_find_kernel<K, false>;
  // (a probe comes before its call is numbered)
  const uint64_t t = mode == kLruProbe ? h->t + 1 : h->t;
  hipLaunchKernelGGL(kernel, dim3(lru_blocks(n)), dim3(kLruBlock), 0, s, h->T, keys, n, mode, t,
                     idx, w[0], w[1], w[2], w[3], admit_below, h->counters);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

// what lru_find_kernel(kLruInsert / kLruProbe) left in ws, in (bucket, key) order by three stable
// passes: key low word, key high word, bucket.  *buckets = the buckets in sorted order, *positions
// = the positions
template <typename K>
int lru_sort_missing(hctr_lru* h, size_t n, hipStream_t s, uint32_t** buckets,
                     uint32_t** positions) {
  const size_t m = h->ws_n;
  uint32_t *bkt = h->ws, *klo = h->ws + m, *khi = h->ws + 2 * m, *seq = h->ws + 3 * m,
           *g = h->ws + 4 * m, *tk = h->ws + 5 * m, *pa = h->ws + 6 * m, *pb = h->ws + 7 * m;
  HCTR_TRY(radix_sort_pairs_u32(h->sort_temp, h->sort_temp_bytes, klo, tk, seq, pa, n, 32, s));
  if (sizeof(K) == 8) {
    hipLaunchKernelGGL(lru_permute_kernel, dim3(lru_blocks(n)), dim3(kLruBlock), 0, s, khi, pa, n,
                       g);
    HCTR_LAUNCH_CHECK();
    HCTR_TRY(radix_sort_pairs_u32(h->sort_temp, h->sort_temp_bytes, g, tk, pa, pb, n, 32, s));
    std::swap(pa, pb);
  }
  hipLaunchKernelGGL(lru_permute_kernel, dim3(lru_blocks(n)), dim3(kLruBlock), 0, s, bkt, pa, n, g);
  HCTR_LAUNCH_CHECK();
  int end_bit = 1;
  while (end_bit < 32 && ((uint64_t)1 << end_bit) <= h->T.nb) end_bit++;
  HCTR_TRY(radix_sort_pairs_u32(h->sort_temp, h->sort_temp_bytes, g, tk, pa, pb, n, end_bit, s));
  *buckets = tk;
  *positions = pb;
  return HCTR_OK;
}

// what a new capacity needs, freed again unless the table took it over
struct LruGrown {
  uint64_t *keys = nullptr, *scores = nullptr;
  uint8_t* digests = nullptr;
  float* hbm[3] = {nullptr, nullptr, nullptr};   // rows, state 0, state 1
  void* host[3] = {nullptr, nullptr, nullptr};   // their pinned host parts
  float* host_dev[3] = {nullptr, nullptr, nullptr};
  uint32_t *rng = nullptr, *evict_cnt = nullptr, *evict_off = nullptr, *list = nullptr;
  unsigned long long* tile_sums = nullptr;
  ~LruGrown() {
    void* dev[] = {keys, scores, digests, hbm[0], hbm[1], hbm[2], rng, evict_cnt, evict_off, list,
                   tile_sums};
    for (void* p : dev)
      if (p) (void)hipFree(p);
    for (void* p : host)
      if (p) (void)hipHostFree(p);
  }
};

// The table grows from C to C2 = C * 2^k slots in one step.  Arrays of the final size are
// allocated beside the current ones (if that fails the table is as it was), the current contents
// become their first C slots, and k passes of lru_split_kernel + lru_move_kernel, each doubling
// the bucket count, run inside them.  H becomes min(C2, Hb): slots the table had stay in their
// tier (there was no host part yet, or H = Hb already), a key that moves lands in its new slot's.
// occ = the occupied slots, which bound the moves of a pass.  Synchronises the stream.
template <typename K>
int lru_double(hctr_lru* h, uint64_t C2, size_t occ, hipStream_t s) {
  LruTbl& T = h->T;
  const uint64_t C = T.C, H = T.H, S = (uint64_t)T.S, nb2 = C2 / S;
  const uint64_t H2 = C2 < h->Hb ? C2 : h->Hb;
  const bool tier2 = H2 < C2;
  const size_t rb = h->row_bytes();
  // HBM rows of the row store, and of a state (untiered: its C slots; tiered: the rows' shape)
  const size_t hbm_rows[3] = {(size_t)H2 + h->scratch, tier2 ? (size_t)H2 + h->scratch : (size_t)C2,
                              tier2 ? (size_t)H2 + h->scratch : (size_t)C2};
  float* const cur[3] = {T.rows, T.st[0], T.st[1]};
  LruGrown g;
  bool ok = true;
  auto dev = [&](auto** p, size_t bytes) {
    if (ok) ok = hipMalloc(p, bytes) == hipSuccess;
  };
  dev(&g.keys, C2 * 8);
  dev(&g.scores, C2 * 8);
  dev(&g.digests, C2);
  dev(&g.rng, 2 * nb2 * sizeof(uint32_t));
  dev(&g.evict_cnt, nb2 * sizeof(uint32_t));
  dev(&g.evict_off, (nb2 + 1) * sizeof(uint32_t));
  dev(&g.tile_sums, (nb2 / 1024 + 2) * 8);
  dev(&g.list, (C2 / 2) * 2 * sizeof(uint32_t));  // the last pass moves at most C2 / 2 keys
  for (int a = 0; a < 3; a++) {
    if (!cur[a]) continue;
    dev(&g.hbm[a], hbm_rows[a] * rb);
    if (ok && tier2)
      ok = hipHostMalloc(&g.host[a], (C2 - H2) * rb, hipHostMallocMapped | hipHostMallocPortable) ==
               hipSuccess &&
           hipHostGetDevicePointer((void**)&g.host_dev[a], g.host[a], 0) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    set_error("hctr_lru: out of memory growing the table from " + std::to_string(C) + " to " +
              std::to_string(C2) + " slots");
    return HCTR_ERR_HIP;
  }
  HCTR_HIP(hipMemcpyAsync(g.keys, T.keys, C * 8, hipMemcpyDeviceToDevice, s));
  HCTR_HIP(hipMemcpyAsync(g.scores, T.scores, C * 8, hipMemcpyDeviceToDevice, s));
  HCTR_HIP(hipMemcpyAsync(g.digests, T.digests, C, hipMemcpyDeviceToDevice, s));
  HCTR_HIP(hipMemsetAsync(g.digests + C, 0, C2 - C, s));
  hipLaunchKernelGGL(lru_clear_kernel, dim3(lru_blocks(C2 - C)), dim3(kLruBlock), 0, s, g.keys + C,
                     g.scores + C, (size_t)(C2 - C));
  HCTR_LAUNCH_CHECK();
  for (int a = 0; a < 3; a++) {
    if (!cur[a]) continue;
    if (H) HCTR_HIP(hipMemcpyAsync(g.hbm[a], cur[a], H * rb, hipMemcpyDeviceToDevice, s));
    HCTR_HIP(hipMemsetAsync(g.hbm[a] + H * (size_t)T.D, 0, (hbm_rows[a] - H) * rb, s));
  }
  HCTR_HIP(hipStreamSynchronize(s));  // the host parts are copied by the host
  for (int a = 0; a < 3; a++) {
    if (!g.host[a]) continue;
    memset(g.host[a], 0, (C2 - H2) * rb);
    if (H < C) memcpy(g.host[a], h->host_alloc[a], (C - H) * rb);
  }
  // the table takes the new arrays over; g keeps the old ones until the passes are done
  std::swap(T.keys, g.keys);
  std::swap(T.scores, g.scores);
  std::swap(T.digests, g.digests);
  std::swap(T.rows, g.hbm[0]);
  std::swap(T.st[0], g.hbm[1]);
  std::swap(T.st[1], g.hbm[2]);
  std::swap(h->rng, g.rng);
  std::swap(h->evict_cnt, g.evict_cnt);
  std::swap(h->evict_off, g.evict_off);
  std::swap(h->tile_sums, g.tile_sums);
  for (int a = 0; a < 3; a++) std::swap(h->host_alloc[a], g.host[a]);
  T.hrows = g.host_dev[0];
  T.hst[0] = g.host_dev[1];
  T.hst[1] = g.host_dev[2];
  T.H = H2;
  const int gl = lru_group_lanes(T.D);
  for (uint64_t c = C; c < C2; c *= 2, h->doublings++) {
    T.C = c;
    T.nb = c / S;
    if (occ == 0) continue;
    HCTR_HIP(hipMemsetAsync(h->d_total, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(lru_split_kernel<K>,
                       dim3((int)ceil_div<size_t>(T.nb, (size_t)kLruWavesPerBlock)),
                       dim3(kLruBlock), 0, s, T, g.list, h->d_total);
    HCTR_LAUNCH_CHECK();
    const size_t pairs = occ < c ? occ : (size_t)c;
    hipLaunchKernelGGL(lru_move_kernel, dim3(lru_blocks(pairs * (size_t)gl)), dim3(kLruBlock), 0, s,
                       T, g.list, h->d_total, pairs, gl);
    HCTR_LAUNCH_CHECK();
  }
  T.C = C2;
  T.nb = nb2;
  if (T.init_mode == 0 && !tier2) {
    // the one per-call row of a constant initializer follows the slots
    hipLaunchKernelGGL(lru_fill_kernel, dim3(lru_blocks((size_t)T.D)), dim3(kLruBlock), 0, s,
                       T.rows + C2 * (size_t)T.D, (size_t)T.D, T.init_val);
    HCTR_LAUNCH_CHECK();
  }
  HCTR_HIP(hipStreamSynchronize(s));  // before g frees the old arrays and the list
  return HCTR_OK;
}

// Below Cmax an inserting call first counts its distinct new keys m (a probe: find, sort, count;
// nothing is written to the table) and reads (occ, m) back -- one host synchronisation -- then
// doubles C while C < Cmax and occ + m > L * C.  *sorted: the table did not grow, so the sort still
// stands for the call itself.
template <typename K>
int lru_grow_for_call(hctr_lru* h, const K* keys, size_t n, uint64_t admit_below, uint64_t* idx,
                      uint32_t** tk, uint32_t** pb, bool* sorted, hipStream_t s) {
  HCTR_HIP(hipMemsetAsync(h->counters + 3, 0, sizeof(unsigned long long), s));
  HCTR_TRY(lru_launch_find(h, keys, n, kLruProbe, admit_below, idx, s));
  HCTR_TRY(lru_sort_missing<K>(h, n, s, tk, pb));
  const int wb = (int)ceil_div<size_t>(h->T.nb, (size_t)kLruWavesPerBlock);
  hipLaunchKernelGGL(lru_count_kernel<K>, dim3(wb), dim3(kLruBlock), 0, s, h->T, keys, *tk, *pb,
                     (uint32_t)n, h->t + 1, h->rng, h->evict_cnt, h->counters + 3);
  HCTR_LAUNCH_CHECK();
  HCTR_HIP(hipMemcpyAsync(h->h_word, h->counters, 4 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, s));
  HCTR_HIP(hipStreamSynchronize(s));
  const uint64_t occ = h->h_word[0], m = h->h_word[3];
  uint64_t C2 = h->T.C;
  while (C2 < h->Cmax && (double)(occ + m) > h->L * (double)C2) C2 *= 2;
  *sorted = C2 == h->T.C;
  if (*sorted) return HCTR_OK;
  HCTR_TRY(lru_double<K>(h, C2, (size_t)occ, s));
  return lru_reserve(h, n, s);  // a table that has become tiered needs a per-call row per key
}

template <typename K>
int lru_lookup(hctr_lru* h, const K* keys, size_t n, int insert, uint64_t admit_below,
               uint64_t* row_index, void* ev_keys, float* ev_rows, size_t* n_evicted,
               hipStream_t s) {
  HCTR_TRY(lru_reserve(h, n, s));
  if (n_evicted) *n_evicted = 0;
  uint32_t *tk = nullptr, *pb = nullptr;
  bool sorted = false;
  if (insert && h->T.C < h->Cmax)
    HCTR_TRY(lru_grow_for_call(h, keys, n, admit_below, row_index, &tk, &pb, &sorted, s));
  // tiered: the find / insert kernels write slots to ws_rows, lru_stage_kernel the rows
  uint64_t* const slot_out = h->tiered() ? h->ws_rows : row_index;
  if (!insert) {
    HCTR_TRY(lru_launch_find(h, keys, n, h->tiered() ? kLruFind : kLruRead, kLruAdmitAll, slot_out,
                             s));
  } else {
    const uint64_t t = ++h->t;
    HCTR_TRY(lru_launch_find(h, keys, n, kLruInsert, admit_below, slot_out, s));
    // tk = buckets in sorted order, pb = positions
    if (!sorted) HCTR_TRY(lru_sort_missing<K>(h, n, s, &tk, &pb));
    const int wb = (int)ceil_div<size_t>(h->T.nb, (size_t)kLruWavesPerBlock);
    hipLaunchKernelGGL(lru_count_kernel<K>, dim3(wb), dim3(kLruBlock), 0, s, h->T, keys, tk, pb,
                       (uint32_t)n, t, h->rng, h->evict_cnt, (unsigned long long*)nullptr);
    HCTR_LAUNCH_CHECK();
    HCTR_TRY(exclusive_scan_to_offsets<uint32_t>(h->evict_cnt, h->T.nb, h->tile_sums, h->d_total,
                                                 h->evict_off, s));
    auto kernel = h->tiered() ? lru_insert_kernel<K, true> : lru_insert_kernel<K, false>;
    hipLaunchKernelGGL(kernel, dim3(wb), dim3(kLruBlock), 0, s, h->T, keys, pb, h->rng,
                       h->evict_off, t, slot_out, ev_keys, (int)sizeof(K), ev_rows, h->counters);
    HCTR_LAUNCH_CHECK();
  }
  if (h->tiered()) {
    const int gl = lru_group_lanes(h->T.D);
    hipLaunchKernelGGL(lru_stage_kernel<K>, dim3(lru_blocks(n * (size_t)gl)), dim3(kLruBlock), 0, s,
                       h->T, keys, n, gl, slot_out, row_index);
    HCTR_LAUNCH_CHECK();
  }
  if (insert && n_evicted) HCTR_TRY(lru_read_word(h, h->d_total, s, n_evicted));
  return HCTR_OK;
}

// the checks and the empty call shared by hctr_lru_lookup_index and _filtered
int lru_lookup_checked(hctr_lru* h, const void* keys, size_t n, int insert, uint64_t admit_below,
                       uint64_t* row_index, void* evict_keys, float* evict_rows, size_t* n_evicted,
                       hctr_stream_t stream) {
  HCTR_REQUIRE(h, "null handle");
  HCTR_REQUIRE(n <= ((size_t)1 << 24), "at most 2^24 keys per call");
  HCTR_REQUIRE(n == 0 || (keys && row_index), "keys / row_index are null");
  HCTR_REQUIRE(!evict_rows || evict_keys, "evict_rows needs evict_keys");
  HCTR_REQUIRE(admit_below <= kLruAdmitAll, "admit_below must be in [0, 2^32]");
  if (n == 0) {
    if (n_evicted) *n_evicted = 0;
    if (insert) h->t++;
    return HCTR_OK;
  }
  return lru_with_keys(h, keys, [&](auto* k) {
    return lru_lookup(h, k, n, insert, admit_below, row_index, evict_keys, evict_rows, n_evicted,
                      as_stream(stream));
  });
}

// device buffers of one call, freed on every return path
struct LruTemps {
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  ~LruTemps() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  template <typename T>
  int alloc(T** out, size_t bytes) {
    HCTR_HIP(hipMalloc(out, bytes));
    p[n++] = *out;
    return HCTR_OK;
  }
};

// occupied slots with score >= min_score in slot order; *total = how many there are, the first
// min(total, max_keys) of them are written
int lru_export(hctr_lru* h, uint64_t min_score, void* keys, uint64_t* slots, uint64_t* scores,
               float* rows, size_t max_keys, size_t* exported, size_t* total, hipStream_t s) {
  const LruTbl& T = h->T;
  const size_t C = T.C;
  LruTemps tmp;
  uint32_t *flag = nullptr, *off = nullptr;
  unsigned long long* tiles = nullptr;
  HCTR_TRY(tmp.alloc(&flag, C * 4));
  HCTR_TRY(tmp.alloc(&off, (C + 1) * 4));
  HCTR_TRY(tmp.alloc(&tiles, (C / 1024 + 2) * 8));
  if (rows && !slots) HCTR_TRY(tmp.alloc(&slots, (max_keys ? max_keys : 1) * 8));
  hipLaunchKernelGGL(lru_occupied_kernel, dim3(lru_blocks(C)), dim3(kLruBlock), 0, s, T.keys,
                     T.scores, C, min_score, flag);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(exclusive_scan_to_offsets<uint32_t>(flag, C, tiles, h->d_total, off, s));
  hipLaunchKernelGGL(lru_export_kernel, dim3(lru_blocks(C)), dim3(kLruBlock), 0, s, T.keys, C, off,
                     T.scores, min_score, max_keys, h->key_bytes(), keys, slots, scores);
  HCTR_LAUNCH_CHECK();
  size_t matched = 0;
  HCTR_TRY(lru_read_word(h, h->d_total, s, &matched));
  const size_t got = matched < max_keys ? matched : max_keys;
  if (rows && got) {
    hipLaunchKernelGGL(lru_slot_io_kernel, dim3(lru_blocks(got * (size_t)T.D)), dim3(kLruBlock), 0,
                       s, T.rows, T.hrows, T.H, T.C, slots, got, T.D, 0, rows);
    HCTR_LAUNCH_CHECK();
  }
  HCTR_HIP(hipStreamSynchronize(s));  // before the temporaries go
  *exported = got;
  if (total) *total = matched;
  return HCTR_OK;
}

// pinned, device-mapped host memory (as hctr_tiered_create's), zeroed; *dev = its device address
bool lru_host_alloc(hctr_lru* h, int which, size_t bytes, float** dev) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 4, hipHostMallocMapped | hipHostMallocPortable) !=
      hipSuccess)
    return false;
  h->host_alloc[which] = p;
  memset(p, 0, bytes);
  return hipHostGetDevicePointer((void**)dev, p, 0) == hipSuccess;
}

// an array's (HBM part, host part): 0 = rows, 1 + i = state i (null while not allocated)
bool lru_array(hctr_lru* h, int array, float** hbm, float** host) {
  if (array == 0) {
    *hbm = h->T.rows;
    *host = h->T.hrows;
    return true;
  }
  if (array < 1 || array > 2 || !h->T.st[array - 1]) return false;
  *hbm = h->T.st[array - 1];
  *host = h->T.hst[array - 1];
  return true;
}

}  // namespace

extern "C" {

int hctr_lru_create(size_t capacity, size_t bucket_size, int dim, int key_type,
                    const char* initializer, uint64_t seed, hctr_lru** out) {
  return hctr_lru_create_tiered(capacity, bucket_size, dim, key_type, initializer, seed,
                                ~(size_t)0, out);
}

int hctr_lru_create_tiered(size_t capacity, size_t bucket_size, int dim, int key_type,
                           const char* initializer, uint64_t seed, size_t hbm_slots,
                           hctr_lru** out) {
  return hctr_lru_create_growing(capacity, capacity, 0.5f, bucket_size, dim, key_type, initializer,
                                 seed, hbm_slots, out);
}

int hctr_lru_create_growing(size_t init_capacity, size_t max_capacity, float max_load_factor,
                            size_t bucket_size, int dim, int key_type, const char* initializer,
                            uint64_t seed, size_t hbm_slots, hctr_lru** out) {
  const size_t capacity = max_capacity;
  HCTR_REQUIRE(out, "out is null");
  HCTR_REQUIRE(bucket_size > 0 && bucket_size % kWave == 0 &&
                   bucket_size <= (size_t)kWave * kLruMaxSlotsPerLane,
               "bucket_size must be 64, 128, 192 or 256");
  HCTR_REQUIRE(capacity > 0, "capacity");
  HCTR_REQUIRE(dim > 0 && dim <= 16384, "dim out of range (1 .. 16384)");
  HCTR_REQUIRE(key_type == HCTR_KEY_U32 || key_type == HCTR_KEY_I64, "key_type");
  const size_t Cmax = ceil_div(capacity, bucket_size) * bucket_size;
  HCTR_REQUIRE(Cmax < 0xFFFFFFFFull, "capacity must stay below 2^32 slots");
  HCTR_REQUIRE(hbm_slots >= Cmax || hbm_slots % bucket_size == 0,
               "hbm_slots must be a multiple of bucket_size");
  HCTR_REQUIRE(init_capacity > 0, "init_capacity");
  const size_t C = ceil_div(init_capacity, bucket_size) * bucket_size;
  size_t reach = C;
  while (reach < Cmax) reach *= 2;
  HCTR_REQUIRE(reach == Cmax, "max_capacity (" + std::to_string(max_capacity) +
                                  ") must be init_capacity (" + std::to_string(init_capacity) +
                                  ") times a power of two, both in whole buckets of " +
                                  std::to_string(bucket_size) + " slots");
  HCTR_REQUIRE(max_load_factor > 0.f && max_load_factor <= 1.f,
               "max_load_factor must be in (0, 1]");
  hctr_lru* h = new hctr_lru();
  LruTbl& T = h->T;
  T.C = C;
  h->Cmax = Cmax;
  h->Hb = hbm_slots < Cmax ? hbm_slots : Cmax;
  h->L = (double)max_load_factor;
  T.H = hbm_slots < C ? hbm_slots : C;
  T.S = (int)bucket_size;
  T.nb = C / bucket_size;
  T.D = dim;
  h->key_type = key_type;
  T.seed = seed;
  T.init_mode = 1;
  const std::string ini = initializer ? initializer : "";
  if (ini == "ones") {
    T.init_mode = 0;
    T.init_val = 1.f;
  } else if (ini == "zeros") {
    T.init_mode = 0;
    T.init_val = 0.f;
  } else {
    char* end = nullptr;
    const float v = ini.empty() ? 0.f : strtof(ini.c_str(), &end);
    if (!ini.empty() && end && *end == '\0') {
      T.init_mode = 0;
      T.init_val = v;
    }
  }
  h->scratch = 1;  // a constant initializer needs one row; others grow it to the largest call
  const size_t hbm_bytes = (T.H + h->scratch) * h->row_bytes();
  bool ok = hipMalloc(&T.keys, C * 8) == hipSuccess &&
            hipMalloc(&T.scores, C * 8) == hipSuccess &&
            hipMalloc(&T.digests, C) == hipSuccess &&
            hipMalloc(&T.rows, hbm_bytes) == hipSuccess &&
            hipMalloc(&h->counters, 4 * sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc(&h->rng, 2 * T.nb * sizeof(uint32_t)) == hipSuccess &&
            hipMalloc(&h->evict_cnt, T.nb * sizeof(uint32_t)) == hipSuccess &&
            hipMalloc(&h->evict_off, (T.nb + 1) * sizeof(uint32_t)) == hipSuccess &&
            hipMalloc(&h->tile_sums, (T.nb / 1024 + 2) * 8) == hipSuccess &&
            hipMalloc(&h->d_total, sizeof(unsigned long long)) == hipSuccess &&
            hipHostMalloc(&h->h_word, 4 * sizeof(unsigned long long)) == hipSuccess;
  if (ok && h->tiered()) ok = lru_host_alloc(h, 0, (C - T.H) * h->row_bytes(), &T.hrows);
  if (ok)
    ok = hipMemset(T.digests, 0, C) == hipSuccess &&
         hipMemset(T.rows, 0, hbm_bytes) == hipSuccess &&
         hipMemset(h->counters, 0, 4 * sizeof(unsigned long long)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    set_error("hctr_lru_create: out of device memory");
    lru_free(h);
    return HCTR_ERR_HIP;
  }
  hipLaunchKernelGGL(lru_clear_kernel, dim3(lru_blocks(C)), dim3(kLruBlock), 0, 0, T.keys,
                     T.scores, C);
  if (T.init_mode == 0 && !h->tiered())
    hipLaunchKernelGGL(lru_fill_kernel, dim3(lru_blocks((size_t)dim)), dim3(kLruBlock), 0, 0,
                       T.rows + C * (size_t)dim, (size_t)dim, T.init_val);
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) {
    set_error("hctr_lru_create: initialisation failed");
    lru_free(h);
    return HCTR_ERR_HIP;
  }
  *out = h;
  return HCTR_OK;
}

int hctr_lru_destroy(hctr_lru* h) {
  if (!h) return HCTR_OK;
  (void)hipDeviceSynchronize();
  lru_free(h);
  return HCTR_OK;
}

int hctr_lru_lookup_index(hctr_lru* h, const void* keys, size_t n, int insert, uint64_t* row_index,
                          void* evict_keys, float* evict_rows, size_t* n_evicted,
                          hctr_stream_t stream) {
  return lru_lookup_checked(h, keys, n, insert, kLruAdmitAll, row_index, evict_keys, evict_rows,
                            n_evicted, stream);
}

int hctr_lru_lookup_index_filtered(hctr_lru* h, const void* keys, size_t n, uint64_t admit_below,
                                   uint64_t* row_index, void* evict_keys, float* evict_rows,
                                   size_t* n_evicted, hctr_stream_t stream) {
  return lru_lookup_checked(h, keys, n, 1, admit_below, row_index, evict_keys, evict_rows,
                            n_evicted, stream);
}

int hctr_lru_compact(hctr_lru* h, size_t batch, size_t n, const long long* offsets,
                     const uint64_t* rows, const void* keys, const float* weights,
                     long long* out_offsets, uint64_t* out_rows, void* out_keys,
                     float* out_weights, size_t* n_kept, hctr_stream_t stream) {
  HCTR_REQUIRE(h, "null handle");
  HCTR_REQUIRE(n_kept, "n_kept is null");
  HCTR_REQUIRE(n <= ((size_t)1 << 24), "at most 2^24 keys per call");
  HCTR_REQUIRE(offsets && out_offsets, "offsets / out_offsets are null");
  HCTR_REQUIRE(n == 0 || (rows && keys && out_rows && out_keys), "rows / keys are null");
  HCTR_REQUIRE(!weights || out_weights, "weights need out_weights");
  const hipStream_t s = as_stream(stream);
  HCTR_TRY(lru_reserve(h, n, s));
  uint32_t *keep = h->ws, *pos = h->ws + h->ws_n;  // pos: n + 1 entries
  hipLaunchKernelGGL(lru_keep_kernel, dim3(lru_blocks(n)), dim3(kLruBlock), 0, s, rows, n, keep);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(exclusive_scan_to_offsets<uint32_t>(keep, n, h->ws_tiles, h->d_total, pos, s));
  const size_t m = n > batch + 1 ? n : batch + 1;
  hipLaunchKernelGGL(lru_compact_kernel, dim3(lru_blocks(m)), dim3(kLruBlock), 0, s, batch,
                     offsets, n, rows, keys, h->key_bytes(), weights, pos, out_offsets, out_rows,
                     out_keys, out_weights);
  HCTR_LAUNCH_CHECK();
  return lru_read_word(h, h->d_total, s, n_kept);
}

int hctr_lru_find(hctr_lru* h, const void* keys, size_t n, uint64_t* row_index,
                  hctr_stream_t stream) {
  HCTR_REQUIRE(h, "null handle");
  HCTR_REQUIRE(n == 0 || (keys && row_index), "keys / row_index are null");
  if (n == 0) return HCTR_OK;
  return lru_with_keys(h, keys, [&](auto* k) {
    return lru_launch_find(h, k, n, kLruFind, kLruAdmitAll, row_index, as_stream(stream));
  });
}

int hctr_lru_rows(hctr_lru* h, float** rows, size_t* capacity) {
  HCTR_REQUIRE(h && rows && capacity, "null argument");
  *rows = h->T.rows;
  *capacity = h->T.H;  // = C on an untiered table
  return HCTR_OK;
}

int hctr_lru_state(hctr_lru* h, int i, float** state, hctr_stream_t stream) {
  HCTR_REQUIRE(h && state, "null argument");
  HCTR_REQUIRE(i == 0 || i == 1, "state index must be 0 or 1");
  LruTbl& T = h->T;
  if (!T.st[i]) {
    // tiered: the HBM part has the rows' shape (H slots + the per-call rows), the rest is host
    // memory; untiered: the C slots
    const size_t bytes = (h->tiered() ? T.H + h->scratch : T.C) * h->row_bytes();
    HCTR_HIP(hipMalloc(&T.st[i], bytes));
    HCTR_HIP(hipMemsetAsync(T.st[i], 0, bytes, as_stream(stream)));
    if (h->tiered() && !lru_host_alloc(h, 1 + i, (T.C - T.H) * h->row_bytes(), &T.hst[i])) {
      (void)hipGetLastError();
      set_error("hctr_lru_state: host allocation failed");
      return HCTR_ERR_HIP;
    }
  }
  *state = T.st[i];
  return HCTR_OK;
}

int hctr_lru_export(hctr_lru* h, void* keys, uint64_t* slots, uint64_t* scores, float* rows,
                    size_t max_keys, size_t* exported, hctr_stream_t stream) {
  HCTR_REQUIRE(h && exported, "null argument");
  return lru_export(h, 0, keys, slots, scores, rows, max_keys, exported, nullptr,
                    as_stream(stream));
}

int hctr_lru_export_if(hctr_lru* h, uint64_t min_score, void* keys, uint64_t* slots,
                       uint64_t* scores, float* rows, size_t max_keys, size_t* exported,
                       size_t* matched, hctr_stream_t stream) {
  HCTR_REQUIRE(h && exported, "null argument");
  return lru_export(h, min_score, keys, slots, scores, rows, max_keys, exported, matched,
                    as_stream(stream));
}

int hctr_lru_size(hctr_lru* h, size_t* out, hctr_stream_t stream) {
  HCTR_REQUIRE(h && out, "null argument");
  return lru_read_word(h, h->counters + 0, as_stream(stream), out);
}

int hctr_lru_rejected_count(hctr_lru* h, uint64_t* out, hctr_stream_t stream) {
  HCTR_REQUIRE(h && out, "null argument");
  return lru_read_word(h, h->counters + 1, as_stream(stream), out);
}

int hctr_lru_filtered_count(hctr_lru* h, uint64_t* out, hctr_stream_t stream) {
  HCTR_REQUIRE(h && out, "null argument");
  return lru_read_word(h, h->counters + 2, as_stream(stream), out);
}

int hctr_lru_placement(const hctr_lru* h, size_t* hbm_slots, size_t* hbm_rows, size_t* host_rows) {
  HCTR_REQUIRE(h && hbm_slots && hbm_rows && host_rows, "null argument");
  *hbm_slots = h->T.H;
  *hbm_rows = h->T.H + h->scratch;
  *host_rows = h->T.C - h->T.H;
  return HCTR_OK;
}

int hctr_lru_host_part(const hctr_lru* h, int array, float** host) {
  HCTR_REQUIRE(h && host, "null argument");
  HCTR_REQUIRE(array >= 0 && array <= 2, "array must be 0 (rows), 1 or 2 (states)");
  *host = array == 0 ? h->T.hrows : h->T.hst[array - 1];
  return HCTR_OK;
}

static int lru_slot_io(hctr_lru* h, int array, const uint64_t* slots, size_t n, int dir,
                       float* buf, hctr_stream_t stream) {
  HCTR_REQUIRE(h, "null handle");
  HCTR_REQUIRE(n == 0 || (slots && buf), "slots / values are null");
  float *hbm = nullptr, *host = nullptr;
  HCTR_REQUIRE(lru_array(h, array, &hbm, &host),
               "array must be 0 (rows) or 1 + i for an allocated state i");
  if (n == 0) return HCTR_OK;
  hipLaunchKernelGGL(lru_slot_io_kernel, dim3(lru_blocks(n * (size_t)h->T.D)), dim3(kLruBlock), 0,
                     as_stream(stream), hbm, host, h->T.H, h->T.C, slots, n, h->T.D, dir, buf);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_lru_gather_slots(hctr_lru* h, int array, const uint64_t* slots, size_t n, float* out,
                          hctr_stream_t stream) {
  return lru_slot_io(h, array, slots, n, 0, out, stream);
}

int hctr_lru_scatter_slots(hctr_lru* h, int array, const uint64_t* slots, size_t n,
                           const float* values, int add, hctr_stream_t stream) {
  return lru_slot_io(h, array, slots, n, add ? 2 : 1, const_cast<float*>(values), stream);
}

int hctr_lru_apply_update(hctr_lru* h, hctr_updater* u, size_t buckets, size_t nnz,
                          const int64_t* bucket_range, const uint64_t* slots, const void* grad,
                          int grad_dtype, int optimizer, float lr, float beta1, float beta2,
                          float epsilon, float momentum_factor, float scaler, uint64_t times,
                          hctr_stream_t stream) {
  HCTR_REQUIRE(h && u, "null handle");
  HCTR_REQUIRE(nnz <= ((size_t)1 << 24), "at most 2^24 keys per call");
  HCTR_REQUIRE(nnz == 0 || slots, "slots are null");
  const LruTbl& T = h->T;
  const int ns = optimizer == HCTR_OPT_ADAM ? 2 : (optimizer == HCTR_OPT_SGD ? 0 : 1);
  HCTR_REQUIRE((ns < 1 || T.st[0]) && (ns < 2 || T.st[1]),
               "the optimizer's states are not allocated (hctr_lru_state)");
  if (!h->tiered() || nnz == 0)
    return hctr_updater_update(u, buckets, nnz, bucket_range, slots, grad, grad_dtype, optimizer,
                               HCTR_UPDATE_LOCAL, lr, beta1, beta2, epsilon, momentum_factor,
                               scaler, times, T.rows, T.st[0], T.st[1], stream);
  const hipStream_t s = as_stream(stream);
  HCTR_TRY(lru_reserve(h, nnz + 1, s));
  const size_t m = h->ws_n;
  uint32_t *ka = h->ws, *kb = h->ws + m, *va = h->ws + 2 * m, *vb = h->ws + 3 * m,
           *first = h->ws + 4 * m, *off = h->ws + 5 * m;
  const uint64_t host_slots = T.C - T.H;
  hipLaunchKernelGGL(lru_step_keys_kernel, dim3(lru_blocks(nnz)), dim3(kLruBlock), 0, s, slots,
                     nnz, T.H, T.C, ka, va, h->ws_rows);
  HCTR_LAUNCH_CHECK();
  // host slots in ascending order (stable: positions of one slot keep their order)
  int end_bit = 1;
  while (end_bit < 32 && ((uint64_t)1 << end_bit) <= host_slots) end_bit++;
  HCTR_TRY(radix_sort_pairs_u32(h->sort_temp, h->sort_temp_bytes, ka, kb, va, vb, nnz, end_bit, s));
  hipLaunchKernelGGL(lru_step_first_kernel, dim3(lru_blocks(nnz)), dim3(kLruBlock), 0, s, kb, nnz,
                     (uint32_t)host_slots, first);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(exclusive_scan_to_offsets<uint32_t>(first, nnz, h->ws_tiles, h->d_total, off, s));
  const int gl = lru_group_lanes(T.D);
  const int blocks = lru_blocks(nnz * (size_t)gl);
  hipLaunchKernelGGL(lru_step_stage_kernel<true>, dim3(blocks), dim3(kLruBlock), 0, s, T, kb, vb,
                     first, off, nnz, gl, h->ws_rows);
  HCTR_LAUNCH_CHECK();
  HCTR_TRY(hctr_updater_update(u, buckets, nnz, bucket_range, h->ws_rows, grad, grad_dtype,
                               optimizer, HCTR_UPDATE_LOCAL, lr, beta1, beta2, epsilon,
                               momentum_factor, scaler, times, T.rows, T.st[0], T.st[1], stream));
  hipLaunchKernelGGL(lru_step_stage_kernel<false>, dim3(blocks), dim3(kLruBlock), 0, s, T, kb, vb,
                     first, off, nnz, gl, h->ws_rows);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int hctr_lru_capacity(const hctr_lru* h, size_t* capacity, size_t* bucket_size) {
  HCTR_REQUIRE(h && capacity && bucket_size, "null argument");
  *capacity = h->Cmax;  // the bound size can reach; hctr_lru_growth tells the capacity now
  *bucket_size = (size_t)h->T.S;
  return HCTR_OK;
}

int hctr_lru_growth(const hctr_lru* h, size_t* capacity_now, size_t* capacity_max,
                    uint64_t* doublings) {
  HCTR_REQUIRE(h && capacity_now && capacity_max && doublings, "null argument");
  *capacity_now = h->T.C;
  *capacity_max = h->Cmax;
  *doublings = h->doublings;
  return HCTR_OK;
}

}  // extern "C"
