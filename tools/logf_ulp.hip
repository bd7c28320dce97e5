// logf_ulp.hip -- how far the two candidate forms of the Raw reader's integer-dense transform
// (csrc/raw_decode.hip, HCTR_RAW_LOG1P) land from the correctly rounded value on gfx950:
//
//   a) logf(x + 1.f)                       the reference's expression (split_batch.cu:35)
//   b) (float)log((double)(x + 1.f))       the form the kernel uses
//
// against float32(log(float64(float32(x) + float32(1)))) computed on the host (glibc's log is
// within 1 ulp of fp64, far below a float's half ulp except at near-ties), for every integer
// x in [0, 2^22) and for 2^22 words spread over [2^22, 2^31).  Prints one histogram of ulp
// distances per form.  Built with the library's flags:
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/logf_ulp.hip -o tools/logf_ulp
//   tools/logf_ulp > profiles/raw_decode_logf.txt
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

__global__ void both_forms(const int32_t* __restrict__ x, float* __restrict__ a,
                           float* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = (float)x[i] + 1.f;
  a[i] = logf(v);
  b[i] = (float)log((double)v);
}

#define CHECK(e)                                                        \
  do {                                                                  \
    hipError_t s_ = (e);                                                \
    if (s_ != hipSuccess) {                                             \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(s_));           \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int64_t bits(float f) {
  int32_t i;
  memcpy(&i, &f, 4);
  return i;
}

int main() {
  const size_t n_low = (size_t)1 << 22, n = 2 * n_low;
  std::vector<int32_t> x(n);
  for (size_t i = 0; i < n_low; i++) x[i] = (int32_t)i;
  const uint64_t span = ((uint64_t)1 << 31) - 1 - n_low;  // the last word is 2^31 - 1
  for (size_t i = 0; i < n_low; i++) x[n_low + i] = (int32_t)(n_low + (i * span) / (n_low - 1));
  int32_t* dx;
  float *da, *db;
  CHECK(hipMalloc(&dx, n * 4));
  CHECK(hipMalloc(&da, n * 4));
  CHECK(hipMalloc(&db, n * 4));
  CHECK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(both_forms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, da, db, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> a(n), b(n);
  CHECK(hipMemcpy(a.data(), da, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(b.data(), db, n * 4, hipMemcpyDeviceToHost));
  long ha[4] = {0, 0, 0, 0}, hb[4] = {0, 0, 0, 0};
  bool cls = true;
  for (size_t i = 0; i < n; i++) {
    const float v = (float)x[i] + 1.f;
    const float ref = (float)std::log((double)v);
    if (std::isfinite(ref) != std::isfinite(a[i]) || std::isfinite(ref) != std::isfinite(b[i]))
      cls = false;
    if (!std::isfinite(ref)) continue;
    int64_t d = bits(a[i]) - bits(ref);
    ha[d < 0 ? (-d > 3 ? 3 : -d) : (d > 3 ? 3 : d)]++;
    d = bits(b[i]) - bits(ref);
    hb[d < 0 ? (-d > 3 ? 3 : -d) : (d > 3 ? 3 : d)]++;
  }
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  printf("device %s (%s), %zu words: x in [0, 2^22) and 2^22 words over [2^22, 2^31 - 1]; "
         "x = 2^31 - 1 included: %s\n", p.name, p.gcnArchName, n,
         x[n - 1] == 2147483647 ? "yes" : "no");
  printf("ulp distance from float32(log(float64(float32(x) + 1))):      0        1        2      >=3\n");
  printf("  logf(x + 1.f)                                       %9ld %8ld %8ld %8ld\n", ha[0], ha[1],
         ha[2], ha[3]);
  printf("  (float)log((double)(x + 1.f))                       %9ld %8ld %8ld %8ld\n", hb[0], hb[1],
         hb[2], hb[3]);
  printf("finite / inf / nan class equal to the host's on every word: %s\n", cls ? "yes" : "NO");
  return 0;
}
