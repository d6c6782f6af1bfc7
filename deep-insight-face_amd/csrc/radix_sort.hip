// The stable LSD radix sort of (key, position) pairs on 8-bit digits that the frame-level features share, and its scan
// (declared in dif_internal.hpp).  Template pooling sorts 64-bit labels under a plan (csrc/templates.hip), detector
// evaluation 32-bit score keys without one (csrc/deteval.hip).
//   radix_hist_kernel     } one pass: a histogram per block of kSortTile keys, an exclusive scan over [digit][block] by one
//   block_scan_kernel     } block, and a scatter that ranks every key among the equal digits in front of it in its block
//   radix_scatter_kernel  } (ballots inside a wave, per-wave counters across the waves)
// A pass reads the pair of buffers (k0, p0) or (k1, p1) and writes the other.  With a RadixPlan in device memory a pass whose
// digit is constant returns at once and the source buffer is the plan's: every pass can be enqueued before the keys are
// known.  With a null plan every pass runs and pass b reads buffer b & 1, so an even number of passes ends in (k0, p0).
// The only atomics are LDS counters whose totals do not depend on the order: the result is a function of the input alone.
#include "dif_internal.hpp"

namespace dif {

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortItems = 8;                               // keys per thread and pass: a wave's share is kSortItems * 64
constexpr int kSortTile = kSortThreads * kSortItems;        // keys per block and pass
static_assert(kSortTile == kRadixSortTile, "dif_internal.hpp states the tile for the callers");
constexpr int kScanThreads = 1024;

__device__ __forceinline__ bool radix_skips(const RadixPlan* __restrict__ plan, int pass) { return plan && !plan->active[pass]; }
__device__ __forceinline__ int radix_source(const RadixPlan* __restrict__ plan, int pass) { return plan ? plan->src[pass] : pass & 1; }

template <typename K>
__global__ __launch_bounds__(kSortThreads) void radix_hist_kernel(const RadixPlan* __restrict__ plan, int pass, const K* __restrict__ k0,
                                                                  const K* __restrict__ k1, int m, int nb, unsigned* __restrict__ hist) {
  if (radix_skips(plan, pass)) return;
  const K* __restrict__ keys = radix_source(plan, pass) ? k1 : k0;
  __shared__ unsigned h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const int64_t i = base + r * kSortThreads + tid;
    if (i < m) atomicAdd(&h[(unsigned)(keys[i] >> (8 * pass)) & 255u], 1u);
  }
  __syncthreads();
  hist[(int64_t)tid * nb + blockIdx.x] = h[tid];
}

// exclusive scan of data[0 .. E) in place, by ONE block: a thread sums a contiguous share, the shares are scanned across
// the block, and the thread rewrites its share.  `active` (or null): a skipped pass has nothing to scan.
__global__ __launch_bounds__(kScanThreads) void block_scan_kernel(const int* __restrict__ active, unsigned* __restrict__ data, int64_t E) {
  if (active && !*active) return;
  __shared__ unsigned wave_total[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t per = (E + kScanThreads - 1) / kScanThreads;
  const int64_t lo = tid * per < E ? tid * per : E, hi = lo + per < E ? lo + per : E;
  unsigned s = 0;
  for (int64_t i = lo; i < hi; ++i) s += data[i];
  unsigned inc = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned v = __shfl_up(inc, off);
    if (lane >= off) inc += v;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  unsigned run = inc - s;
  for (int w = 0; w < wave; ++w) run += wave_total[w];
  for (int64_t i = lo; i < hi; ++i) {
    const unsigned v = data[i];
    data[i] = run;
    run += v;
  }
}

// Key i of the block's tile goes to hist[digit][block] (keys with a smaller digit, and keys with this digit in the blocks
// in front) + the keys with this digit in front of it in the tile.  Tile order: wave w holds keys [w * 512, (w + 1) * 512)
// of the tile, round r of the wave keys [r * 64, (r + 1) * 64) of those, lane by lane.
template <typename K>
__global__ __launch_bounds__(kSortThreads) void radix_scatter_kernel(const RadixPlan* __restrict__ plan, int pass, K* __restrict__ k0,
                                                                     K* __restrict__ k1, int* __restrict__ p0, int* __restrict__ p1, int m,
                                                                     int nb, const unsigned* __restrict__ hist) {
  if (radix_skips(plan, pass)) return;
  const int src = radix_source(plan, pass);
  const K* kin = src ? k1 : k0;
  K* kout = src ? k0 : k1;
  const int* pin = src ? p1 : p0;
  int* pout = src ? p0 : p1;
  __shared__ unsigned cnt[kSortWaves][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) cnt[w][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile + wave * (kSortItems * 64);
  K key[kSortItems];
  int p[kSortItems];
  unsigned off[kSortItems];
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool valid = i < m;
    key[r] = valid ? kin[i] : (K)0;
    p[r] = valid ? pin[i] : 0;
    const unsigned dg = (unsigned)(key[r] >> (8 * pass)) & 255u;
    unsigned long long same = __ballot(valid);       // the valid lanes of the wave that hold this lane's digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (dg >> bit) & 1u;
      const unsigned long long bal = __ballot(one);
      same &= one ? bal : ~bal;
    }
    const unsigned long long below = same & ((1ull << lane) - 1ull);
    off[r] = valid ? cnt[wave][dg] + (unsigned)__popcll(below) : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0ull) cnt[wave][dg] += (unsigned)__popcll(same);   // one lane per digit: distinct addresses
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __syncthreads();
  {
    unsigned run = hist[(int64_t)tid * nb + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
      const unsigned c = cnt[w][tid];
      cnt[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const int64_t i = base + r * 64 + lane;
    if (i < m) {
      const unsigned dst = cnt[wave][(unsigned)(key[r] >> (8 * pass)) & 255u] + off[r];
      kout[dst] = key[r];
      pout[dst] = p[r];
    }
  }
}

int radix_sort_tile() { return kSortTile; }

size_t radix_sort_hist_bytes(int64_t m) { return (size_t)((m + kSortTile - 1) / kSortTile) * 256 * 4; }

int block_scan_run(unsigned* data, int64_t E, hipStream_t st) {
  hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const int*)nullptr, data, E);
  DIF_HIP(hipGetLastError());
  return 0;
}

template <typename K>
int radix_sort_run(const RadixPlan* plan_dev, int passes, K* k0, K* k1, int* p0, int* p1, int64_t m, unsigned* hist, hipStream_t st) {
  const int nb = (int)((m + kSortTile - 1) / kSortTile);
  for (int pass = 0; pass < passes; ++pass) {
    hipLaunchKernelGGL(radix_hist_kernel<K>, dim3(nb), dim3(kSortThreads), 0, st, plan_dev, pass, k0, k1, (int)m, nb, hist);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, plan_dev ? &plan_dev->active[pass] : nullptr, hist,
                       (int64_t)256 * nb);
    hipLaunchKernelGGL(radix_scatter_kernel<K>, dim3(nb), dim3(kSortThreads), 0, st, plan_dev, pass, k0, k1, p0, p1, (int)m, nb, hist);
  }
  DIF_HIP(hipGetLastError());
  return 0;
}

template int radix_sort_run<unsigned>(const RadixPlan*, int, unsigned*, unsigned*, int*, int*, int64_t, unsigned*, hipStream_t);
template int radix_sort_run<unsigned long long>(const RadixPlan*, int, unsigned long long*, unsigned long long*, int*, int*, int64_t,
                                                unsigned*, hipStream_t);

}  // namespace dif
