// Sharded gallery: the merges of per-shard query results, on the device (dif_shard_merge_topk, dif_shard_merge_topk_ids,
// dif_shard_merge_within, dif_shard_merge_rank; dif_match_merge, the top-1 merge, lives in match.hip).
//
// Every merge takes the R per-shard results of n probes laid out [R][n][...] -- what an all-gather of the ranks' records gives --
// and produces the answer of ONE handle holding all the rows.  Shards hold disjoint sets of global indices; nothing here
// assumes that they are contiguous or come in rank order.  Nothing is read on the host, there are no atomics, every output
// slot is written by exactly one thread: the results are deterministic.
//
//   shard_merge_lists_kernel<BY_DIST>   dif_shard_merge_topk (key (dist, idx)) and dif_shard_merge_within (key idx alone).
//     R sorted lists of L slots, live entries first, padding (idx < 0) behind.  One block per probe, one thread per input
//     element: the element's place in the union is its place in its own list plus, for every other list, the number of that
//     list's entries that precede it -- a binary search.  The element is written when its place is below L.  No sort, no
//     LDS beyond 64 list lengths, any R up to 64.  Keys of different lists never compare equal while shards are disjoint;
//     for overlapping shards the order is still total: equal keys go to the lower rank first.
//   shard_merge_ids_kernel              dif_shard_merge_topk_ids: one entry per label.  The lists are folded one at a time
//     into a k-entry accumulator in LDS (R k entries -- up to 8192 -- would not fit): merge the accumulator and the list by
//     the same ranking (2 k entries), strike every entry that has an earlier entry of its label, keep the first k.
//     Why the fold is the whole answer.  F(S) = "S in (dist, idx) order, each label's first entry, the first k of those".
//     (a) F(F(A) + B) = F(A + B): an entry x of F(A + B) is the best of its label in A + B and fewer than k labels have a
//     better best there; if x is in A the same holds inside A, so x is in F(A); either way x is in F(A) + B, a subset of
//     A + B, where it keeps both properties.  Both sides hold min(k, labels of A + B) entries, so inclusion is equality.
//     (b) The union of the shards' lists gives F of the whole gallery: an identity of the whole-gallery list has its best row in
//     some shard s; every identity ahead of it in s is ahead of it in the whole gallery, so fewer than k are, and it is in s's list
//     at its true distance.  An identity outside the whole-gallery list appears, if at all, at a distance no better than its
//     true one and displaces nothing.
//   shard_merge_rank_kernel             dif_shard_merge_rank: per probe the sum of the shards' counts and the owner's distance.
//     count_r = count(d < dm) + count(d == dm and global row < m) over shard r (dif_match_rank_at); the rows of the shards
//     partition the rows of the gallery, so the counts add up to count(d < dm) + count(d[:m] == dm) over all of it.  With dm NaN
//     every shard reports its size, and the sum is the size of the gallery: dif_match_rank's "behind every row".
//
// Distances in live slots are >= +0 or +inf, never NaN, so the order-preserving integer image of match_within.hip (ord_f32) is
// a valid key; a slot with idx < 0 is padding whatever its distance says.
#include "dif_internal.hpp"

namespace dif {

constexpr int SHARD_MAX = 64;                                 // DIF_SHARD_MAX
constexpr int SHARD_NT = 256;
constexpr int SHARD_KMAX = 128;                               // DIF_TOPK_MAX

// order-preserving integer image of a float that is not NaN (match_within.hip)
__device__ __forceinline__ unsigned ord_f32(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// does entry b come before entry a?  `b_first`: what an exact tie of the whole key answers (b's list is the lower rank)
template <bool BY_DIST>
__device__ __forceinline__ bool shard_before(float db, int64_t ib, float da, int64_t ia, bool b_first) {
  if (BY_DIST) {
    const unsigned ob = ord_f32(db), oa = ord_f32(da);
    if (ob != oa) return ob < oa;
  }
  if (ib != ia) return ib < ia;
  return b_first;
}

template <bool BY_DIST>
__global__ __launch_bounds__(SHARD_NT) void shard_merge_lists_kernel(const int64_t* __restrict__ count,
                                                                    const int64_t* __restrict__ idx,
                                                                    const float* __restrict__ dist, int R, int64_t n, int L,
                                                                    int64_t* __restrict__ count_out,
                                                                    int64_t* __restrict__ idx_out, float* __restrict__ dist_out) {
  __shared__ int s_len[SHARD_MAX];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  if (count_out && tid == 0) {
    int64_t c = 0;
    for (int r = 0; r < R; ++r) c += count[(int64_t)r * n + p];
    count_out[p] = c;
  }
  if (L == 0) return;                                         // counts only (block-uniform)
  if (tid < R) {                                              // live entries of list tid: the first slot with idx < 0
    const int64_t* li = idx + ((int64_t)tid * n + p) * L;
    int lo = 0, hi = L;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (li[mid] >= 0) lo = mid + 1;
      else hi = mid;
    }
    s_len[tid] = lo;
  }
  __syncthreads();
  int64_t total = 0;
  for (int r = 0; r < R; ++r) total += s_len[r];
  if (total > L) total = L;

  const int64_t elems = (int64_t)R * L;
  for (int64_t e = tid; e < elems; e += SHARD_NT) {
    const int r = (int)(e / L), j = (int)(e % L);
    if (j >= s_len[r]) continue;
    const int64_t mine = ((int64_t)r * n + p) * L + j;
    const int64_t ia = idx[mine];
    const float da = BY_DIST ? dist[mine] : 0.f;
    int pos = j;
    for (int r2 = 0; r2 < R && pos < L; ++r2) {
      if (r2 == r) continue;
      const int64_t base = ((int64_t)r2 * n + p) * L;
      int lo = 0, hi = s_len[r2];                             // entries of list r2 that precede mine: a prefix of it
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (shard_before<BY_DIST>(BY_DIST ? dist[base + mid] : 0.f, idx[base + mid], da, ia, r2 < r)) lo = mid + 1;
        else hi = mid;
      }
      pos += lo;
    }
    if (pos < L) {
      idx_out[p * L + pos] = ia;
      dist_out[p * L + pos] = dist[mine];
    }
  }
  for (int64_t i = total + tid; i < L; i += SHARD_NT) {
    idx_out[p * L + i] = -1;
    dist_out[p * L + i] = __builtin_nanf("");
  }
}

// One block per probe.  All control flow is block-uniform: na, nl and the kept total come from barriers' counts and LDS words.
__global__ __launch_bounds__(SHARD_NT) void shard_merge_ids_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                                  const int64_t* __restrict__ label, int R, int64_t n, int k,
                                                                  int64_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                                  int64_t* __restrict__ label_out) {
  static_assert(2 * SHARD_KMAX == SHARD_NT, "one thread per entry of the accumulator and of the list being folded in");
  __shared__ int64_t a_i[SHARD_KMAX], a_l[SHARD_KMAX], l_i[SHARD_KMAX], l_l[SHARD_KMAX], m_i[2 * SHARD_KMAX], m_l[2 * SHARD_KMAX];
  __shared__ float a_d[SHARD_KMAX], l_d[SHARD_KMAX], m_d[2 * SHARD_KMAX];
  __shared__ int s_w[SHARD_NT / 64];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int na = 0;                                                 // entries of the accumulator: ascending, distinct labels
  for (int r = 0; r < R; ++r) {
    const int64_t base = ((int64_t)r * n + p) * k;
    bool live = false;
    if (tid < k) {
      l_i[tid] = idx[base + tid];
      l_d[tid] = dist[base + tid];
      l_l[tid] = label[base + tid];
      live = l_i[tid] >= 0;
    }
    const int nl = __syncthreads_count(live);                 // (padding is at the tail; also the barrier behind the loads)
    if (nl == 0) continue;
    // merge by ranking: accumulator entry t < 128, list entry t - 128; on an exact tie the accumulator (lower ranks) goes first
    if (tid < SHARD_KMAX) {
      if (tid < na) {
        int lo = 0, hi = nl;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (shard_before<true>(l_d[mid], l_i[mid], a_d[tid], a_i[tid], false)) lo = mid + 1;
          else hi = mid;
        }
        m_i[tid + lo] = a_i[tid];
        m_d[tid + lo] = a_d[tid];
        m_l[tid + lo] = a_l[tid];
      }
    } else {
      const int j = tid - SHARD_KMAX;
      if (j < nl) {
        int lo = 0, hi = na;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (shard_before<true>(a_d[mid], a_i[mid], l_d[j], l_i[j], true)) lo = mid + 1;
          else hi = mid;
        }
        m_i[j + lo] = l_i[j];
        m_d[j + lo] = l_d[j];
        m_l[j + lo] = l_l[j];
      }
    }
    __syncthreads();
    const int nm = na + nl;
    bool keep = tid < nm;
    if (keep) {
      const int64_t ml = m_l[tid];
      for (int i = 0; i < tid; ++i)
        if (m_l[i] == ml) {
          keep = false;
          break;
        }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
    for (int w = 0; w < SHARD_NT / 64; ++w) {
      before += w < wave ? s_w[w] : 0;
      kept += s_w[w];
    }
    if (keep && before < k) {
      a_i[before] = m_i[tid];
      a_d[before] = m_d[tid];
      a_l[before] = m_l[tid];
    }
    na = kept < k ? kept : k;
    __syncthreads();                                          // the accumulator is read, l_* and s_w rewritten, by the next fold
  }
  if (tid < k) {
    const bool has = tid < na;
    idx_out[p * k + tid] = has ? a_i[tid] : -1;
    dist_out[p * k + tid] = has ? a_d[tid] : __builtin_nanf("");
    if (label_out) label_out[p * k + tid] = has ? a_l[tid] : -1;
  }
}

__global__ __launch_bounds__(SHARD_NT) void shard_merge_rank_kernel(const int64_t* __restrict__ count,
                                                                   const int64_t* __restrict__ owned,
                                                                   const float* __restrict__ mate_dist, int R, int64_t n,
                                                                   int64_t* __restrict__ rank_out,
                                                                   float* __restrict__ mate_dist_out) {
  const int64_t p = (int64_t)blockIdx.x * SHARD_NT + threadIdx.x;
  if (p >= n) return;
  int64_t sum = 0;
  int owner = -1;                                             // the lowest rank that names the mate its own
  for (int r = 0; r < R; ++r) {
    sum += count[(int64_t)r * n + p];
    if (owner < 0 && owned[(int64_t)r * n + p] != 0) owner = r;
  }
  rank_out[p] = owner < 0 ? -1 : sum;
  if (mate_dist_out) mate_dist_out[p] = owner < 0 ? __builtin_nanf("") : mate_dist[(int64_t)owner * n + p];
}

int shard_merge_lists_run(bool by_dist, const int64_t* count, const int64_t* idx, const float* dist, int R, int n, int L,
                          int64_t* count_out, int64_t* idx_out, float* dist_out, hipStream_t st) {
  if (n <= 0) return 0;
  if (by_dist)
    hipLaunchKernelGGL(shard_merge_lists_kernel<true>, dim3(n), dim3(SHARD_NT), 0, st, count, idx, dist, R, (int64_t)n, L,
                       count_out, idx_out, dist_out);
  else
    hipLaunchKernelGGL(shard_merge_lists_kernel<false>, dim3(n), dim3(SHARD_NT), 0, st, count, idx, dist, R, (int64_t)n, L,
                       count_out, idx_out, dist_out);
  DIF_HIP(hipGetLastError());
  return 0;
}

int shard_merge_ids_run(const int64_t* idx, const float* dist, const int64_t* label, int R, int n, int k, int64_t* idx_out,
                        float* dist_out, int64_t* label_out, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(shard_merge_ids_kernel, dim3(n), dim3(SHARD_NT), 0, st, idx, dist, label, R, (int64_t)n, k, idx_out, dist_out,
                     label_out);
  DIF_HIP(hipGetLastError());
  return 0;
}

int shard_merge_rank_run(const int64_t* count, const int64_t* owned, const float* mate_dist, int R, int n, int64_t* rank_out,
                         float* mate_dist_out, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(shard_merge_rank_kernel, dim3((n + SHARD_NT - 1) / SHARD_NT), dim3(SHARD_NT), 0, st, count, owned, mate_dist,
                     R, (int64_t)n, rank_out, mate_dist_out);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dif
