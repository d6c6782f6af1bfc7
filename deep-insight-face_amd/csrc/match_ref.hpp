// The reference's float32 distance arithmetic on the device, shared by the 1:N match (match.hip) and the range search
// (match_within.hip): NumPy's summation order (SumPlan / np_sum), the distance of one pair of rows (ref_distance) and the
// error bound of the MFMA search key (key_err).
// Every translation unit that includes this file is built with -ffp-contract=off (its `// hipcc-flags:` line): the
// functions below restate the reference's float32 operations one by one.
#pragma once
#include "dif_internal.hpp"

namespace dif {

// NumPy's tree over n <= 8192 elements has at most 65 leaves (441 sizes in [7689, 8191], e.g. 8191 = 4088 | 4103 -> ... ->
// 128 | 64 | 71; a power of two has n / 128) and keeps at most 7 partial sums on the combine stack
// (tests/test_oracle_golden.py walks every size); make_sum_plan fails on a tree that exceeds either.
constexpr int NP_LEAVES = 72;   // leaf capacity of a SumPlan (np_sum runs eight leaves per pass)
constexpr int NP_STACK = 8;     // combine-stack capacity
constexpr int NP_PLANE = NP_LEAVES + NP_STACK;   // LDS floats a wave needs for one np_sum: the leaf sums + the combine stack
constexpr int NP_SCRATCH = 3 * NP_PLANE;   // np_sum3 runs three sums side by side (the cosine distance's dot, |a|^2, |b|^2)
constexpr float NORM_LO = 1e-30f, NORM_HI = 1e30f;   // |x|^2 range inside which the filter's error bounds hold

// ---------------------------------------------------------------------------------------------
// NumPy's float32 add.reduce over a contiguous axis (numpy/_core/src/umath/loops_utils.h.src,
// @TYPE@_pairwise_sum; NumPy 2.2.6, the pinned interpreter of this image):
//   n < 8:     res = 0; res += a[i] in order
//   n <= 128:  r[j] = a[j] (j < 8); r[j] += a[i + j] for i = 8, 16, ... < n - n % 8;
//              res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then res += a[i] for the rest
//   else:      n2 = n / 2, n2 -= n2 % 8;  sum(a, n2) + sum(a + n2, n - n2)
// The plan flattens the recursion: leaves in order, and after leaf l `pops[l]` additions of the two
// topmost partial sums (a stack machine).  tests/test_oracle_golden.py checks this restatement against
// np.sum bit for bit; tests/test_match_gpu.py checks the device against NumPy.
struct SumPlan {
  int nleaf;
  unsigned short start[NP_LEAVES], len[NP_LEAVES];
  unsigned char pops[NP_LEAVES];
};

int make_sum_plan(int d, SumPlan* out);   // match.hip

// One wave evaluates sum_k term(k) in NumPy's order; every lane returns the result.  Eight lanes
// share a leaf (one accumulator each), so eight leaves run per pass.  `scratch` = NP_SCRATCH floats of
// LDS private to the wave.
template <class F>
__device__ __forceinline__ float np_sum(const SumPlan& plan, float* scratch, int lane, F term) {
#pragma clang fp contract(off)
  const int grp = lane >> 3, j = lane & 7;
  for (int l0 = 0; l0 < plan.nleaf; l0 += 8) {
    const int l = l0 + grp;
    float res = 0.f;
    if (l < plan.nleaf) {
      const int st = plan.start[l], n = plan.len[l];
      if (n < 8) {
        for (int i = 0; i < n; ++i) res = res + term(st + i);
      } else {
        const int body = n - (n % 8);
        float r = term(st + j);
        for (int i = 8; i < body; i += 8) r = r + term(st + i + j);
        // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)): float addition commutes, so the butterfly gives every
        // lane of the group exactly that value
        r = r + __shfl_xor(r, 1);
        r = r + __shfl_xor(r, 2);
        r = r + __shfl_xor(r, 4);
        res = r;
        for (int i = body; i < n; ++i) res = res + term(st + i);
      }
    }
    if (j == 0 && l < plan.nleaf) scratch[l] = res;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // the stack machine, run by every lane on the same values (the stack lives behind the leaf sums, NP_STACK deep:
  // make_sum_plan checks the depth; identical stores to one address are benign)
  float* stack = scratch + NP_LEAVES;
  int sp = 0;
  float top = 0.f;
#pragma unroll 1
  for (int l = 0; l < plan.nleaf; ++l) {
    top = scratch[l];
    for (int c = 0; c < plan.pops[l]; ++c) {
      --sp;
      top = stack[sp] + top;
    }
    stack[sp] = top;
    ++sp;
  }
  __builtin_amdgcn_wave_barrier();
  return top;
}

// Three sums in one pass (the same leaves, the same order per sum as np_sum: bit-identical to three calls): the cosine
// distance reads each row once instead of twice and pays one LDS round trip and one stack walk instead of three.
struct F3 {
  float x, y, z;
};
template <class F>
__device__ __forceinline__ F3 np_sum3(const SumPlan& plan, float* scratch, int lane, F term) {
#pragma clang fp contract(off)
  const int grp = lane >> 3, j = lane & 7;
  for (int l0 = 0; l0 < plan.nleaf; l0 += 8) {
    const int l = l0 + grp;
    F3 res = {0.f, 0.f, 0.f};
    if (l < plan.nleaf) {
      const int st = plan.start[l], n = plan.len[l];
      if (n < 8) {
        for (int i = 0; i < n; ++i) {
          const F3 t = term(st + i);
          res.x = res.x + t.x;
          res.y = res.y + t.y;
          res.z = res.z + t.z;
        }
      } else {
        const int body = n - (n % 8);
        F3 r = term(st + j);
        for (int i = 8; i < body; i += 8) {
          const F3 t = term(st + i + j);
          r.x = r.x + t.x;
          r.y = r.y + t.y;
          r.z = r.z + t.z;
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
          r.x = r.x + __shfl_xor(r.x, o);
          r.y = r.y + __shfl_xor(r.y, o);
          r.z = r.z + __shfl_xor(r.z, o);
        }
        res = r;
        for (int i = body; i < n; ++i) {
          const F3 t = term(st + i);
          res.x = res.x + t.x;
          res.y = res.y + t.y;
          res.z = res.z + t.z;
        }
      }
    }
    if (j == 0 && l < plan.nleaf) {
      scratch[l] = res.x;
      scratch[NP_PLANE + l] = res.y;
      scratch[2 * NP_PLANE + l] = res.z;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float* stack = scratch + NP_LEAVES;
  int sp = 0;
  F3 top = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int l = 0; l < plan.nleaf; ++l) {
    top.x = scratch[l];
    top.y = scratch[NP_PLANE + l];
    top.z = scratch[2 * NP_PLANE + l];
    for (int c = 0; c < plan.pops[l]; ++c) {
      --sp;
      top.x = stack[sp] + top.x;
      top.y = stack[NP_PLANE + sp] + top.y;
      top.z = stack[2 * NP_PLANE + sp] + top.z;
    }
    stack[sp] = top.x;
    stack[NP_PLANE + sp] = top.y;
    stack[2 * NP_PLANE + sp] = top.z;
    ++sp;
  }
  __builtin_amdgcn_wave_barrier();
  return top;
}

// The reference's float32 distance of one pair of rows (utility.py:54-62), evaluated by one wave.
//   metric 0: np.sum(np.square(np.subtract(a, b)), 1)
//   metric 1: np.arccos(np.sum(a*b, 1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))) / math.pi
// Returns the ranking key: the distance itself, or -inf where the reference's distance is NaN
// (|similarity| > 1 by rounding, 0/0, non-finite input): np.argmin ranks NaN before every number.
// `dist` receives the reported distance: NaN where the reference has NaN, or -- with `clamp` -- the
// distance of the similarity clamped to [-1, 1] (0 or 1; DESIGN.md "NaN distances").
// `sim_out` (optional) receives the similarity of metric 1, bit-identical to the reference's.
__device__ __forceinline__ float ref_distance(const SumPlan& plan, float* scratch, const float* a, const float* b,
                                              int metric, int lane, float* dist, bool clamp = false,
                                              float* sim_out = nullptr) {
#pragma clang fp contract(off)
  if (metric == 0) {
    const float s = np_sum(plan, scratch, lane, [&](int k) {
      const float d = a[k] - b[k];
      return d * d;
    });
    *dist = s;
    return s != s ? -__builtin_inff() : s;
  }
  const F3 s3 = np_sum3(plan, scratch, lane, [&](int k) {
    const float x = a[k], y = b[k];
    return F3{x * y, x * x, y * y};
  });
  const float dot = s3.x, aa = s3.y, bb = s3.z;
  const float norm = __builtin_sqrtf(aa) * __builtin_sqrtf(bb);
  const float s = dot / norm;
  if (sim_out) *sim_out = s;
  constexpr float PI_F = 3.14159274101257324f;     // float32(math.pi): NumPy divides a float32 array by it in float32
  const bool is_nan = !(s >= -1.f && s <= 1.f);
  const float sc = is_nan ? (s > 1.f ? 1.f : (s < -1.f ? -1.f : s)) : s;
  const float d = (float)acos((double)sc) / PI_F;
  *dist = (is_nan && !clamp) ? __builtin_nanf("") : d;
  return is_nan ? -__builtin_inff() : d;
}

// ---------------------------------------------------------------------------------------------
// Bound E on |search key - exact key| of the MFMA stage, per probe (u = 2^-24, gmax = the longest gallery row the stage
// sees).  |dot_mfma - q.g| <= c |q| |g| with
//     f32 MFMA:      c = D u          (a D-term fma chain: |err| <= D u sum|q_k g_k|)
//     bf16x2 filter: c = 3 2^-16 + (D + 64) u   (bf16 keeps 8 significant bits: x = hi + mid + r, |r| <= 2^-16 |x|, for either
//                    operand, and the dropped mid.mid product is <= 2^-16 |q_k g_k|; the 3 D / 16 accumulating MFMAs, each
//                    with at most five roundings on an element's way into the sum, stay below (D + 64) u)
//   metric 1: key = -dot/|g|            -> E = (c + 8 u) |q|
//   metric 0: key = |g|^2 - 2 dot       -> E = u 18 gmax^2 + (2 c + 2 u) |q| gmax
constexpr float U24 = 5.9604645e-8f;
__device__ __forceinline__ float key_err1_rel(float c) { return c + 8.f * U24; }          // E / |q|, metric 1
__device__ __forceinline__ float key_err0(float c, float qn, float gmax) {                  // E, metric 0
  return U24 * 18.f * gmax * gmax + (2.f * c + 2.f * U24) * qn * gmax;
}

// workspace of `need` elements of `elem` bytes, tracked by a capacity of ITS OWN (contents are not kept)
template <class P>
static int grow(P** p, size_t* cap, size_t need, size_t elem) {
  if (need <= *cap) return 0;
  if (*p) DIF_HIP(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  DIF_HIP(hipMalloc(p, need * elem));
  *cap = need;
  return 0;
}

// Lifts a kernel's dynamic-LDS limit to `bytes`, once per (device, kernel): the kernel is the template argument, so every
// instantiation has flags of its own
template <auto Kern>
static int allow_lds_once(int bytes) {
  static bool done[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!done[dev]) {
    DIF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done[dev] = true;
  }
  return 0;
}

int match_tile_kind(int B);                                  // match.hip: the f32 tile shape for B probes
// match.hip: gallery parts (blocks along the rows) of a tile launch over the first `rows` rows (-1: all of them)
int match_plan_parts(const Gallery* g, int B, bool bd, int64_t rows = -1);

}  // namespace dif
