// st_csr_pattern.h — the matrix-free CSR round on a PATTERN-ONLY matrix
//   M = diag(r) P diag(c),
// P[i][j] = the number of entries of row i with column j (row_ptr int64
// [n+1], col_idx int32 [nnz]; no value array exists), r and c optional dense
// device vectors [n] (null = all ones): adjacency, row- and column-stochastic
// and symmetric normalised operators of an unweighted graph.  For gfx950.
// Included by st_csr_pattern.hip (the launchers); not a public header.
//
// The round reads nnz * 4 bytes of matrix where st_csr.h reads nnz * (b + 4).
// It is st_csr.h's round with the weights moved out of the sweep:
//   k_csr_pattern_prep  k_csr_prep's body with one more store: xi = v_prev[i]
//                       * s_prev[i], z[i] = c[i] * xi (each one rounding);
//                       ONLY z goes to the scratch vector.  Dots (terms) are
//                       taken on xi.  Without c the launcher runs k_csr_prep
//                       itself: z = x.
//   k_csr_pattern_spmv  row i: the sum of z[col[e]] in st_csr.h's order - the
//                       same lane classes, R / U tables, lane t on entries t,
//                       t + L, ..., DPP tree, four wave adds for L = 256 -
//                       every step acc = acc + z, which is fma(1, z, acc) bit
//                       for bit; then tot = r[i] * tot (RS), the terms' fmas
//                       (CsrTerms' order), s_next = tot / (v_prev[i] *
//                       s_prev[i]) - the divisor recomputed, x[i]'s bits -
//                       and v_cur as k_csr_spmv.
// Launch 0 is the same sweep gathering c itself (ZONE: ones, no load at all):
// s_0 = r ∘ (P c).  All launches are no-ops once state->end says an earlier
// round stopped.  The sweep holds no load of a value: a load past a row's end
// goes to col[0] and its z is dropped.
//
// Bit claims ("Pattern-only CSR"): without scales every bit is the
// values kernels' on vals ≡ 1 (1 * x is exact, fma(1, x, acc) = acc + x); with
// power-of-two scales every bit is theirs on vals[e] = r[row] * c[col] as long
// as nothing under- or overflows (scaling by 2^k commutes with every
// rounding).
#pragma once

#include "st_csr_terms.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

// entries of a row in flight per lane (st_csr_host.h's kUnroll: the pattern
// sweep holds R * U fewer registers, a deeper U is an A/B not taken here)
constexpr uint32_t kPatUnroll[csr::kClasses] = { csr::kUnroll[0], csr::kUnroll[1],
                                                 csr::kUnroll[2], csr::kUnroll[3] };

// what hipcc --offload-arch=gfx950 --resource-usage reports for the row
// kernels of a round (st_csr_pattern_shape_desc; DESIGN.md has the table)
// (k_csr_pattern_spmv<T, RS, CsrOne>: vgpr / waves per SIMD without a row
// scale, vgpr_rs / waves_rs with one)
#define ST_CSR_PATTERN_REGS                                                      \
  "vgpr_f32=92 vgpr_f64=120 waves_f32=5 waves_f64=4 vgpr_rs_f32=102 "           \
  "vgpr_rs_f64=136 waves_rs_f32=4 waves_rs_f64=3"

// csr_rows without values.  ZONE: z ≡ 1 (launch 0 without c).  SUM: s_next =
// tot (launch 0), no division, no v.  RS: the row scale is given.  G: CsrOne
// or CsrTerms<T, KM>.
template <typename T, int L, int R, int U, bool ZONE, bool SUM, bool RS, typename G>
__device__ __forceinline__ void
csr_pattern_rows(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                 const uint32_t* __restrict__ order, uint32_t first, uint32_t last,
                 uint32_t blk, const T* __restrict__ z, const T* __restrict__ rs,
                 const T* __restrict__ s_prev, const T* __restrict__ v_prev,
                 T* __restrict__ s_next, T* __restrict__ v_cur, T m, T* red, const G g)
{
  constexpr uint32_t RPB = kBlock / L; // rows side by side in a workgroup
  static_assert(L <= 64 || R == 1, "a workgroup-wide row stands alone");
  const uint32_t sub = threadIdx.x / L, t = threadIdx.x % L;
  uint32_t r[R];
  bool live[R];
  uint64_t e[R], end[R];
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint64_t i = (uint64_t)first + ((uint64_t)blk * R + j) * RPB + sub;
    live[j] = i < last;
    r[j] = live[j] ? order[i] : 0u;
  }
#pragma unroll
  for (int j = 0; j < R; j++) {
    e[j] = live[j] ? (uint64_t)row_ptr[r[j]] + t : 0;
    end[j] = live[j] ? (uint64_t)row_ptr[r[j] + 1] : 0;
  }
  // what the row's last step needs, asked for before the sweep
  T sp[R], vp[R], rr[R];
  if constexpr (!SUM) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      sp[j] = s_prev[r[j]];
      vp[j] = v_prev[r[j]];
    }
  }
  if constexpr (RS) {
#pragma unroll
    for (int j = 0; j < R; j++)
      rr[j] = rs[r[j]];
  }
  T ut[R][G::kTerms ? G::kK : 1];
  if constexpr (G::kTerms) {
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
      for (int q = 0; q < G::kK; q++)
        ut[j][q] = (uint32_t)q < g.K ? g.u[q][r[j]] : (T)0;
  }
  T acc[R];
#pragma unroll
  for (int j = 0; j < R; j++)
    acc[j] = (T)0;
  for (;;) {
    bool more = false;
#pragma unroll
    for (int j = 0; j < R; j++)
      more |= e[j] < end[j];
    if (!more)
      break;
    T zs[R][U];
    bool in[R][U];
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t idx = e[j] + (uint64_t)u * L;
        in[j][u] = idx < end[j];
        if constexpr (ZONE) {
          zs[j][u] = (T)1;
        } else {
          const uint64_t at = in[j][u] ? idx : 0; // entry 0 exists: nnz >= 1
          zs[j][u] = z[col[at]];
        }
      }
#pragma unroll
    for (int j = 0; j < R; j++) {
#pragma unroll
      for (int u = 0; u < U; u++) { // the row's entries in order
        const T f = acc[j] + zs[j][u];
        acc[j] = in[j][u] ? f : acc[j];
      }
      e[j] += (uint64_t)U * L;
    }
  }

  T dq[G::kTerms ? G::kK : 1];
  if constexpr (G::kTerms) {
#pragma unroll
    for (int q = 0; q < G::kK; q++)
      dq[q] = (uint32_t)q < g.K ? ld_vector(g.dots + q) : (T)0;
  }
  if constexpr (L <= 64) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      T tot = csr_lanes_sum<T, L>(acc[j]);
      if constexpr (RS)
        tot = rr[j] * tot;
      if constexpr (G::kTerms) {
#pragma unroll
        for (int q = 0; q < G::kK; q++)
          tot = (uint32_t)q < g.K ? __builtin_fma(ut[j][q], dq[q], tot) : tot;
      }
      if (live[j] && t == L - 1) {
        if constexpr (SUM) {
          s_next[r[j]] = tot;
        } else {
          const T xr = vp[j] * sp[j]; // x[r]'s bits (k_csr_prep)
          s_next[r[j]] = tot / xr;
          v_cur[r[j]] = vp[j] * (sp[j] / m);
        }
      }
    }
  } else {
    const T w = wave_sum(acc[0]);
    if ((threadIdx.x & 63) == 0)
      red[threadIdx.x >> 6] = w;
    __syncthreads();
    T tot = red[0];
#pragma unroll
    for (int j = 1; j < kBlock / 64; j++)
      tot += red[j];
    if constexpr (RS)
      tot = rr[0] * tot;
    if constexpr (G::kTerms) {
#pragma unroll
      for (int q = 0; q < G::kK; q++)
        tot = (uint32_t)q < g.K ? __builtin_fma(ut[0][q], dq[q], tot) : tot;
    }
    if (live[0] && threadIdx.x == 0) {
      if constexpr (SUM) {
        s_next[r[0]] = tot;
      } else {
        const T xr = vp[0] * sp[0];
        s_next[r[0]] = tot / xr;
        v_cur[r[0]] = vp[0] * (sp[0] / m);
      }
    }
  }
}

template <typename T, bool ZONE, bool SUM, bool RS, typename G>
__device__ __forceinline__ void
csr_pattern_dispatch(const int64_t* row_ptr, const int32_t* col, const uint32_t* order,
                     const CsrTab& tab, const T* z, const T* rs, const T* s_prev,
                     const T* v_prev, T* s_next, T* v_cur, T m, T* red, const G g)
{
  const uint32_t b = blockIdx.x;
  int c = 0; // workgroup-uniform
  while (c < csr::kClasses - 1 && b >= tab.blk_first[c + 1])
    c++;
  const uint32_t first = tab.row_first[c], last = tab.row_first[c + 1];
  const uint32_t blk = b - tab.blk_first[c];
#define ST_CSR_PAT_ROWS(LL, CC)                                                    \
  csr_pattern_rows<T, LL, csr::kRows[CC], kPatUnroll[CC], ZONE, SUM, RS, G>(   \
    row_ptr, col, order, first, last, blk, z, rs, s_prev, v_prev, s_next,      \
    v_cur, m, red, g)
  static_assert(csr::kLanes[0] == 4 && csr::kLanes[1] == 16 &&
                  csr::kLanes[2] == 64 && csr::kLanes[3] == 256,
                "the class bodies below");
  if (c == 0)
    ST_CSR_PAT_ROWS(4, 0);
  else if (c == 1)
    ST_CSR_PAT_ROWS(16, 1);
  else if (c == 2)
    ST_CSR_PAT_ROWS(64, 2);
  else
    ST_CSR_PAT_ROWS(256, 3);
#undef ST_CSR_PAT_ROWS
}

// launch 0: s[i] = r[i] * (the sum of c[col] over row i), then the terms
// (zc = c, unused under ZONE; G = CsrOne: no terms)
template <typename T, bool ZONE, bool RS, typename G>
__global__ __launch_bounds__(kBlock) void
k_csr_pattern_rowsum(const int64_t* row_ptr, const int32_t* col, const uint32_t* order,
                     CsrTab tab, const T* __restrict__ zc, const T* __restrict__ rs,
                     T* __restrict__ s, G g)
{
  __shared__ T red[kBlock / 64];
  csr_pattern_dispatch<T, ZONE, true, RS, G>(row_ptr, col, order, tab, zc, rs, nullptr,
                                             nullptr, s, nullptr, (T)0, red, g);
}

// launch k >= 1, second half: the row sums of z and the v update
template <typename T, bool RS, typename G>
__global__ __launch_bounds__(kBlock) void
k_csr_pattern_spmv(const int64_t* row_ptr, const int32_t* col, const uint32_t* order,
                   CsrTab tab, const T* __restrict__ z, const T* __restrict__ rs,
                   const T* __restrict__ s_prev, const T* __restrict__ v_prev,
                   T* __restrict__ s_next, T* __restrict__ v_cur, uint32_t k,
                   const st_state* state, G g)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T red[kBlock / 64];
  const T m = (T)state->max; // published by the vector pass of this launch k
  csr_pattern_dispatch<T, false, false, RS, G>(row_ptr, col, order, tab, z, rs, s_prev,
                                               v_prev, s_next, v_cur, m, red, g);
}

// launch k >= 1, first half with a column scale: k_csr_prep's body, except
// that z[i] = c[i] * x[i] is stored where x was (x itself goes nowhere; the
// dots are taken on it)
template <typename T, typename... DOTS>
__global__ __launch_bounds__(kBlock) void
k_csr_pattern_prep(const T* __restrict__ s_prev, const T* __restrict__ v_prev,
                   const T* __restrict__ cs, T* __restrict__ z, uint32_t n, T eps,
                   uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* state,
                   const DOTS... dots)
{
  constexpr bool kDots = sizeof...(DOTS) != 0;
  static_assert(sizeof...(DOTS) <= 1, "at most one CsrDots");
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T mx_sh[kBlock / 64];
  const bool cyclic = semantics == ST_SEM_SYCL;
  T mx = (T)0;
  int fail = 0;
  T dacc[kCsrTermsMax];
  if constexpr (kDots) {
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      dacc[q] = (T)0;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const T sv = s_prev[i];
    const T xi = v_prev[i] * sv;
    z[i] = cs[i] * xi;
    if constexpr (kDots) {
      const CsrDots<T>& d = csr_first(dots...);
#pragma unroll
      for (int q = 0; q < kCsrTermsMax; q++)
        if ((uint32_t)q < d.K)
          dacc[q] = __builtin_fma(d.w[q][i], xi, dacc[q]);
    }
    mx = sv > mx ? sv : mx;
    if (i + 1 < n || cyclic) {
      const T d = sv - s_prev[i + 1 < n ? i + 1 : 0];
      fail |= (d < (T)0 ? -d : d) < eps ? 0 : 1;
    }
  }
  if constexpr (kDots) {
    const CsrDots<T>& d = csr_first(dots...);
    csr_dot_partials<T>(dacc, d.K, d.partial);
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0)
    mx_sh[threadIdx.x >> 6] = mx;
  fail = __syncthreads_or(fail);
  if (threadIdx.x == 0) {
    T m = mx_sh[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++)
      m = mx_sh[w] > m ? mx_sh[w] : m;
    stats_publish<T>(m, fail, gridDim.x, s_prev, k - 1, max_itr, semantics, state);
  }
}

// validation, one pass per handle: err[0] = the lowest (which << 32 | i) whose
// scale is not finite and > 0 (which: 0 = row_scale, 1 = col_scale;
// st_csr_host.h: scale_entry_bad); either pointer may be null
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_pattern_check_scales(const T* __restrict__ rs, const T* __restrict__ cs,
                           uint32_t n, unsigned long long* err)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    if (rs) {
      const T a = rs[i];
      if (!(a > (T)0) || a - a != (T)0)
        atomicMin(&err[0], (unsigned long long)i);
    }
    if (cs) {
      const T b = cs[i];
      if (!(b > (T)0) || b - b != (T)0)
        atomicMin(&err[0], (1ull << 32) | i);
    }
  }
}

} // namespace dev
} // namespace st
