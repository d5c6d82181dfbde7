// st_csr.h — the matrix-free round on a nonnegative SPARSE matrix in CSR
// storage (row_ptr int64 [n+1], col_idx int32 [nnz], vals fp32 / fp64 [nnz]),
// for gfx950.  Included by st_csr.hip (the launchers); not a public header.
//
// The matrix-free round (k_mfree, st_device.h) keeps all of its state in
// vectors and computes s_k = (A_0 x) ⊘ x, x = v ∘ s; its only dense part is
// the sweep over a row.  Here that sweep is a CSR row product, nnz * (b + 4)
// bytes per round, and everything else is k_mfree's arithmetic.
//
// Row classes (st_csr_host.h: kLanes / kNnzMax): a row is shared by L = 4, 16,
// 64 or 256 lanes according to its own nnz, and the plan (order[]: row
// indices sorted by class, built once per matrix) lets one launch serve all
// classes: the block range is partitioned by class from a small table in the
// kernel arguments, and a workgroup-uniform branch picks the class's body.
// A workgroup of 256 lanes holds kRows * 256 / L rows.
//
// Summation order of a row (fixed, no atomics): lane t of the row's L lanes
// takes the entries start + t, start + t + L, ... in storage order, one fused
// multiply-add each (K0: the same fma with 1); the L lanes combine by the
// first log2(L) steps of wave_sum's DPP tree (quad_perm, quad_perm, row_ror
// 4, row_ror 8, row_bcast 15, row_bcast 31), read in the row's LAST lane,
// which for L = 64 is wave_sum itself; L = 256 adds the four wave_sums
// serially in wave order, as mfree_group does.  So a row's result depends on
// its own entries and on x only - not on the other rows, nor on its place.
//
// A row's entries start at an arbitrary offset, so every load is one element
// wide, consecutive lanes on consecutive entries.  The x gathers are the only
// irregular traffic.
//
// The round (launch k >= 1) is two launches, because every workgroup
// sweeping all of s_prev (k_mfree's way to m and stop) would cost more than
// the matrix here:
//   k_csr_prep  over the vectors: x = v_prev ∘ s_prev to scratch, max / stop
//               of s_prev folded through st_state's stats scratch
//               (stats_publish: the last workgroup publishes round k-1
//               exactly as k_mfree records it, scratch left zero)
//   k_csr_spmv  over the row classes: s_next[r] = (Σ a x[col]) / x[r] and
//               v_cur[r] = v_prev[r] * (s_prev[r] / m), m from the state
// both no-ops once state->end says an earlier round stopped.
#pragma once

#define ST_DEVICE_TEMPLATES_ONLY 1
#include "st_device.h"
#include "st_csr_host.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

// where each class starts in the plan (rows) and in the launch (workgroups)
struct CsrTab
{
  uint32_t row_first[csr::kClasses + 1];
  uint32_t blk_first[csr::kClasses + 1];
};

// one element by a vector (per-lane) load, never through the scalar cache:
// what an earlier launch of the same stream wrote (dots)
__device__ __forceinline__ float
ld_vector(const float* p)
{
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t*>(p),
                                           __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ double
ld_vector(const double* p)
{
  return __longlong_as_double((long long)__hip_atomic_load(
    reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
    __HIP_MEMORY_SCOPE_AGENT));
}

// the sum over the L lanes that share a row, valid in the row's last lane
// (L <= 64) - wave_sum_l63's steps, cut off after log2(L)
template <typename T, int L>
__device__ __forceinline__ T
csr_lanes_sum(T x)
{
  static_assert(L == 4 || L == 16 || L == 64, "part of a wave");
  x += dpp_mov<0xB1>(x); // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E>(x); // quad_perm [2,3,0,1]
  if constexpr (L >= 16) {
    x += dpp_mov<0x124>(x); // row_ror 4
    x += dpp_mov<0x128>(x); // row_ror 8
  }
  if constexpr (L == 64) {
    x += dpp_mov<0x142, 0xa>(x); // row_bcast 15
    x += dpp_mov<0x143, 0xc>(x); // row_bcast 31
  }
  return x;
}

// One workgroup of class L: R * (256 / L) rows of the plan from
// order[first + blk * R * (256 / L)], at most `last`; the lanes that share a
// row take R rows side by side (row j of the group: plan position
// ... + j * (256 / L) + group, so that one load instruction of the workgroup
// covers neighbouring rows) with U entries of each in flight, R * U loads per
// lane - the row product is latency-bound, not ALU-bound.  Loads past a row's
// end are redirected to entry 0 (always valid) and their products dropped, so
// the sweep has no branch; a row's own order is untouched by R and U.
// ONES: x ≡ 1, no division, no v (K0).
// G: what a row takes from outside itself.  CsrOne (one matrix): m and x as
// passed, nothing else.  CsrStack (st_csr_batch.h: the stacked rows of a
// batch): the row's own matrix b = row_mat[r] gives the gate (a row of a
// matrix that ended before launch k is a row past `last`: live = false, no
// entry read, nothing written - every lane still walks to the tree and the
// barrier), m = states[b].max and the first row of the matrix's slice of x
// (col is local to the matrix).  The lanes, the fma order and the tree are
// the same for both.
// CsrTerms<T> (the operator A + sum_j u_j w_j^T, j < K <= 4): CsrOne, and
// after the lane tree and before the division tot = fma(u_j[r], dots[j], tot),
// j = 0 .. K-1 in that order; u_j[r] is asked for with the row's other
// last-step loads, dots [K] (k_csr_dots of this launch) is read by a vector
// load.  An empty row (legal under such an operator) takes no trip through
// the sweep - e == end from the start - and its tot starts the fmas at 0.
// KM >= K is the number of terms the instantiation holds registers for (the
// u_j[r] live through the sweep: R * KM of them); it changes no result.
// CsrPlain / CsrDivisor<T> (st_csr_product.h: the operator B A, two row
// products per round).  CsrPlain: CsrOne's sweep and tree, then s_next[r] =
// tot - no division, no v, nothing asked for but the row's entries and the
// gathers (an empty row writes exactly 0).  CsrDivisor<T>: CsrOne, except
// that the divisor is xdiv[r] and not the gathered vector's own element.
// csr_mode<G> says which; every other policy is neither.
struct CsrOne
{
  static constexpr bool kStack = false;
  static constexpr bool kTerms = false;
  static constexpr int kK = 0;
};
struct CsrPlain
{
  static constexpr bool kStack = false;
  static constexpr bool kTerms = false;
  static constexpr int kK = 0;
};
template <typename T>
struct CsrDivisor
{
  static constexpr bool kStack = false;
  static constexpr bool kTerms = false;
  static constexpr int kK = 0;
  const T* xdiv; // [n] the divisor of each row
};
template <typename G>
struct csr_mode
{
  static constexpr bool kPlain = false;
  static constexpr bool kDivisor = false;
};
template <>
struct csr_mode<CsrPlain>
{
  static constexpr bool kPlain = true;
  static constexpr bool kDivisor = false;
};
template <typename T>
struct csr_mode<CsrDivisor<T>>
{
  static constexpr bool kPlain = false;
  static constexpr bool kDivisor = true;
};
constexpr int kCsrTermsMax = (int)csr::kTermsMax;
template <typename T, int KM = kCsrTermsMax>
struct CsrTerms
{
  static_assert(KM >= 1 && KM <= kCsrTermsMax, "1 .. ST_CSR_TERMS_MAX terms");
  static constexpr bool kStack = false;
  static constexpr bool kTerms = true;
  static constexpr int kK = KM;
  uint32_t K; // <= KM
  const T* u[KM];
  const T* dots;
};
struct CsrStack
{
  static constexpr bool kStack = true;
  static constexpr bool kTerms = false;
  static constexpr int kK = 0;
  const uint32_t* row_mat;   // [N] the matrix of each stacked row
  const uint32_t* mat_first; // [batch + 1] the first stacked row of each matrix
  const st_state* states;    // [batch]
  uint32_t k;                // this launch
};

template <typename T, int L, int R, int U, bool ONES, typename G = CsrOne>
__device__ __forceinline__ void
csr_rows(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
         const T* __restrict__ vals, const uint32_t* __restrict__ order,
         uint32_t first, uint32_t last, uint32_t blk, const T* __restrict__ x,
         const T* __restrict__ s_prev, const T* __restrict__ v_prev,
         T* __restrict__ s_next, T* __restrict__ v_cur, T m, T* red,
         const G g = G())
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
  T mr[R];         // CsrStack: the row's own m ...
  uint32_t xo[R];  // ... and where its matrix starts in x
  if constexpr (G::kStack) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      const uint32_t b = g.row_mat[r[j]];
      const uint32_t en = __hip_atomic_load(&g.states[b].end, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
      live[j] = live[j] && !(en != 0 && en < g.k);
      xo[j] = g.mat_first[b];
      mr[j] = (T)g.states[b].max; // published by k_csrb_prep of this launch
    }
  }
#pragma unroll
  for (int j = 0; j < R; j++) {
    e[j] = live[j] ? (uint64_t)row_ptr[r[j]] + t : 0;
    end[j] = live[j] ? (uint64_t)row_ptr[r[j] + 1] : 0;
  }
  // what the row's last step needs, asked for before the sweep
  T xr[R], sp[R], vp[R];
  constexpr bool kSumOnly = ONES || csr_mode<G>::kPlain; // s_next = tot
  if constexpr (!kSumOnly) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      if constexpr (csr_mode<G>::kDivisor)
        xr[j] = g.xdiv[r[j]];
      else
        xr[j] = x[r[j]];
      sp[j] = s_prev[r[j]];
      vp[j] = v_prev[r[j]];
    }
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
    T a[R][U], xs[R][U];
    bool in[R][U];
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t idx = e[j] + (uint64_t)u * L;
        in[j][u] = idx < end[j];
        const uint64_t at = in[j][u] ? idx : 0; // entry 0 exists: nnz >= n >= 1
        a[j][u] = vals[at];
        if constexpr (ONES)
          xs[j][u] = (T)1;
        else if constexpr (G::kStack) // a redirected load reads col[0], which is
          // local to matrix 0: it gets no base, so x needs no slack past N
          xs[j][u] = x[(in[j][u] ? (uint64_t)xo[j] : 0) + (uint32_t)col[at]];
        else
          xs[j][u] = x[col[at]];
      }
#pragma unroll
    for (int j = 0; j < R; j++) {
#pragma unroll
      for (int u = 0; u < U; u++) { // the row's entries in order
        const T f = __builtin_fma(a[j][u], xs[j][u], acc[j]);
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
      if constexpr (G::kTerms) {
#pragma unroll
        for (int q = 0; q < G::kK; q++)
          tot = (uint32_t)q < g.K ? __builtin_fma(ut[j][q], dq[q], tot) : tot;
      }
      if (live[j] && t == L - 1) {
        if constexpr (kSumOnly) {
          s_next[r[j]] = tot;
        } else {
          s_next[r[j]] = tot / xr[j];
          if constexpr (G::kStack)
            v_cur[r[j]] = vp[j] * (sp[j] / mr[j]);
          else
            v_cur[r[j]] = vp[j] * (sp[j] / m); // k_mfree's v update (cpp:260)
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
    if constexpr (G::kTerms) {
#pragma unroll
      for (int q = 0; q < G::kK; q++)
        tot = (uint32_t)q < g.K ? __builtin_fma(ut[0][q], dq[q], tot) : tot;
    }
    if (live[0] && threadIdx.x == 0) {
      if constexpr (kSumOnly) {
        s_next[r[0]] = tot;
      } else {
        s_next[r[0]] = tot / xr[0];
        if constexpr (G::kStack)
          v_cur[r[0]] = vp[0] * (sp[0] / mr[0]);
        else
          v_cur[r[0]] = vp[0] * (sp[0] / m);
      }
    }
  }
}

template <typename T, bool ONES, typename G = CsrOne>
__device__ __forceinline__ void
csr_dispatch(const int64_t* row_ptr, const int32_t* col, const T* vals,
             const uint32_t* order, const CsrTab& tab, const T* x,
             const T* s_prev, const T* v_prev, T* s_next, T* v_cur, T m, T* red,
             const G g = G())
{
  const uint32_t b = blockIdx.x;
  int c = 0; // workgroup-uniform
  while (c < csr::kClasses - 1 && b >= tab.blk_first[c + 1])
    c++;
  const uint32_t first = tab.row_first[c], last = tab.row_first[c + 1];
  const uint32_t blk = b - tab.blk_first[c];
#define ST_CSR_ROWS(LL, CC)                                                        \
  csr_rows<T, LL, csr::kRows[CC], csr::kUnroll[CC], ONES, G>(                  \
    row_ptr, col, vals, order, first, last, blk, x, s_prev, v_prev, s_next,    \
    v_cur, m, red, g)
  static_assert(csr::kLanes[0] == 4 && csr::kLanes[1] == 16 &&
                  csr::kLanes[2] == 64 && csr::kLanes[3] == 256,
                "the class bodies below");
  if (c == 0)
    ST_CSR_ROWS(4, 0);
  else if (c == 1)
    ST_CSR_ROWS(16, 1);
  else if (c == 2)
    ST_CSR_ROWS(64, 2);
  else
    ST_CSR_ROWS(256, 3);
#undef ST_CSR_ROWS
}

// The workgroup's share of up to four dots, from every lane's own sum:
// wave_sum of each, the four wave sums added in wave order by lane 0, to
// partial[q * gridDim.x + blockIdx.x].  Ends in a barrier, so the LDS it
// uses is free again.
template <typename T>
__device__ __forceinline__ void
csr_dot_partials(const T (&dacc)[kCsrTermsMax], uint32_t K, T* __restrict__ partial)
{
  __shared__ T dsh[kCsrTermsMax][kBlock / 64];
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    if ((uint32_t)q < K) { // workgroup-uniform
      const T w = wave_sum(dacc[q]);
      if ((threadIdx.x & 63) == 0)
        dsh[q][threadIdx.x >> 6] = w;
    }
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      if ((uint32_t)q < K) {
        T tot = dsh[q][0];
#pragma unroll
        for (int w = 1; w < kBlock / 64; w++)
          tot += dsh[q][w];
        partial[(uint64_t)q * gridDim.x + blockIdx.x] = tot;
      }
  __syncthreads();
}

// K0: s[r] = Σ a (x ≡ 1)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_rowsum(const int64_t* row_ptr, const int32_t* col, const T* vals,
             const uint32_t* order, CsrTab tab, T* __restrict__ s)
{
  __shared__ T red[kBlock / 64];
  csr_dispatch<T, true>(row_ptr, col, vals, order, tab, nullptr, nullptr,
                        nullptr, s, nullptr, (T)0, red);
}

// what the vector pass also does under CsrTerms: partial[j * gridDim.x +
// blockIdx.x] = this workgroup's share of w_j . x (st_csr_terms.h has the
// order)
template <typename T>
struct CsrDots
{
  uint32_t K;
  const T* w[kCsrTermsMax];
  T* partial; // [K][gridDim.x]
};
template <typename D>
__device__ __forceinline__ const D&
csr_first(const D& d)
{
  return d;
}

// launch k >= 1, first half: x, and round k-1's stats through the state.
// DOTS is empty (k_csr_prep<T>, the kernel and the arguments it always had)
// or one CsrDots<T> (k_csr_prep<T, CsrDots<T>>, the vector pass of a round
// with terms): one body, in the kernel itself.
template <typename T, typename... DOTS>
__global__ __launch_bounds__(kBlock) void
k_csr_prep(const T* __restrict__ s_prev, const T* __restrict__ v_prev,
           T* __restrict__ x, uint32_t n, T eps, uint32_t k, uint32_t max_itr,
           uint32_t semantics, st_state* state, const DOTS... dots)
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
  T mx = (T)0; // find_max starts from 0 (cpp:185): negatives and NaN never win
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
    x[i] = xi;
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
      fail |= (d < (T)0 ? -d : d) < eps ? 0 : 1; // cpp:419-421; NaN fails
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
    // round k-1: end = k when it stops or exhausts, as k_mfree writes it
    stats_publish<T>(m, fail, gridDim.x, s_prev, k - 1, max_itr, semantics,
                     state);
  }
}

// launch k >= 1, second half: the row products and the v update
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_spmv(const int64_t* row_ptr, const int32_t* col, const T* vals,
           const uint32_t* order, CsrTab tab, const T* __restrict__ x,
           const T* __restrict__ s_prev, const T* __restrict__ v_prev,
           T* __restrict__ s_next, T* __restrict__ v_cur, uint32_t k,
           const st_state* state)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T red[kBlock / 64];
  const T m = (T)state->max; // published by k_csr_prep of this launch k
  csr_dispatch<T, false>(row_ptr, col, vals, order, tab, x, s_prev, v_prev,
                         s_next, v_cur, m, red);
}

} // namespace dev
} // namespace st
