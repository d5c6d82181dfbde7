// st_csr_multi.h — the CSR round with terms (st_csr_terms.h) for up to 8
// operators on ONE matrix,
//   M_c = A + sum_{j < K} u_{c,j} w_{c,j}^T,   c < C <= 8 (ST_CSR_MULTI_MAX),
// in one pass over the matrix per round: personalised PageRank ranks one link
// graph under many teleport vectors.  For gfx950.  Included by
// st_csr_multi.hip (the launchers); not a public header.
//
// Storage.  Every vector of the round is packed [n][CP], the column index
// fastest, CP = the smallest of 2, 4, 8 that is >= C: s (two buffers), v
// (two), x, and the terms u, w as [K][n][CP].  One aligned load of CP * b
// bytes brings row i of a vector for all columns, so a gather of x pays its
// cache line for CP useful scalars instead of one.  Every index into these
// arrays is 64-bit (n * CP passes 2^32).  Columns C .. CP-1 are padding: never
// gated in, never stored to, never published; their slots hold 1.
//
// Every column keeps the bits st_csr_terms.h gives it alone, because each
// value of column c passes through the same operations on the same operands
// in the same order:
//   k_csrm_prep   k_csr_prep<T, CsrDots<T>>'s pass: the same grid (a function
//                 of n alone), the same elements per lane in the same
//                 ascending order, one accumulator per (column, term) with its
//                 own fma chain, wave_sum, the four wave sums in wave order
//                 -> partial[c][j][workgroup]; max and the failed-pair flag
//                 per column, stats_publish on the column's own st_state
//   k_csrm_dots   k_csr_dots' order, one workgroup per column -> dots[c][j]
//   k_csrm_spmv   csr_rows' structure under the matrix's own classes: the
//                 same lanes per row, the same entries per lane in the same
//                 order, the same DPP tree, the same serial adds for L = 256;
//                 every loaded (val, col) pair feeds CP fmas against
//                 x[col][0 .. CP), one accumulator per column; after the tree
//                 tot_c = fma(u_{c,j}[r], dots[c][j], tot_c), j ascending,
//                 then the division and the v update with the column's own m
// K0 is the same three launches with x ≡ 1 (k_csrm_wsum, k_csrm_dots,
// k_csrm_rowsum).  R (rows side by side) and U (entries in flight) differ from
// csr_rows' - a row of x is CP * b bytes of registers, not b - and change no
// bit (st_csr.h: a row's own order is untouched by R and U).
//
// The gate is per column: a column whose state has `end` set and below this
// launch k gets nothing published and nothing stored (its arithmetic may
// still run in a lane that serves a live column: it reads only stale finite
// values).  When every column has ended a workgroup returns at once.  No
// float atomics; no workgroup waits on another.
#pragma once

#include "st_csr_terms.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

constexpr int kCsrMultiMax = (int)csr::kMultiMax;

template <typename T, int CP>
struct CsrmVec
{
  typedef T type __attribute__((ext_vector_type(CP)));
};

// row i of a packed [n][CP] array, one aligned load / store
template <typename T, int CP>
__device__ __forceinline__ typename CsrmVec<T, CP>::type
csrm_ld(const T* p, uint64_t i)
{
  return *reinterpret_cast<const typename CsrmVec<T, CP>::type*>(p + i * CP);
}
template <typename T, int CP>
__device__ __forceinline__ void
csrm_st(T* p, uint64_t i, typename CsrmVec<T, CP>::type v)
{
  *reinterpret_cast<typename CsrmVec<T, CP>::type*>(p + i * CP) = v;
}

// bit c: column c < C takes part in launch k (workgroup-uniform)
__device__ __forceinline__ uint32_t
csrm_active(const st_state* states, uint32_t C, uint32_t k)
{
  uint32_t act = 0;
  for (uint32_t c = 0; c < C; c++) {
    const uint32_t e = __hip_atomic_load(&states[c].end, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (!(e != 0 && e < k))
      act |= 1u << c;
  }
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)act);
}

// The workgroup's share of the dots of the columns in `act`: csr_dot_partials
// per column -> partial[(c * K + q) * gridDim.x + blockIdx.x].  Ends in a
// barrier.
template <typename T, int CP>
__device__ __forceinline__ void
csrm_dot_partials(const typename CsrmVec<T, CP>::type (&dacc)[kCsrTermsMax],
                  uint32_t K, uint32_t act, T* __restrict__ partial)
{
  __shared__ T dsh[kCsrTermsMax][CP][kBlock / 64];
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    if ((uint32_t)q < K) { // workgroup-uniform
#pragma unroll
      for (int c = 0; c < CP; c++)
        if ((act >> c) & 1u) { // workgroup-uniform
          const T w = wave_sum(dacc[q][c]);
          if ((threadIdx.x & 63) == 0)
            dsh[q][c][threadIdx.x >> 6] = w;
        }
    }
  __syncthreads();
  // lane c * 4 + q finishes (column c, term q)
  const uint32_t c = threadIdx.x / kCsrTermsMax, q = threadIdx.x % kCsrTermsMax;
  if (c < (uint32_t)CP && q < K && ((act >> c) & 1u)) {
    T tot = dsh[q][c][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++)
      tot += dsh[q][c][w];
    partial[((uint64_t)c * K + q) * gridDim.x + blockIdx.x] = tot;
  }
  __syncthreads();
}

// K0's dots: partial[c][j][b] of w_{c,j} . 1 in the vector pass's order
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_wsum(uint32_t n, uint32_t C, uint32_t K, const T* __restrict__ w,
            T* __restrict__ partial)
{
  typedef typename CsrmVec<T, CP>::type V;
  V dacc[kCsrTermsMax];
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    dacc[q] = (V)(T)0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      if ((uint32_t)q < K) {
        const V wv = csrm_ld<T, CP>(w + (uint64_t)q * n * CP, i);
#pragma unroll
        for (int c = 0; c < CP; c++)
          dacc[q][c] = __builtin_fma(wv[c], (T)1, dacc[q][c]);
      }
  }
  csrm_dot_partials<T, CP>(dacc, K, (1u << C) - 1u, partial);
}

// one workgroup per column: dots[c][j] = the sum of partial[c][j][0 .. P) in
// k_csr_dots' order (states == nullptr: K0, never gated)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrm_dots(const T* __restrict__ partial, uint32_t P, uint32_t K,
            T* __restrict__ dots, uint32_t k, const st_state* states)
{
  const uint32_t c = blockIdx.x;
  if (states) {
    const uint32_t e = __hip_atomic_load(&states[c].end, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  const T* __restrict__ part = partial + (uint64_t)c * K * P;
  __shared__ T sh[kCsrTermsMax][kBlock / 64];
  for (uint32_t q = 0; q < K && q < (uint32_t)kCsrTermsMax; q++) {
    T acc = (T)0;
    for (uint32_t i = threadIdx.x; i < P; i += kBlock)
      acc += part[(uint64_t)q * P + i];
    const T w = wave_sum(acc);
    if ((threadIdx.x & 63) == 0)
      sh[q][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < K && threadIdx.x < (uint32_t)kCsrTermsMax) {
    T tot = sh[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++)
      tot += sh[threadIdx.x][w];
    dots[(uint64_t)c * K + threadIdx.x] = tot;
  }
}

// launch k >= 1, first launch: x, the dots' partials and round k-1's stats of
// every live column; the publisher of a round that sets a column's `end` adds
// 1 to *finished
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_prep(const T* __restrict__ s_prev, const T* __restrict__ v_prev,
            T* __restrict__ x, const T* __restrict__ w, T* __restrict__ partial,
            uint32_t n, uint32_t C, uint32_t K, T eps, uint32_t k,
            uint32_t max_itr, uint32_t semantics, st_state* states,
            uint32_t* finished)
{
  typedef typename CsrmVec<T, CP>::type V;
  const uint32_t act = csrm_active(states, C, k);
  if (act == 0)
    return;
  const bool all = act == (1u << CP) - 1u; // no padding, nothing ended
  __shared__ T mx_sh[CP][kBlock / 64];
  __shared__ uint32_t fail_sh;
  if (threadIdx.x == 0)
    fail_sh = 0u;
  const bool cyclic = semantics == ST_SEM_SYCL;
  V mx = (V)(T)0; // find_max starts from 0 (cpp:185): negatives and NaN never win
  uint32_t fail = 0;
  V dacc[kCsrTermsMax];
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    dacc[q] = (V)(T)0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const V sv = csrm_ld<T, CP>(s_prev, i);
    const V vv = csrm_ld<T, CP>(v_prev, i);
    V xi;
#pragma unroll
    for (int c = 0; c < CP; c++)
      xi[c] = vv[c] * sv[c];
    if (all)
      csrm_st<T, CP>(x, i, xi);
    else {
#pragma unroll
      for (int c = 0; c < CP; c++)
        if ((act >> c) & 1u)
          x[i * CP + c] = xi[c];
    }
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      if ((uint32_t)q < K) {
        const V wv = csrm_ld<T, CP>(w + (uint64_t)q * n * CP, i);
#pragma unroll
        for (int c = 0; c < CP; c++)
          dacc[q][c] = __builtin_fma(wv[c], xi[c], dacc[q][c]);
      }
#pragma unroll
    for (int c = 0; c < CP; c++)
      mx[c] = sv[c] > mx[c] ? sv[c] : mx[c];
    if (i + 1 < n || cyclic) {
      const V nx = csrm_ld<T, CP>(s_prev, i + 1 < n ? i + 1 : 0);
#pragma unroll
      for (int c = 0; c < CP; c++) {
        const T d = sv[c] - nx[c];
        fail |= ((d < (T)0 ? -d : d) < eps ? 0u : 1u) << c; // NaN fails
      }
    }
  }
  csrm_dot_partials<T, CP>(dacc, K, act, partial); // its barriers order fail_sh = 0
#pragma unroll
  for (int c = 0; c < CP; c++)
    if ((act >> c) & 1u) { // workgroup-uniform
      const T m = wave_max(mx[c]);
      if ((threadIdx.x & 63) == 0)
        mx_sh[c][threadIdx.x >> 6] = m;
    }
  if (fail)
    atomicOr(&fail_sh, fail);
  __syncthreads();
  // lane c publishes column c: round k-1, end = k when it stops or exhausts
  if (threadIdx.x < (uint32_t)CP && ((act >> threadIdx.x) & 1u)) {
    const uint32_t c = threadIdx.x;
    T m = mx_sh[c][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++)
      m = mx_sh[c][w] > m ? mx_sh[c][w] : m;
    st_state* const state = states + c;
    if (stats_publish<T>(m, (int)((fail_sh >> c) & 1u), gridDim.x, s_prev + c,
                         k - 1, max_itr, semantics, state) &&
        state->end == k)
      atomicAdd(finished, 1u);
  }
}

// What the lane that holds a row's sums does with them: the terms, the
// division, the v update, the gated stores.  Everything it needs of row r is
// asked for here, after the sweep, so that it stays out of the sweep's live
// range.
template <typename T, int CP, bool ONES>
__device__ __forceinline__ void
csrm_finish(uint32_t r, typename CsrmVec<T, CP>::type tot, const T* __restrict__ x,
            const T* __restrict__ s_prev, const T* __restrict__ v_prev,
            T* __restrict__ s_next, T* __restrict__ v_cur,
            const T* __restrict__ u, const T* __restrict__ dots, uint32_t n,
            uint32_t C, uint32_t K, uint32_t act, const st_state* states)
{
  typedef typename CsrmVec<T, CP>::type V;
  V xr = (V)(T)1, sp = (V)(T)1, vp = (V)(T)1;
  if constexpr (!ONES) {
    xr = csrm_ld<T, CP>(x, r);
    sp = csrm_ld<T, CP>(s_prev, r);
    vp = csrm_ld<T, CP>(v_prev, r);
  }
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    if ((uint32_t)q < K) {
      const V uv = csrm_ld<T, CP>(u + (uint64_t)q * n * CP, r);
#pragma unroll
      for (int c = 0; c < CP; c++) {
        const T d = (uint32_t)c < C ? ld_vector(dots + (uint64_t)c * K + q) : (T)0;
        tot[c] = __builtin_fma(uv[c], d, tot[c]);
      }
    }
  if constexpr (ONES) {
    csrm_st<T, CP>(s_next, r, tot); // K0 is never gated; padding sums are finite
  } else {
    V sn, vc;
#pragma unroll
    for (int c = 0; c < CP; c++) {
      // published by k_csrm_prep of this launch k
      const T m = (uint32_t)c < C ? (T)states[c].max : (T)1;
      sn[c] = tot[c] / xr[c];
      vc[c] = vp[c] * (sp[c] / m); // k_mfree's v update (cpp:260)
    }
    if (act == (1u << CP) - 1u) {
      csrm_st<T, CP>(s_next, r, sn);
      csrm_st<T, CP>(v_cur, r, vc);
    } else {
#pragma unroll
      for (int c = 0; c < CP; c++)
        if ((act >> c) & 1u) {
          s_next[(uint64_t)r * CP + c] = sn[c];
          v_cur[(uint64_t)r * CP + c] = vc[c];
        }
    }
  }
}

// csr_rows (st_csr.h) with CP columns of x per entry: the same lanes, entry
// order, redirection of loads past a row's end to entry 0, tree and serial
// adds.  red: [CP][kBlock / 64] (L = 256 only).
template <typename T, int L, int R, int U, int CP, bool ONES>
__device__ __forceinline__ void
csrm_rows(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
          const T* __restrict__ vals, const uint32_t* __restrict__ order,
          uint32_t first, uint32_t last, uint32_t blk, const T* __restrict__ x,
          const T* __restrict__ s_prev, const T* __restrict__ v_prev,
          T* __restrict__ s_next, T* __restrict__ v_cur, const T* __restrict__ u,
          const T* __restrict__ dots, uint32_t n, uint32_t C, uint32_t K,
          uint32_t act, const st_state* states, T (*red)[kBlock / 64])
{
  typedef typename CsrmVec<T, CP>::type V;
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
  V acc[R];
#pragma unroll
  for (int j = 0; j < R; j++)
    acc[j] = (V)(T)0;
  for (;;) {
    bool more = false;
#pragma unroll
    for (int j = 0; j < R; j++)
      more |= e[j] < end[j];
    if (!more)
      break;
    T a[R][U];
    V xs[R][U];
    bool in[R][U];
#pragma unroll
    for (int j = 0; j < R; j++)
#pragma unroll
      for (int q = 0; q < U; q++) {
        const uint64_t idx = e[j] + (uint64_t)q * L;
        in[j][q] = idx < end[j];
        const uint64_t at = in[j][q] ? idx : 0; // entry 0 exists: nnz >= 1
        a[j][q] = vals[at];
        if constexpr (ONES)
          xs[j][q] = (V)(T)1;
        else
          xs[j][q] = csrm_ld<T, CP>(x, (uint64_t)(uint32_t)col[at]);
      }
#pragma unroll
    for (int j = 0; j < R; j++) {
#pragma unroll
      for (int q = 0; q < U; q++) { // the row's entries in order
#pragma unroll
        for (int c = 0; c < CP; c++) {
          const T f = __builtin_fma(a[j][q], xs[j][q][c], acc[j][c]);
          acc[j][c] = in[j][q] ? f : acc[j][c];
        }
      }
      e[j] += (uint64_t)U * L;
    }
  }

  if constexpr (L <= 64) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      V tot;
#pragma unroll
      for (int c = 0; c < CP; c++)
        tot[c] = csr_lanes_sum<T, L>(acc[j][c]);
      if (live[j] && t == L - 1)
        csrm_finish<T, CP, ONES>(r[j], tot, x, s_prev, v_prev, s_next, v_cur, u,
                                 dots, n, C, K, act, states);
    }
  } else {
#pragma unroll
    for (int c = 0; c < CP; c++) {
      const T w = wave_sum(acc[0][c]);
      if ((threadIdx.x & 63) == 0)
        red[c][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (live[0] && threadIdx.x == 0) {
      V tot;
#pragma unroll
      for (int c = 0; c < CP; c++) {
        T s = red[c][0];
#pragma unroll
        for (int j = 1; j < kBlock / 64; j++)
          s += red[c][j];
        tot[c] = s;
      }
      csrm_finish<T, CP, ONES>(r[0], tot, x, s_prev, v_prev, s_next, v_cur, u,
                               dots, n, C, K, act, states);
    }
  }
}

// the class of this workgroup from the launch's own table (tab.blk_first is
// made from csr::multi_rows, not from the handle's kRows)
template <typename T, int CP, bool ONES>
__device__ __forceinline__ void
csrm_dispatch(const int64_t* row_ptr, const int32_t* col, const T* vals,
              const uint32_t* order, const CsrTab& tab, const T* x,
              const T* s_prev, const T* v_prev, T* s_next, T* v_cur, const T* u,
              const T* dots, uint32_t n, uint32_t C, uint32_t K, uint32_t act,
              const st_state* states, T (*red)[kBlock / 64])
{
  constexpr uint32_t RB = (uint32_t)(CP * sizeof(T)); // bytes of a packed row
  const uint32_t b = blockIdx.x;
  int c = 0; // workgroup-uniform
  while (c < csr::kClasses - 1 && b >= tab.blk_first[c + 1])
    c++;
  const uint32_t first = tab.row_first[c], last = tab.row_first[c + 1];
  const uint32_t blk = b - tab.blk_first[c];
#define ST_CSRM_ROWS(LL, CC)                                                       \
  csrm_rows<T, LL, (int)csr::multi_rows(CC, RB), (int)csr::multi_unroll(CC, RB),   \
            CP, ONES>(row_ptr, col, vals, order, first, last, blk, x, s_prev,  \
                      v_prev, s_next, v_cur, u, dots, n, C, K, act, states, red)
  static_assert(csr::kLanes[0] == 4 && csr::kLanes[1] == 16 &&
                  csr::kLanes[2] == 64 && csr::kLanes[3] == 256,
                "the class bodies below");
  if (c == 0)
    ST_CSRM_ROWS(4, 0);
  else if (c == 1)
    ST_CSRM_ROWS(16, 1);
  else if (c == 2)
    ST_CSRM_ROWS(64, 2);
  else
    ST_CSRM_ROWS(256, 3);
#undef ST_CSRM_ROWS
}

// K0 of every M_c: s[r][c] = (sum of row r of A) then fma(u_{c,j}[r], dots[c][j], .)
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_rowsum(const int64_t* row_ptr, const int32_t* col, const T* vals,
              const uint32_t* order, CsrTab tab, T* __restrict__ s,
              const T* __restrict__ u, const T* __restrict__ dots, uint32_t n,
              uint32_t C, uint32_t K)
{
  __shared__ T red[CP][kBlock / 64];
  csrm_dispatch<T, CP, true>(row_ptr, col, vals, order, tab, nullptr, nullptr,
                             nullptr, s, nullptr, u, dots, n, C, K,
                             (1u << CP) - 1u, nullptr, red);
}

// launch k >= 1, third launch: the row products of every live column
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_spmv(const int64_t* row_ptr, const int32_t* col, const T* vals,
            const uint32_t* order, CsrTab tab, const T* __restrict__ x,
            const T* __restrict__ s_prev, const T* __restrict__ v_prev,
            T* __restrict__ s_next, T* __restrict__ v_cur,
            const T* __restrict__ u, const T* __restrict__ dots, uint32_t n,
            uint32_t C, uint32_t K, uint32_t k, const st_state* states)
{
  const uint32_t act = csrm_active(states, C, k);
  if (act == 0)
    return;
  __shared__ T red[CP][kBlock / 64];
  csrm_dispatch<T, CP, false>(row_ptr, col, vals, order, tab, x, s_prev, v_prev,
                              s_next, v_cur, u, dots, n, C, K, act, states, red);
}

// the caller's dense vectors [n] -> one packed [n][CP] array; a null source
// is a padding column: its slots get 1
template <typename T, int CP>
struct CsrmSrc
{
  const T* p[CP];
};
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_pack(CsrmSrc<T, CP> src, T* __restrict__ dst, uint32_t n)
{
  typedef typename CsrmVec<T, CP>::type V;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    V row;
#pragma unroll
    for (int c = 0; c < CP; c++)
      row[c] = src.p[c] ? src.p[c][i] : (T)1;
    csrm_st<T, CP>(dst, i, row);
  }
}

// err[2 c + 1] = the lowest row whose s_0 of M_c is not finite and > 0
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_check_s0(const T* __restrict__ s0, uint32_t n, uint32_t C,
                unsigned long long* err)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const typename CsrmVec<T, CP>::type s = csrm_ld<T, CP>(s0, i);
#pragma unroll
    for (int c = 0; c < CP; c++)
      if ((uint32_t)c < C && (!(s[c] > (T)0) || s[c] - s[c] != (T)0))
        atomicMin(&err[2 * c + 1], (unsigned long long)i);
  }
}

// out[c][i] = the final v of column c (buffer end & 1 of the ping-pong pair,
// as k_csrb_collect), and res[c] = what the host reads of states[c]
template <typename T, int CP>
__global__ __launch_bounds__(kBlock) void
k_csrm_collect(const T* __restrict__ v0, const T* __restrict__ v1,
               T* __restrict__ out, const st_state* __restrict__ states,
               uint32_t n, uint32_t C, CsrBatchResult* __restrict__ res)
{
  typedef typename CsrmVec<T, CP>::type V;
  uint32_t odd = 0;
  for (uint32_t c = 0; c < C; c++)
    odd |= (states[c].end & 1u) << c;
  const uint32_t top = n > C ? n : C;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < top;
       i += (uint64_t)gridDim.x * kBlock) {
    if (i < n) {
      const V a = csrm_ld<T, CP>(v0, i), b = csrm_ld<T, CP>(v1, i);
#pragma unroll
      for (int c = 0; c < CP; c++)
        if ((uint32_t)c < C)
          out[(uint64_t)c * n + i] = ((odd >> c) & 1u) ? b[c] : a[c];
    }
    if (i < C) {
      CsrBatchResult r;
      r.lambda = states[i].lambda;
      r.iters = states[i].iters;
      r.stop = states[i].stop;
      r.end = states[i].end;
      r.done = states[i].done;
      res[i] = r;
    }
  }
}

} // namespace dev
} // namespace st
