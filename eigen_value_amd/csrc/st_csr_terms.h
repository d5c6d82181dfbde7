// st_csr_terms.h — the matrix-free CSR round on the operator
//   M = A + sum_{j < K} u_j w_j^T,   1 <= K <= 4 (ST_CSR_TERMS_MAX),
// A a CSR handle (st_csr.h), u_j / w_j dense nonnegative device vectors [n]:
// the Google matrix of PageRank is alpha P^T plus one or two such terms.  No
// entry of M is stored; a term adds u_j[r] * (w_j . x) to row r.  For gfx950.
// Included by st_csr_terms.hip (the launchers); not a public header.
//
// The round is st_csr.h's with one launch in between:
//   k_csr_prep<T, CsrDots<T>>
//                     k_csr_prep's body (x, max / stop through the state)
//                     instantiated to also leave partial[j][workgroup], the
//                     workgroup's share of d_j = w_j . x
//   k_csr_dots        one workgroup: dots[j] = the sum of partial[j][*]
//   k_csr_terms_spmv  k_csr_spmv's row products under CsrTerms: after the
//                     lane tree tot = fma(u_j[r], dots[j], tot), j ascending,
//                     then the division
// K0 is the same with x ≡ 1: k_csr_wsum (the dot by fma against 1), k_csr_dots,
// k_csr_terms_rowsum.  All three launches of a round are no-ops once
// state->end says an earlier round stopped.  No float atomics; no workgroup
// waits on another: every dependency is a launch boundary.
//
// The order of a dot (fixed; a function of n alone - not of K, the other
// terms, the matrix or timing).  G = min(ceil(n / 256), 2048) workgroups of
// 256 lanes.  Lane t of workgroup b starts from 0 and takes the elements
// i = b * 256 + t + g * G * 256, g = 0, 1, ..., in ascending order, one
// fma(w[i], x[i], acc) each; the 64 lanes of a wave combine by wave_sum's
// DPP tree; the four wave sums are added in wave order (((w0 + w1) + w2) +
// w3) -> partial[j][b].  k_csr_dots: lane t starts from 0 and adds
// partial[j][t], partial[j][t + 256], ... in ascending order (at most 8),
// wave_sum, the four wave sums in wave order -> dots[j].  Terms are
// independent of each other: each has its own accumulator through every step.
// Worst-case depth of roundings for nonnegative data:
//   ceil(n / (256 G)) + 6 + 3   (the vector pass)
// + ceil(G / 256) + 6 + 3       (the combine).
#pragma once

#include "st_csr.h"

namespace st {
namespace dev {

constexpr uint32_t kCsrDotGrid = 2048; // = k_csr_prep's workgroup cap

// K0's dots: partial[j][b] of w_j . 1 in the vector pass's order
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_wsum(uint32_t n, CsrDots<T> d)
{
  T dacc[kCsrTermsMax];
#pragma unroll
  for (int q = 0; q < kCsrTermsMax; q++)
    dacc[q] = (T)0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      if ((uint32_t)q < d.K)
        dacc[q] = __builtin_fma(d.w[q][i], (T)1, dacc[q]);
  }
  csr_dot_partials<T>(dacc, d.K, d.partial);
}

// one workgroup: dots[j] = the sum of partial[j][0 .. P), j < K
// (state == nullptr: K0, never gated)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_dots(const T* __restrict__ partial, uint32_t P, uint32_t K,
           T* __restrict__ dots, uint32_t k, const st_state* state)
{
  if (state) {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T sh[kCsrTermsMax][kBlock / 64];
  for (uint32_t q = 0; q < K && q < (uint32_t)kCsrTermsMax; q++) {
    T acc = (T)0;
    for (uint32_t i = threadIdx.x; i < P; i += kBlock)
      acc += partial[(uint64_t)q * P + i];
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
    dots[threadIdx.x] = tot;
  }
}

// K0 of M: s[r] = (sum of row r of A) then fma(u_j[r], dots[j], .)
// (KM = 1, 2 or 4 >= K: the instantiation's registers, st_csr.h)
template <typename T, int KM>
__global__ __launch_bounds__(kBlock) void
k_csr_terms_rowsum(const int64_t* row_ptr, const int32_t* col, const T* vals,
                   const uint32_t* order, CsrTab tab, T* __restrict__ s,
                   CsrTerms<T, KM> g)
{
  __shared__ T red[kBlock / 64];
  csr_dispatch<T, true, CsrTerms<T, KM>>(row_ptr, col, vals, order, tab, nullptr,
                                         nullptr, nullptr, s, nullptr, (T)0, red,
                                         g);
}

template <typename T, int KM>
__global__ __launch_bounds__(kBlock) void
k_csr_terms_spmv(const int64_t* row_ptr, const int32_t* col, const T* vals,
                 const uint32_t* order, CsrTab tab, const T* __restrict__ x,
                 const T* __restrict__ s_prev, const T* __restrict__ v_prev,
                 T* __restrict__ s_next, T* __restrict__ v_cur, uint32_t k,
                 const st_state* state, CsrTerms<T, KM> g)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T red[kBlock / 64];
  const T m = (T)state->max; // published by k_csr_prep of this launch k
  csr_dispatch<T, false, CsrTerms<T, KM>>(row_ptr, col, vals, order, tab, x,
                                          s_prev, v_prev, s_next, v_cur, m, red,
                                          g);
}

// validation, one pass per terms object: err[0] = the lowest
// ((2 j + which) << 32 | i) whose entry is not finite and >= 0 (which: 0 = u,
// 1 = w; st_csr_host.h: term_entry_bad)
template <typename T>
struct CsrTermVecs
{
  uint32_t K;
  const T* u[kCsrTermsMax];
  const T* w[kCsrTermsMax];
};

template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_terms_check(CsrTermVecs<T> t, uint32_t n, unsigned long long* err)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int q = 0; q < kCsrTermsMax; q++)
      if ((uint32_t)q < t.K) {
        const T a = t.u[q][i], b = t.w[q][i];
        if (!(a >= (T)0) || a - a != (T)0)
          atomicMin(&err[0], ((unsigned long long)(2 * q) << 32) | i);
        if (!(b >= (T)0) || b - b != (T)0)
          atomicMin(&err[0], ((unsigned long long)(2 * q + 1) << 32) | i);
      }
  }
}

// err[1] = the lowest row whose s_0 (K0 of M) is not finite and > 0
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_terms_check_s0(const T* __restrict__ s0, uint32_t n, unsigned long long* err)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const T s = s0[i];
    if (!(s > (T)0) || s - s != (T)0)
      atomicMin(&err[1], (unsigned long long)i);
  }
}

} // namespace dev
} // namespace st
