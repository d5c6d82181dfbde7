// st_csr_product.h — the matrix-free CSR round on the PRODUCT operator
//   M = B A,
// A and B two CSR handles (st_csr.h) of the same n, dtype and device (the same
// handle twice gives A^2).  No entry of M is stored: s = (B (A x)) ⊘ x is two
// CSR row products.  HITS (A^T A), the spectral norm, SALSA, two-step chains
// and bipartite projections are such operators.  For gfx950.  Included by
// st_csr_product.hip (the launchers); not a public header.
//
// The round (launch k >= 1) is three launches:
//   k_csr_prep<T>   unchanged (st_csr.h): x = v_prev ∘ s_prev to scratch, max /
//                   stop of s_prev and round k-1 through the state
//   k_csrp_apply    over A's plan: y[r] = Σ a x[col] - csr_rows under CsrPlain:
//                   the row order of st_csr.h (lane t of L, fma in storage
//                   order, the cut DPP tree, four wave sums serially for L =
//                   256), no division, no v; an empty row of A (legal under
//                   ST_CSR_EMPTY_ROWS_OK) takes no trip through the sweep and
//                   writes exactly 0
//   k_csrp_final    over B's plan, csr_rows under CsrDivisor: tot = Σ b y[col]
//                   in the same order, s_next[r] = tot / x[r] (the divisor is
//                   x, not the gathered vector) and v_cur[r] = v_prev[r] *
//                   (s_prev[r] / m), m from the state
// all no-ops once state->end says an earlier round stopped.  K0 is
// k_csr_rowsum of A into y, then k_csrp_apply of B on y (never gated).  No
// float atomics; no workgroup waits on another: every dependency is a launch
// boundary.  A row's result depends only on its own entries and the gathered
// vector.
//
// With the identity as one factor every bit is st_csr.h's round on the other:
// fma(1, x, 0) = x, and the tree adds zeros to it.
#pragma once

#include "st_csr.h"

namespace st {
namespace dev {

// y[r] = Σ a x[col] over the handle's plan (state == nullptr: never gated -
// K0's second half and st_csr_apply)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrp_apply(const int64_t* row_ptr, const int32_t* col, const T* vals,
             const uint32_t* order, CsrTab tab, const T* __restrict__ x,
             T* __restrict__ y, uint32_t k, const st_state* state)
{
  if (state) {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T red[kBlock / 64];
  csr_dispatch<T, false, CsrPlain>(row_ptr, col, vals, order, tab, x, nullptr,
                                   nullptr, y, nullptr, (T)0, red);
}

// launch k >= 1, last third: B's row products on y, the division by x and
// the v update
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrp_final(const int64_t* row_ptr, const int32_t* col, const T* vals,
             const uint32_t* order, CsrTab tab, const T* __restrict__ y,
             const T* __restrict__ x, const T* __restrict__ s_prev,
             const T* __restrict__ v_prev, T* __restrict__ s_next,
             T* __restrict__ v_cur, uint32_t k, const st_state* state)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ T red[kBlock / 64];
  const T m = (T)state->max; // published by k_csr_prep of this launch k
  CsrDivisor<T> g;
  g.xdiv = x;
  csr_dispatch<T, false, CsrDivisor<T>>(row_ptr, col, vals, order, tab, y, s_prev,
                                        v_prev, s_next, v_cur, m, red, g);
}

// validation: err[0] = the lowest row whose s_0 (K0 of B A) is not finite and
// > 0 (st_csr_host.h: product_row_bad)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrp_check_s0(const T* __restrict__ s0, uint32_t n, unsigned long long* err)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const T s = s0[i];
    if (!(s > (T)0) || s - s != (T)0)
      atomicMin(&err[0], (unsigned long long)i);
  }
}

} // namespace dev
} // namespace st
