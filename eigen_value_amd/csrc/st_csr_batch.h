// st_csr_batch.h — the CSR round (st_csr.h) for a BATCH of sparse matrices in
// one pair of launches per round, for gfx950.  Included by st_csr_batch.hip
// (the launchers) only; not a public header.
//
// Stacked CSR: `batch` matrices, matrix b of n_b rows from stacked row
// mat_first[b]; row_ptr int64 [N + 1] over the concatenated entries (N = Σ
// n_b); col_idx int32 [nnz] LOCAL to its matrix; vals [nnz].  All vectors (s,
// v, x) are stacked the same way, and there is one st_state per matrix.
//
// Why every matrix gets the bits of a solve on it alone:
//   - a row's product depends on its own entries and on x only, and its lane
//     class on its own nnz (st_csr.h), so the plan over the N stacked rows -
//     st_csr_plan of the stacked row_ptr - gives every row the lanes, the fma
//     order and the tree it has alone (csr_rows, unchanged but for CsrStack);
//   - max and the stop test fold with max / or through the matrix's own state
//     (stats_publish, unchanged), exact under any partition of its rows.
//
//   k_csrb_rowsum  K0 over the stacked rows (k_csr_rowsum's body)
//   k_csrb_prep    launch k >= 1, first half.  Workgroup w works for exactly
//                  one matrix: b with wg_first[b] <= w < wg_first[b + 1]
//                  (found by bisection of the uniform block index), as
//                  participant w - wg_first[b] of that matrix's
//                  wg_first[b + 1] - wg_first[b].  It is k_csr_prep on the
//                  matrix's slice: the cyclic pair of the last row wraps to
//                  the matrix's first row.  The participant that publishes a
//                  round that sets `end` adds 1 to *finished.
//   k_csrb_spmv    launch k >= 1, second half, over the batch's plan: per
//                  row the gate, m and the base of x come from the row's own
//                  matrix (CsrStack)
//   k_csrb_collect after the loop: matrix b's eigenvector lies in ping-pong
//                  buffer end_b & 1; and the B results in one array
// A matrix whose end is set and below k gets no writes at all.
#pragma once

#include "st_csr.h"
#include "st_internal.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

// row_mat[r] = the matrix of stacked row r
__global__ __launch_bounds__(kBlock) void
k_csrb_rowmat(const uint32_t* __restrict__ mat_first, uint32_t batch, uint32_t n,
              uint32_t* __restrict__ row_mat)
{
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n)
    return;
  uint32_t lo = 0, hi = batch;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (mat_first[mid] <= (uint32_t)r)
      lo = mid;
    else
      hi = mid;
  }
  row_mat[r] = lo;
}

// every column against its OWN matrix's n_b; 16 lanes share a row (rows past
// the grid: grid-stride).  Runs only after row_ptr passed, reads col_idx[0,
// nnz) only.  err[1] = the lowest offending entry.
__global__ __launch_bounds__(kBlock) void
k_csrb_check_col(const int64_t* __restrict__ row_ptr,
                 const int32_t* __restrict__ col,
                 const uint32_t* __restrict__ row_mat,
                 const uint32_t* __restrict__ mat_first, uint32_t n,
                 unsigned long long* err)
{
  constexpr uint32_t L = 16, RPB = kBlock / L;
  const uint32_t sub = threadIdx.x / L, t = threadIdx.x % L;
  for (uint64_t r = (uint64_t)blockIdx.x * RPB + sub; r < n;
       r += (uint64_t)gridDim.x * RPB) {
    const uint32_t b = row_mat[r];
    const uint32_t nb = mat_first[b + 1] - mat_first[b];
    const uint64_t end = (uint64_t)row_ptr[r + 1];
    for (uint64_t e = (uint64_t)row_ptr[r] + t; e < end; e += L) {
      const int32_t c = col[e];
      if (c < 0 || (uint32_t)c >= nb)
        atomicMin(&err[1], (unsigned long long)e);
    }
  }
}

// K0 over the stacked rows: s[r] = Σ a (x ≡ 1)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrb_rowsum(const int64_t* row_ptr, const int32_t* col, const T* vals,
              const uint32_t* order, CsrTab tab, T* __restrict__ s)
{
  __shared__ T red[kBlock / 64];
  csr_dispatch<T, true>(row_ptr, col, vals, order, tab, nullptr, nullptr,
                        nullptr, s, nullptr, (T)0, red);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrb_prep(const T* __restrict__ s_prev, const T* __restrict__ v_prev,
            T* __restrict__ x, const uint32_t* __restrict__ mat_first,
            const uint32_t* __restrict__ wg_first, uint32_t batch, T eps,
            uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* states,
            uint32_t* finished)
{
  uint32_t b = 0; // workgroup-uniform
  {
    uint32_t hi = batch;
    while (hi - b > 1) {
      const uint32_t mid = b + (hi - b) / 2;
      if (wg_first[mid] <= blockIdx.x)
        b = mid;
      else
        hi = mid;
    }
  }
  st_state* const state = states + b;
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  const uint32_t row0 = mat_first[b], n = mat_first[b + 1] - row0;
  const uint32_t part = blockIdx.x - wg_first[b];
  const uint32_t nwg = wg_first[b + 1] - wg_first[b];
  const T* __restrict__ s = s_prev + row0; // the matrix's own slices
  const T* __restrict__ v = v_prev + row0;
  T* __restrict__ xb = x + row0;
  __shared__ T mx_sh[kBlock / 64];
  const bool cyclic = semantics == ST_SEM_SYCL;
  T mx = (T)0; // find_max starts from 0 (cpp:185): negatives and NaN never win
  int fail = 0;
  for (uint64_t i = (uint64_t)part * kBlock + threadIdx.x; i < n;
       i += (uint64_t)nwg * kBlock) {
    const T sv = s[i];
    xb[i] = v[i] * sv;
    mx = sv > mx ? sv : mx;
    if (i + 1 < n || cyclic) { // the last row's pair wraps to the matrix's first
      const T d = sv - s[i + 1 < n ? i + 1 : 0];
      fail |= (d < (T)0 ? -d : d) < eps ? 0 : 1; // cpp:419-421; NaN fails
    }
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
    // round k-1 of matrix b: end = k when it stops or exhausts
    if (stats_publish<T>(m, fail, nwg, s, k - 1, max_itr, semantics, state) &&
        state->end == k)
      atomicAdd(finished, 1u);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrb_spmv(const int64_t* row_ptr, const int32_t* col, const T* vals,
            const uint32_t* order, CsrTab tab, const T* __restrict__ x,
            const T* __restrict__ s_prev, const T* __restrict__ v_prev,
            T* __restrict__ s_next, T* __restrict__ v_cur, CsrStack stack)
{
  __shared__ T red[kBlock / 64];
  csr_dispatch<T, false, CsrStack>(row_ptr, col, vals, order, tab, x, s_prev,
                                   v_prev, s_next, v_cur, (T)0, red, stack);
}

// out[r] = the final v of row r's matrix (buffer end & 1 of the ping-pong
// pair), and res[b] = what the host reads of states[b]
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csrb_collect(const T* __restrict__ v0, const T* __restrict__ v1,
               T* __restrict__ out, const uint32_t* __restrict__ row_mat,
               const st_state* __restrict__ states, uint32_t n, uint32_t batch,
               CsrBatchResult* __restrict__ res)
{
  const uint32_t top = n > batch ? n : batch;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < top;
       i += (uint64_t)gridDim.x * kBlock) {
    if (i < n)
      out[i] = (states[row_mat[i]].end & 1u) ? v1[i] : v0[i];
    if (i < batch) {
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
