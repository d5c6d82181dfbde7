// st_csr_plan.h — the kernels that validate a CSR matrix and build its plan
// (rows sorted by class), for gfx950.  Not templates, so included by
// st_csr.hip alone; st_csr_batch.hip reaches them through st_csr.hip's
// launchers (launch_csr_check_ptr, launch_csr_plan), because the plan of a
// stacked batch is the plan of its stacked row_ptr.  Not a public header.
#pragma once

#include "st_csr.h"

namespace st {
namespace dev {

// ---------------------------------------------------------------------------
// validation and plan, once per matrix (st_csr_create).  Nothing here reads
// col_idx or vals except k_csr_check_col, which reads col_idx[0, nnz) only
// and runs only after row_ptr passed.
// ---------------------------------------------------------------------------
// err[0] = the lowest offending row, err[1] = the lowest offending entry
// (both start at ~0)
__device__ __forceinline__ int
csr_row_class(int64_t len)
{
  int c = 0;
  while (c < csr::kClasses - 1 && (uint64_t)len > csr::kNnzMax[c])
    c++;
  return c;
}

// one row per lane: the row_ptr predicate of st_csr_host.h (row_bad), and
// cnt[block][class] = the block's rows of each class.  empty != nullptr
// (ST_CSR_EMPTY_ROWS_OK): a row of no entries is legal and of class 0;
// *empty counts such rows (an integer count does not depend on the order of
// its increments) and err[1] takes the lowest one.
__global__ __launch_bounds__(kBlock) void
k_csr_check_ptr(const int64_t* __restrict__ row_ptr, uint32_t n, uint64_t nnz,
                uint32_t* __restrict__ cnt, unsigned long long* err,
                uint32_t* empty)
{
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  int cls = -1;
  if (r < n) {
    const int64_t a = row_ptr[r], b = row_ptr[r + 1];
    const bool bad = (r == 0 && a != 0) || (empty ? b < a : b <= a) ||
                     (r == (uint64_t)n - 1 && (uint64_t)b != nnz);
    if (bad)
      atomicMin(&err[0], (unsigned long long)r);
    else {
      cls = csr_row_class(b - a);
      if (b == a) {
        atomicMin(&err[1], (unsigned long long)r);
        atomicAdd(empty, 1u);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < csr::kClasses; c++) {
    const int k = __syncthreads_count(cls == c);
    if (threadIdx.x == 0)
      cnt[(uint64_t)blockIdx.x * csr::kClasses + c] = (uint32_t)k;
  }
}

__global__ __launch_bounds__(kBlock) void
k_csr_check_col(const int32_t* __restrict__ col, uint32_t n, uint64_t nnz,
                unsigned long long* err)
{
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (uint64_t)gridDim.x * kBlock) {
    const int32_t c = col[e];
    if (c < 0 || (uint32_t)c >= n)
      atomicMin(&err[1], (unsigned long long)e);
  }
}

// one workgroup: cnt[nblk][class] -> where the block's rows of that class
// start in the plan (in place), and class_first[kClasses + 1]
__global__ __launch_bounds__(kBlock) void
k_csr_scan(uint32_t* __restrict__ cnt, uint32_t nblk,
           uint32_t* __restrict__ class_first)
{
  __shared__ uint32_t part[kBlock][csr::kClasses];
  __shared__ uint32_t cf[csr::kClasses + 1];
  const uint32_t per = (nblk + kBlock - 1) / kBlock;
  const uint64_t lo64 = (uint64_t)threadIdx.x * per;
  const uint32_t lo = lo64 < nblk ? (uint32_t)lo64 : nblk;
  const uint32_t hi = lo64 + per < nblk ? (uint32_t)(lo64 + per) : nblk;
  uint32_t sum[csr::kClasses] = { 0, 0, 0, 0 };
  for (uint32_t b = lo; b < hi; b++)
#pragma unroll
    for (int c = 0; c < csr::kClasses; c++)
      sum[c] += cnt[(uint64_t)b * csr::kClasses + c];
#pragma unroll
  for (int c = 0; c < csr::kClasses; c++)
    part[threadIdx.x][c] = sum[c];
  __syncthreads();
  if (threadIdx.x < csr::kClasses) { // exclusive scan over the 256 spans
    uint32_t run = 0;
    for (int t = 0; t < kBlock; t++) {
      const uint32_t v = part[t][threadIdx.x];
      part[t][threadIdx.x] = run;
      run += v;
    }
    cf[threadIdx.x + 1] = run; // the class's total, for now
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cf[0] = 0;
    for (int c = 0; c < csr::kClasses; c++)
      cf[c + 1] += cf[c];
    for (int c = 0; c <= csr::kClasses; c++)
      class_first[c] = cf[c];
  }
  __syncthreads();
  uint32_t run[csr::kClasses];
#pragma unroll
  for (int c = 0; c < csr::kClasses; c++)
    run[c] = cf[c] + part[threadIdx.x][c];
  for (uint32_t b = lo; b < hi; b++)
#pragma unroll
    for (int c = 0; c < csr::kClasses; c++) {
      const uint32_t v = cnt[(uint64_t)b * csr::kClasses + c];
      cnt[(uint64_t)b * csr::kClasses + c] = run[c];
      run[c] += v;
    }
}

// order[base[block][class] + the row's rank among the block's rows of its
// class] = row: stable within a class
__global__ __launch_bounds__(kBlock) void
k_csr_order(const int64_t* __restrict__ row_ptr, uint32_t n,
            const uint32_t* __restrict__ base, uint32_t* __restrict__ order)
{
  __shared__ uint32_t wcnt[kBlock / 64][csr::kClasses];
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cls = -1;
  if (r < n)
    cls = csr_row_class(row_ptr[r + 1] - row_ptr[r]);
  uint32_t rank = 0;
#pragma unroll
  for (int c = 0; c < csr::kClasses; c++) {
    const unsigned long long mask = __ballot(cls == c);
    if (cls == c)
      rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0)
      wcnt[wave][c] = (uint32_t)__popcll(mask);
  }
  __syncthreads();
  if (cls >= 0) {
    uint32_t at = base[(uint64_t)blockIdx.x * csr::kClasses + cls] + rank;
    for (int w = 0; w < wave; w++)
      at += wcnt[w][cls];
    if (at < n) // always, for a row_ptr that did not change since the check
      order[at] = (uint32_t)r;
  }
}

} // namespace dev
} // namespace st
