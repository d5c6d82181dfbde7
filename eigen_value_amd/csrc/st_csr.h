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
template <typename T, int L, int R, int U, bool ONES>
__device__ __forceinline__ void
csr_rows(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
         const T* __restrict__ vals, const uint32_t* __restrict__ order,
         uint32_t first, uint32_t last, uint32_t blk, const T* __restrict__ x,
         const T* __restrict__ s_prev, const T* __restrict__ v_prev,
         T* __restrict__ s_next, T* __restrict__ v_cur, T m, T* red)
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
  T xr[R], sp[R], vp[R];
  if constexpr (!ONES) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      xr[j] = x[r[j]];
      sp[j] = s_prev[r[j]];
      vp[j] = v_prev[r[j]];
    }
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

  if constexpr (L <= 64) {
#pragma unroll
    for (int j = 0; j < R; j++) {
      const T tot = csr_lanes_sum<T, L>(acc[j]);
      if (live[j] && t == L - 1) {
        if constexpr (ONES) {
          s_next[r[j]] = tot;
        } else {
          s_next[r[j]] = tot / xr[j];
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
    if (live[0] && threadIdx.x == 0) {
      if constexpr (ONES) {
        s_next[r[0]] = tot;
      } else {
        s_next[r[0]] = tot / xr[0];
        v_cur[r[0]] = vp[0] * (sp[0] / m);
      }
    }
  }
}

template <typename T, bool ONES>
__device__ __forceinline__ void
csr_dispatch(const int64_t* row_ptr, const int32_t* col, const T* vals,
             const uint32_t* order, const CsrTab& tab, const T* x,
             const T* s_prev, const T* v_prev, T* s_next, T* v_cur, T m, T* red)
{
  const uint32_t b = blockIdx.x;
  int c = 0; // workgroup-uniform
  while (c < csr::kClasses - 1 && b >= tab.blk_first[c + 1])
    c++;
  const uint32_t first = tab.row_first[c], last = tab.row_first[c + 1];
  const uint32_t blk = b - tab.blk_first[c];
#define ST_CSR_ROWS(LL, CC)                                                        \
  csr_rows<T, LL, csr::kRows[CC], csr::kUnroll[CC], ONES>(                     \
    row_ptr, col, vals, order, first, last, blk, x, s_prev, v_prev, s_next,    \
    v_cur, m, red)
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

// launch k >= 1, first half: x, and round k-1's stats through the state
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_csr_prep(const T* __restrict__ s_prev, const T* __restrict__ v_prev,
           T* __restrict__ x, uint32_t n, T eps, uint32_t k, uint32_t max_itr,
           uint32_t semantics, st_state* state)
{
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
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const T sv = s_prev[i];
    x[i] = v_prev[i] * sv;
    mx = sv > mx ? sv : mx;
    if (i + 1 < n || cyclic) {
      const T d = sv - s_prev[i + 1 < n ? i + 1 : 0];
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
// cnt[block][class] = the block's rows of each class
__global__ __launch_bounds__(kBlock) void
k_csr_check_ptr(const int64_t* __restrict__ row_ptr, uint32_t n, uint64_t nnz,
                uint32_t* __restrict__ cnt, unsigned long long* err)
{
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  int cls = -1;
  if (r < n) {
    const int64_t a = row_ptr[r], b = row_ptr[r + 1];
    const bool bad = (r == 0 && a != 0) || b <= a ||
                     (r == (uint64_t)n - 1 && (uint64_t)b != nnz);
    if (bad)
      atomicMin(&err[0], (unsigned long long)r);
    else
      cls = csr_row_class(b - a);
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
