// st_left.h — the matrix-free round for the LEFT Perron vector of a dense
// matrix (u A = lambda u), for gfx950.  Included by st_left.hip (the
// launchers); not a public header.
//
// The left round is k_mfree's iteration (st_device.h) with the sweep turned
// by 90 degrees: s_k[c] = (Σ_r A_0[r][c] x[r]) / x[c], x = v_{k-2} ∘ s_{k-1}.
// The matrix is read where it lies, row-major, N^2 b bytes per round; no
// transposed copy exists at any time.  A column sum needs no cross-lane
// reduction: a lane owns its columns and walks down the rows.
//
//   launch 0   k_colsum + k_left_finish<ONES>: s_0[c] = Σ_r A[r][c], the same
//              fma with 1 (as the CSR K0)
//   launch k   k_csr_prep<T> as it stands (st_csr.h): x to scratch, round
//              k-1's max / stop through st_state, the last workgroup publishes
//              k_left_sweep: part[rb][c] = the column products of row block rb
//              k_left_finish: s_next[c] = (Σ_rb part[rb][c]) / x[c] and
//              v_cur[c] = v_prev[c] * (s_prev[c] / m), m from the state
// every one a no-op once state->end says an earlier round stopped.  No float
// atomics, no workgroup waits on another: every dependency is a launch
// boundary.
//
// Summation order of a column (fixed): the rows are cut into blocks of RB
// consecutive rows (the last one shorter); within a block one accumulator
// starts from 0 and takes the rows in ascending order, one fused multiply-add
// each, acc = fma(A[r][c], x[r], acc); the block values are then added
// SERIALLY in ascending block order, starting from block 0's value (not from
// 0).  RB is a function of (dtype, n) alone (left_rows, st_left.hip;
// published by st_left_shape with combine = 0, serial), so a column's sum
// depends on n, the dtype, that column's entries and x only - not on the
// grid, the strip a column falls in, the vector width, the rows in flight or
// the kind of load.
//
// A workgroup owns RB rows by one strip of BLK * W columns; a lane owns W
// adjacent columns (16 bytes per load when n * b is a multiple of 16 and the
// matrix is 16-byte aligned, else W = 1: rows after the first are not
// aligned then) and keeps W accumulators.  Adjacent lanes read adjacent
// addresses, so the stream is coalesced exactly as k_mfree's.  U rows'
// vectors are issued before the first fma.  x[r] is uniform across the
// workgroup (a scalar load).  A lane whose first column is >= n does nothing
// and rows stop at n: nothing outside A is read.
#pragma once

#include "st_csr.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

constexpr int kLeftUnroll = 8; // rows in flight per lane

// part[tile][c] for the tile's rows [tile * rb, min(n, (tile + 1) * rb)) and
// the lane's W columns.  ONES: x ≡ 1 and no gate (launch 0).
// blockIdx.x = tile * nstrips + strip.
template <typename T, int W, int U, bool NT, bool ONES>
__device__ __forceinline__ void
left_tile(const T* __restrict__ a, const T* __restrict__ x, T* __restrict__ part,
          uint32_t n, uint32_t rb, uint32_t nstrips)
{
  using V = typename vec<T, W>::type;
  const uint32_t strip = blockIdx.x % nstrips;
  const uint32_t tile = blockIdx.x / nstrips;
  const uint64_t c0 = ((uint64_t)strip * kBlock + threadIdx.x) * W;
  if (c0 >= n) // (W > 1: n % W == 0, so c0 + W <= n for every other lane)
    return;
  const uint64_t r0 = (uint64_t)tile * rb;
  const uint64_t r1 = r0 + rb < n ? r0 + rb : n;
  const T* p = a + r0 * n + c0;
  T acc[W];
#pragma unroll
  for (int i = 0; i < W; i++)
    acc[i] = (T)0;
  uint64_t r = r0;
  for (; r + U <= r1; r += U) {
    V m[U];
    T xr[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      m[u] = ld<V, NT>(reinterpret_cast<const V*>(p + (uint64_t)u * n));
#pragma unroll
    for (int u = 0; u < U; u++)
      xr[u] = ONES ? (T)1 : x[r + u];
#pragma unroll
    for (int u = 0; u < U; u++) {
      if constexpr (W == 1) {
        acc[0] = __builtin_fma(m[u], xr[u], acc[0]);
      } else {
#pragma unroll
        for (int i = 0; i < W; i++)
          acc[i] = __builtin_fma(m[u][i], xr[u], acc[i]);
      }
    }
    p += (uint64_t)U * n;
  }
  for (; r < r1; r++) { // the block's last rows, fewer than U
    const V m = ld<V, NT>(reinterpret_cast<const V*>(p));
    const T xr = ONES ? (T)1 : x[r];
    if constexpr (W == 1) {
      acc[0] = __builtin_fma(m, xr, acc[0]);
    } else {
#pragma unroll
      for (int i = 0; i < W; i++)
        acc[i] = __builtin_fma(m[i], xr, acc[i]);
    }
    p += n;
  }
  T* q = part + (uint64_t)tile * n + c0;
  if constexpr (W == 1) {
    q[0] = acc[0];
  } else {
    V o;
#pragma unroll
    for (int i = 0; i < W; i++)
      o[i] = acc[i];
    *reinterpret_cast<V*>(q) = o;
  }
}

// launch 0, first half
template <typename T, int W, int U, bool NT>
__global__ __launch_bounds__(kBlock) void
k_colsum(const T* __restrict__ a, T* __restrict__ part, uint32_t n, uint32_t rb,
         uint32_t nstrips)
{
  left_tile<T, W, U, NT, true>(a, nullptr, part, n, rb, nstrips);
}

// launch k >= 1, second of three
template <typename T, int W, int U, bool NT>
__global__ __launch_bounds__(kBlock) void
k_left_sweep(const T* __restrict__ a, const T* __restrict__ x, T* __restrict__ part,
             uint32_t n, uint32_t rb, uint32_t nstrips, uint32_t k,
             const st_state* state)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  left_tile<T, W, U, NT, false>(a, x, part, n, rb, nstrips);
}

constexpr int kLeftFinishBlock = 64;

// the partials of a column in ascending block order, serially; ONES (launch
// 0): s_next[c] = t, nothing else read or written
template <typename T, bool ONES>
__global__ __launch_bounds__(kLeftFinishBlock) void
k_left_finish(const T* __restrict__ part, uint32_t nrb, const T* __restrict__ x,
              const T* __restrict__ s_prev, const T* __restrict__ v_prev,
              T* __restrict__ s_next, T* __restrict__ v_cur, uint32_t n, uint32_t k,
              const st_state* state)
{
  T m = (T)0;
  if constexpr (!ONES) {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
    m = (T)state->max; // published by k_csr_prep of this launch k
  }
  const uint64_t c = (uint64_t)blockIdx.x * kLeftFinishBlock + threadIdx.x;
  if (c >= n)
    return;
  T xc = (T)0, sp = (T)0, vp = (T)0; // asked for before the walk
  if constexpr (!ONES) {
    xc = x[c];
    sp = s_prev[c];
    vp = v_prev[c];
  }
  const T* p = part + c;
  T t = p[0];
  uint32_t j = 1;
  constexpr int UF = 16;
  for (; j + UF <= nrb; j += UF) {
    T q[UF];
#pragma unroll
    for (int u = 0; u < UF; u++)
      q[u] = p[(uint64_t)(j + u) * n];
#pragma unroll
    for (int u = 0; u < UF; u++)
      t += q[u];
  }
  for (; j < nrb; j++)
    t += p[(uint64_t)j * n];
  if constexpr (ONES) {
    s_next[c] = t;
  } else {
    s_next[c] = t / xc;
    v_cur[c] = vp * (sp / m); // k_mfree's v update (cpp:260)
  }
}

} // namespace dev
} // namespace st
