// st_pair.h — the matrix-free round for BOTH Perron vectors of a dense
// matrix (A v = lambda v and u A = lambda u) from one pass over A, for gfx950.
// Included by st_pair.hip (the launchers); not a public header.
//
// Two independent iterations - side 0 the right one, s_R = (A x_R) / x_R as
// k_mfree's, side 1 the left one, s_L = (x_L^T A) / x_L as st_left.h's - with
// a state, an s and a v ping-pong pair and a stop round each.  They share the
// loads of A and nothing else.
//
//   launch 0   k_pair_sum + k_left_finish<ONES> twice: both s_0 (x ≡ 1)
//   launch k   k_csr_prep<T> as it stands (st_csr.h) once per side: x_R / x_L
//              to scratch, round k-1's max / stop through that side's state
//              k_pair_sweep: colpart[tile][c] = the column products of the
//              tile's rows (left_tile's arithmetic), rowpart[strip][r] = the
//              row products of the strip's columns
//              k_left_finish as it stands (st_left.h) once per side: the
//              partials of a column (a row) added serially, / x, and v_cur
// every one a no-op for a side whose state->end says an earlier round
// stopped.  No float atomics, no workgroup waits on another.
//
// Order of a column: st_left.h's, unchanged (RB rows per block, serial fma,
// blocks added serially).  Order of a row (fixed): the row is cut into strips
// of S = 256 * Wc columns, Wc = 16 / sizeof(T); in a strip lane l takes
// columns strip * S + l * Wc + i, i ascending, t = fma(A[r][c], x[c], t) from
// 0 (columns >= n left out); the 64 lanes of a wave go through wave_sum's
// tree, the four wave sums are added serially in wave order, and the strip
// values serially in ascending strip order, starting from strip 0's value.
// Neither the grid, RB, the rows in flight nor the kind of load enters.
//
// A workgroup owns RB rows by one strip; a lane owns Wc adjacent columns, one
// 16-byte load when VEC (n * b a multiple of 16, matrix and scratch 16-byte
// aligned), else the same columns element-wide.  Lanes past n load nothing
// and hold +0, but stay for the tree and the barrier.  U rows' loads are
// issued before the first fma; the U row values go through wave_sum_rows
// together; lane 63 of each wave leaves them in LDS, and after the tile's last
// row - one barrier - lane t adds row t's four wave sums.
#pragma once

#include "st_left.h"
#include "st_pair_host.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

constexpr int kPairChunk = (int)pair::kChunkRows; // rows per LDS flush
static_assert(kPairChunk == kBlock && kPairChunk % kLeftUnroll == 0,
              "one lane per row at the flush; whole groups of rows per chunk");

// one tile: rows [tile * rb, min(n, (tile + 1) * rb)) by the strip's columns.
// ONES: x ≡ 1 on both sides (launch 0).  LEFT / RIGHT: the halves that run
// (workgroup-uniform; a half that does not run writes nothing).
template <typename T, bool VEC, int U, bool NT, bool ONES, bool LEFT, bool RIGHT>
__device__ __forceinline__ void
pair_tile(const T* __restrict__ a, const T* __restrict__ xr, const T* __restrict__ xl,
          T* __restrict__ colpart, T* __restrict__ rowpart, uint32_t n, uint32_t rb,
          uint32_t nstrips, T (*red)[kPairChunk])
{
  constexpr int W = 16 / sizeof(T);
  using V = typename vec<T, W>::type;
  const uint32_t strip = blockIdx.x % nstrips;
  const uint32_t tile = blockIdx.x / nstrips;
  const uint64_t c0 = ((uint64_t)strip * kBlock + threadIdx.x) * W;
  // this lane's columns below n (VEC: 0 or W)
  const int nc = c0 >= n ? 0 : (n - c0 < (uint64_t)W ? (int)(n - c0) : W);
  const uint64_t r0 = (uint64_t)tile * rb;
  const uint64_t r1 = r0 + rb < n ? r0 + rb : n;
  const T* p = a + r0 * n + (nc ? c0 : 0);
  const uint32_t wave = threadIdx.x >> 6;
  const bool last_lane = (threadIdx.x & 63u) == 63u;

  T xv[W]; // the lane's x_R, once per tile; +0 beyond n
  if constexpr (RIGHT) {
#pragma unroll
    for (int i = 0; i < W; i++)
      xv[i] = i < nc ? (ONES ? (T)1 : xr[c0 + i]) : (T)0;
  }
  T acc[W];
#pragma unroll
  for (int i = 0; i < W; i++)
    acc[i] = (T)0;

  for (uint64_t lo = r0; lo < r1; lo += kPairChunk) {
    const uint64_t hi = lo + kPairChunk < r1 ? lo + kPairChunk : r1;
    uint64_t r = lo;
    for (; r + U <= hi; r += U) {
      T m[U][W];
      if constexpr (VEC) {
        if (nc) {
#pragma unroll
          for (int u = 0; u < U; u++) {
            const V q = ld<V, NT>(reinterpret_cast<const V*>(p + (uint64_t)u * n));
#pragma unroll
            for (int i = 0; i < W; i++)
              m[u][i] = q[i];
          }
        } else {
#pragma unroll
          for (int u = 0; u < U; u++)
#pragma unroll
            for (int i = 0; i < W; i++)
              m[u][i] = (T)0;
        }
      } else {
#pragma unroll
        for (int i = 0; i < W; i++) {
          if (i < nc) {
#pragma unroll
            for (int u = 0; u < U; u++)
              m[u][i] = ld<T, NT>(p + (uint64_t)u * n + i);
          } else {
#pragma unroll
            for (int u = 0; u < U; u++)
              m[u][i] = (T)0;
          }
        }
      }
      if constexpr (LEFT) {
        T xs[U];
#pragma unroll
        for (int u = 0; u < U; u++)
          xs[u] = ONES ? (T)1 : xl[r + u];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int i = 0; i < W; i++)
            acc[i] = __builtin_fma(m[u][i], xs[u], acc[i]);
      }
      if constexpr (RIGHT) {
        T t[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          t[u] = (T)0;
#pragma unroll
          for (int i = 0; i < W; i++)
            t[u] = __builtin_fma(m[u][i], xv[i], t[u]); // (0 * 0 + t = t beyond n)
        }
        wave_sum_rows<T, U>(t);
        if (last_lane) {
#pragma unroll
          for (int u = 0; u < U; u++)
            red[wave][(uint32_t)(r - lo) + u] = t[u];
        }
      }
      p += (uint64_t)U * n;
    }
    for (; r < hi; r++) { // the tile's last rows, fewer than U
      T m[W];
      if constexpr (VEC) {
        V q;
#pragma unroll
        for (int i = 0; i < W; i++)
          q[i] = (T)0;
        if (nc)
          q = ld<V, NT>(reinterpret_cast<const V*>(p));
#pragma unroll
        for (int i = 0; i < W; i++)
          m[i] = q[i];
      } else {
#pragma unroll
        for (int i = 0; i < W; i++)
          m[i] = i < nc ? ld<T, NT>(p + i) : (T)0;
      }
      if constexpr (LEFT) {
        const T xs = ONES ? (T)1 : xl[r];
#pragma unroll
        for (int i = 0; i < W; i++)
          acc[i] = __builtin_fma(m[i], xs, acc[i]);
      }
      if constexpr (RIGHT) {
        T t = (T)0;
#pragma unroll
        for (int i = 0; i < W; i++)
          t = __builtin_fma(m[i], xv[i], t);
        t = wave_sum_l63(t);
        if (last_lane)
          red[wave][(uint32_t)(r - lo)] = t;
      }
      p += n;
    }
    if constexpr (RIGHT) {
      __syncthreads();
      if (threadIdx.x < (uint32_t)(hi - lo)) {
        T s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBlock / 64; w++)
          s += red[w][threadIdx.x];
        rowpart[(uint64_t)strip * n + lo + threadIdx.x] = s;
      }
      if (hi < r1) // (a tuning override of RB above kPairChunk only)
        __syncthreads();
    }
  }
  if constexpr (LEFT) {
    T* q = colpart + (uint64_t)tile * n + c0;
    if constexpr (VEC) {
      if (nc) {
        V o;
#pragma unroll
        for (int i = 0; i < W; i++)
          o[i] = acc[i];
        *reinterpret_cast<V*>(q) = o;
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; i++)
        if (i < nc)
          q[i] = acc[i];
    }
  }
}

// launch 0: both s_0's partials
template <typename T, bool VEC, int U, bool NT>
__global__ __launch_bounds__(kBlock) void
k_pair_sum(const T* __restrict__ a, T* __restrict__ colpart, T* __restrict__ rowpart,
           uint32_t n, uint32_t rb, uint32_t nstrips)
{
  __shared__ T red[kBlock / 64][kPairChunk];
  pair_tile<T, VEC, U, NT, true, true, true>(a, nullptr, nullptr, colpart, rowpart, n, rb,
                                             nstrips, red);
}

// launch k >= 1, third of five; states[0]: the right side, states[1]: the left
template <typename T, bool VEC, int U, bool NT>
__global__ __launch_bounds__(kBlock) void
k_pair_sweep(const T* __restrict__ a, const T* __restrict__ xr, const T* __restrict__ xl,
             T* __restrict__ colpart, T* __restrict__ rowpart, uint32_t n, uint32_t rb,
             uint32_t nstrips, uint32_t k, const st_state* states)
{
  __shared__ T red[kBlock / 64][kPairChunk];
  const uint32_t er = __hip_atomic_load(&states[pair::kRight].end, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t el = __hip_atomic_load(&states[pair::kLeft].end, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
  const bool right = !(er != 0 && er < k);
  const bool left = !(el != 0 && el < k);
  if (left && right)
    pair_tile<T, VEC, U, NT, false, true, true>(a, xr, xl, colpart, rowpart, n, rb, nstrips,
                                                red);
  else if (left)
    pair_tile<T, VEC, U, NT, false, true, false>(a, xr, xl, colpart, rowpart, n, rb,
                                                 nstrips, red);
  else if (right)
    pair_tile<T, VEC, U, NT, false, false, true>(a, xr, xl, colpart, rowpart, n, rb,
                                                 nstrips, red);
}

// the end of a round of the solve loop: the sides that are done, for the
// host's one word per check (one lane, a plain store)
__global__ __launch_bounds__(64) void
k_pair_count(const st_state* __restrict__ states, uint32_t* __restrict__ count)
{
  if (threadIdx.x == 0 && blockIdx.x == 0)
    *count = states[pair::kRight].done + states[pair::kLeft].done;
}

} // namespace dev
} // namespace st
