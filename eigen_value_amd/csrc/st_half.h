// st_half.h — the matrix-free round on a matrix STORED in 16 bits (IEEE
// binary16 or bfloat16) with fp32 arithmetic, for gfx950.  Included by
// st_half.hip (the launchers); not a public header.
//
// The matrix-free round (k_mfree, st_device.h) never writes the matrix: it
// reads A_0 once per round and keeps all of its state in vectors.  So A_0 can
// sit in HBM at 2 bytes per element and be widened in registers - bf16 by a
// shift / mask of the packed dword, fp16 by v_cvt_f32_f16, both exact - and
// everything after the load is k_mfree<float>'s arithmetic: N^2 * 2 bytes per
// round.  No fp32 copy of the matrix exists anywhere.
//
// The sweep (half_group): a lane takes CHUNKS of 8 consecutive columns (one
// 16-byte load), lane t the chunks t, t + 256, ... of the row, U chunks in
// flight; per chunk it needs 8 values of s and 8 of v (x = v ∘ s, rounded to
// fp32 as k_mfree does), shared by the R rows of the group.  8 elements per
// lane rather than k_mfree<float>'s 4 because an 8-byte access runs at 0.54 -
// 0.70x the 16-byte rate on this part, so the lane -> column map, and with it
// the association of a row's sum, differs from the fp32 kernel's.
//
// Summation order of a row (fixed, no atomics): the lane's fused multiply-adds
// in column order (chunk by chunk, 8 per chunk), wave_sum's DPP tree over the
// 64 lanes, then the 4 wave partials added serially in wave order - the
// structure of mfree_group with 8 columns per chunk.
//
// The element-wide path (ncols % 8 != 0 or a pointer off 16 bytes) loads the
// same 8 columns of a chunk one element at a time, columns past the row as
// zeros, into the same packed registers: the same lanes hold the same
// numbers, so both paths give the same bits.
//
// The fold of max / stop over s_{k-1} is half_group's own (its STATS block):
// 8 columns per lane and chunk where mfree_group has 4, the chunk's last
// column paired with s_prev[next chunk] or s_prev[0], zeros past the row on
// the element-wide path.  max and the stop conjunction do not depend on the
// order of the fold, so the results are k_mfree<float>'s; which pair and
// which element it visits is pinned by tests/test_gpu_stats_positions.py
// (test_mfree_half_round*), position by position.  The rest that does not
// touch the matrix - the v update, the state bookkeeping, the gating on
// state->end - is k_mfree's code.
#pragma once

// wave_sum, ld<>, sweep_tail, kBlock: the templates of st_device.h, without
// its two non-template kernels (they live in st_kernels.hip's unit)
#define ST_DEVICE_TEMPLATES_ONLY 1
#include "st_device.h"

#pragma clang fp contract(off)

namespace st {
namespace dev {

// storage tags: the matrix is addressed as 16-bit patterns
struct StoreF16
{
};
struct StoreBF16
{
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kHalfW = 8;    // columns per chunk: one 16-byte load
constexpr int kHalfRows = 8; // most rows per group (red[][kHalfRows])

// the two elements of a packed dword (element 2j in the low half), exact
template <typename S>
__device__ __forceinline__ void
widen2(uint32_t d, float& lo, float& hi)
{
  if constexpr (std::is_same<S, StoreBF16>::value) {
    lo = __uint_as_float(d << 16);
    hi = __uint_as_float(d & 0xffff0000u);
  } else {
    const f16x2 p = __builtin_bit_cast(f16x2, d);
    lo = (float)p[0];
    hi = (float)p[1];
  }
}

// One group of R rows [rbase, rbase + R) over the full width.
//   VEC    16-byte loads (ncols % 8 == 0, 16-byte aligned a0 / s_prev / v_prev)
//   ONES   x ≡ 1 and no division: the plain row sums (K0)
//   XV     x is read from xvec (precomputed v_prev ∘ s_prev) instead of being
//          formed from s and v (the A/B of the x stream; probe builds)
//   STATS  fold max / stop of s_prev into mx / ok (the workgroup's first group)
template <typename S, int R, int U, bool VEC, bool NT, bool ONES, bool XV,
          bool STATS, int BLK>
__device__ __forceinline__ void
half_group(const uint16_t* a0, const float* __restrict__ s_prev,
           const float* __restrict__ v_prev, const float* __restrict__ xvec,
           float* __restrict__ s_next, uint32_t rbase, uint32_t ncols,
           uint32_t row0, bool cyclic, float eps, float& mx, int& ok,
           float (*red)[kHalfRows])
{
  static_assert(R <= kHalfRows, "red[] holds kHalfRows rows");
  constexpr int W = kHalfW;
  const uint32_t nch = (ncols + W - 1) / W; // chunks of a row (the last ragged)
  const uint16_t* rows[R];
  float acc[R];
#pragma unroll
  for (int j = 0; j < R; j++) {
    rows[j] = a0 + (size_t)(rbase + j) * ncols;
    acc[j] = 0.f;
  }
  // 8 floats of a vector at chunk q (zeros past ncols on the element path)
  auto ld8 = [&](const float* p, uint32_t q, float (&o)[W]) {
    if constexpr (VEC) {
      const f32x4 lo = reinterpret_cast<const f32x4*>(p)[2 * q];
      const f32x4 hi = reinterpret_cast<const f32x4*>(p)[2 * q + 1];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        o[i] = lo[i];
        o[4 + i] = hi[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; i++) {
        const uint32_t col = q * W + i;
        o[i] = col < ncols ? p[col] : 0.f;
      }
    }
  };
  auto body = [&](uint32_t c, auto ucount) {
    constexpr int UU = decltype(ucount)::value;
    u32x4 m[UU][R];
    float xs[UU][W];
#pragma unroll
    for (int u = 0; u < UU; u++) {
      const uint32_t q = c + u * BLK;
#pragma unroll
      for (int j = 0; j < R; j++) {
        if constexpr (VEC) {
          m[u][j] = ld<u32x4, NT>(reinterpret_cast<const u32x4*>(rows[j]) + q);
        } else {
#pragma unroll
          for (int d = 0; d < 4; d++) {
            const uint32_t col = q * W + 2 * d;
            const uint32_t lo = col < ncols ? ld<uint16_t, NT>(rows[j] + col) : 0u;
            const uint32_t hi =
              col + 1 < ncols ? ld<uint16_t, NT>(rows[j] + col + 1) : 0u;
            m[u][j][d] = lo | (hi << 16);
          }
        }
      }
    }
    if constexpr (!ONES) {
#pragma unroll
      for (int u = 0; u < UU; u++) {
        const uint32_t q = c + u * BLK;
        float sc[W];
        if constexpr (STATS || !XV)
          ld8(s_prev, q, sc);
        if constexpr (XV) {
          ld8(xvec, q, xs[u]);
        } else {
          float vv[W];
          ld8(v_prev, q, vv);
#pragma unroll
          for (int i = 0; i < W; i++)
            xs[u][i] = vv[i] * sc[i];
        }
        if constexpr (STATS) { // mfree_group's fold, rewritten for W = 8
          const float s0 = s_prev[0];
          const uint32_t nxt = (q + 1) * W;
#pragma unroll
          for (int i = 0; i < W; i++) {
            const uint32_t col = q * W + i;
            if (VEC || col < ncols) {
              mx = sc[i] > mx ? sc[i] : mx;
              const bool last = col + 1 >= ncols;
              if (!last || cyclic) {
                float e1;
                if (i < W - 1)
                  e1 = last ? s0 : sc[i + 1];
                else
                  e1 = nxt < ncols ? s_prev[nxt] : s0;
                const float d = sc[i] - e1;
                ok &= (d < 0.f ? -d : d) < eps ? 1 : 0;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UU; u++)
#pragma unroll
      for (int j = 0; j < R; j++)
#pragma unroll
        for (int d = 0; d < 4; d++) {
          float lo, hi;
          widen2<S>(m[u][j][d], lo, hi);
          if constexpr (ONES) {
            acc[j] = __builtin_fmaf(lo, 1.f, acc[j]);
            acc[j] = __builtin_fmaf(hi, 1.f, acc[j]);
          } else {
            acc[j] = __builtin_fmaf(lo, xs[u][2 * d], acc[j]);
            acc[j] = __builtin_fmaf(hi, xs[u][2 * d + 1], acc[j]);
          }
        }
  };
  uint32_t c = threadIdx.x;
  for (; c + (U - 1) * BLK < nch; c += U * BLK)
    body(c, std::integral_constant<int, U>{});
  sweep_tail<U, BLK>(c, nch, body);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < R; j++) {
    float t = wave_sum(acc[j]);
    if (lane == 0)
      red[wave][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < R) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < BLK / 64; w++)
      t += red[w][threadIdx.x];
    if constexpr (ONES) {
      s_next[rbase + threadIdx.x] = t;
    } else {
      const uint32_t r = row0 + rbase + threadIdx.x;
      s_next[rbase + threadIdx.x] = t / (v_prev[r] * s_prev[r]);
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// launch k >= 1 of the matrix-free scheme on a 16-bit matrix: k_mfree's
// contract (m, stop, lambda of round k-1 from the full s_prev; v_cur =
// v_prev * (s_prev / m) over all n; s_next[r] = (Σ_c A_0[r][c] x[c]) / x[r],
// x = v_prev ∘ s_prev; gated on state->end), its row-group schedule (main
// groups of ROWS rows, remainder rows alone, walked backwards on odd k) and
// its code for everything but the sweep.
// ---------------------------------------------------------------------------
template <typename S, int ROWS, int U, bool VEC, bool NT, bool XV,
          int BLK = kBlock>
__global__ __launch_bounds__(BLK) void
k_mfree_half(const uint16_t* a0, const float* __restrict__ s_prev,
             float* __restrict__ s_next, const float* __restrict__ v_prev,
             float* __restrict__ v_cur, const float* __restrict__ xvec,
             uint32_t ng_main, uint32_t nrem, uint32_t ncols, uint32_t row0,
             float eps, uint32_t k, uint32_t max_itr, uint32_t semantics,
             st_state* state)
{
  {
    const uint32_t e =
      __hip_atomic_load(&state->end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e < k)
      return;
  }
  __shared__ float red[BLK / 64][kHalfRows];
  __shared__ float mx_sh[BLK / 64];
  __shared__ float m_sh;
  const bool cyclic = semantics == ST_SEM_SYCL;
  const uint32_t ngroups = ng_main + nrem;
  float mx = 0.f;
  int ok = 1;
  float dmx = 0.f;
  int dok = 1;
  const uint32_t cnt = // as k_mfree
    blockIdx.x < ngroups ? (ngroups - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  const bool rev = (k & 1u) != 0;
  for (uint32_t i = 0; i < cnt; i++) {
    const bool first = i == 0;
    const uint32_t g = blockIdx.x + (rev ? cnt - 1 - i : i) * gridDim.x;
    if (g < ng_main) {
      if (first)
        half_group<S, ROWS, U, VEC, NT, false, XV, true, BLK>(
          a0, s_prev, v_prev, xvec, s_next, g * ROWS, ncols, row0, cyclic, eps,
          mx, ok, red);
      else
        half_group<S, ROWS, U, VEC, NT, false, XV, false, BLK>(
          a0, s_prev, v_prev, xvec, s_next, g * ROWS, ncols, row0, cyclic, eps,
          dmx, dok, red);
    } else {
      const uint32_t rb = ng_main * ROWS + (g - ng_main);
      if (first)
        half_group<S, 1, U, VEC, NT, false, XV, true, BLK>(
          a0, s_prev, v_prev, xvec, s_next, rb, ncols, row0, cyclic, eps, mx,
          ok, red);
      else
        half_group<S, 1, U, VEC, NT, false, XV, false, BLK>(
          a0, s_prev, v_prev, xvec, s_next, rb, ncols, row0, cyclic, eps, dmx,
          dok, red);
    }
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0)
    mx_sh[threadIdx.x >> 6] = mx;
  const int stop = __syncthreads_and(ok);
  if (threadIdx.x == 0) {
    float m = mx_sh[0];
#pragma unroll
    for (int w = 1; w < BLK / 64; w++)
      m = mx_sh[w] > m ? mx_sh[w] : m;
    m_sh = m;
  }
  __syncthreads();
  const float m = m_sh;
  // v_{k-1} = v_{k-2} * (s_{k-1} / m_{k-1}) over the FULL vector (cpp:260)
  {
    const uint32_t per = (ncols + gridDim.x - 1) / gridDim.x;
    const uint32_t lo = blockIdx.x * per;
    const uint32_t hi = lo + per < ncols ? lo + per : ncols;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += BLK)
      v_cur[i] = v_prev[i] * (s_prev[i] / m);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t rk = k - 1; // the round evaluated by this launch
    state->lambda = (double)s_prev[0];
    state->max = (double)m;
    state->stop = stop ? 1u : 0u;
    state->round = rk;
    if (stop) {
      state->iters = semantics == ST_SEM_SYCL ? rk : rk + 1;
      state->end = k;
      state->done = 1u;
    } else if (k >= max_itr) {
      state->iters = max_itr;
      state->end = k;
      state->done = 1u;
    }
  }
}

// K0 on a 16-bit matrix: s[r] = Σ_c A_0[r][c], the same sweep with x ≡ 1
// (no vectors read, no division)
template <typename S, int ROWS, int U, bool VEC, bool NT, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void
k_rowsum_half(const uint16_t* a0, float* __restrict__ s, uint32_t ng_main,
              uint32_t nrem, uint32_t ncols)
{
  __shared__ float red[BLK / 64][kHalfRows];
  const uint32_t ngroups = ng_main + nrem;
  float mx = 0.f;
  int ok = 1;
  for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    if (g < ng_main)
      half_group<S, ROWS, U, VEC, NT, true, false, false, BLK>(
        a0, nullptr, nullptr, nullptr, s, g * ROWS, ncols, 0, false, 0.f, mx,
        ok, red);
    else
      half_group<S, 1, U, VEC, NT, true, false, false, BLK>(
        a0, nullptr, nullptr, nullptr, s, ng_main * ROWS + (g - ng_main), ncols,
        0, false, 0.f, mx, ok, red);
  }
}

// x = v ∘ s (the A/B of a precomputed x vector; probe builds only)
__global__ __launch_bounds__(kBlock) void
k_xvec(const float* __restrict__ s, const float* __restrict__ v,
       float* __restrict__ x, uint32_t n)
{
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n;
       i += gridDim.x * kBlock)
    x[i] = v[i] * s[i];
}

// d_out[i] = d_in[i] rounded to nearest even in the storage format
template <typename S>
__global__ __launch_bounds__(kBlock) void
k_narrow(const float* __restrict__ in, uint16_t* __restrict__ out,
         uint64_t count)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * kBlock) {
    const float x = in[i];
    if constexpr (std::is_same<S, StoreBF16>::value) {
      uint32_t b = __float_as_uint(x);
      if (x != x)
        b = 0x7fc00000u; // the quiet NaN
      else
        b += 0x7fffu + ((b >> 16) & 1u); // ties to even
      out[i] = (uint16_t)(b >> 16);
    } else {
      out[i] = __builtin_bit_cast(uint16_t, (_Float16)x); // v_cvt_f16_f32: RNE
    }
  }
}

} // namespace dev
} // namespace st
