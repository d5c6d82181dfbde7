// st_csr_transpose.h — the kernels of the stable device transposition of a
// CSR matrix (st_csr_host.h: T(A)), for gfx950.  Not templates except the
// gather, so included by st_csr_transpose.hip alone; not a public header.
//
// T(A) is the entries of A sorted by column, entries of one column kept in
// storage order.  That is a stable LSD radix sort with the column as the key
// and the 32-bit source entry index as the payload, kDigitBits bits per pass:
//
//   k_tr_count      cnt[c] = the entries of column c (integer atomics: a
//                   count does not depend on the order of its increments)
//   k_tr_colsum     per block of kColsPerBlock columns the sum of cnt, and
//                   the lowest empty column through atomicMin
//   k_tr_top        one workgroup: the block sums -> where each block starts
//   k_tr_rowptr     t_row_ptr = the exclusive scan of cnt
//   per pass:
//   k_tr_hist       tab[digit][tile] = the tile's entries holding that digit
//                   (LDS integer atomics), dtot[digit] += the same
//   k_tr_scan       workgroup d: tab[d][*] -> where the tile's entries of
//                   digit d start in the pass's output (all smaller digits
//                   first - dtot -, then the tiles before it)
//   k_tr_scatter    k_csr_order generalised: a tile is kTileRounds rounds of
//                   256 entries, entry = tile * kTile + round * 256 + lane of
//                   the workgroup; a lane's rank among the wave's lanes with
//                   the same digit comes from the digit's peer mask (one
//                   ballot per digit bit), the waves before it through LDS,
//                   the rounds before it from the running per-digit base,
//                   the tiles before it from the scanned table
//   k_tr_gather     t_vals[i] = vals[perm[i]], t_col_idx[i] = the row of
//                   entry perm[i] (bisection of row_ptr)
//   k_tr_gather_rows  the same without values (st_csr_pattern_transpose)
//
// No workgroup waits on another anywhere: every dependency is a launch
// boundary.  Every computed destination is bounded, so that a matrix changed
// under the handle cannot make a kernel write outside its output.
#pragma once

#include "st_csr.h"

namespace st {
namespace dev {

constexpr uint32_t kDigitBits = 8;
constexpr uint32_t kDigits = 1u << kDigitBits; // one per lane of a workgroup
constexpr uint32_t kTileRounds = 8;
constexpr uint32_t kTile = kTileRounds * kBlock; // entries of a workgroup
constexpr uint32_t kColsPerLane = 8;
constexpr uint32_t kColsPerBlock = kColsPerLane * kBlock;
static_assert(kDigits == kBlock, "lane d of a workgroup owns digit d");

// the exclusive prefix of v over the workgroup's lanes and the workgroup's
// total; sh holds 2 * kBlock words and is free again on return
__device__ __forceinline__ uint32_t
tr_block_scan(uint32_t v, uint32_t* sh, uint32_t* total)
{
  const uint32_t t = threadIdx.x;
  uint32_t in = 0;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (uint32_t off = 1; off < kBlock; off <<= 1) {
    uint32_t x = sh[in * kBlock + t];
    if (t >= off)
      x += sh[in * kBlock + t - off];
    sh[(in ^ 1) * kBlock + t] = x;
    __syncthreads();
    in ^= 1;
  }
  const uint32_t incl = sh[in * kBlock + t];
  *total = sh[in * kBlock + kBlock - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kBlock) void
k_tr_count(const int32_t* __restrict__ col, uint32_t n, uint64_t nnz,
           uint32_t* cnt)
{
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz;
       e += (uint64_t)gridDim.x * kBlock) {
    const uint32_t c = (uint32_t)col[e];
    if (c < n) // always, for a col_idx that did not change since the check
      atomicAdd(&cnt[c], 1u);
  }
}

// block b: bsum[b] = the entries of its columns; err[0] = the lowest column
// without any
__global__ __launch_bounds__(kBlock) void
k_tr_colsum(const uint32_t* __restrict__ cnt, uint32_t n,
            uint32_t* __restrict__ bsum, unsigned long long* err)
{
  __shared__ uint32_t sh[2 * kBlock];
  const uint64_t c0 =
    (uint64_t)blockIdx.x * kColsPerBlock + (uint64_t)threadIdx.x * kColsPerLane;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kColsPerLane; j++)
    if (c0 + j < n) {
      const uint32_t k = cnt[c0 + j];
      if (k == 0)
        atomicMin(&err[0], (unsigned long long)(c0 + j));
      sum += k;
    }
  uint32_t total;
  (void)tr_block_scan(sum, sh, &total);
  if (threadIdx.x == 0)
    bsum[blockIdx.x] = total;
}

// one workgroup: x[count] -> its exclusive scan, in place
__global__ __launch_bounds__(kBlock) void
k_tr_top(uint32_t* __restrict__ x, uint32_t count)
{
  __shared__ uint32_t sh[2 * kBlock];
  const uint32_t per = (count + kBlock - 1) / kBlock;
  const uint64_t lo64 = (uint64_t)threadIdx.x * per;
  const uint32_t lo = lo64 < count ? (uint32_t)lo64 : count;
  const uint32_t hi = lo64 + per < count ? (uint32_t)(lo64 + per) : count;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++)
    sum += x[i];
  uint32_t total;
  uint32_t run = tr_block_scan(sum, sh, &total);
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = x[i];
    x[i] = run;
    run += v;
  }
}

// t_row_ptr[c] = bfirst[block] + the block's columns before c; [n] = the total
__global__ __launch_bounds__(kBlock) void
k_tr_rowptr(const uint32_t* __restrict__ cnt, uint32_t n,
            const uint32_t* __restrict__ bfirst, int64_t* __restrict__ t_row_ptr)
{
  __shared__ uint32_t sh[2 * kBlock];
  const uint64_t c0 =
    (uint64_t)blockIdx.x * kColsPerBlock + (uint64_t)threadIdx.x * kColsPerLane;
  uint32_t k[kColsPerLane];
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kColsPerLane; j++) {
    k[j] = c0 + j < n ? cnt[c0 + j] : 0u;
    sum += k[j];
  }
  uint32_t total;
  uint64_t run = (uint64_t)bfirst[blockIdx.x] + tr_block_scan(sum, sh, &total);
#pragma unroll
  for (uint32_t j = 0; j < kColsPerLane; j++)
    if (c0 + j < n) {
      t_row_ptr[c0 + j] = (int64_t)run;
      run += k[j];
      if (c0 + j == (uint64_t)n - 1)
        t_row_ptr[n] = (int64_t)run;
    }
}

// the key of entry e in this pass: col_idx itself in pass 0
__device__ __forceinline__ uint32_t
tr_digit(const uint32_t* __restrict__ keys, uint64_t e, uint32_t shift)
{
  return (keys[e] >> shift) & (kDigits - 1);
}

// tab is digit-major: tab[d * ntiles + tile]
__global__ __launch_bounds__(kBlock) void
k_tr_hist(const uint32_t* __restrict__ keys, uint64_t nnz, uint32_t shift,
          uint32_t ntiles, uint32_t* __restrict__ tab, uint32_t* dtot)
{
  __shared__ uint32_t hist[kDigits];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
#pragma unroll
  for (uint32_t j = 0; j < kTileRounds; j++) {
    const uint64_t e = base + (uint64_t)j * kBlock;
    if (e < nnz)
      atomicAdd(&hist[tr_digit(keys, e, shift)], 1u);
  }
  __syncthreads();
  const uint32_t k = hist[threadIdx.x];
  tab[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = k;
  if (k)
    atomicAdd(&dtot[threadIdx.x], k);
}

// workgroup d: tab[d][tile] -> the entries of smaller digits + the entries of
// digit d in the tiles before `tile`, in place
__global__ __launch_bounds__(kBlock) void
k_tr_scan(uint32_t* __restrict__ tab, uint32_t ntiles,
          const uint32_t* __restrict__ dtot)
{
  __shared__ uint32_t sh[2 * kBlock];
  const uint32_t d = blockIdx.x;
  uint32_t* row = tab + (uint64_t)d * ntiles;
  uint32_t total, before;
  (void)tr_block_scan(threadIdx.x < d ? dtot[threadIdx.x] : 0u, sh, &before);
  const uint32_t per = (ntiles + kBlock - 1) / kBlock;
  const uint64_t lo64 = (uint64_t)threadIdx.x * per;
  const uint32_t lo = lo64 < ntiles ? (uint32_t)lo64 : ntiles;
  const uint32_t hi = lo64 + per < ntiles ? (uint32_t)(lo64 + per) : ntiles;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++)
    sum += row[i];
  uint32_t run = before + tr_block_scan(sum, sh, &total);
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = row[i];
    row[i] = run;
    run += v;
  }
}

// idx_in == nullptr: pass 0, the payload of entry e is e itself.
// keys_out == nullptr: the last pass, whose keys nobody reads.
__global__ __launch_bounds__(kBlock) void
k_tr_scatter(const uint32_t* __restrict__ keys_in,
             const uint32_t* __restrict__ idx_in, uint64_t nnz, uint32_t shift,
             uint32_t ntiles, const uint32_t* __restrict__ tab,
             uint32_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out)
{
  __shared__ uint32_t base[kDigits];
  __shared__ uint32_t wcnt[kBlock / 64][kDigits];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  base[t] = tab[(uint64_t)t * ntiles + blockIdx.x];
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; w++)
    wcnt[w][t] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t j = 0; j < kTileRounds; j++) { // workgroup-uniform
    const uint64_t e = (uint64_t)blockIdx.x * kTile + (uint64_t)j * kBlock + t;
    const bool valid = e < nnz;
    const uint32_t key = valid ? keys_in[e] : 0u;
    const uint32_t idx = !valid ? 0u : idx_in ? idx_in[e] : (uint32_t)e;
    const uint32_t digit = (key >> shift) & (kDigits - 1);
    // the wave's valid lanes that hold this lane's digit
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < kDigitBits; b++) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    if (valid && rank == 0)
      wcnt[wave][digit] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t at = base[digit] + rank;
      for (uint32_t w = 0; w < wave; w++)
        at += wcnt[w][digit];
      if (at < nnz) { // always, for a col_idx that did not change
        if (keys_out)
          keys_out[at] = key;
        idx_out[at] = idx;
      }
    }
    __syncthreads();
    uint32_t add = 0; // lane d owns digit d
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; w++) {
      add += wcnt[w][t];
      wcnt[w][t] = 0;
    }
    base[t] += add;
    __syncthreads();
  }
}

// perm == nullptr: the identity (n == 1: no pass at all)
template <typename T>
__global__ __launch_bounds__(kBlock) void
k_tr_gather(const int64_t* __restrict__ row_ptr, const T* __restrict__ vals,
            const uint32_t* __restrict__ perm, uint32_t n, uint64_t nnz,
            int32_t* __restrict__ t_col, T* __restrict__ t_vals)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t e = perm ? (uint64_t)perm[i] : i;
    if (e >= nnz) // never, for a matrix that did not change
      continue;
    uint32_t lo = 0, hi = n; // the row with row_ptr[lo] <= e < row_ptr[lo + 1]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)row_ptr[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    t_col[i] = (int32_t)lo;
    t_vals[i] = vals[e];
  }
}

// k_tr_gather without values (a pattern handle): the source rows only
__global__ __launch_bounds__(kBlock) void
k_tr_gather_rows(const int64_t* __restrict__ row_ptr,
                 const uint32_t* __restrict__ perm, uint32_t n, uint64_t nnz,
                 int32_t* __restrict__ t_col)
{
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t e = perm ? (uint64_t)perm[i] : i;
    if (e >= nnz) // never, for a matrix that did not change
      continue;
    uint32_t lo = 0, hi = n; // the row with row_ptr[lo] <= e < row_ptr[lo + 1]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)row_ptr[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    t_col[i] = (int32_t)lo;
  }
}

} // namespace dev
} // namespace st
