// st_left_host.h — the host arithmetic of the dense left-vector solve: the
// rows per block of the order contract, the scratch layout, the launch grid
// and the host twin's staging.  Plain C++ (no HIP), so that
// tests/cpp/left_sanitize.cpp runs it under the host sanitizers; included by
// st_left.hip and st_solve.hip.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace st {
namespace left {

constexpr uint32_t kBlockLanes = 256;         // = dev::kBlock
constexpr uint32_t kNMax = 0x7fffffffu;       // n in [1, 2^31)
constexpr uint64_t kGridMax = 0x7fffffffull;  // workgroups of one launch
// non-temporal loads from the size at which k_mfree's shape table takes them
// (mfree_shape, st_kernels.hip: beyond the memory-side cache)
constexpr uint64_t kNtBytes = (uint64_t)512 << 20;

// RB of the order contract: a function of (dtype, n) and nothing else (the
// same table for both element sizes).  Small blocks keep enough workgroups on
// a small matrix; from 16384 the partials are 2 / 256 of the matrix's bytes.
constexpr uint32_t
rows(int /* dtype */, uint32_t n)
{
  if (n >= 16384)
    return 256;
  if (n >= 4096)
    return 128;
  if (n >= 2048)
    return 64;
  return 32;
}

inline uint64_t
blocks(uint32_t n, uint32_t rb)
{
  return ((uint64_t)n + rb - 1) / rb;
}

// the step-level scratch, in elements: [x (rounded up to 64, so that the
// partials start 256-byte aligned) | part (blocks * n)]
inline uint64_t
x_elems(uint32_t n)
{
  return ((uint64_t)n + 63) & ~(uint64_t)63;
}

inline uint64_t
part_elems(uint32_t n, uint32_t rb)
{
  return blocks(n, rb) * (uint64_t)n;
}

// the launch of the sweep for lanes of w columns: false when it needs more
// workgroups than one launch holds
struct Grid
{
  uint32_t rb, nrb, nstrips, grid;
  bool nt;
};

inline bool
grid(uint32_t n, uint32_t rb, uint32_t w, size_t elem, Grid* g, uint64_t* want)
{
  const uint64_t strip = (uint64_t)kBlockLanes * w;
  const uint64_t nrb = blocks(n, rb);
  const uint64_t nstrips = ((uint64_t)n + strip - 1) / strip;
  *want = nrb * nstrips; // < 2^31 * 2^23: no wrap
  if (*want > kGridMax)
    return false;
  g->rb = rb;
  g->nrb = (uint32_t)nrb;
  g->nstrips = (uint32_t)nstrips;
  g->grid = (uint32_t)*want;
  g->nt = (uint64_t)n * n >= kNtBytes / elem; // (n * n * elem may pass 2^64)
  return true;
}

// the host twin's workspace: the matrix as the caller has it, one slot,
// 256-byte granular.  stage_fits first: n * n * elem reaches 2^65 for n near
// 2^31 and 8-byte elements
inline bool
stage_fits(uint32_t n, size_t elem)
{
  return (uint64_t)n * n <= (~(uint64_t)0 - 255) / elem;
}

inline uint64_t
stage_bytes(uint32_t n, size_t elem)
{
  return ((uint64_t)n * n * elem + 255) & ~(uint64_t)255;
}

} // namespace left
} // namespace st
