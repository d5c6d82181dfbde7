// st_pair_host.h — the host arithmetic of the dense Perron pair solve: the
// strip of the right side's order contract, the scratch layout and the launch
// grid.  Plain C++ (no HIP), so that tests/cpp/pair_sanitize.cpp runs it under
// the host sanitizers; included by st_pair.hip and st_solve.hip.  The rows per
// block, the workgroup limit and the non-temporal threshold are the left
// solve's (st_left_host.h).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "st_left_host.h"

namespace st {
namespace pair {

constexpr uint32_t kRight = 0; // = ST_PAIR_RIGHT: states[0], vecs[0]
constexpr uint32_t kLeft = 1;  // = ST_PAIR_LEFT

// rows of a tile whose four wave sums LDS holds at a time (8 KB in fp64): the
// table's RB never passes it, a tuning override above it takes more barriers
constexpr uint32_t kChunkRows = 256;

// columns of a lane: 16 bytes of elements, whatever the kind of load
constexpr uint32_t
lane_cols(size_t elem)
{
  return (uint32_t)(16 / elem);
}

// S of the order contract: the columns of one workgroup, 1024 (fp32) / 512
// (fp64).  It enters the right side's order (a row's strips), so it does NOT
// depend on the kind of load, unlike the left solve's strip
constexpr uint32_t
strip_cols(size_t elem)
{
  return left::kBlockLanes * lane_cols(elem);
}

inline uint64_t
strips(uint32_t n, size_t elem)
{
  return ((uint64_t)n + strip_cols(elem) - 1) / strip_cols(elem);
}

inline uint64_t
up64(uint64_t e)
{
  return (e + 63) & ~(uint64_t)63;
}

// the step-level scratch, in elements, every part 256-byte aligned when the
// scratch is: [x_R | x_L | colpart (blocks * n) | rowpart (strips * n)]
struct Layout
{
  uint64_t x_right, x_left, colpart, rowpart, total;
};

inline Layout
layout(uint32_t n, uint32_t rb, size_t elem)
{
  Layout l;
  l.x_right = 0;
  l.x_left = left::x_elems(n);
  l.colpart = 2 * left::x_elems(n);
  l.rowpart = l.colpart + up64(left::part_elems(n, rb));
  l.total = l.rowpart + strips(n, elem) * (uint64_t)n;
  return l;
}

// the launch of the sweep (blockIdx.x = tile * nstrips + strip): false when it
// needs more workgroups than one launch holds
inline bool
grid(uint32_t n, uint32_t rb, size_t elem, left::Grid* g, uint64_t* want)
{
  return left::grid(n, rb, lane_cols(elem), elem, g, want);
}

} // namespace pair
} // namespace st
