// st_left.hip — launchers of the dense left-vector kernels in st_left.h and
// the part of their C-ABI that needs no queue (similarity_transform.h section
// 3i and its step-level entries: st_left_shape, st_left_scratch,
// st_left_shape_desc, st_colsum_*, st_mfree_left_round_*).
// st_solve_device_left_* and max_eigen_value_left_ex live with the queue in
// st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <atomic>

#include "st_left.h"
#include "st_left_host.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kLeftPrepGrid = 2048; // = k_csr_prep's workgroup cap (st_csr.hip)
static_assert(left::kBlockLanes == (uint32_t)kBlock, "st_left_host.h's strip");

// the tuning build's override of the rows per block (0 = the table)
std::atomic<uint32_t> g_left_rows{ 0u };

int
check_launch(const char* what)
{
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s launch failed: %s", what, hipGetErrorString(e));
    return -1;
  }
  return 0;
}

inline bool
aligned16(const void* p)
{
  return ((uintptr_t)p & 15u) == 0;
}

// everything a launch derives from (dtype, n) and the vector width
// (blockIdx.x = tile * nstrips + strip)
using LeftGrid = left::Grid;

template <typename T>
int
left_grid(uint32_t n, int w, LeftGrid* g)
{
  uint64_t want = 0;
  ST_REQUIRE(left::grid(n, left_rows(sizeof(T) == 8, n), (uint32_t)w, sizeof(T), g, &want),
             "dense left: dim = %u needs %llu workgroups per launch, above %llu", n,
             (unsigned long long)want, (unsigned long long)left::kGridMax);
  return 0;
}

template <typename T, int W>
int
colsum_w(const T* a, T* s, T* part, uint32_t n, hipStream_t stream)
{
  LeftGrid g;
  if (left_grid<T>(n, W, &g))
    return -1;
  constexpr int U = dev::kLeftUnroll;
  if (g.nt)
    hipLaunchKernelGGL((dev::k_colsum<T, W, U, true>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, part, n, g.rb, g.nstrips);
  else
    hipLaunchKernelGGL((dev::k_colsum<T, W, U, false>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, part, n, g.rb, g.nstrips);
  if (check_launch("colsum"))
    return -1;
  const uint32_t fgrid = (n + dev::kLeftFinishBlock - 1) / dev::kLeftFinishBlock;
  hipLaunchKernelGGL((dev::k_left_finish<T, true>), dim3(fgrid),
                     dim3(dev::kLeftFinishBlock), 0, stream, (const T*)part, g.nrb,
                     (const T*)nullptr, (const T*)nullptr, (const T*)nullptr, s,
                     (T*)nullptr, n, 0u, (const st_state*)nullptr);
  return check_launch("left_finish");
}

template <typename T, int W>
int
left_round_w(const T* a, const T* s_prev, T* s_next, const T* v_prev, T* v_cur, T* x,
             T* part, uint32_t n, T eps, uint32_t k, uint32_t max_itr,
             uint32_t semantics, st_state* st, hipStream_t stream)
{
  LeftGrid g;
  if (left_grid<T>(n, W, &g))
    return -1;
  const uint32_t want = (n + kBlock - 1) / kBlock;
  const uint32_t pgrid = want < kLeftPrepGrid ? want : kLeftPrepGrid;
  hipLaunchKernelGGL(dev::k_csr_prep<T>, dim3(pgrid), dim3(kBlock), 0, stream, s_prev,
                     v_prev, x, n, eps, k, max_itr, semantics, st);
  if (check_launch("left_prep"))
    return -1;
  constexpr int U = dev::kLeftUnroll;
  if (g.nt)
    hipLaunchKernelGGL((dev::k_left_sweep<T, W, U, true>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, (const T*)x, part, n, g.rb, g.nstrips, k,
                       (const st_state*)st);
  else
    hipLaunchKernelGGL((dev::k_left_sweep<T, W, U, false>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, (const T*)x, part, n, g.rb, g.nstrips, k,
                       (const st_state*)st);
  if (check_launch("left_sweep"))
    return -1;
  const uint32_t fgrid = (n + dev::kLeftFinishBlock - 1) / dev::kLeftFinishBlock;
  hipLaunchKernelGGL((dev::k_left_finish<T, false>), dim3(fgrid),
                     dim3(dev::kLeftFinishBlock), 0, stream, (const T*)part, g.nrb,
                     (const T*)x, s_prev, v_prev, s_next, v_cur, n, k,
                     (const st_state*)st);
  return check_launch("left_finish");
}

// 16-byte loads where every row starts on a 16-byte boundary
template <typename T>
bool
left_vec_ok(const T* a, const T* part, uint32_t n)
{
  constexpr uint32_t W = 16 / sizeof(T);
  return n % W == 0 && aligned16(a) && aligned16(part);
}

} // namespace

// RB of the order contract (left::rows' table; tools/bench_left.py carries
// the A/B through the tuning build's override)
uint32_t
left_rows(int dtype, uint32_t n)
{
  const uint32_t ov = g_left_rows.load(std::memory_order_relaxed);
  return ov != 0 ? ov : left::rows(dtype, n);
}

size_t
left_x_elems(uint32_t n)
{
  return (size_t)left::x_elems(n);
}

size_t
left_part_elems(int dtype, uint32_t n)
{
  return (size_t)left::part_elems(n, left_rows(dtype, n));
}

template <typename T>
int
launch_colsum(const T* a, T* s, T* part, uint32_t n, hipStream_t stream)
{
  ST_REQUIRE(a, "colsum: null matrix");
  ST_REQUIRE(s && part, "colsum: null pointer");
  ST_REQUIRE(n > 0, "colsum: dim must be > 0");
  ST_REQUIRE(((uintptr_t)a & (sizeof(T) - 1)) == 0,
             "colsum: matrix not aligned to its element size");
  if (left_vec_ok<T>(a, part, n))
    return colsum_w<T, 16 / sizeof(T)>(a, s, part, n, stream);
  return colsum_w<T, 1>(a, s, part, n, stream);
}

template <typename T>
int
launch_left_round(const T* a, const T* s_prev, T* s_next, const T* v_prev, T* v_cur,
                  T* x, T* part, uint32_t n, T eps, uint32_t k, uint32_t max_itr,
                  uint32_t semantics, st_state* st, hipStream_t stream)
{
  ST_REQUIRE(a, "mfree_left_round: null matrix");
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && x && part && st,
             "mfree_left_round: null pointer");
  ST_REQUIRE(n > 0, "mfree_left_round: dim must be > 0");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "mfree_left_round: bad semantics %u", semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "mfree_left_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "mfree_left_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "mfree_left_round: s_prev and s_next must differ");
  ST_REQUIRE(((uintptr_t)a & (sizeof(T) - 1)) == 0,
             "mfree_left_round: matrix not aligned to its element size");
  if (left_vec_ok<T>(a, part, n))
    return left_round_w<T, 16 / sizeof(T)>(a, s_prev, s_next, v_prev, v_cur, x, part, n,
                                           eps, k, max_itr, semantics, st, stream);
  return left_round_w<T, 1>(a, s_prev, s_next, v_prev, v_cur, x, part, n, eps, k, max_itr,
                            semantics, st, stream);
}

template int launch_colsum<float>(const float*, float*, float*, uint32_t, hipStream_t);
template int launch_colsum<double>(const double*, double*, double*, uint32_t, hipStream_t);
template int launch_left_round<float>(const float*, const float*, float*, const float*,
                                      float*, float*, float*, uint32_t, float, uint32_t,
                                      uint32_t, uint32_t, st_state*, hipStream_t);
template int launch_left_round<double>(const double*, const double*, double*, const double*,
                                       double*, double*, double*, uint32_t, double, uint32_t,
                                       uint32_t, uint32_t, st_state*, hipStream_t);

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_left_shape(int dtype, unsigned int n, uint32_t* rows_per_block, uint32_t* combine)
{
  st::clear_error();
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "st_left_shape: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  ST_REQUIRE(n >= 1 && n <= st::left::kNMax, "st_left_shape: n must be in [1, 2^31), got %u",
             n);
  if (rows_per_block)
    *rows_per_block = st::left_rows(dtype, n);
  if (combine)
    *combine = 0; // serial, ascending block order
  return 0;
}

uint64_t
st_left_scratch(int dtype, unsigned int n)
{
  st::clear_error();
  if (dtype != 0 && dtype != 1) {
    st::set_error("st_left_scratch: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
    return 0;
  }
  if (n < 1 || n > st::left::kNMax) {
    st::set_error("st_left_scratch: n must be in [1, 2^31), got %u", n);
    return 0;
  }
  return (uint64_t)st::left_x_elems(n) + (uint64_t)st::left_part_elems(dtype, n);
}

const char*
st_left_shape_desc(void)
{
  static_assert(st::dev::kBlock == 256 && st::dev::kLeftUnroll == 8 &&
                  st::dev::kLeftFinishBlock == 64 && st::kLeftPrepGrid == 2048 &&
                  st::left::kNtBytes == ((uint64_t)512 << 20) &&
                  st::left::rows(0, 1) == 32 && st::left::rows(0, 2048) == 64 &&
                  st::left::rows(1, 4096) == 128 && st::left::rows(1, 16384) == 256,
                "the description below");
  return "block=256 bytes_per_load=16 rows_in_flight=8 rows_per_block=32,64,128,256 "
         "rows_from=1,2048,4096,16384 combine=serial finish_block=64 prep_grid=2048 "
         "nt_from_mib=512";
}

#define ST_LEFT_EXPORTS(T, SFX)                                                         \
  int st_colsum_##SFX(const T* d_mat, T* d_s, T* d_scratch, unsigned int n, void* stream) \
  {                                                                                     \
    st::clear_error();                                                                  \
    ST_REQUIRE(d_mat, "colsum: null matrix");                                           \
    ST_REQUIRE(d_scratch, "colsum: null scratch");                                      \
    ST_REQUIRE(n > 0, "colsum: dim must be > 0");                                       \
    return st::launch_colsum<T>(d_mat, d_s, d_scratch + st::left_x_elems(n), n,         \
                                ST_STREAM(stream));                                     \
  }                                                                                     \
  int st_mfree_left_round_##SFX(const T* d_mat0, const T* d_s_prev, T* d_s_next,        \
                                const T* d_v_prev, T* d_v_cur, T* d_scratch,            \
                                unsigned int n, T eps, unsigned int k,                  \
                                unsigned int max_itr, unsigned int semantics,           \
                                st_state* d_state, void* stream)                        \
  {                                                                                     \
    st::clear_error();                                                                  \
    ST_REQUIRE(d_mat0, "mfree_left_round: null matrix");                                \
    ST_REQUIRE(d_scratch, "mfree_left_round: null scratch");                            \
    ST_REQUIRE(n > 0, "mfree_left_round: dim must be > 0");                             \
    ST_REQUIRE(d_scratch != d_s_prev && d_scratch != d_s_next &&                        \
                 d_scratch != d_v_prev && d_scratch != d_v_cur,                         \
               "mfree_left_round: d_scratch must be scratch of its own");               \
    return st::launch_left_round<T>(d_mat0, d_s_prev, d_s_next, d_v_prev, d_v_cur,      \
                                    d_scratch, d_scratch + st::left_x_elems(n), n, eps, \
                                    k, max_itr, semantics, d_state, ST_STREAM(stream)); \
  }

ST_LEFT_EXPORTS(float, f32)
ST_LEFT_EXPORTS(double, f64)

#if defined(ST_TUNING_ABI) && ST_TUNING_ABI
// the tuning build only: rows per block of the dense left kernels, 0 = the
// table.  Unlike the setters of st_tuning.h it CHANGES results - it enters the
// order of a column, and st_left_shape reports it - so it is declared where it
// is used (tools/bench_left.py's A/B of rows per block), not in that header
// (hence the visibility attribute here: no header gives it one).
__attribute__((visibility("default"))) int
st_set_left_rows(unsigned int rows)
{
  st::clear_error();
  ST_REQUIRE(rows <= 65536, "st_set_left_rows: rows must be in [0, 65536], got %u", rows);
  st::g_left_rows.store(rows, std::memory_order_relaxed);
  return 0;
}
#endif

} // extern "C"
