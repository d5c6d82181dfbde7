// st_pair.hip — launchers of the dense Perron pair kernels in st_pair.h and
// the part of their C-ABI that needs no queue (similarity_transform.h section
// 3j and its step-level entries: st_pair_shape, st_pair_scratch,
// st_pair_shape_desc, st_pair_sum_*, st_mfree_pair_round_*).
// st_solve_device_pair_* and max_eigen_value_pair_ex live with the queue in
// st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "st_pair.h"
#include "st_pair_host.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kPairPrepGrid = 2048; // = k_csr_prep's workgroup cap (st_csr.hip)

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

template <typename T>
int
pair_grid(uint32_t n, left::Grid* g)
{
  uint64_t want = 0;
  ST_REQUIRE(pair::grid(n, left_rows(sizeof(T) == 8, n), sizeof(T), g, &want),
             "dense pair: dim = %u needs %llu workgroups per launch, above %llu", n,
             (unsigned long long)want, (unsigned long long)left::kGridMax);
  return 0;
}

// the four parts of the step-level scratch
template <typename T>
struct Parts
{
  T *x_right, *x_left, *colpart, *rowpart;
  Parts(T* scratch, uint32_t n)
  {
    const pair::Layout l = pair::layout(n, left_rows(sizeof(T) == 8, n), sizeof(T));
    x_right = scratch + l.x_right;
    x_left = scratch + l.x_left;
    colpart = scratch + l.colpart;
    rowpart = scratch + l.rowpart;
  }
};

// 16-byte loads where every row starts on a 16-byte boundary
template <typename T>
bool
pair_vec_ok(const T* a, const T* scratch, uint32_t n)
{
  constexpr uint32_t W = 16 / sizeof(T);
  return n % W == 0 && aligned16(a) && aligned16(scratch);
}

template <typename T>
uint32_t
finish_grid(uint32_t n)
{
  return (n + dev::kLeftFinishBlock - 1) / dev::kLeftFinishBlock;
}

template <typename T, bool VEC>
int
pair_sum_w(const T* a, T* s_right, T* s_left, const Parts<T>& sc, uint32_t n,
           hipStream_t stream)
{
  left::Grid g;
  if (pair_grid<T>(n, &g))
    return -1;
  constexpr int U = dev::kLeftUnroll;
  if (g.nt)
    hipLaunchKernelGGL((dev::k_pair_sum<T, VEC, U, true>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, sc.colpart, sc.rowpart, n, g.rb, g.nstrips);
  else
    hipLaunchKernelGGL((dev::k_pair_sum<T, VEC, U, false>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, sc.colpart, sc.rowpart, n, g.rb, g.nstrips);
  if (check_launch("pair_sum"))
    return -1;
  const T* none = nullptr;
  hipLaunchKernelGGL((dev::k_left_finish<T, true>), dim3(finish_grid<T>(n)),
                     dim3(dev::kLeftFinishBlock), 0, stream, (const T*)sc.colpart, g.nrb,
                     none, none, none, s_left, (T*)nullptr, n, 0u, (const st_state*)nullptr);
  if (check_launch("pair_finish_left"))
    return -1;
  hipLaunchKernelGGL((dev::k_left_finish<T, true>), dim3(finish_grid<T>(n)),
                     dim3(dev::kLeftFinishBlock), 0, stream, (const T*)sc.rowpart, g.nstrips,
                     none, none, none, s_right, (T*)nullptr, n, 0u,
                     (const st_state*)nullptr);
  return check_launch("pair_finish_right");
}

template <typename T, bool VEC>
int
pair_round_w(const T* a, const PairVectors<T>& v, const Parts<T>& sc, uint32_t n, T eps,
             uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
             uint32_t* d_count, hipStream_t stream)
{
  left::Grid g;
  if (pair_grid<T>(n, &g))
    return -1;
  const uint32_t want = (n + kBlock - 1) / kBlock;
  const uint32_t pgrid = want < kPairPrepGrid ? want : kPairPrepGrid;
  T* const x[2] = { sc.x_right, sc.x_left };
  for (uint32_t side = 0; side < 2; side++) {
    hipLaunchKernelGGL(dev::k_csr_prep<T>, dim3(pgrid), dim3(kBlock), 0, stream,
                       v.s_prev[side], v.v_prev[side], x[side], n, eps, k, max_itr, semantics,
                       st + side);
    if (check_launch("pair_prep"))
      return -1;
  }
  constexpr int U = dev::kLeftUnroll;
  if (g.nt)
    hipLaunchKernelGGL((dev::k_pair_sweep<T, VEC, U, true>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, (const T*)sc.x_right, (const T*)sc.x_left, sc.colpart,
                       sc.rowpart, n, g.rb, g.nstrips, k, (const st_state*)st);
  else
    hipLaunchKernelGGL((dev::k_pair_sweep<T, VEC, U, false>), dim3(g.grid), dim3(kBlock), 0,
                       stream, a, (const T*)sc.x_right, (const T*)sc.x_left, sc.colpart,
                       sc.rowpart, n, g.rb, g.nstrips, k, (const st_state*)st);
  if (check_launch("pair_sweep"))
    return -1;
  // the left side's partials are [row block][column], the right side's
  // [strip][row]: one finish kernel, nrb := nstrips for the right side
  const T* const part[2] = { sc.rowpart, sc.colpart };
  const uint32_t nparts[2] = { g.nstrips, g.nrb };
  for (int j = 0; j < 2; j++) {
    const uint32_t side = j == 0 ? pair::kLeft : pair::kRight;
    hipLaunchKernelGGL((dev::k_left_finish<T, false>), dim3(finish_grid<T>(n)),
                       dim3(dev::kLeftFinishBlock), 0, stream, part[side], nparts[side],
                       (const T*)x[side], v.s_prev[side], v.v_prev[side], v.s_next[side],
                       v.v_cur[side], n, k, (const st_state*)(st + side));
    if (check_launch("pair_finish"))
      return -1;
  }
  if (d_count) {
    hipLaunchKernelGGL(dev::k_pair_count, dim3(1), dim3(64), 0, stream,
                       (const st_state*)st, d_count);
    if (check_launch("pair_count"))
      return -1;
  }
  return 0;
}

} // namespace

size_t
pair_scratch_elems(int dtype, uint32_t n)
{
  return (size_t)pair::layout(n, left_rows(dtype, n), dtype ? 8 : 4).total;
}

template <typename T>
int
launch_pair_sum(const T* a, T* s_right, T* s_left, T* scratch, uint32_t n,
                hipStream_t stream)
{
  ST_REQUIRE(a, "pair_sum: null matrix");
  ST_REQUIRE(scratch, "pair_sum: null scratch");
  ST_REQUIRE(n > 0, "pair_sum: dim must be > 0");
  ST_REQUIRE(s_right && s_left, "pair_sum: null pointer");
  ST_REQUIRE(s_right != s_left, "pair_sum: the two outputs must differ");
  ST_REQUIRE(((uintptr_t)a & (sizeof(T) - 1)) == 0,
             "pair_sum: matrix not aligned to its element size");
  ST_REQUIRE(((uintptr_t)scratch & (sizeof(T) - 1)) == 0,
             "pair_sum: scratch not aligned to its element size");
  const Parts<T> sc(scratch, n);
  if (pair_vec_ok<T>(a, scratch, n))
    return pair_sum_w<T, true>(a, s_right, s_left, sc, n, stream);
  return pair_sum_w<T, false>(a, s_right, s_left, sc, n, stream);
}

template <typename T>
int
launch_pair_round(const T* a, const PairVectors<T>& v, T* scratch, uint32_t n, T eps,
                  uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
                  uint32_t* d_count, hipStream_t stream)
{
  ST_REQUIRE(a, "mfree_pair_round: null matrix");
  ST_REQUIRE(scratch, "mfree_pair_round: null scratch");
  ST_REQUIRE(n > 0, "mfree_pair_round: dim must be > 0");
  ST_REQUIRE(st, "mfree_pair_round: null pointer");
  for (int side = 0; side < 2; side++) {
    ST_REQUIRE(v.s_prev[side] && v.s_next[side] && v.v_prev[side] && v.v_cur[side],
               "mfree_pair_round: null pointer");
    ST_REQUIRE(v.v_prev[side] != v.v_cur[side],
               "mfree_pair_round: v_prev and v_cur must differ");
    ST_REQUIRE(v.s_prev[side] != v.s_next[side],
               "mfree_pair_round: s_prev and s_next must differ");
    ST_REQUIRE(scratch != v.s_prev[side] && scratch != v.s_next[side] &&
                 scratch != v.v_prev[side] && scratch != v.v_cur[side],
               "mfree_pair_round: d_scratch must be scratch of its own");
  }
  ST_REQUIRE(v.s_next[0] != v.s_next[1] && v.v_cur[0] != v.v_cur[1],
             "mfree_pair_round: the two sides' outputs must differ");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "mfree_pair_round: bad semantics %u", semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "mfree_pair_round: launch index k must be >= 1");
  ST_REQUIRE(((uintptr_t)a & (sizeof(T) - 1)) == 0,
             "mfree_pair_round: matrix not aligned to its element size");
  ST_REQUIRE(((uintptr_t)scratch & (sizeof(T) - 1)) == 0,
             "mfree_pair_round: scratch not aligned to its element size");
  const Parts<T> sc(scratch, n);
  if (pair_vec_ok<T>(a, scratch, n))
    return pair_round_w<T, true>(a, v, sc, n, eps, k, max_itr, semantics, st, d_count,
                                 stream);
  return pair_round_w<T, false>(a, v, sc, n, eps, k, max_itr, semantics, st, d_count,
                                stream);
}

template int launch_pair_sum<float>(const float*, float*, float*, float*, uint32_t,
                                    hipStream_t);
template int launch_pair_sum<double>(const double*, double*, double*, double*, uint32_t,
                                     hipStream_t);
template int launch_pair_round<float>(const float*, const PairVectors<float>&, float*,
                                      uint32_t, float, uint32_t, uint32_t, uint32_t,
                                      st_state*, uint32_t*, hipStream_t);
template int launch_pair_round<double>(const double*, const PairVectors<double>&, double*,
                                       uint32_t, double, uint32_t, uint32_t, uint32_t,
                                       st_state*, uint32_t*, hipStream_t);

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_pair_shape(int dtype, unsigned int n, uint32_t* rows_per_block, uint32_t* strip_cols,
              uint32_t* combine_left, uint32_t* combine_right)
{
  st::clear_error();
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "st_pair_shape: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  ST_REQUIRE(n >= 1 && n <= st::left::kNMax, "st_pair_shape: n must be in [1, 2^31), got %u",
             n);
  if (rows_per_block)
    *rows_per_block = st::left_rows(dtype, n);
  if (strip_cols)
    *strip_cols = st::pair::strip_cols(dtype ? 8 : 4);
  if (combine_left)
    *combine_left = 0; // serial, ascending block order (st_left_shape's)
  if (combine_right)
    *combine_right = 0; // serial, ascending strip order
  return 0;
}

uint64_t
st_pair_scratch(int dtype, unsigned int n)
{
  st::clear_error();
  if (dtype != 0 && dtype != 1) {
    st::set_error("st_pair_scratch: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
    return 0;
  }
  if (n < 1 || n > st::left::kNMax) {
    st::set_error("st_pair_scratch: n must be in [1, 2^31), got %u", n);
    return 0;
  }
  return (uint64_t)st::pair_scratch_elems(dtype, n);
}

const char*
st_pair_shape_desc(void)
{
  static_assert(st::dev::kBlock == 256 && st::dev::kLeftUnroll == 8 &&
                  st::dev::kLeftFinishBlock == 64 && st::kPairPrepGrid == 2048 &&
                  st::left::kNtBytes == ((uint64_t)512 << 20) &&
                  st::pair::strip_cols(4) == 1024 && st::pair::strip_cols(8) == 512 &&
                  st::pair::kChunkRows == 256 && st::left::rows(0, 1) == 32 &&
                  st::left::rows(0, 2048) == 64 && st::left::rows(1, 4096) == 128 &&
                  st::left::rows(1, 16384) == 256,
                "the description below");
  return "block=256 bytes_per_load=16 rows_in_flight=8 strip_cols=1024,512 "
         "rows_per_block=32,64,128,256 rows_from=1,2048,4096,16384 combine_left=serial "
         "combine_right=serial lds_rows=256 finish_block=64 prep_grid=2048 nt_from_mib=512 "
         "launches_per_round=5";
}

#define ST_PAIR_EXPORTS(T, SFX)                                                          \
  int st_pair_sum_##SFX(const T* d_mat, T* d_s_right, T* d_s_left, T* d_scratch,         \
                        unsigned int n, void* stream)                                    \
  {                                                                                      \
    st::clear_error();                                                                   \
    return st::launch_pair_sum<T>(d_mat, d_s_right, d_s_left, d_scratch, n,              \
                                  ST_STREAM(stream));                                    \
  }                                                                                      \
  int st_mfree_pair_round_##SFX(                                                         \
    const T* d_mat0, const T* d_s_prev_right, T* d_s_next_right, const T* d_v_prev_right, \
    T* d_v_cur_right, const T* d_s_prev_left, T* d_s_next_left, const T* d_v_prev_left,  \
    T* d_v_cur_left, T* d_scratch, unsigned int n, T eps, unsigned int k,                \
    unsigned int max_itr, unsigned int semantics, st_state* d_states, void* stream)      \
  {                                                                                      \
    st::clear_error();                                                                   \
    const st::PairVectors<T> v = { { d_s_prev_right, d_s_prev_left },                    \
                                   { d_s_next_right, d_s_next_left },                    \
                                   { d_v_prev_right, d_v_prev_left },                    \
                                   { d_v_cur_right, d_v_cur_left } };                    \
    return st::launch_pair_round<T>(d_mat0, v, d_scratch, n, eps, k, max_itr, semantics, \
                                    d_states, nullptr, ST_STREAM(stream));               \
  }

ST_PAIR_EXPORTS(float, f32)
ST_PAIR_EXPORTS(double, f64)

} // extern "C"
