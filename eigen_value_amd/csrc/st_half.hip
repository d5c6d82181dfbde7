// st_half.hip — launchers of the 16-bit-storage kernels in st_half.h (the
// matrix-free round and K0 on an fp16 / bf16 matrix, fp32 arithmetic) and
// their step-level C-ABI (similarity_transform.h layer 4: st_rowsum_half,
// st_mfree_round_half, st_narrow_f32).

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "st_half.h"
#include "st_internal.h"

// A/B probe switches of this file (`make probe PROBE="-DST_HALF_ROWS=4"`,
// which passes -DST_PROBES=1; a library build with other values fails below)
#ifndef ST_HALF_ROWS // rows per group of the 4-row shapes of k_mfree's table
#define ST_HALF_ROWS 8
#endif
#ifndef ST_HALF_XVEC // 1 = x = v ∘ s from a launch of its own, read as one vector
#define ST_HALF_XVEC 0
#endif
#ifndef ST_HALF_UNROLL // 16-byte chunks in flight per lane and row
#define ST_HALF_UNROLL 2
#endif
#ifndef ST_HALF_UNROLL_MID // the same for the cached 2-row shape (64 - 280 MiB)
#define ST_HALF_UNROLL_MID 1
#endif
#ifndef ST_HALF_GRID // workgroup cap of the grouped shapes (2 per CU)
#define ST_HALF_GRID 512
#endif
#ifndef ST_HALF_NT_MIB // non-temporal matrix loads from this many MiB (N^2 * 2)
#define ST_HALF_NT_MIB 512
#endif
#ifndef ST_PROBES
static_assert(ST_HALF_ROWS == 8 && ST_HALF_XVEC == 0 && ST_HALF_UNROLL == 2 &&
                ST_HALF_UNROLL_MID == 1 && ST_HALF_GRID == 512 &&
                ST_HALF_NT_MIB == 512,
              "A/B probe switch set in a library build (use -DST_PROBES=1)");
#endif
static_assert(ST_HALF_ROWS == 4 || ST_HALF_ROWS == 8, "ST_HALF_ROWS: 4 or 8");

namespace st {
namespace {

using dev::kBlock;

inline bool
aligned16(const void* p)
{
  return ((uintptr_t)p & 15u) == 0;
}

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

// Launch shapes.  The table is k_mfree's (mfree_shape, st_kernels.hip), read
// with the block's real bytes N^2 * 2 - so 8192^2 (128 MiB, inside the 256 MiB
// memory-side cache) takes the cached 2-row shape and 16384^2 (512 MiB) the
// non-temporal one - with kHalfBigRows rows where k_mfree takes 4: per 16
// bytes of matrix a lane reads 8 floats of s and 8 of v (k_mfree<float>: 4 and
// 4), so at 4 rows the L2-served x stream is as many bytes as the matrix
// itself, at 8 rows half of it, k_mfree<float>'s ratio.
// The A/B behind the constants (tools/bench_half.py --ab on probe builds of
// this file, fp16, random input, ms per round, all variants interleaved in
// one process; profiles/half_mfree.json "ab"; two runs, in which identical
// code differed by up to 1.3 %):
//   * rows per group, x formed in the sweep: 8 rows 0.0915 / 0.3377 at
//     16384^2 / 32768^2 against 4 rows 0.0986 / 0.3627 (7 % slower);
//   * x = v ∘ s precomputed by a launch of its own and read as one vector
//     (ST_HALF_XVEC=1; it needs a scratch vector the step API has no argument
//     for): with 4 rows 0.0936 / 0.3237 and 0.0944 / 0.3246 in the second run,
//     with 8 rows 0.0949 / 0.3359, against 8 rows without it 0.0915 / 0.3377
//     and 0.0903 / 0.3296 - 3 - 4 % slower at 16384^2, within 1.5 - 4 % at
//     32768^2, 5 - 6 % slower at 8192^2 (0.0309 vs 0.0290: the extra launch).
//     So: 8 rows, x formed in the sweep;
//   * chunks in flight per lane and row: 2 (1: 0.0982 / 0.3392, 4: 0.1026 /
//     0.3451 against 0.0915 / 0.3377) - but 1 for the cached 2-row shape:
//     8192^2 0.0272 vs 0.0295, 10240^2 0.0383 vs 0.0413 (7 % faster, as are
//     768 / 1024 workgroups instead of 512 there: 0.0275 / 0.0270; nothing
//     at 16384^2 and above, so the cap stays 512);
//   * cached vs non-temporal loads: 16384^2 (512 MiB) 0.0916 cached vs 0.0915,
//     32768^2 0.3531 cached vs 0.3377 (non-temporal 4 % faster); 8192^2
//     (128 MiB, inside the memory-side cache) 0.0276 non-temporal vs 0.0290
//     in the first run, 0.0278 vs 0.0272 in the second (no difference): the
//     threshold stays k_mfree's 512 MiB.
constexpr int kHalfBigRows = ST_HALF_ROWS;
constexpr int kHalfUnroll = ST_HALF_UNROLL;
constexpr int kHalfUnrollMid = ST_HALF_UNROLL_MID;
constexpr uint32_t kHalfGrid = ST_HALF_GRID;
constexpr bool kHalfXvec = ST_HALF_XVEC != 0;
constexpr size_t kHalfNtBytes = (size_t)ST_HALF_NT_MIB << 20;
constexpr uint32_t kHalfSmallRows = 1024; // below: 1 row per group (as mfree_shape)

struct HalfShape
{
  int rows;      // rows per group: 1, 2 or kHalfBigRows
  bool nt;       // non-temporal matrix loads
  uint32_t grid; // workgroup cap
};

inline HalfShape
half_shape(uint32_t nrows, uint32_t ncols)
{
  const size_t b = (size_t)nrows * ncols * 2;
  if (nrows < kHalfSmallRows)
    return { 1, false, 1024u };
  if (b <= ((size_t)64 << 20))
    return { kHalfBigRows, false, kHalfGrid };
  if (b < kHalfNtBytes)
    return { b >= ((size_t)280 << 20) ? kHalfBigRows : 2, false, kHalfGrid };
  return { kHalfBigRows, true, kHalfGrid };
}

#if ST_HALF_XVEC
// probe builds only: the x vector of the precomputed-x form (one per process,
// grown on demand; not thread-safe)
float* g_xvec = nullptr;
uint32_t g_xvec_n = 0;
float*
xvec_scratch(uint32_t n)
{
  if (g_xvec_n < n) {
    if (g_xvec)
      (void)hipFree(g_xvec);
    g_xvec = nullptr;
    g_xvec_n = 0;
    if (hipMalloc((void**)&g_xvec, sizeof(float) * (size_t)n) != hipSuccess)
      return nullptr;
    g_xvec_n = n;
  }
  return g_xvec;
}
#endif

template <typename S, int ROWS, bool VEC, bool NT, int U>
void
launch_mfree_half_cfg(const uint16_t* a0, const float* s_prev, float* s_next,
                      const float* v_prev, float* v_cur, const float* xvec,
                      uint32_t nrows, uint32_t ncols, uint32_t row0, float eps,
                      uint32_t k, uint32_t max_itr, uint32_t semantics,
                      st_state* st, uint32_t cap, hipStream_t stream)
{
  const uint32_t ng_main = nrows / ROWS, nrem = nrows % ROWS;
  const uint32_t ng = ng_main + nrem;
  const uint32_t grid = ng < cap ? ng : cap;
  hipLaunchKernelGGL(
    (dev::k_mfree_half<S, ROWS, U, VEC, NT, kHalfXvec, kBlock>),
    dim3(grid), dim3(kBlock), 0, stream, a0, s_prev, s_next, v_prev, v_cur,
    xvec, ng_main, nrem, ncols, row0, eps, k, max_itr, semantics, st);
}

template <typename S, int ROWS, bool VEC, bool NT, int U>
void
launch_rowsum_half_cfg(const uint16_t* a0, float* s, uint32_t nrows,
                       uint32_t ncols, uint32_t cap, hipStream_t stream)
{
  const uint32_t ng_main = nrows / ROWS, nrem = nrows % ROWS;
  const uint32_t ng = ng_main + nrem;
  const uint32_t grid = ng < cap ? ng : cap;
  hipLaunchKernelGGL((dev::k_rowsum_half<S, ROWS, U, VEC, NT, kBlock>),
                     dim3(grid), dim3(kBlock), 0, stream, a0, s, ng_main, nrem,
                     ncols);
}

// the shape's instantiation: CALL(R, NT, U) for (1, cached), (2, cached),
// (kHalfBigRows, cached / non-temporal)
#define ST_HALF_DISPATCH(sh, CALL)                                             \
  do {                                                                         \
    if ((sh).rows == 1)                                                        \
      CALL(1, false, kHalfUnroll);                                             \
    else if ((sh).rows == 2)                                                   \
      CALL(2, false, kHalfUnrollMid);                                          \
    else if ((sh).nt)                                                          \
      CALL(kHalfBigRows, true, kHalfUnroll);                                   \
    else                                                                       \
      CALL(kHalfBigRows, false, kHalfUnroll);                                  \
  } while (0)

template <typename S>
int
mfree_half(const void* a0v, const float* s_prev, float* s_next,
           const float* v_prev, float* v_cur, uint32_t nrows, uint32_t ncols,
           uint32_t row0, float eps, uint32_t k, uint32_t max_itr,
           uint32_t semantics, st_state* st, hipStream_t stream)
{
  const uint16_t* a0 = static_cast<const uint16_t*>(a0v);
  const float* xvec = nullptr;
#if ST_HALF_XVEC
  float* xw = xvec_scratch(ncols);
  ST_REQUIRE(xw, "mfree_half: x vector allocation failed");
  hipLaunchKernelGGL(dev::k_xvec, dim3((ncols + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, stream, s_prev, v_prev, xw, ncols);
  xvec = xw;
#endif
  const bool vec_ok = (ncols % dev::kHalfW) == 0 && aligned16(a0) &&
                      aligned16(s_prev) && aligned16(v_prev) && aligned16(xvec);
  const HalfShape sh = half_shape(nrows, ncols);
#define ST_HALF_MF(R, N, UU)                                                   \
  (vec_ok ? launch_mfree_half_cfg<S, R, true, N, UU>(                          \
              a0, s_prev, s_next, v_prev, v_cur, xvec, nrows, ncols, row0,     \
              eps, k, max_itr, semantics, st, sh.grid, stream)                 \
          : launch_mfree_half_cfg<S, R, false, N, UU>(                         \
              a0, s_prev, s_next, v_prev, v_cur, xvec, nrows, ncols, row0,     \
              eps, k, max_itr, semantics, st, sh.grid, stream))
  ST_HALF_DISPATCH(sh, ST_HALF_MF);
#undef ST_HALF_MF
  return check_launch("mfree_half");
}

template <typename S>
int
rowsum_half(const void* av, float* s, uint32_t nrows, uint32_t ncols,
            hipStream_t stream)
{
  const uint16_t* a = static_cast<const uint16_t*>(av);
  const bool vec_ok = (ncols % dev::kHalfW) == 0 && aligned16(a);
  const HalfShape sh = half_shape(nrows, ncols);
#define ST_HALF_RS(R, N, UU)                                                   \
  (vec_ok ? launch_rowsum_half_cfg<S, R, true, N, UU>(a, s, nrows, ncols,      \
                                                      sh.grid, stream)         \
          : launch_rowsum_half_cfg<S, R, false, N, UU>(a, s, nrows, ncols,     \
                                                       sh.grid, stream))
  ST_HALF_DISPATCH(sh, ST_HALF_RS);
#undef ST_HALF_RS
  return check_launch("rowsum_half");
}

} // namespace

int
check_storage(const char* what, int storage)
{
  ST_REQUIRE(storage == ST_STORE_F16 || storage == ST_STORE_BF16,
             "%s: storage must be %d (ST_STORE_F16) or %d (ST_STORE_BF16), "
             "got %d", what, ST_STORE_F16, ST_STORE_BF16, storage);
  return 0;
}

int
launch_rowsum_half(int storage, const void* a, float* s, uint32_t nrows,
                   uint32_t ncols, hipStream_t stream)
{
  if (check_storage("rowsum_half", storage))
    return -1;
  ST_REQUIRE(a && s, "rowsum_half: null pointer");
  ST_REQUIRE(((uintptr_t)a & 1u) == 0, "rowsum_half: matrix not 2-byte aligned");
  if (nrows == 0)
    return 0;
  ST_REQUIRE(ncols > 0, "rowsum_half: ncols must be > 0");
  return storage == ST_STORE_F16
           ? rowsum_half<dev::StoreF16>(a, s, nrows, ncols, stream)
           : rowsum_half<dev::StoreBF16>(a, s, nrows, ncols, stream);
}

int
launch_mfree_half(int storage, const void* a0, const float* s_prev,
                  float* s_next, const float* v_prev, float* v_cur,
                  uint32_t nrows, uint32_t ncols, uint32_t row0, float eps,
                  uint32_t k, uint32_t max_itr, uint32_t semantics,
                  st_state* st, hipStream_t stream)
{
  if (check_storage("mfree_half", storage))
    return -1;
  ST_REQUIRE(a0 && s_prev && s_next && v_prev && v_cur && st,
             "mfree_half: null pointer");
  ST_REQUIRE(((uintptr_t)a0 & 1u) == 0, "mfree_half: matrix not 2-byte aligned");
  ST_REQUIRE(nrows > 0 && ncols > 0, "mfree_half: empty block");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "mfree_half: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "mfree_half: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "mfree_half: v_prev and v_cur must differ");
  ST_REQUIRE((uint64_t)row0 + nrows <= ncols,
             "mfree_half: rows [%u, %u + %u) exceed the %u columns", row0, row0,
             nrows, ncols);
  return storage == ST_STORE_F16
           ? mfree_half<dev::StoreF16>(a0, s_prev, s_next, v_prev, v_cur, nrows,
                                       ncols, row0, eps, k, max_itr, semantics,
                                       st, stream)
           : mfree_half<dev::StoreBF16>(a0, s_prev, s_next, v_prev, v_cur,
                                        nrows, ncols, row0, eps, k, max_itr,
                                        semantics, st, stream);
}

int
launch_narrow(int storage, const float* in, void* out, uint64_t count,
              hipStream_t stream)
{
  if (check_storage("st_narrow_f32", storage))
    return -1;
  if (count == 0)
    return 0;
  ST_REQUIRE(in && out, "st_narrow_f32: null pointer");
  const uint64_t want = (count + kBlock - 1) / kBlock;
  const uint32_t grid = want < 65536u ? (uint32_t)want : 65536u;
  if (storage == ST_STORE_F16)
    hipLaunchKernelGGL(dev::k_narrow<dev::StoreF16>, dim3(grid), dim3(kBlock), 0,
                       stream, in, static_cast<uint16_t*>(out), count);
  else
    hipLaunchKernelGGL(dev::k_narrow<dev::StoreBF16>, dim3(grid), dim3(kBlock),
                       0, stream, in, static_cast<uint16_t*>(out), count);
  return check_launch("st_narrow_f32");
}

#define ST_HALF_STR2(x) #x
#define ST_HALF_STR(x) ST_HALF_STR2(x)
const char*
half_shape_desc()
{
  return "rows=" ST_HALF_STR(ST_HALF_ROWS) " xvec=" ST_HALF_STR(ST_HALF_XVEC)
    " unroll=" ST_HALF_STR(ST_HALF_UNROLL) " unroll_mid=" ST_HALF_STR(ST_HALF_UNROLL_MID)
    " grid=" ST_HALF_STR(ST_HALF_GRID) " nt_mib=" ST_HALF_STR(ST_HALF_NT_MIB);
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_rowsum_half(int storage, const void* d_mat, float* d_s, unsigned int nrows,
               unsigned int ncols, void* stream)
{
  st::clear_error();
  return st::launch_rowsum_half(storage, d_mat, d_s, nrows, ncols,
                                ST_STREAM(stream));
}

int
st_mfree_round_half(int storage, const void* d_mat0, const float* d_s_prev,
                    float* d_s_next, const float* d_v_prev, float* d_v_cur,
                    unsigned int nrows, unsigned int ncols, unsigned int row0,
                    float eps, unsigned int k, unsigned int max_itr,
                    unsigned int semantics, st_state* d_state, void* stream)
{
  st::clear_error();
  return st::launch_mfree_half(storage, d_mat0, d_s_prev, d_s_next, d_v_prev,
                               d_v_cur, nrows, ncols, row0, eps, k, max_itr,
                               semantics, d_state, ST_STREAM(stream));
}

int
st_narrow_f32(int storage, const float* d_in, void* d_out, uint64_t count,
              void* stream)
{
  st::clear_error();
  return st::launch_narrow(storage, d_in, d_out, count, ST_STREAM(stream));
}

const char*
st_half_shape_desc(void)
{
  return st::half_shape_desc();
}

} // extern "C"
