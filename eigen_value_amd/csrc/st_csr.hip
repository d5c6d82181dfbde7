// st_csr.hip — launchers of the sparse (CSR) kernels in st_csr.h, the matrix
// handle (validation and plan on the device) and the part of the CSR C-ABI
// that needs no queue (similarity_transform.h section 3c: st_csr_class_limits,
// st_csr_plan, st_csr_shape_desc, st_csr_destroy, st_csr_rowsum,
// st_csr_mfree_round).  st_csr_create, st_solve_csr and
// max_eigen_value_csr_ex live with the queue in st_solve.hip.
// launch_csr_check_ptr and launch_csr_plan run the row_ptr check and the plan
// kernels for st_csr_batch.hip, whose stacked rows take the same plan, and
// for st_csr_transpose.hip, which ends in csr_make_handle as csr_create does.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <new>

#include "st_csr.h"
#include "st_csr_plan.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kCsrPrepGrid = 2048;  // workgroup cap of k_csr_prep (8 per CU)
constexpr uint32_t kCsrCheckGrid = 8192; // and of the column check

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

dev::CsrTab
tab_of(const CsrHandle* h)
{
  dev::CsrTab t;
  for (int c = 0; c <= csr::kClasses; c++) {
    t.row_first[c] = h->row_first[c];
    t.blk_first[c] = h->blk_first[c];
  }
  return t;
}

template <typename T>
int
csr_round(const CsrHandle* h, const T* s_prev, T* s_next, const T* v_prev,
          T* v_cur, T* x, T eps, uint32_t k, uint32_t max_itr,
          uint32_t semantics, st_state* st, hipStream_t stream)
{
  const uint32_t want = (h->n + kBlock - 1) / kBlock;
  const uint32_t pgrid = want < kCsrPrepGrid ? want : kCsrPrepGrid;
  hipLaunchKernelGGL(dev::k_csr_prep<T>, dim3(pgrid), dim3(kBlock), 0, stream,
                     s_prev, v_prev, x, h->n, eps, k, max_itr, semantics, st);
  if (check_launch("csr_prep"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_spmv<T>, dim3(h->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                     static_cast<const T*>(h->vals), h->d_order, tab_of(h),
                     (const T*)x, s_prev, v_prev, s_next, v_cur, k,
                     (const st_state*)st);
  return check_launch("csr_spmv");
}

// frees what a failed or finished create still holds
struct Scratch
{
  void* p[3] = { nullptr, nullptr, nullptr };
  ~Scratch()
  {
    for (void* q : p)
      if (q)
        (void)hipFree(q);
  }
};

} // namespace

int
csr_check_flags(const st_options* opt)
{
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNo =
    ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND | ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNo) == 0,
             "csr solve: ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix "
             "is read only and every round is the same two launches", flags);
  ST_REQUIRE(!opt || opt->semantics <= ST_SEM_MAINPY, "unknown semantics %u",
             opt->semantics);
  return 0;
}

int
csr_check_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
               const int32_t* col_idx, const void* vals, uint32_t flags)
{
  char msg[384];
  if (csr::check_host(dtype, n, nnz, row_ptr, col_idx, vals, msg, sizeof(msg),
                      (flags & csr::kEmptyRowsOk) != 0)) {
    set_error("%s", msg);
    return -1;
  }
  return 0;
}

const CsrHandle*
as_csr(const void* p, const char* what)
{
  const CsrHandle* h = static_cast<const CsrHandle*>(p);
  if (!h || h->magic != kCsrMagic) {
    set_error("%s: not a CSR matrix handle (st_csr_create)", what);
    return nullptr;
  }
  return h;
}

int
csr_refuse_empty(const CsrHandle* h, const char* what)
{
  if (h->empty_rows == 0)
    return 0;
  char msg[384];
  csr::describe_needs_terms(what, h->first_empty, h->empty_rows, msg, sizeof(msg));
  set_error("%s", msg);
  return -1;
}

int
csr_create(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
           const int32_t* d_col_idx, const void* d_vals, hipStream_t stream,
           CsrHandle** out, uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0, "st_csr_create_ex: unknown flags %u",
             flags);
  const bool empty_ok = (flags & csr::kEmptyRowsOk) != 0;
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  ST_REQUIRE(n >= 1 && n < 0x80000000u, "csr: n must be in [1, 2^31), got %u", n);
  if (empty_ok) { // arrays of no entry may be null
    char m0[128];
    if (csr::check_nnz_min(nnz, m0, sizeof(m0))) {
      set_error("%s", m0);
      return -1;
    }
  }
  ST_REQUIRE(d_row_ptr && d_col_idx && d_vals,
             "csr: null row_ptr / col_idx / vals");
  ST_REQUIRE(((uintptr_t)d_row_ptr & 7u) == 0 && ((uintptr_t)d_col_idx & 3u) == 0 &&
               ((uintptr_t)d_vals & (dtype ? 7u : 3u)) == 0,
             "csr: an array is not aligned to its element size");
  Scratch mem; // [0] order, until the handle takes it
  uint32_t* d_order = nullptr;
  uint32_t cf[csr::kClasses + 1];
  uint32_t empty_rows = 0, first_empty = n;
  if (csr_check_and_plan(n, nnz, d_row_ptr, d_col_idx, stream, empty_ok, &d_order, cf,
                         &empty_rows, &first_empty))
    return -1;
  mem.p[0] = d_order;
  CsrHandle* h = nullptr;
  if (csr_make_handle(dtype, n, nnz, d_row_ptr, d_col_idx, d_vals, d_order, cf, &h,
                      empty_rows, first_empty))
    return -1;
  mem.p[0] = nullptr; // the handle's now
  *out = h;
  return 0;
}

int
csr_check_and_plan(uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                   const int32_t* d_col_idx, hipStream_t stream, bool empty_ok,
                   uint32_t** d_order_out, uint32_t* cf, uint32_t* empty_rows_out,
                   uint32_t* first_empty_out)
{
  *d_order_out = nullptr;
  const uint32_t nblk = (n + kBlock - 1) / kBlock;
  Scratch mem; // [0] err (2 words) + class_first (5), [1] cnt, [2] order
  ST_CHECK(hipMalloc(&mem.p[0], 2 * sizeof(unsigned long long) + 8 * sizeof(uint32_t)));
  ST_CHECK(hipMalloc(&mem.p[1], sizeof(uint32_t) * csr::kClasses * (size_t)nblk));
  ST_CHECK(hipMalloc(&mem.p[2], sizeof(uint32_t) * (size_t)n));
  unsigned long long* d_err = static_cast<unsigned long long*>(mem.p[0]);
  uint32_t* d_cf = reinterpret_cast<uint32_t*>(d_err + 2);
  uint32_t* d_cnt = static_cast<uint32_t*>(mem.p[1]);
  uint32_t* d_order = static_cast<uint32_t*>(mem.p[2]);
  uint32_t* d_empty = d_cf + 5; // the empty rows (ST_CSR_EMPTY_ROWS_OK)
  unsigned long long err[2];
  char msg[384];

  // 1. row_ptr on its own
  ST_CHECK(hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), stream));
  ST_CHECK(hipMemsetAsync(d_empty, 0, sizeof(uint32_t), stream));
  if (launch_csr_check_ptr(d_row_ptr, n, nnz, d_cnt, d_err, stream,
                           empty_ok ? d_empty : nullptr))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  const uint32_t first_empty = err[1] != ~0ull ? (uint32_t)err[1] : n;
  uint32_t empty_rows = 0;
  if (empty_ok && err[0] == ~0ull) {
    ST_CHECK(hipMemcpy(&empty_rows, d_empty, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // err[1] serves the column check next
    ST_CHECK(hipMemsetAsync(d_err + 1, 0xff, sizeof(unsigned long long), stream));
  }
  if (err[0] != ~0ull) {
    const uint32_t r = (uint32_t)err[0];
    int64_t w[2];
    ST_CHECK(hipMemcpy(w, d_row_ptr + r, sizeof(w), hipMemcpyDeviceToHost));
    csr::describe_row(r, w[0], w[1], n, nnz, msg, sizeof(msg), empty_ok);
    set_error("%s", msg);
    return -1;
  }
  // 2. only now the column indices, entries [0, nnz)
  {
    const uint64_t want = (nnz + kBlock - 1) / kBlock;
    const uint32_t grid = want < kCsrCheckGrid ? (uint32_t)want : kCsrCheckGrid;
    hipLaunchKernelGGL(dev::k_csr_check_col, dim3(grid), dim3(kBlock), 0, stream,
                       d_col_idx, n, nnz, d_err);
    if (check_launch("csr_check_col"))
      return -1;
  }
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[1] != ~0ull) {
    const uint64_t e = err[1];
    int32_t c = 0;
    ST_CHECK(hipMemcpy(&c, d_col_idx + e, sizeof(c), hipMemcpyDeviceToHost));
    uint32_t lo = 0, hi = n; // the row with row_ptr[lo] <= e < row_ptr[lo + 1]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      int64_t p = 0;
      ST_CHECK(hipMemcpy(&p, d_row_ptr + mid, sizeof(p), hipMemcpyDeviceToHost));
      if ((uint64_t)p <= e)
        lo = mid;
      else
        hi = mid;
    }
    set_error("csr: column index %d of entry %llu (row %u) is outside [0, %u)",
              c, (unsigned long long)e, lo, n);
    return -1;
  }
  // 3. the plan (order starts as zeros: every row index a kernel may read
  // from it is in range whatever happens)
  ST_CHECK(hipMemsetAsync(d_order, 0, sizeof(uint32_t) * (size_t)n, stream));
  if (launch_csr_plan(d_row_ptr, n, d_cnt, d_cf, d_order, stream))
    return -1;
  ST_CHECK(hipMemcpyAsync(cf, d_cf, sizeof(uint32_t) * (csr::kClasses + 1),
                          hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  mem.p[2] = nullptr; // the caller's now
  *d_order_out = d_order;
  *empty_rows_out = empty_rows;
  *first_empty_out = first_empty;
  return 0;
}

int
csr_make_handle(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                const int32_t* d_col_idx, const void* d_vals, uint32_t* d_order,
                const uint32_t* cf, CsrHandle** out, uint32_t empty_rows,
                uint32_t first_empty)
{
  ST_REQUIRE(cf[0] == 0 && cf[csr::kClasses] == n,
             "internal: csr plan covers %u of %u rows", cf[csr::kClasses], n);
  for (int c = 0; c < csr::kClasses; c++)
    ST_REQUIRE(cf[c] <= cf[c + 1], "internal: csr plan not monotone");

  CsrHandle* h = new (std::nothrow) CsrHandle();
  ST_REQUIRE(h, "st_csr_create: out of memory");
  h->magic = kCsrMagic;
  h->dtype = dtype;
  (void)hipGetDevice(&h->device);
  h->n = n;
  h->nnz = nnz;
  h->row_ptr = d_row_ptr;
  h->col_idx = d_col_idx;
  h->vals = d_vals;
  h->d_order = d_order;
  h->empty_rows = empty_rows;
  h->first_empty = empty_rows ? first_empty : n;
  uint64_t blocks = 0;
  for (int c = 0; c < csr::kClasses; c++) {
    const uint32_t rpb = csr::kRows[c] * (kBlock / csr::kLanes[c]);
    h->row_first[c] = cf[c];
    h->blk_first[c] = (uint32_t)blocks;
    blocks += ((uint64_t)(cf[c + 1] - cf[c]) + rpb - 1) / rpb;
  }
  h->row_first[csr::kClasses] = n;
  h->blk_first[csr::kClasses] = (uint32_t)blocks;
  *out = h;
  return 0;
}

int
launch_csr_check_ptr(const int64_t* d_row_ptr, uint32_t n, uint64_t nnz,
                     uint32_t* d_cnt, unsigned long long* d_err,
                     hipStream_t stream, uint32_t* d_empty)
{
  hipLaunchKernelGGL(dev::k_csr_check_ptr, dim3((n + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, stream, d_row_ptr, n, nnz, d_cnt, d_err,
                     d_empty);
  return check_launch("csr_check_ptr");
}

int
launch_csr_plan(const int64_t* d_row_ptr, uint32_t n, uint32_t* d_cnt,
                uint32_t* d_cf, uint32_t* d_order, hipStream_t stream)
{
  const uint32_t nblk = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(dev::k_csr_scan, dim3(1), dim3(kBlock), 0, stream, d_cnt,
                     nblk, d_cf);
  if (check_launch("csr_scan"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_order, dim3(nblk), dim3(kBlock), 0, stream,
                     d_row_ptr, n, (const uint32_t*)d_cnt, d_order);
  return check_launch("csr_order");
}

int
csr_destroy(CsrHandle* h)
{
  if (!h)
    return 0;
  ST_REQUIRE(h->magic == kCsrMagic, "st_csr_destroy: not a CSR matrix handle");
  h->magic = 0;
  if (h->d_order)
    (void)hipFree(h->d_order);
  delete h;
  return 0;
}

int
launch_csr_rowsum(const CsrHandle* h, void* s, hipStream_t stream)
{
  ST_REQUIRE(s, "csr_rowsum: null pointer");
  if (h->dtype)
    hipLaunchKernelGGL(dev::k_csr_rowsum<double>, dim3(h->blk_first[csr::kClasses]),
                       dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                       static_cast<const double*>(h->vals), h->d_order,
                       tab_of(h), static_cast<double*>(s));
  else
    hipLaunchKernelGGL(dev::k_csr_rowsum<float>, dim3(h->blk_first[csr::kClasses]),
                       dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                       static_cast<const float*>(h->vals), h->d_order,
                       tab_of(h), static_cast<float*>(s));
  return check_launch("csr_rowsum");
}

int
launch_csr_round(const CsrHandle* h, const void* s_prev, void* s_next,
                 const void* v_prev, void* v_cur, void* x, double eps,
                 uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
                 hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && x && st,
             "csr_mfree_round: null pointer");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_mfree_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0,
             "csr_mfree_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_mfree_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_mfree_round: s_prev and s_next must differ");
  ST_REQUIRE(x != s_prev && x != s_next && x != v_prev && x != v_cur,
             "csr_mfree_round: d_x must be scratch of its own");
  if (h->dtype)
    return csr_round<double>(h, static_cast<const double*>(s_prev),
                             static_cast<double*>(s_next),
                             static_cast<const double*>(v_prev),
                             static_cast<double*>(v_cur), static_cast<double*>(x),
                             eps, k, max_itr, semantics, st, stream);
  return csr_round<float>(h, static_cast<const float*>(s_prev),
                          static_cast<float*>(s_next),
                          static_cast<const float*>(v_prev),
                          static_cast<float*>(v_cur), static_cast<float*>(x),
                          (float)eps, k, max_itr, semantics, st, stream);
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_csr_class_limits(int dtype, uint32_t* nnz_max, uint32_t* lanes, int cap)
{
  st::clear_error();
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "st_csr_class_limits: dtype must be 0 (f32) or 1 (f64), got %d",
             dtype);
  ST_REQUIRE(cap >= 0, "st_csr_class_limits: negative cap");
  for (int c = 0; c < st::csr::kClasses && c < cap; c++) {
    if (nnz_max)
      nnz_max[c] = st::csr::kNnzMax[c];
    if (lanes)
      lanes[c] = st::csr::kLanes[c];
  }
  return st::csr::kClasses;
}

int
st_csr_plan(const int64_t* row_ptr, uint32_t n, uint32_t* order_out,
            uint32_t* class_first)
{
  st::clear_error();
  ST_REQUIRE(row_ptr && order_out && class_first, "st_csr_plan: null pointer");
  ST_REQUIRE(n >= 1 && n < 0x80000000u,
             "st_csr_plan: n must be in [1, 2^31), got %u", n);
  char msg[384];
  const int used =
    st::csr::plan(row_ptr, n, order_out, class_first, msg, sizeof(msg));
  if (used < 0)
    st::set_error("%s", msg);
  return used;
}

// (similarity_transform.h carries what tools/bench_csr.py measured with it)
const char*
st_csr_shape_desc(void)
{
  static_assert(st::csr::kRows[0] == 8 && st::csr::kRows[1] == 4 &&
                  st::csr::kRows[2] == 2 && st::csr::kRows[3] == 1 &&
                  st::csr::kUnroll[0] == 1 && st::csr::kUnroll[1] == 2 &&
                  st::csr::kUnroll[2] == 4 && st::csr::kUnroll[3] == 8 &&
                  st::csr::kNnzMax[0] == 16 && st::csr::kNnzMax[1] == 128 &&
                  st::csr::kNnzMax[2] == 2048 && st::kCsrPrepGrid == 2048 &&
                  st::kCsrCheckGrid == 8192,
                "the description below");
  return "lanes=4,16,64,256 nnz_max=16,128,2048,inf rows=8,4,2,1 "
         "unroll=1,2,4,8 prep_grid=2048 check_grid=8192";
}

int
st_csr_destroy(void* csr)
{
  st::clear_error();
  return st::csr_destroy(static_cast<st::CsrHandle*>(csr));
}

int
st_csr_get_plan(void* csr, uint32_t* order_out, uint32_t* class_first)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_get_plan");
  if (!h)
    return -1;
  int used = 0;
  for (int c = 0; c < st::csr::kClasses; c++)
    used += h->row_first[c + 1] != h->row_first[c];
  if (class_first)
    for (int c = 0; c <= st::csr::kClasses; c++)
      class_first[c] = h->row_first[c];
  if (order_out)
    ST_CHECK(hipMemcpy(order_out, h->d_order, sizeof(uint32_t) * (size_t)h->n,
                       hipMemcpyDeviceToHost));
  return used;
}

int
st_csr_rowsum(void* csr, void* d_s, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_rowsum");
  if (!h)
    return -1;
  return st::launch_csr_rowsum(h, d_s, ST_STREAM(stream));
}

int
st_csr_mfree_round(void* csr, const void* d_s_prev, void* d_s_next,
                   const void* d_v_prev, void* d_v_cur, void* d_x, double eps,
                   unsigned int k, unsigned int max_itr, unsigned int semantics,
                   st_state* d_state, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_mfree_round");
  if (!h || st::csr_refuse_empty(h, "st_csr_mfree_round"))
    return -1;
  return st::launch_csr_round(h, d_s_prev, d_s_next, d_v_prev, d_v_cur, d_x, eps,
                              k, max_itr, semantics, d_state, ST_STREAM(stream));
}

} // extern "C"
