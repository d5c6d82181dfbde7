// st_csr_batch.hip — launchers of the batched sparse (CSR) kernels in
// st_csr_batch.h, the batch handle (validation, row_mat and plan on the
// device) and the part of the C-ABI that needs no queue
// (similarity_transform.h section 3d: st_csr_batch_destroy,
// st_csr_batch_get_plan, st_csr_batch_rowsum, st_csr_batch_mfree_round).
// st_csr_batch_create, st_solve_csr_batched and
// max_eigen_value_csr_batched_ex live with the queue in st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "st_csr_batch.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kCsrbPrepCap = 2048;  // k_csrb_prep workgroups per matrix
constexpr uint32_t kCsrbCheckGrid = 8192; // workgroup cap of the column check
constexpr uint32_t kCsrbCollectGrid = 2048;

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
tab_of(const CsrBatchHandle* h)
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
csrb_round(const CsrBatchHandle* h, const T* s_prev, T* s_next, const T* v_prev,
           T* v_cur, T* x, T eps, uint32_t k, uint32_t max_itr,
           uint32_t semantics, st_state* states, uint32_t* finished,
           hipStream_t stream)
{
  hipLaunchKernelGGL(dev::k_csrb_prep<T>, dim3(h->prep_grid), dim3(kBlock), 0,
                     stream, s_prev, v_prev, x,
                     (const uint32_t*)h->d_mat_first,
                     (const uint32_t*)h->d_wg_first, h->batch, eps, k, max_itr,
                     semantics, states, finished);
  if (check_launch("csrb_prep"))
    return -1;
  dev::CsrStack stack;
  stack.row_mat = h->d_row_mat;
  stack.mat_first = h->d_mat_first;
  stack.states = states;
  stack.k = k;
  hipLaunchKernelGGL(dev::k_csrb_spmv<T>, dim3(h->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                     static_cast<const T*>(h->vals),
                     (const uint32_t*)h->d_order, tab_of(h), (const T*)x,
                     s_prev, v_prev, s_next, v_cur, stack);
  return check_launch("csrb_spmv");
}

// frees what a failed or finished create still holds
struct Scratch
{
  void* p[4] = { nullptr, nullptr, nullptr, nullptr };
  ~Scratch()
  {
    for (void* q : p)
      if (q)
        (void)hipFree(q);
  }
};

} // namespace

int
csr_batch_check_flags(const st_options* opt)
{
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNo = ST_FLAG_TIME_KERNELS | ST_FLAG_TRACE_SUMS |
                           ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND |
                           ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNo) == 0,
             "csr batched solve: ST_FLAG_TIME_KERNELS, ST_FLAG_TRACE_SUMS, "
             "ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the batch is "
             "read only and every round is the same two launches for all of it",
             flags);
  ST_REQUIRE(!opt || opt->semantics <= ST_SEM_MAINPY, "unknown semantics %u",
             opt->semantics);
  return 0;
}

int
csr_batch_check_host(int dtype, uint32_t batch, const uint32_t* mat_first,
                     uint64_t nnz, const int64_t* row_ptr,
                     const int32_t* col_idx, const void* vals)
{
  char msg[448];
  if (csr::check_batch_host(dtype, batch, mat_first, nnz, row_ptr, col_idx, vals,
                            msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  return 0;
}

const CsrBatchHandle*
as_csr_batch(const void* p, const char* what)
{
  const CsrBatchHandle* h = static_cast<const CsrBatchHandle*>(p);
  if (!h || h->magic != kCsrBatchMagic) {
    set_error("%s: not a CSR batch handle (st_csr_batch_create)", what);
    return nullptr;
  }
  return h;
}

int
csr_batch_create(int dtype, uint32_t batch, const uint32_t* mat_first,
                 uint64_t nnz, const int64_t* d_row_ptr,
                 const int32_t* d_col_idx, const void* d_vals,
                 hipStream_t stream, CsrBatchHandle** out)
{
  ST_REQUIRE(out, "st_csr_batch_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  char msg[448];
  if (csr::check_mat_first(batch, mat_first, msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  ST_REQUIRE(d_row_ptr && d_col_idx && d_vals,
             "csr: null row_ptr / col_idx / vals");
  ST_REQUIRE(((uintptr_t)d_row_ptr & 7u) == 0 && ((uintptr_t)d_col_idx & 3u) == 0 &&
               ((uintptr_t)d_vals & (dtype ? 7u : 3u)) == 0,
             "csr: an array is not aligned to its element size");
  const uint32_t n = mat_first[batch];
  const uint32_t nblk = (n + kBlock - 1) / kBlock;
  // the host's tables: mat_first and the first k_csrb_prep workgroup of each
  // matrix, one array [mat_first | wg_first]
  const size_t tab_words = 2 * ((size_t)batch + 1);
  uint32_t* tabs = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * tab_words));
  ST_REQUIRE(tabs, "st_csr_batch_create: out of memory");
  struct FreeHost
  {
    uint32_t* p;
    ~FreeHost() { free(p); }
  } host{ tabs };
  uint32_t* wg_first = tabs + batch + 1;
  memcpy(tabs, mat_first, sizeof(uint32_t) * ((size_t)batch + 1));
  wg_first[0] = 0;
  for (uint32_t b = 0; b < batch; b++) // <= N / 256 + batch: fits
    wg_first[b + 1] = wg_first[b] + csr::batch_prep_wgs(mat_first[b + 1] - mat_first[b],
                                                        kCsrbPrepCap);

  Scratch mem; // [0] err (2 words) + class_first (5), [1] cnt, [2] order, [3] aux
  ST_CHECK(hipMalloc(&mem.p[0], 2 * sizeof(unsigned long long) + 8 * sizeof(uint32_t)));
  ST_CHECK(hipMalloc(&mem.p[1], sizeof(uint32_t) * csr::kClasses * (size_t)nblk));
  ST_CHECK(hipMalloc(&mem.p[2], sizeof(uint32_t) * (size_t)n));
  ST_CHECK(hipMalloc(&mem.p[3], sizeof(uint32_t) * (tab_words + (size_t)n)));
  unsigned long long* d_err = static_cast<unsigned long long*>(mem.p[0]);
  uint32_t* d_cf = reinterpret_cast<uint32_t*>(d_err + 2);
  uint32_t* d_cnt = static_cast<uint32_t*>(mem.p[1]);
  uint32_t* d_order = static_cast<uint32_t*>(mem.p[2]);
  uint32_t* d_aux = static_cast<uint32_t*>(mem.p[3]);
  uint32_t* d_mat_first = d_aux;
  uint32_t* d_wg_first = d_aux + batch + 1;
  uint32_t* d_row_mat = d_aux + tab_words;
  unsigned long long err[2];

  // 1. row_ptr on its own, over the N stacked rows; meanwhile row_mat
  ST_CHECK(hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), stream));
  ST_CHECK(hipMemcpyAsync(d_aux, tabs, sizeof(uint32_t) * tab_words,
                          hipMemcpyHostToDevice, stream));
  if (launch_csr_check_ptr(d_row_ptr, n, nnz, d_cnt, d_err, stream))
    return -1;
  hipLaunchKernelGGL(dev::k_csrb_rowmat, dim3(nblk), dim3(kBlock), 0, stream,
                     (const uint32_t*)d_mat_first, batch, n, d_row_mat);
  if (check_launch("csrb_rowmat"))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[0] != ~0ull) {
    const uint32_t r = (uint32_t)err[0];
    int64_t w[2];
    ST_CHECK(hipMemcpy(w, d_row_ptr + r, sizeof(w), hipMemcpyDeviceToHost));
    csr::describe_batch_row(mat_first, batch, r, w[0], w[1], nnz, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  // 2. only now the column indices, each against its own matrix's size
  {
    const uint32_t rpb = kBlock / 16;
    const uint64_t want = ((uint64_t)n + rpb - 1) / rpb;
    const uint32_t grid = want < kCsrbCheckGrid ? (uint32_t)want : kCsrbCheckGrid;
    hipLaunchKernelGGL(dev::k_csrb_check_col, dim3(grid), dim3(kBlock), 0, stream,
                       d_row_ptr, d_col_idx, (const uint32_t*)d_row_mat,
                       (const uint32_t*)d_mat_first, n, d_err);
    if (check_launch("csrb_check_col"))
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
    csr::describe_batch_col(mat_first, batch, lo, e, c, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  // 3. the plan over the stacked rows (order starts as zeros: every row
  // index a kernel may read from it is in range whatever happens)
  ST_CHECK(hipMemsetAsync(d_order, 0, sizeof(uint32_t) * (size_t)n, stream));
  if (launch_csr_plan(d_row_ptr, n, d_cnt, d_cf, d_order, stream))
    return -1;
  uint32_t cf[csr::kClasses + 1];
  ST_CHECK(hipMemcpyAsync(cf, d_cf, sizeof(cf), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  ST_REQUIRE(cf[0] == 0 && cf[csr::kClasses] == n,
             "internal: csr batch plan covers %u of %u rows", cf[csr::kClasses], n);
  for (int c = 0; c < csr::kClasses; c++)
    ST_REQUIRE(cf[c] <= cf[c + 1], "internal: csr batch plan not monotone");

  CsrBatchHandle* h = new (std::nothrow) CsrBatchHandle();
  ST_REQUIRE(h, "st_csr_batch_create: out of memory");
  h->magic = kCsrBatchMagic;
  h->dtype = dtype;
  (void)hipGetDevice(&h->device);
  h->batch = batch;
  h->n = n;
  h->nnz = nnz;
  h->row_ptr = d_row_ptr;
  h->col_idx = d_col_idx;
  h->vals = d_vals;
  h->d_order = d_order;
  h->d_aux = d_aux;
  h->d_mat_first = d_mat_first;
  h->d_wg_first = d_wg_first;
  h->d_row_mat = d_row_mat;
  h->prep_grid = wg_first[batch];
  h->mat_first = tabs;
  mem.p[2] = mem.p[3] = nullptr; // the handle's now
  host.p = nullptr;
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
csr_batch_destroy(CsrBatchHandle* h)
{
  if (!h)
    return 0;
  ST_REQUIRE(h->magic == kCsrBatchMagic,
             "st_csr_batch_destroy: not a CSR batch handle");
  h->magic = 0;
  if (h->d_order)
    (void)hipFree(h->d_order);
  if (h->d_aux)
    (void)hipFree(h->d_aux);
  free(h->mat_first);
  delete h;
  return 0;
}

int
launch_csrb_rowsum(const CsrBatchHandle* h, void* s, hipStream_t stream)
{
  ST_REQUIRE(s, "csr_batch_rowsum: null pointer");
  if (h->dtype)
    hipLaunchKernelGGL(dev::k_csrb_rowsum<double>, dim3(h->blk_first[csr::kClasses]),
                       dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                       static_cast<const double*>(h->vals),
                       (const uint32_t*)h->d_order, tab_of(h),
                       static_cast<double*>(s));
  else
    hipLaunchKernelGGL(dev::k_csrb_rowsum<float>, dim3(h->blk_first[csr::kClasses]),
                       dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                       static_cast<const float*>(h->vals),
                       (const uint32_t*)h->d_order, tab_of(h),
                       static_cast<float*>(s));
  return check_launch("csrb_rowsum");
}

int
launch_csrb_round(const CsrBatchHandle* h, const void* s_prev, void* s_next,
                  const void* v_prev, void* v_cur, void* x, double eps,
                  uint32_t k, uint32_t max_itr, uint32_t semantics,
                  st_state* states, uint32_t* finished, hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && x && states && finished,
             "csr_batch_mfree_round: null pointer");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_batch_mfree_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0,
             "csr_batch_mfree_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_batch_mfree_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_batch_mfree_round: s_prev and s_next must differ");
  ST_REQUIRE(x != s_prev && x != s_next && x != v_prev && x != v_cur,
             "csr_batch_mfree_round: d_x must be scratch of its own");
  if (h->dtype)
    return csrb_round<double>(h, static_cast<const double*>(s_prev),
                              static_cast<double*>(s_next),
                              static_cast<const double*>(v_prev),
                              static_cast<double*>(v_cur), static_cast<double*>(x),
                              eps, k, max_itr, semantics, states, finished, stream);
  return csrb_round<float>(h, static_cast<const float*>(s_prev),
                           static_cast<float*>(s_next),
                           static_cast<const float*>(v_prev),
                           static_cast<float*>(v_cur), static_cast<float*>(x),
                           (float)eps, k, max_itr, semantics, states, finished,
                           stream);
}

int
launch_csrb_collect(const CsrBatchHandle* h, const void* v0, const void* v1,
                    void* out, const st_state* states, CsrBatchResult* res,
                    hipStream_t stream)
{
  ST_REQUIRE(v0 && v1 && out && states && res, "csr_batch_collect: null pointer");
  ST_REQUIRE(out != v0 && out != v1,
             "csr_batch_collect: the output must differ from both v buffers");
  const uint32_t top = h->n > h->batch ? h->n : h->batch;
  const uint32_t want = (top + kBlock - 1) / kBlock;
  const uint32_t grid = want < kCsrbCollectGrid ? want : kCsrbCollectGrid;
  if (h->dtype)
    hipLaunchKernelGGL(dev::k_csrb_collect<double>, dim3(grid), dim3(kBlock), 0,
                       stream, static_cast<const double*>(v0),
                       static_cast<const double*>(v1), static_cast<double*>(out),
                       (const uint32_t*)h->d_row_mat, states, h->n, h->batch, res);
  else
    hipLaunchKernelGGL(dev::k_csrb_collect<float>, dim3(grid), dim3(kBlock), 0,
                       stream, static_cast<const float*>(v0),
                       static_cast<const float*>(v1), static_cast<float*>(out),
                       (const uint32_t*)h->d_row_mat, states, h->n, h->batch, res);
  return check_launch("csrb_collect");
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

// (similarity_transform.h carries what tools/bench_csr_batched.py measured)
const char*
st_csr_batch_shape_desc(void)
{
  static_assert(st::kCsrbPrepCap == 2048 && st::kCsrbCollectGrid == 2048 &&
                  st::kCsrbCheckGrid == 8192,
                "the description below");
  return "prep: 1 workgroup per 256 rows of a matrix, at most 2048 per matrix, "
         "no workgroup shared by two matrices; spmv: st_csr_shape_desc over the "
         "stacked rows; collect_grid=2048; check: 16 lanes per row, at most 8192 "
         "workgroups";
}

int
st_csr_batch_destroy(void* h)
{
  st::clear_error();
  return st::csr_batch_destroy(static_cast<st::CsrBatchHandle*>(h));
}

int
st_csr_batch_get_plan(void* hp, uint32_t* order_out, uint32_t* class_first)
{
  st::clear_error();
  const st::CsrBatchHandle* h = st::as_csr_batch(hp, "st_csr_batch_get_plan");
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
st_csr_batch_rowsum(void* hp, void* d_s, void* stream)
{
  st::clear_error();
  const st::CsrBatchHandle* h = st::as_csr_batch(hp, "st_csr_batch_rowsum");
  if (!h)
    return -1;
  return st::launch_csrb_rowsum(h, d_s, ST_STREAM(stream));
}

int
st_csr_batch_mfree_round(void* hp, const void* d_s_prev, void* d_s_next,
                         const void* d_v_prev, void* d_v_cur, void* d_x,
                         double eps, unsigned int k, unsigned int max_itr,
                         unsigned int semantics, st_state* d_states,
                         uint32_t* d_finished, void* stream)
{
  st::clear_error();
  const st::CsrBatchHandle* h = st::as_csr_batch(hp, "st_csr_batch_mfree_round");
  if (!h)
    return -1;
  return st::launch_csrb_round(h, d_s_prev, d_s_next, d_v_prev, d_v_cur, d_x, eps,
                               k, max_itr, semantics, d_states, d_finished,
                               ST_STREAM(stream));
}

} // extern "C"
