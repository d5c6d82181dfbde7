// Internal helpers shared by the HIP translation units of
// libsimilarity_transform.so (not part of the public C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "similarity_transform.h"

namespace st {

// thread-local last-error message (eigen_last_error)
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();

#define ST_CHECK(expr)                                                         \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      ::st::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr,       \
                      hipGetErrorString(e_));                                  \
      return -1;                                                               \
    }                                                                          \
  } while (0)

#define ST_REQUIRE(cond, ...)                                                  \
  do {                                                                         \
    if (!(cond)) {                                                             \
      ::st::set_error(__VA_ARGS__);                                            \
      return -1;                                                               \
    }                                                                          \
  } while (0)

// "RCCL X.Y.Z (path of the library that holds the bound ncclAllGather)"
// (st_multi.hip; st_version, st_rccl_version)
std::string rccl_desc();

// Restores the caller's current HIP device when a C entry point returns
// (by any path): contexts, shards and communicators switch devices
// internally, and the caller's thread must not see that.
struct DeviceGuard
{
  int prev = -1;
  DeviceGuard()
  {
    if (hipGetDevice(&prev) != hipSuccess)
      prev = -1;
  }
  ~DeviceGuard()
  {
    if (prev >= 0)
      (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// kernel launchers (st_kernels.hip); all asynchronous on `stream`
template <typename T>
int launch_rowsum(const T* a, T* s, uint32_t nrows, uint32_t ncols,
                  hipStream_t stream);
// K0 in the flat form (k_flat_sum + k_parts) for blocks where the flat round
// pays; `part` holds round_flat_scratch(nrows, ncols) elements
template <typename T>
int launch_rowsum_flat(const T* a, T* s, T* part, uint32_t nrows,
                       uint32_t ncols, hipStream_t stream);
template <typename T>
int launch_scale_rowsum(T* a, const T* s_cur, T* s_next, uint32_t nrows,
                        uint32_t ncols, uint32_t row0, uint32_t semantics,
                        const st_state* st, hipStream_t stream);
template <typename T>
int launch_round(T* a, const T* s_cur, T* s_next, T* v, uint32_t nrows,
                 uint32_t ncols, uint32_t row0, T eps, uint32_t k,
                 uint32_t max_itr, uint32_t semantics, st_state* st,
                 hipStream_t stream);
// round k of every matrix of a contiguous [batch][n][n] array in one launch
// (k_round_batched; n below the flat threshold): s_cur / s_next / v are
// [batch][n], st [batch]; each matrix runs launch_round's instantiation for
// n x n and adds 1 to *finished in the round that ends it
template <typename T>
int launch_round_batched(T* a, const T* s_cur, T* s_next, T* v, uint32_t batch,
                         uint32_t n, T eps, uint32_t k, uint32_t max_itr,
                         uint32_t semantics, st_state* st, uint32_t* finished,
                         hipStream_t stream);
// the finished counter -> a pinned host-coherent word, in stream order
int launch_count_mirror(const uint32_t* d_count, uint32_t* h_count,
                        hipStream_t stream);
// the flat round for large blocks (k_flat + k_parts); `part`
// holds round_flat_scratch(nrows, ncols) elements
template <typename T>
int launch_round_flat(T* a, const T* s_cur, T* s_next, T* part, T* v,
                      uint32_t nrows, uint32_t ncols, uint32_t row0, T eps,
                      uint32_t k, uint32_t max_itr, uint32_t semantics,
                      st_state* st, hipStream_t stream);
size_t round_flat_scratch(uint32_t nrows, uint32_t ncols);
bool round_flat_pays(uint32_t nrows, uint32_t ncols, size_t elem);
// the flat round with deferred writes (A stored every defer_rounds(...)
// rounds, bit-identical results; FlatPending in st_device.h): npend pending
// rounds' s and 1/s (oldest first), inv_cur = 1/s_cur, inv_next <- 1/s_{k+1};
// flush = store the matrix only (after the loop; no row sums, no v)
// rounds per store for a block: 6 (launch_flat_deferred's shapes,
// profiles/r02_flat_map_np5_*.log)
uint32_t defer_rounds(uint32_t nrows, uint32_t ncols, size_t elem);
constexpr uint32_t kDeferRoundsMax = 6;
template <typename T>
int launch_round_flat_deferred(T* a, const T* s_cur, const T* inv_cur,
                               T* s_next, T* inv_next, T* part, T* v,
                               uint32_t nrows, uint32_t ncols, uint32_t row0,
                               T eps, uint32_t k, uint32_t max_itr,
                               uint32_t semantics, st_state* st,
                               const T* const* pend_s,
                               const T* const* pend_inv, uint32_t npend,
                               bool store, bool flush, hipStream_t stream);
template <typename T>
int launch_recip(const T* s, T* inv, uint32_t n, hipStream_t stream);
template <typename T>
int launch_mfree(const T* a0, const T* s_prev, T* s_next, const T* v_prev,
                 T* v_cur, uint32_t nrows, uint32_t ncols, uint32_t row0,
                 T eps, uint32_t k, uint32_t max_itr, uint32_t semantics,
                 st_state* st, hipStream_t stream);
// the matrix-free round in the flat form (k_flat<MF> + k_mparts); `part`
// holds round_flat_scratch(nrows, ncols) elements
template <typename T>
int launch_mfree_flat(const T* a0, const T* s_prev, T* s_next, const T* v_prev,
                      T* v_cur, T* part, uint32_t nrows, uint32_t ncols,
                      uint32_t row0, T eps, uint32_t k, uint32_t max_itr,
                      uint32_t semantics, st_state* st, hipStream_t stream);
// the matrix-free round and K0 on a matrix stored in 16 bits (st_half.hip;
// storage = ST_STORE_F16 / ST_STORE_BF16, fp32 vectors and arithmetic), and
// the fp32 -> 16-bit rounding that makes such a matrix
int check_storage(const char* what, int storage);
int launch_rowsum_half(int storage, const void* a, float* s, uint32_t nrows,
                       uint32_t ncols, hipStream_t stream);
int launch_mfree_half(int storage, const void* a0, const float* s_prev,
                      float* s_next, const float* v_prev, float* v_cur,
                      uint32_t nrows, uint32_t ncols, uint32_t row0, float eps,
                      uint32_t k, uint32_t max_itr, uint32_t semantics,
                      st_state* st, hipStream_t stream);
int launch_narrow(int storage, const float* in, void* out, uint64_t count,
                  hipStream_t stream);
// the dense left-vector round (st_left.hip): launch 0 (the column sums) and
// launch k >= 1 (k_csr_prep, k_left_sweep, k_left_finish) on an n x n matrix
// that is only read.  x holds n elements, part left_part_elems(dtype, n);
// the step-level scratch is [x (left_x_elems) | part].  left_rows is RB of
// the order contract, a function of (dtype, n)
uint32_t left_rows(int dtype, uint32_t n);
size_t left_x_elems(uint32_t n);
size_t left_part_elems(int dtype, uint32_t n);
template <typename T>
int launch_colsum(const T* a, T* s, T* part, uint32_t n, hipStream_t stream);
template <typename T>
int launch_left_round(const T* a, const T* s_prev, T* s_next, const T* v_prev,
                      T* v_cur, T* x, T* part, uint32_t n, T eps, uint32_t k,
                      uint32_t max_itr, uint32_t semantics, st_state* st,
                      hipStream_t stream);
// the dense Perron pair round (st_pair.hip): both vectors of an n x n matrix
// that is only read, from one pass over it per launch.  Index 0 of every pair
// is the right side, index 1 the left one; scratch holds
// pair_scratch_elems(dtype, n) elements ([x_R | x_L | colpart | rowpart]).
// d_count (may be null): where the launch's last kernel leaves the number of
// sides whose state is done
template <typename T>
struct PairVectors
{
  const T* s_prev[2];
  T* s_next[2];
  const T* v_prev[2];
  T* v_cur[2];
};
size_t pair_scratch_elems(int dtype, uint32_t n);
template <typename T>
int launch_pair_sum(const T* a, T* s_right, T* s_left, T* scratch, uint32_t n,
                    hipStream_t stream);
template <typename T>
int launch_pair_round(const T* a, const PairVectors<T>& v, T* scratch, uint32_t n, T eps,
                      uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
                      uint32_t* d_count, hipStream_t stream);
// the sparse (CSR) solve (st_csr.hip): a validated matrix with its plan.
// The three arrays stay the caller's; order is the handle's own.
struct CsrHandle
{
  uint32_t magic; // kCsrMagic while alive
  int dtype;      // 0 = f32, 1 = f64
  int device;
  uint32_t n;
  uint64_t nnz;
  const int64_t* row_ptr;
  const int32_t* col_idx;
  const void* vals;
  uint32_t* d_order;     // [n] row indices sorted by class
  uint32_t row_first[5]; // class starts in d_order
  uint32_t blk_first[5]; // class starts in the launch's workgroup range
  // ST_CSR_EMPTY_ROWS_OK handles: the rows without an entry and the lowest
  // one (n when none).  A handle with any is refused by whatever divides by
  // a row sum of A alone (csr_refuse_empty).
  uint32_t empty_rows;
  uint32_t first_empty;
};
constexpr uint32_t kCsrMagic = 0x43535231u;
// the operator A + sum_j u_j w_j^T (st_csr_terms.hip): validated term vectors
// bound to their matrix handle.  The vectors stay the caller's.
struct CsrTermsHandle
{
  uint32_t magic; // kCsrTermsMagic while alive
  int dtype;
  int device;
  uint32_t n;
  uint32_t K;
  const CsrHandle* csr; // the matrix it was checked against
  const void* u[4];
  const void* w[4];
  // st_csr_pattern_terms_create: the pattern handle it was checked against
  // (csr is null then, so every values call refuses the object)
  const struct CsrPatternHandle* pattern;
};
constexpr uint32_t kCsrTermsMagic = 0x43535454u;
// the pattern-only operator diag(r) P diag(c) (st_csr_pattern.hip): validated
// row_ptr / col_idx with their plan, no values at all.  A kind of its own:
// as_csr refuses it by its magic, as_csr_pattern refuses a CsrHandle.  The
// two arrays and the scales (either may be null = all ones) stay the caller's.
struct CsrPatternHandle
{
  uint32_t magic; // kCsrPatternMagic while alive
  int dtype;      // 0 = f32, 1 = f64: the scales' and the vectors'
  int device;
  uint32_t n;
  uint64_t nnz;
  const int64_t* row_ptr;
  const int32_t* col_idx;
  const void* row_scale; // [n] or null
  const void* col_scale; // [n] or null
  uint32_t* d_order;     // [n] row indices sorted by class
  uint32_t row_first[5];
  uint32_t blk_first[5];
  uint32_t empty_rows;
  uint32_t first_empty;
};
constexpr uint32_t kCsrPatternMagic = 0x43535250u;
const CsrPatternHandle* as_csr_pattern(const void* p, const char* what);
// null + error unless t is a live terms object made for this pattern handle
const CsrTermsHandle* as_csr_pattern_terms(const void* t, const CsrPatternHandle* p,
                                           const char* what);
int csr_pattern_refuse_empty(const CsrPatternHandle* p, const char* what);
// validates as csr_create (row_ptr, col_idx, the plan), then the scales in one
// device pass (row_scale before col_scale, the lowest index); synchronises
int csr_pattern_create(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                       const int32_t* d_col_idx, const void* d_row_scale,
                       const void* d_col_scale, hipStream_t stream,
                       CsrPatternHandle** out, uint32_t flags = 0);
int csr_pattern_destroy(CsrPatternHandle* p);
// T(P) into the caller's two arrays, the scales swapped; synchronises
int csr_pattern_transpose(const CsrPatternHandle* p, int64_t* d_t_row_ptr,
                          int32_t* d_t_col_idx, hipStream_t stream,
                          CsrPatternHandle** out, uint32_t flags = 0);
// csr_terms_create's contract on the pattern operator (the vectors, launch 0,
// the rows); synchronises
int csr_pattern_terms_create(const CsrPatternHandle* p, uint32_t K,
                             const void* const* d_u, const void* const* d_w,
                             hipStream_t stream, CsrTermsHandle** out);
// scratch: dots | partial (csr_terms_dots_bytes(K), unused when t is null);
// z [n] apart
int launch_csr_pattern_rowsum(const CsrPatternHandle* p, const CsrTermsHandle* t,
                              void* s, void* dots_part, hipStream_t stream);
int launch_csr_pattern_round(const CsrPatternHandle* p, const CsrTermsHandle* t,
                             const void* s_prev, void* s_next, const void* v_prev,
                             void* v_cur, void* z, void* dots_part, double eps,
                             uint32_t k, uint32_t max_itr, uint32_t semantics,
                             st_state* st, hipStream_t stream);
// the two checked passes and the plan that csr_create and csr_pattern_create
// share: row_ptr on its own, the columns only after it passed, then the plan.
// *d_order_out [n] is the caller's to free or to hand to a handle; cf [5]
int csr_check_and_plan(uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                       const int32_t* d_col_idx, hipStream_t stream, bool empty_ok,
                       uint32_t** d_order_out, uint32_t* cf, uint32_t* empty_rows,
                       uint32_t* first_empty);
// the stable sort by column that csr_transpose and csr_pattern_transpose
// share: vals / d_t_vals null = source rows only.  Outputs as above
int csr_transpose_arrays(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                         const int32_t* col_idx, const void* vals,
                         int64_t* d_t_row_ptr, int32_t* d_t_col_idx, void* d_t_vals,
                         hipStream_t stream, uint32_t flags, uint32_t** d_order_out,
                         uint32_t* cf, uint32_t* empty_rows, uint32_t* first_empty);
int csr_refuse_empty(const CsrHandle* h, const char* what); // -1 + error if it has empty rows
// validates u / w on the device (one pass), then s_0 of the operator;
// synchronises `stream`
int csr_terms_create(const CsrHandle* h, uint32_t K, const void* const* d_u,
                     const void* const* d_w, hipStream_t stream,
                     CsrTermsHandle** out);
int csr_terms_destroy(CsrTermsHandle* t);
// null + error unless t is a live terms object made for h
const CsrTermsHandle* as_csr_terms(const void* t, const CsrHandle* h, const char* what);
// bytes of the round's scratch: dots [K] | partial [K][2048] | x [n]
size_t csr_terms_scratch_bytes(uint32_t n, uint32_t K);
size_t csr_terms_dots_bytes(uint32_t K); // the part before x
// scratch: dots | partial (csr_terms_dots_bytes); x [n] apart
int launch_csr_terms_rowsum(const CsrHandle* h, const CsrTermsHandle* t, void* s,
                            void* dots_part, hipStream_t stream);
int launch_csr_terms_round(const CsrHandle* h, const CsrTermsHandle* t,
                           const void* s_prev, void* s_next, const void* v_prev,
                           void* v_cur, void* x, void* dots_part, double eps,
                           uint32_t k, uint32_t max_itr, uint32_t semantics,
                           st_state* st, hipStream_t stream);
// the product operator B A of two matrix handles (st_csr_product.hip), never
// formed.  -1 + error unless b and a agree in n, dtype and device (in that
// order)
int csr_product_check_pair(const CsrHandle* b, const CsrHandle* a, const char* what);
// bytes of one of the round's two scratch vectors (x, then y), 256-byte aligned
size_t csr_product_vec_bytes(uint32_t n);
// y = H x in the row order of the solve; no division, an empty row gives 0
int launch_csr_apply(const CsrHandle* h, const void* x, void* y, hipStream_t stream);
// K0: y = the row sums of A, s = B y
int launch_csr_product_rowsum(const CsrHandle* b, const CsrHandle* a, void* s, void* y,
                              hipStream_t stream);
int launch_csr_product_round(const CsrHandle* b, const CsrHandle* a, const void* s_prev,
                             void* s_next, const void* v_prev, void* v_cur, void* x,
                             void* y, double eps, uint32_t k, uint32_t max_itr,
                             uint32_t semantics, st_state* st, hipStream_t stream);
// d_err[0] (preset to ~0) <- the lowest row whose s0 is not finite and > 0
int launch_csr_product_check_s0(int dtype, const void* s0, uint32_t n,
                                unsigned long long* d_err, hipStream_t stream);
// up to 8 operators A + sum_j u_{c,j} w_{c,j}^T on one matrix handle
// (st_csr_multi.hip): the validated term vectors packed [K][n][CP], and the
// packed vectors of the solve loop.  Everything is the object's own (one
// allocation); one solve at a time runs on it.
struct CsrMultiHandle
{
  uint32_t magic; // kCsrMultiMagic while alive
  int dtype;
  int device;
  uint32_t n;
  uint32_t C;  // columns
  uint32_t K;  // terms per column
  uint32_t CP; // packed width: 2, 4 or 8 >= C
  const CsrHandle* csr; // the matrix it was checked against
  void* mem;
  void* u; // [K][n][CP]
  void* w;
  void* s[2]; // [n][CP]
  void* v[2];
  void* scratch;         // dots | partial | x (csr_multi_scratch_bytes)
  uint32_t blk_first[5]; // class starts in the row pass's workgroup range
};
constexpr uint32_t kCsrMultiMagic = 0x4353524du;
// validates on the device per column (the vectors, then s_0 of every M_c) and
// packs; synchronises `stream`.  h_pu / h_pw != nullptr (the host twin, which
// validated the vectors itself): packed host arrays [K][n][CP] copied in
// instead of d_u / d_w
int csr_multi_create(const CsrHandle* h, uint32_t C, uint32_t K,
                     const void* const* d_u, const void* const* d_w,
                     hipStream_t stream, CsrMultiHandle** out,
                     const void* h_pu = nullptr, const void* h_pw = nullptr);
int csr_multi_destroy(CsrMultiHandle* t);
const CsrMultiHandle* as_csr_multi(const void* t, const CsrHandle* h, const char* what);
// dots [C][K] | partial [C][K][2048] (csr_multi_dots_bytes, x [n][CP] behind)
size_t csr_multi_scratch_bytes(uint32_t n, uint32_t C, uint32_t K);
size_t csr_multi_dots_bytes(uint32_t C, uint32_t K);
int launch_csr_multi_rowsum(const CsrHandle* h, const CsrMultiHandle* t, void* s,
                            void* scratch, hipStream_t stream);
int launch_csr_multi_round(const CsrHandle* h, const CsrMultiHandle* t,
                           const void* s_prev, void* s_next, const void* v_prev,
                           void* v_cur, void* scratch, double eps, uint32_t k,
                           uint32_t max_itr, uint32_t semantics, st_state* states,
                           uint32_t* finished, hipStream_t stream);
struct CsrBatchResult;
// out [C][n] <- each column's final v from v0 / v1 by the parity of its end
int launch_csr_multi_collect(const CsrMultiHandle* t, const void* v0, const void* v1,
                             void* out, const st_state* states, CsrBatchResult* res,
                             hipStream_t stream);
// what is checked on the host before anything is enqueued: the flags of a
// CSR solve, and a host-resident matrix (dtype, n, row_ptr, then col_idx)
int csr_check_flags(const st_options* opt);
int csr_check_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                   const int32_t* col_idx, const void* vals, uint32_t flags = 0);
// validates on the device (row_ptr first, col_idx only after it passed),
// builds the plan; synchronises `stream`
int csr_create(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
               const int32_t* d_col_idx, const void* d_vals, hipStream_t stream,
               CsrHandle** out, uint32_t flags = 0);
// the handle over checked arrays and their plan (d_order [n], which becomes
// the handle's own; cf [5] the class starts on the host)
int csr_make_handle(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                    const int32_t* d_col_idx, const void* d_vals,
                    uint32_t* d_order, const uint32_t* cf, CsrHandle** out,
                    uint32_t empty_rows = 0, uint32_t first_empty = 0);
// the stable transposition (st_csr_transpose.hip): T(a) into the caller's
// device arrays, which must not overlap a's, and a handle over them with its
// plan; synchronises `stream`.  The host twin needs no GPU.
int csr_transpose(const CsrHandle* a, int64_t* d_t_row_ptr, int32_t* d_t_col_idx,
                  void* d_t_vals, hipStream_t stream, CsrHandle** out,
                  uint32_t flags = 0);
int csr_transpose_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                       const int32_t* col_idx, const void* vals,
                       int64_t* t_row_ptr, int32_t* t_col_idx, void* t_vals,
                       uint32_t flags = 0);
int csr_destroy(CsrHandle* h);
const CsrHandle* as_csr(const void* p, const char* what); // null + error if not one
int launch_csr_rowsum(const CsrHandle* h, void* s, hipStream_t stream);
int launch_csr_round(const CsrHandle* h, const void* s_prev, void* s_next,
                     const void* v_prev, void* v_cur, void* x, double eps,
                     uint32_t k, uint32_t max_itr, uint32_t semantics,
                     st_state* st, hipStream_t stream);
// the two device passes of csr_create that a stacked batch shares: row_ptr's
// predicate over n rows (d_err[0] = the lowest offending row, d_cnt
// [ceil(n / 256)][4] = the rows of each class per block) and, from d_cnt,
// the plan (d_cf [5] class starts, d_order [n])
// d_empty != nullptr (ST_CSR_EMPTY_ROWS_OK): empty rows are legal, counted
// there (zeroed by the caller), d_err[1] = the lowest one
int launch_csr_check_ptr(const int64_t* d_row_ptr, uint32_t n, uint64_t nnz,
                         uint32_t* d_cnt, unsigned long long* d_err,
                         hipStream_t stream, uint32_t* d_empty = nullptr);
int launch_csr_plan(const int64_t* d_row_ptr, uint32_t n, uint32_t* d_cnt,
                    uint32_t* d_cf, uint32_t* d_order, hipStream_t stream);
// a batch of sparse matrices in stacked CSR storage (st_csr_batch.hip),
// validated, with the plan over its N stacked rows.  The three arrays stay
// the caller's; the rest is the handle's own.
struct CsrBatchHandle
{
  uint32_t magic; // kCsrBatchMagic while alive
  int dtype;      // 0 = f32, 1 = f64
  int device;
  uint32_t batch;
  uint32_t n; // N, the stacked rows
  uint64_t nnz;
  const int64_t* row_ptr;
  const int32_t* col_idx;
  const void* vals;
  uint32_t* d_order;     // [N] stacked row indices sorted by class
  uint32_t* d_aux;       // one allocation: the three arrays below
  uint32_t* d_mat_first; // [batch + 1]
  uint32_t* d_wg_first;  // [batch + 1] k_csrb_prep's first workgroup per matrix
  uint32_t* d_row_mat;   // [N] the matrix of each stacked row
  uint32_t prep_grid;    // wg_first[batch]
  uint32_t row_first[5]; // class starts in d_order
  uint32_t blk_first[5]; // class starts in the launch's workgroup range
  uint32_t* mat_first;   // host copy [batch + 1]
};
constexpr uint32_t kCsrBatchMagic = 0x43535242u;
// what k_csrb_collect hands the host of each matrix's st_state
struct CsrBatchResult
{
  double lambda;
  uint32_t iters, stop, end, done;
};
static_assert(sizeof(CsrBatchResult) == 24, "result layout");
int csr_batch_check_flags(const st_options* opt);
int csr_batch_check_host(int dtype, uint32_t batch, const uint32_t* mat_first,
                         uint64_t nnz, const int64_t* row_ptr,
                         const int32_t* col_idx, const void* vals);
// validates on the device (mat_first on the host, row_ptr, then col_idx
// against each matrix's own size), builds row_mat and the plan; synchronises
int csr_batch_create(int dtype, uint32_t batch, const uint32_t* mat_first,
                     uint64_t nnz, const int64_t* d_row_ptr,
                     const int32_t* d_col_idx, const void* d_vals,
                     hipStream_t stream, CsrBatchHandle** out);
int csr_batch_destroy(CsrBatchHandle* h);
const CsrBatchHandle* as_csr_batch(const void* p, const char* what);
int launch_csrb_rowsum(const CsrBatchHandle* h, void* s, hipStream_t stream);
int launch_csrb_round(const CsrBatchHandle* h, const void* s_prev, void* s_next,
                      const void* v_prev, void* v_cur, void* x, double eps,
                      uint32_t k, uint32_t max_itr, uint32_t semantics,
                      st_state* states, uint32_t* finished, hipStream_t stream);
// out [N] <- each matrix's final v from v0 / v1 by the parity of its end;
// res [batch] <- the states
int launch_csrb_collect(const CsrBatchHandle* h, const void* v0, const void* v1,
                        void* out, const st_state* states, CsrBatchResult* res,
                        hipStream_t stream);
template <typename T>
int launch_epilogue(const T* s, T* v, uint32_t n, T eps, uint32_t max_itr,
                    uint32_t semantics, st_state* st, hipStream_t stream);
// st_state -> pinned host-coherent memory, in stream order (the solve loops'
// per-batch flag read)
int launch_state_mirror(const st_state* d_state, st_state* h_state,
                        hipStream_t stream);

template <typename T>
int launch_fill(T* x, uint64_t count, T value, hipStream_t stream);
// the whole solve in one workgroup (k_solve_small): v = 1, s_0, every round,
// the final state; for n <= 128 (fp64) / 256 (fp32), n % (16/sizeof(T)) == 0
template <typename T>
bool solve_small_fits(const T* a, uint32_t n);
template <typename T>
int launch_solve_small(T* a, T* v, uint32_t n, T eps, uint32_t max_itr,
                       uint32_t semantics, st_state* st, hipStream_t stream);
// the same solve for every matrix of a contiguous [batch][n][n] array in one
// launch (k_solve_batched, a workgroup per matrix): v to v + b n, the result
// to st[b]; any n from 1 to solve_batched_max_n (128 fp64 / 256 fp32)
template <typename T>
uint32_t solve_batched_max_n();
template <typename T>
int launch_solve_batched(T* a, T* v, uint32_t batch, uint32_t n, T eps,
                         uint32_t max_itr, uint32_t semantics, st_state* st,
                         hipStream_t stream);
// The workgroup shape classes of the two launchers above and below:
// class c holds n <= 4 << c (4, 8, 16, 32, 64, 128, 256; the last fp32
// only).  solve_shape_class(n) is the one place that maps n to its class;
// kSolveShapeClasses is returned for an n beyond all of them.
constexpr uint32_t kSolveShapeClasses = 7;
uint32_t solve_shape_class(uint32_t n);
// one matrix of a variable-size batch, as k_solve_vbatched reads it
struct VBatchDesc
{
  uint64_t mat;   // device address of the n x n row-major matrix
  uint64_t v_off; // element offset of its eigenvector in the packed v buffer
  uint32_t n;
  uint32_t id;    // its index in the caller's arrays (and in the state array)
};
static_assert(sizeof(VBatchDesc) == 24, "descriptor layout");
// one shape class of a variable-size batch in one launch (k_solve_vbatched):
// descs is the device table in plan order (descs[j] describes matrix
// order[j]); workgroup i solves the matrix of descs[first + i] (i < count,
// every one of class cls) as launch_solve_batched's workgroup would, v to
// v + v_off, the result to st[id]
template <typename T>
int launch_solve_vbatched(const VBatchDesc* descs, uint32_t first,
                          uint32_t count, uint32_t cls, T* v, T eps,
                          uint32_t max_itr, uint32_t semantics, st_state* st,
                          hipStream_t stream);

} // namespace st
