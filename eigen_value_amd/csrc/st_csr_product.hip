// st_csr_product.hip — launchers of the kernels in st_csr_product.h (the CSR
// round on the product operator B A, never formed), the pair check and the
// part of its C-ABI that needs no queue (similarity_transform.h section 3g:
// st_csr_apply, st_csr_product_scratch_bytes, st_csr_product_shape_desc,
// st_csr_product_rowsum, st_csr_product_round).  st_solve_csr_product,
// max_eigen_value_csr_product_ex and max_eigen_value_csr_gram_ex live with the
// queue in st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "st_csr_product.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kCsrPrepGrid = 2048; // k_csr_prep's workgroup cap (st_csr.hip)
constexpr uint32_t kCheckGrid = 8192;   // and of the s_0 check

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

// y = H x over H's plan; st == nullptr: not gated
template <typename T>
int
apply(const CsrHandle* h, const T* x, T* y, uint32_t k, const st_state* st,
      hipStream_t stream)
{
  hipLaunchKernelGGL(dev::k_csrp_apply<T>, dim3(h->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                     static_cast<const T*>(h->vals), h->d_order, tab_of(h), x, y, k,
                     st);
  return check_launch("csrp_apply");
}

template <typename T>
int
product_round(const CsrHandle* b, const CsrHandle* a, const T* s_prev, T* s_next,
              const T* v_prev, T* v_cur, T* x, T* y, T eps, uint32_t k,
              uint32_t max_itr, uint32_t semantics, st_state* st, hipStream_t stream)
{
  const uint32_t want = (a->n + kBlock - 1) / kBlock;
  const uint32_t pgrid = want < kCsrPrepGrid ? want : kCsrPrepGrid;
  hipLaunchKernelGGL(dev::k_csr_prep<T>, dim3(pgrid), dim3(kBlock), 0, stream,
                     s_prev, v_prev, x, a->n, eps, k, max_itr, semantics, st);
  if (check_launch("csr_prep (product)"))
    return -1;
  if (apply<T>(a, x, y, k, st, stream))
    return -1;
  hipLaunchKernelGGL(dev::k_csrp_final<T>, dim3(b->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, b->row_ptr, b->col_idx,
                     static_cast<const T*>(b->vals), b->d_order, tab_of(b),
                     (const T*)y, (const T*)x, s_prev, v_prev, s_next, v_cur, k,
                     (const st_state*)st);
  return check_launch("csrp_final");
}

} // namespace

size_t
csr_product_vec_bytes(uint32_t n)
{
  return ((size_t)n * 8 + 255) & ~(size_t)255;
}

int
csr_product_check_pair(const CsrHandle* b, const CsrHandle* a, const char* what)
{
  ST_REQUIRE(b->n == a->n,
             "%s: the factors differ in n (B: %u, A: %u): both are square of one "
             "size", what, b->n, a->n);
  ST_REQUIRE(b->dtype == a->dtype,
             "%s: the factors differ in dtype (B: %d, A: %d; 0 = f32, 1 = f64)",
             what, b->dtype, a->dtype);
  ST_REQUIRE(b->device == a->device,
             "%s: the factors live on different devices (B: %d, A: %d)", what,
             b->device, a->device);
  return 0;
}

int
launch_csr_apply(const CsrHandle* h, const void* x, void* y, hipStream_t stream)
{
  ST_REQUIRE(x && y, "csr_apply: null pointer");
  ST_REQUIRE(x != y, "csr_apply: d_x and d_y must differ");
  if (h->dtype)
    return apply<double>(h, static_cast<const double*>(x), static_cast<double*>(y),
                         0u, nullptr, stream);
  return apply<float>(h, static_cast<const float*>(x), static_cast<float*>(y), 0u,
                      nullptr, stream);
}

int
launch_csr_product_rowsum(const CsrHandle* b, const CsrHandle* a, void* s, void* y,
                          hipStream_t stream)
{
  ST_REQUIRE(s && y, "csr_product_rowsum: null pointer");
  ST_REQUIRE(s != y, "csr_product_rowsum: d_s must not be the scratch");
  if (launch_csr_rowsum(a, y, stream))
    return -1;
  return launch_csr_apply(b, y, s, stream);
}

int
launch_csr_product_round(const CsrHandle* b, const CsrHandle* a, const void* s_prev,
                         void* s_next, const void* v_prev, void* v_cur, void* x,
                         void* y, double eps, uint32_t k, uint32_t max_itr,
                         uint32_t semantics, st_state* st, hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && x && y && st,
             "csr_product_round: null pointer");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_product_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "csr_product_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_product_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_product_round: s_prev and s_next must differ");
  ST_REQUIRE(x != y && x != s_prev && x != s_next && x != v_prev && x != v_cur &&
               y != s_prev && y != s_next && y != v_prev && y != v_cur,
             "csr_product_round: x and y must be scratch of their own");
  if (a->dtype)
    return product_round<double>(
      b, a, static_cast<const double*>(s_prev), static_cast<double*>(s_next),
      static_cast<const double*>(v_prev), static_cast<double*>(v_cur),
      static_cast<double*>(x), static_cast<double*>(y), eps, k, max_itr, semantics,
      st, stream);
  return product_round<float>(
    b, a, static_cast<const float*>(s_prev), static_cast<float*>(s_next),
    static_cast<const float*>(v_prev), static_cast<float*>(v_cur),
    static_cast<float*>(x), static_cast<float*>(y), (float)eps, k, max_itr,
    semantics, st, stream);
}

int
launch_csr_product_check_s0(int dtype, const void* s0, uint32_t n,
                            unsigned long long* d_err, hipStream_t stream)
{
  const uint32_t want = (n + kBlock - 1) / kBlock;
  const uint32_t grid = want < kCheckGrid ? want : kCheckGrid;
  if (dtype)
    hipLaunchKernelGGL(dev::k_csrp_check_s0<double>, dim3(grid), dim3(kBlock), 0,
                       stream, static_cast<const double*>(s0), n, d_err);
  else
    hipLaunchKernelGGL(dev::k_csrp_check_s0<float>, dim3(grid), dim3(kBlock), 0,
                       stream, static_cast<const float*>(s0), n, d_err);
  return check_launch("csrp_check_s0");
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_csr_apply(void* csr, const void* d_x, void* d_y, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_apply");
  if (!h)
    return -1;
  return st::launch_csr_apply(h, d_x, d_y, ST_STREAM(stream));
}

uint64_t
st_csr_product_scratch_bytes(uint32_t n)
{
  if (n == 0 || n >= 0x80000000u)
    return 0;
  return 2 * st::csr_product_vec_bytes(n);
}

const char*
st_csr_product_shape_desc(void)
{
  static_assert(st::kCsrPrepGrid == 2048 && st::kCheckGrid == 8192,
                "the description below");
  return "factors=2 launches_per_round=3 launches_k0=2 prep_grid=2048 "
         "x_offset=0 y_offset=align256(8n) empty_rows=A check_grid=8192";
}

int
st_csr_product_rowsum(void* csr_b, void* csr_a, void* d_s, void* d_scratch,
                      void* stream)
{
  st::clear_error();
  const st::CsrHandle* b = st::as_csr(csr_b, "st_csr_product_rowsum (B)");
  if (!b)
    return -1;
  const st::CsrHandle* a = st::as_csr(csr_a, "st_csr_product_rowsum (A)");
  if (!a || st::csr_product_check_pair(b, a, "st_csr_product_rowsum"))
    return -1;
  ST_REQUIRE(d_scratch, "csr_product_rowsum: null pointer");
  ST_REQUIRE(((uintptr_t)d_scratch & 255u) == 0,
             "csr_product_rowsum: the scratch must be aligned to 256 bytes");
  void* y = static_cast<char*>(d_scratch) + st::csr_product_vec_bytes(a->n);
  return st::launch_csr_product_rowsum(b, a, d_s, y, ST_STREAM(stream));
}

int
st_csr_product_round(void* csr_b, void* csr_a, const void* d_s_prev, void* d_s_next,
                     const void* d_v_prev, void* d_v_cur, void* d_scratch, double eps,
                     unsigned int k, unsigned int max_itr, unsigned int semantics,
                     st_state* d_state, void* stream)
{
  st::clear_error();
  const st::CsrHandle* b = st::as_csr(csr_b, "st_csr_product_round (B)");
  if (!b)
    return -1;
  const st::CsrHandle* a = st::as_csr(csr_a, "st_csr_product_round (A)");
  if (!a || st::csr_product_check_pair(b, a, "st_csr_product_round"))
    return -1;
  ST_REQUIRE(d_scratch, "csr_product_round: null pointer");
  ST_REQUIRE(((uintptr_t)d_scratch & 255u) == 0,
             "csr_product_round: the scratch must be aligned to 256 bytes");
  void* x = d_scratch;
  void* y = static_cast<char*>(d_scratch) + st::csr_product_vec_bytes(a->n);
  return st::launch_csr_product_round(b, a, d_s_prev, d_s_next, d_v_prev, d_v_cur, x,
                                      y, eps, k, max_itr, semantics, d_state,
                                      ST_STREAM(stream));
}

} // extern "C"
