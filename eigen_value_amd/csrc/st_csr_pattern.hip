// st_csr_pattern.hip — launchers of the kernels in st_csr_pattern.h (the CSR
// round on the pattern-only operator diag(r) P diag(c)), the pattern handle
// (validation and plan on the device, shared with st_csr.hip; the scales in
// one more pass), its transposition (st_csr_transpose.hip's sort, the scales
// swapped), its terms object and the part of its C-ABI that needs no queue
// (similarity_transform.h section 3h: st_csr_pattern_destroy,
// st_csr_pattern_get_plan, st_csr_pattern_empty_rows,
// st_csr_pattern_scratch_bytes, st_csr_pattern_shape_desc,
// st_csr_pattern_rowsum, st_csr_pattern_round).  st_csr_pattern_create,
// st_csr_pattern_transpose, st_csr_pattern_terms_create, st_solve_csr_pattern
// and max_eigen_value_csr_pattern_ex live with the queue in st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <new>

#include "st_csr_pattern.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kPatPrepGrid = 2048;  // workgroup cap of the vector pass
constexpr uint32_t kPatCheckGrid = 8192; // and of the validation passes
constexpr size_t kDotsBytes = 256;       // dots [K], then partial (st_csr_terms.hip)

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
tab_of(const CsrPatternHandle* h)
{
  dev::CsrTab t;
  for (int c = 0; c <= csr::kClasses; c++) {
    t.row_first[c] = h->row_first[c];
    t.blk_first[c] = h->blk_first[c];
  }
  return t;
}

uint32_t
prep_grid(uint32_t n)
{
  static_assert(kPatPrepGrid == dev::kCsrDotGrid, "the dots' order is the vector pass's");
  const uint32_t want = (n + kBlock - 1) / kBlock;
  return want < kPatPrepGrid ? want : kPatPrepGrid;
}

template <typename T>
dev::CsrDots<T>
dots_of(const CsrTermsHandle* t, void* dots_part)
{
  dev::CsrDots<T> d;
  d.K = t->K;
  for (uint32_t j = 0; j < csr::kTermsMax; j++)
    d.w[j] = j < t->K ? static_cast<const T*>(t->w[j]) : nullptr;
  d.partial = reinterpret_cast<T*>(static_cast<char*>(dots_part) + kDotsBytes);
  return d;
}

template <typename T, int KM>
dev::CsrTerms<T, KM>
terms_of(const CsrTermsHandle* t, void* dots_part)
{
  dev::CsrTerms<T, KM> g;
  g.K = t->K;
  for (uint32_t j = 0; j < (uint32_t)KM; j++)
    g.u[j] = j < t->K ? static_cast<const T*>(t->u[j]) : nullptr;
  g.dots = static_cast<const T*>(dots_part);
  return g;
}

// the row pass of launch 0 for one G; the scales pick the instantiation, so
// that a null scale costs nothing
template <typename T, typename G>
void
launch_rowsum_g(const CsrPatternHandle* h, T* s, const G& g, hipStream_t stream)
{
  const T* cs = static_cast<const T*>(h->col_scale);
  const T* rs = static_cast<const T*>(h->row_scale);
  const dim3 grid(h->blk_first[csr::kClasses]), block(kBlock);
#define ST_PAT_K0(ZONE, RS)                                                        \
  hipLaunchKernelGGL((dev::k_csr_pattern_rowsum<T, ZONE, RS, G>), grid, block, 0,  \
                     stream, h->row_ptr, h->col_idx, h->d_order, tab_of(h), cs,    \
                     rs, s, g)
  if (!cs && !rs)
    ST_PAT_K0(true, false);
  else if (!cs)
    ST_PAT_K0(true, true);
  else if (!rs)
    ST_PAT_K0(false, false);
  else
    ST_PAT_K0(false, true);
#undef ST_PAT_K0
}

template <typename T, typename G>
void
launch_spmv_g(const CsrPatternHandle* h, const T* z, const T* s_prev, const T* v_prev,
              T* s_next, T* v_cur, uint32_t k, const st_state* st, const G& g,
              hipStream_t stream)
{
  const T* rs = static_cast<const T*>(h->row_scale);
  const dim3 grid(h->blk_first[csr::kClasses]), block(kBlock);
  if (rs)
    hipLaunchKernelGGL((dev::k_csr_pattern_spmv<T, true, G>), grid, block, 0, stream,
                       h->row_ptr, h->col_idx, h->d_order, tab_of(h), z, rs, s_prev,
                       v_prev, s_next, v_cur, k, st, g);
  else
    hipLaunchKernelGGL((dev::k_csr_pattern_spmv<T, false, G>), grid, block, 0, stream,
                       h->row_ptr, h->col_idx, h->d_order, tab_of(h), z, rs, s_prev,
                       v_prev, s_next, v_cur, k, st, g);
}

template <typename T>
int
pattern_rowsum(const CsrPatternHandle* h, const CsrTermsHandle* t, T* s, void* dots_part,
               hipStream_t stream)
{
  if (!t) {
    launch_rowsum_g<T>(h, s, dev::CsrOne(), stream);
    return check_launch("csr_pattern_rowsum");
  }
  // the dots of launch 0 are taken on x ≡ 1: w_j . 1
  const uint32_t pgrid = prep_grid(h->n);
  const dev::CsrDots<T> d = dots_of<T>(t, dots_part);
  hipLaunchKernelGGL(dev::k_csr_wsum<T>, dim3(pgrid), dim3(kBlock), 0, stream, h->n, d);
  if (check_launch("csr_wsum"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_dots<T>, dim3(1), dim3(kBlock), 0, stream,
                     (const T*)d.partial, pgrid, t->K, static_cast<T*>(dots_part), 0u,
                     (const st_state*)nullptr);
  if (check_launch("csr_dots"))
    return -1;
  // launch 0 runs once per solve: one instantiation with registers for 4 terms
  launch_rowsum_g<T>(h, s, terms_of<T, dev::kCsrTermsMax>(t, dots_part), stream);
  return check_launch("csr_pattern_rowsum (terms)");
}

template <typename T>
int
pattern_round(const CsrPatternHandle* h, const CsrTermsHandle* t, const T* s_prev,
              T* s_next, const T* v_prev, T* v_cur, T* z, void* dots_part, T eps,
              uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
              hipStream_t stream)
{
  const uint32_t pgrid = prep_grid(h->n);
  const T* cs = static_cast<const T*>(h->col_scale);
  // the vector pass: without c, k_csr_prep as it is (z = x)
  if (!t) {
    if (cs)
      hipLaunchKernelGGL(dev::k_csr_pattern_prep<T>, dim3(pgrid), dim3(kBlock), 0,
                         stream, s_prev, v_prev, cs, z, h->n, eps, k, max_itr,
                         semantics, st);
    else
      hipLaunchKernelGGL(dev::k_csr_prep<T>, dim3(pgrid), dim3(kBlock), 0, stream,
                         s_prev, v_prev, z, h->n, eps, k, max_itr, semantics, st);
    if (check_launch("csr_pattern_prep"))
      return -1;
    launch_spmv_g<T>(h, z, s_prev, v_prev, s_next, v_cur, k, st, dev::CsrOne(), stream);
    return check_launch("csr_pattern_spmv");
  }
  const dev::CsrDots<T> d = dots_of<T>(t, dots_part);
  if (cs)
    hipLaunchKernelGGL((dev::k_csr_pattern_prep<T, dev::CsrDots<T>>), dim3(pgrid),
                       dim3(kBlock), 0, stream, s_prev, v_prev, cs, z, h->n, eps, k,
                       max_itr, semantics, st, d);
  else
    hipLaunchKernelGGL((dev::k_csr_prep<T, dev::CsrDots<T>>), dim3(pgrid), dim3(kBlock),
                       0, stream, s_prev, v_prev, z, h->n, eps, k, max_itr, semantics,
                       st, d);
  if (check_launch("csr_pattern_prep (terms)"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_dots<T>, dim3(1), dim3(kBlock), 0, stream,
                     (const T*)d.partial, pgrid, t->K, static_cast<T*>(dots_part), k,
                     (const st_state*)st);
  if (check_launch("csr_dots"))
    return -1;
  if (t->K == 1) // the instantiation with registers for K terms (1, 2 or 4)
    launch_spmv_g<T>(h, z, s_prev, v_prev, s_next, v_cur, k, st,
                     terms_of<T, 1>(t, dots_part), stream);
  else if (t->K == 2)
    launch_spmv_g<T>(h, z, s_prev, v_prev, s_next, v_cur, k, st,
                     terms_of<T, 2>(t, dots_part), stream);
  else
    launch_spmv_g<T>(h, z, s_prev, v_prev, s_next, v_cur, k, st,
                     terms_of<T, 4>(t, dots_part), stream);
  return check_launch("csr_pattern_spmv (terms)");
}

struct Freed
{
  void* p = nullptr;
  ~Freed()
  {
    if (p)
      (void)hipFree(p);
  }
};

int
read_elem(int dtype, const void* base, uint64_t i, double* x)
{
  if (dtype) {
    ST_CHECK(hipMemcpy(x, static_cast<const char*>(base) + 8 * i, 8,
                       hipMemcpyDeviceToHost));
  } else {
    float f = 0;
    ST_CHECK(hipMemcpy(&f, static_cast<const char*>(base) + 4 * i, 4,
                       hipMemcpyDeviceToHost));
    *x = (double)f;
  }
  return 0;
}

int
make_pattern(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
             const int32_t* d_col_idx, const void* rs, const void* cs, uint32_t* d_order,
             const uint32_t* cf, uint32_t empty_rows, uint32_t first_empty,
             CsrPatternHandle** out)
{
  ST_REQUIRE(cf[0] == 0 && cf[csr::kClasses] == n,
             "internal: csr plan covers %u of %u rows", cf[csr::kClasses], n);
  for (int c = 0; c < csr::kClasses; c++)
    ST_REQUIRE(cf[c] <= cf[c + 1], "internal: csr plan not monotone");
  CsrPatternHandle* h = new (std::nothrow) CsrPatternHandle();
  ST_REQUIRE(h, "st_csr_pattern_create: out of memory");
  h->magic = kCsrPatternMagic;
  h->dtype = dtype;
  (void)hipGetDevice(&h->device);
  h->n = n;
  h->nnz = nnz;
  h->row_ptr = d_row_ptr;
  h->col_idx = d_col_idx;
  h->row_scale = rs;
  h->col_scale = cs;
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

} // namespace

const CsrPatternHandle*
as_csr_pattern(const void* p, const char* what)
{
  const CsrPatternHandle* h = static_cast<const CsrPatternHandle*>(p);
  if (!h || h->magic != kCsrPatternMagic) {
    set_error("%s: not a CSR pattern handle (st_csr_pattern_create)", what);
    return nullptr;
  }
  return h;
}

const CsrTermsHandle*
as_csr_pattern_terms(const void* p, const CsrPatternHandle* h, const char* what)
{
  const CsrTermsHandle* t = static_cast<const CsrTermsHandle*>(p);
  if (!t || t->magic != kCsrTermsMagic) {
    set_error("%s: not a terms object (st_csr_pattern_terms_create), or a destroyed "
              "one", what);
    return nullptr;
  }
  if (t->pattern != h || t->n != h->n || t->dtype != h->dtype || t->device != h->device) {
    set_error("%s: the terms object belongs to another handle (its own: n = %u, dtype "
              "%d, device %d; this one: n = %u, dtype %d, device %d)",
              what, t->n, t->dtype, t->device, h->n, h->dtype, h->device);
    return nullptr;
  }
  return t;
}

int
csr_pattern_refuse_empty(const CsrPatternHandle* h, const char* what)
{
  if (h->empty_rows == 0)
    return 0;
  char msg[384];
  csr::describe_pattern_needs_terms(what, h->first_empty, h->empty_rows, msg,
                                    sizeof(msg));
  set_error("%s", msg);
  return -1;
}

int
csr_pattern_create(int dtype, uint32_t n, uint64_t nnz, const int64_t* d_row_ptr,
                   const int32_t* d_col_idx, const void* d_row_scale,
                   const void* d_col_scale, hipStream_t stream, CsrPatternHandle** out,
                   uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_pattern_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "st_csr_pattern_create: unknown flags %u", flags);
  const bool empty_ok = (flags & csr::kEmptyRowsOk) != 0;
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  ST_REQUIRE(n >= 1 && n < 0x80000000u, "csr: n must be in [1, 2^31), got %u", n);
  if (empty_ok) {
    char m0[128];
    if (csr::check_nnz_min(nnz, m0, sizeof(m0))) {
      set_error("%s", m0);
      return -1;
    }
  }
  ST_REQUIRE(d_row_ptr && d_col_idx, "csr: null row_ptr / col_idx");
  const uintptr_t em = dtype ? 7u : 3u;
  ST_REQUIRE(((uintptr_t)d_row_ptr & 7u) == 0 && ((uintptr_t)d_col_idx & 3u) == 0 &&
               ((uintptr_t)d_row_scale & em) == 0 && ((uintptr_t)d_col_scale & em) == 0,
             "csr: an array is not aligned to its element size");
  Freed order;
  uint32_t* d_order = nullptr;
  uint32_t cf[csr::kClasses + 1];
  uint32_t empty_rows = 0, first_empty = n;
  if (csr_check_and_plan(n, nnz, d_row_ptr, d_col_idx, stream, empty_ok, &d_order, cf,
                         &empty_rows, &first_empty))
    return -1;
  order.p = d_order;
  if (d_row_scale || d_col_scale) { // the scales, one pass
    Freed mem;
    ST_CHECK(hipMalloc(&mem.p, sizeof(unsigned long long)));
    unsigned long long* d_err = static_cast<unsigned long long*>(mem.p);
    unsigned long long err = 0;
    ST_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(err), stream));
    const uint32_t want = (n + kBlock - 1) / kBlock;
    const dim3 grid(want < kPatCheckGrid ? want : kPatCheckGrid);
    if (dtype)
      hipLaunchKernelGGL(dev::k_csr_pattern_check_scales<double>, grid, dim3(kBlock), 0,
                         stream, static_cast<const double*>(d_row_scale),
                         static_cast<const double*>(d_col_scale), n, d_err);
    else
      hipLaunchKernelGGL(dev::k_csr_pattern_check_scales<float>, grid, dim3(kBlock), 0,
                         stream, static_cast<const float*>(d_row_scale),
                         static_cast<const float*>(d_col_scale), n, d_err);
    if (check_launch("csr_pattern_check_scales"))
      return -1;
    ST_CHECK(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
    ST_CHECK(hipStreamSynchronize(stream));
    if (err != ~0ull) {
      const int which = (int)(err >> 32);
      const uint32_t i = (uint32_t)err;
      double x = 0;
      if (read_elem(dtype, which ? d_col_scale : d_row_scale, i, &x))
        return -1;
      char msg[384];
      csr::describe_scale_entry(which, i, x, msg, sizeof(msg));
      set_error("%s", msg);
      return -1;
    }
  }
  CsrPatternHandle* h = nullptr;
  if (make_pattern(dtype, n, nnz, d_row_ptr, d_col_idx, d_row_scale, d_col_scale,
                   d_order, cf, empty_rows, first_empty, &h))
    return -1;
  order.p = nullptr; // the handle's now
  *out = h;
  return 0;
}

int
csr_pattern_destroy(CsrPatternHandle* h)
{
  if (!h)
    return 0;
  ST_REQUIRE(h->magic == kCsrPatternMagic,
             "st_csr_pattern_destroy: not a CSR pattern handle");
  h->magic = 0;
  if (h->d_order)
    (void)hipFree(h->d_order);
  delete h;
  return 0;
}

int
csr_pattern_transpose(const CsrPatternHandle* p, int64_t* d_t_row_ptr,
                      int32_t* d_t_col_idx, hipStream_t stream, CsrPatternHandle** out,
                      uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_pattern_transpose: null output pointer");
  *out = nullptr;
  Freed order;
  uint32_t* d_order = nullptr;
  uint32_t cf[csr::kClasses + 1];
  uint32_t empty_rows = 0, first_empty = p->n;
  if (csr_transpose_arrays(p->dtype, p->n, p->nnz, p->row_ptr, p->col_idx, nullptr,
                           d_t_row_ptr, d_t_col_idx, nullptr, stream, flags, &d_order,
                           cf, &empty_rows, &first_empty))
    return -1;
  order.p = d_order;
  CsrPatternHandle* h = nullptr; // (D_r P D_c)^T = D_c P^T D_r
  if (make_pattern(p->dtype, p->n, p->nnz, d_t_row_ptr, d_t_col_idx, p->col_scale,
                   p->row_scale, d_order, cf, empty_rows, first_empty, &h))
    return -1;
  order.p = nullptr;
  *out = h;
  return 0;
}

int
csr_pattern_terms_create(const CsrPatternHandle* h, uint32_t K, const void* const* d_u,
                         const void* const* d_w, hipStream_t stream,
                         CsrTermsHandle** out)
{
  ST_REQUIRE(out, "st_csr_pattern_terms_create: null output pointer");
  *out = nullptr;
  char msg[384];
  if (csr::check_terms_count(K, msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  ST_REQUIRE(d_u && d_w, "csr terms: null vector table");
  const size_t elem = h->dtype ? 8 : 4;
  CsrTermsHandle tmp{};
  tmp.magic = kCsrTermsMagic;
  tmp.dtype = h->dtype;
  tmp.device = h->device;
  tmp.n = h->n;
  tmp.K = K;
  tmp.csr = nullptr;
  tmp.pattern = h;
  dev::CsrTermVecs<double> vd{};
  dev::CsrTermVecs<float> vf{};
  vd.K = vf.K = K;
  for (uint32_t j = 0; j < K; j++) {
    ST_REQUIRE(d_u[j], "csr terms: null u_%u", j);
    ST_REQUIRE(d_w[j], "csr terms: null w_%u", j);
    ST_REQUIRE(((uintptr_t)d_u[j] & (elem - 1)) == 0 &&
                 ((uintptr_t)d_w[j] & (elem - 1)) == 0,
               "csr terms: a vector of term %u is not aligned to its element size", j);
    tmp.u[j] = d_u[j];
    tmp.w[j] = d_w[j];
    vd.u[j] = static_cast<const double*>(d_u[j]);
    vd.w[j] = static_cast<const double*>(d_w[j]);
    vf.u[j] = static_cast<const float*>(d_u[j]);
    vf.w[j] = static_cast<const float*>(d_w[j]);
  }
  Freed mem; // err (2 words) | dots + partial | s0 [n]
  const size_t dp = csr_terms_dots_bytes(K);
  ST_CHECK(hipMalloc(&mem.p, 256 + dp + elem * (size_t)h->n));
  unsigned long long* d_err = static_cast<unsigned long long*>(mem.p);
  void* dots_part = static_cast<char*>(mem.p) + 256;
  void* s0 = static_cast<char*>(mem.p) + 256 + dp;
  unsigned long long err[2];
  const uint32_t want = (h->n + kBlock - 1) / kBlock;
  const dim3 cgrid(want < kPatCheckGrid ? want : kPatCheckGrid);

  // 1. the vectors, one pass
  ST_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(err), stream));
  if (h->dtype)
    hipLaunchKernelGGL(dev::k_csr_terms_check<double>, cgrid, dim3(kBlock), 0, stream,
                       vd, h->n, d_err);
  else
    hipLaunchKernelGGL(dev::k_csr_terms_check<float>, cgrid, dim3(kBlock), 0, stream, vf,
                       h->n, d_err);
  if (check_launch("csr_terms_check"))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[0] != ~0ull) {
    const uint32_t code = (uint32_t)(err[0] >> 32), i = (uint32_t)err[0];
    const uint32_t j = code >> 1;
    const int which = (int)(code & 1u);
    double x = 0;
    if (read_elem(h->dtype, which ? tmp.w[j] : tmp.u[j], i, &x))
      return -1;
    csr::describe_term_entry(j, which, i, x, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  // 2. s_0 of the operator (launch 0): a row with a positive entry stays
  // positive for every positive x, so no round divides by zero
  if (h->dtype ? pattern_rowsum<double>(h, &tmp, static_cast<double*>(s0), dots_part, stream)
               : pattern_rowsum<float>(h, &tmp, static_cast<float*>(s0), dots_part, stream))
    return -1;
  if (h->dtype)
    hipLaunchKernelGGL(dev::k_csr_terms_check_s0<double>, cgrid, dim3(kBlock), 0, stream,
                       static_cast<const double*>(s0), h->n, d_err);
  else
    hipLaunchKernelGGL(dev::k_csr_terms_check_s0<float>, cgrid, dim3(kBlock), 0, stream,
                       static_cast<const float*>(s0), h->n, d_err);
  if (check_launch("csr_terms_check_s0"))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[1] != ~0ull) {
    const uint32_t r = (uint32_t)err[1];
    double x = 0;
    if (read_elem(h->dtype, s0, r, &x))
      return -1;
    csr::describe_term_row(r, x, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  CsrTermsHandle* t = new (std::nothrow) CsrTermsHandle(tmp);
  ST_REQUIRE(t, "st_csr_pattern_terms_create: out of memory");
  *out = t;
  return 0;
}

int
launch_csr_pattern_rowsum(const CsrPatternHandle* h, const CsrTermsHandle* t, void* s,
                          void* dots_part, hipStream_t stream)
{
  ST_REQUIRE(s && (!t || dots_part), "csr_pattern_rowsum: null pointer");
  ST_REQUIRE(((uintptr_t)dots_part & 255u) == 0,
             "csr_pattern_rowsum: the scratch must be aligned to 256 bytes");
  if (h->dtype)
    return pattern_rowsum<double>(h, t, static_cast<double*>(s), dots_part, stream);
  return pattern_rowsum<float>(h, t, static_cast<float*>(s), dots_part, stream);
}

int
launch_csr_pattern_round(const CsrPatternHandle* h, const CsrTermsHandle* t,
                         const void* s_prev, void* s_next, const void* v_prev,
                         void* v_cur, void* z, void* dots_part, double eps, uint32_t k,
                         uint32_t max_itr, uint32_t semantics, st_state* st,
                         hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && z && st && (!t || dots_part),
             "csr_pattern_round: null pointer");
  ST_REQUIRE(((uintptr_t)dots_part & 255u) == 0,
             "csr_pattern_round: the scratch must be aligned to 256 bytes");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_pattern_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "csr_pattern_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_pattern_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_pattern_round: s_prev and s_next must differ");
  ST_REQUIRE(z != s_prev && z != s_next && z != v_prev && z != v_cur,
             "csr_pattern_round: z must be scratch of its own");
  if (h->dtype)
    return pattern_round<double>(h, t, static_cast<const double*>(s_prev),
                                 static_cast<double*>(s_next),
                                 static_cast<const double*>(v_prev),
                                 static_cast<double*>(v_cur), static_cast<double*>(z),
                                 dots_part, eps, k, max_itr, semantics, st, stream);
  return pattern_round<float>(h, t, static_cast<const float*>(s_prev),
                              static_cast<float*>(s_next),
                              static_cast<const float*>(v_prev),
                              static_cast<float*>(v_cur), static_cast<float*>(z), dots_part,
                              (float)eps, k, max_itr, semantics, st, stream);
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_csr_pattern_destroy(void* pat)
{
  st::clear_error();
  return st::csr_pattern_destroy(static_cast<st::CsrPatternHandle*>(pat));
}

int
st_csr_pattern_get_plan(void* pat, uint32_t* order_out, uint32_t* class_first)
{
  st::clear_error();
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_csr_pattern_get_plan");
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
st_csr_pattern_empty_rows(void* pat, uint32_t* count, uint32_t* lowest)
{
  st::clear_error();
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_csr_pattern_empty_rows");
  if (!h)
    return -1;
  if (count)
    *count = h->empty_rows;
  if (lowest)
    *lowest = h->first_empty;
  return 0;
}

uint64_t
st_csr_pattern_scratch_bytes(uint32_t n, uint32_t K)
{
  if (n == 0 || n >= 0x80000000u || K > st::csr::kTermsMax)
    return 0;
  return st::csr_terms_scratch_bytes(n, K);
}

// the registers and waves are what the gfx950 compile of this file reports
// (hipcc --resource-usage; DESIGN.md, "Pattern-only CSR", has the table next
// to the values kernels')
const char*
st_csr_pattern_shape_desc(void)
{
  static_assert(st::csr::kRows[0] == 8 && st::csr::kRows[1] == 4 &&
                  st::csr::kRows[2] == 2 && st::csr::kRows[3] == 1 &&
                  st::dev::kPatUnroll[0] == 1 && st::dev::kPatUnroll[1] == 2 &&
                  st::dev::kPatUnroll[2] == 4 && st::dev::kPatUnroll[3] == 8 &&
                  st::kPatPrepGrid == 2048 && st::kPatCheckGrid == 8192,
                "the description below");
  return "lanes=4,16,64,256 rows=8,4,2,1 unroll=1,2,4,8 matrix_bytes_per_entry=4 "
         "launches_per_round=2 launches_per_round_terms=3 prep_grid=2048 "
         "check_grid=8192 " ST_CSR_PATTERN_REGS;
}

int
st_csr_pattern_rowsum(void* pat, void* terms, void* d_s, void* d_scratch, void* stream)
{
  st::clear_error();
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_csr_pattern_rowsum");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = nullptr;
  if (terms && !(t = st::as_csr_pattern_terms(terms, h, "st_csr_pattern_rowsum")))
    return -1;
  return st::launch_csr_pattern_rowsum(h, t, d_s, d_scratch, ST_STREAM(stream));
}

int
st_csr_pattern_round(void* pat, void* terms, const void* d_s_prev, void* d_s_next,
                     const void* d_v_prev, void* d_v_cur, void* d_scratch, double eps,
                     unsigned int k, unsigned int max_itr, unsigned int semantics,
                     st_state* d_state, void* stream)
{
  st::clear_error();
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_csr_pattern_round");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = nullptr;
  if (terms && !(t = st::as_csr_pattern_terms(terms, h, "st_csr_pattern_round")))
    return -1;
  if (!t && st::csr_pattern_refuse_empty(h, "st_csr_pattern_round"))
    return -1;
  ST_REQUIRE(d_scratch, "csr_pattern_round: null pointer");
  void* z = static_cast<char*>(d_scratch) + st::csr_terms_dots_bytes(t ? t->K : 0);
  return st::launch_csr_pattern_round(h, t, d_s_prev, d_s_next, d_v_prev, d_v_cur, z,
                                      d_scratch, eps, k, max_itr, semantics, d_state,
                                      ST_STREAM(stream));
}

} // extern "C"
