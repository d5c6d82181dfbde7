// st_csr_terms.hip — launchers of the kernels in st_csr_terms.h (the CSR
// round on A + sum_j u_j w_j^T), the terms object (validation on the device)
// and the part of its C-ABI that needs no queue (similarity_transform.h
// section 3e: st_csr_terms_destroy, st_csr_terms_scratch_bytes,
// st_csr_terms_shape_desc, st_csr_terms_rowsum, st_csr_terms_round).
// st_csr_terms_create, st_solve_csr_terms and max_eigen_value_csr_terms_ex
// live with the queue in st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <new>

#include "st_csr_terms.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kCheckGrid = 8192; // workgroup cap of the validation passes

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

// the vector pass's workgroups: a function of n alone
uint32_t
dot_grid(uint32_t n)
{
  const uint32_t want = (n + kBlock - 1) / kBlock;
  return want < dev::kCsrDotGrid ? want : dev::kCsrDotGrid;
}

constexpr size_t kDotsBytes = 256; // dots [K] of either dtype, then partial

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

template <typename T, int KM>
void
launch_terms_rowsum(const CsrHandle* h, const CsrTermsHandle* t, T* s,
                    void* dots_part, hipStream_t stream)
{
  hipLaunchKernelGGL((dev::k_csr_terms_rowsum<T, KM>),
                     dim3(h->blk_first[csr::kClasses]), dim3(kBlock), 0, stream,
                     h->row_ptr, h->col_idx, static_cast<const T*>(h->vals),
                     h->d_order, tab_of(h), s, terms_of<T, KM>(t, dots_part));
}

template <typename T, int KM>
void
launch_terms_spmv(const CsrHandle* h, const CsrTermsHandle* t, const T* x,
                  const T* s_prev, const T* v_prev, T* s_next, T* v_cur,
                  void* dots_part, uint32_t k, const st_state* st,
                  hipStream_t stream)
{
  hipLaunchKernelGGL((dev::k_csr_terms_spmv<T, KM>),
                     dim3(h->blk_first[csr::kClasses]), dim3(kBlock), 0, stream,
                     h->row_ptr, h->col_idx, static_cast<const T*>(h->vals),
                     h->d_order, tab_of(h), x, s_prev, v_prev, s_next, v_cur, k, st,
                     terms_of<T, KM>(t, dots_part));
}

template <typename T>
int
terms_rowsum(const CsrHandle* h, const CsrTermsHandle* t, T* s, void* dots_part,
             hipStream_t stream)
{
  const uint32_t pgrid = dot_grid(h->n);
  const dev::CsrDots<T> d = dots_of<T>(t, dots_part);
  hipLaunchKernelGGL(dev::k_csr_wsum<T>, dim3(pgrid), dim3(kBlock), 0, stream,
                     h->n, d);
  if (check_launch("csr_wsum"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_dots<T>, dim3(1), dim3(kBlock), 0, stream,
                     (const T*)d.partial, pgrid, t->K, static_cast<T*>(dots_part),
                     0u, (const st_state*)nullptr);
  if (check_launch("csr_dots"))
    return -1;
  if (t->K == 1) // the instantiation with registers for K terms (1, 2 or 4)
    launch_terms_rowsum<T, 1>(h, t, s, dots_part, stream);
  else if (t->K == 2)
    launch_terms_rowsum<T, 2>(h, t, s, dots_part, stream);
  else
    launch_terms_rowsum<T, 4>(h, t, s, dots_part, stream);
  return check_launch("csr_terms_rowsum");
}

template <typename T>
int
terms_round(const CsrHandle* h, const CsrTermsHandle* t, const T* s_prev,
            T* s_next, const T* v_prev, T* v_cur, T* x, void* dots_part, T eps,
            uint32_t k, uint32_t max_itr, uint32_t semantics, st_state* st,
            hipStream_t stream)
{
  const uint32_t pgrid = dot_grid(h->n);
  const dev::CsrDots<T> d = dots_of<T>(t, dots_part);
  hipLaunchKernelGGL((dev::k_csr_prep<T, dev::CsrDots<T>>), dim3(pgrid),
                     dim3(kBlock), 0, stream, s_prev, v_prev, x, h->n, eps, k,
                     max_itr, semantics, st, d);
  if (check_launch("csr_prep (terms)"))
    return -1;
  hipLaunchKernelGGL(dev::k_csr_dots<T>, dim3(1), dim3(kBlock), 0, stream,
                     (const T*)d.partial, pgrid, t->K, static_cast<T*>(dots_part),
                     k, (const st_state*)st);
  if (check_launch("csr_dots"))
    return -1;
  if (t->K == 1)
    launch_terms_spmv<T, 1>(h, t, x, s_prev, v_prev, s_next, v_cur, dots_part, k, st,
                            stream);
  else if (t->K == 2)
    launch_terms_spmv<T, 2>(h, t, x, s_prev, v_prev, s_next, v_cur, dots_part, k, st,
                            stream);
  else
    launch_terms_spmv<T, 4>(h, t, x, s_prev, v_prev, s_next, v_cur, dots_part, k, st,
                            stream);
  return check_launch("csr_terms_spmv");
}

template <typename T>
int
terms_check(const CsrTermsHandle* t, unsigned long long* d_err, hipStream_t stream)
{
  dev::CsrTermVecs<T> v;
  v.K = t->K;
  for (uint32_t j = 0; j < csr::kTermsMax; j++) {
    v.u[j] = j < t->K ? static_cast<const T*>(t->u[j]) : nullptr;
    v.w[j] = j < t->K ? static_cast<const T*>(t->w[j]) : nullptr;
  }
  const uint32_t want = (t->n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(dev::k_csr_terms_check<T>,
                     dim3(want < kCheckGrid ? want : kCheckGrid), dim3(kBlock), 0,
                     stream, v, t->n, d_err);
  return check_launch("csr_terms_check");
}

template <typename T>
int
terms_check_s0(const T* s0, uint32_t n, unsigned long long* d_err,
               hipStream_t stream)
{
  const uint32_t want = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(dev::k_csr_terms_check_s0<T>,
                     dim3(want < kCheckGrid ? want : kCheckGrid), dim3(kBlock), 0,
                     stream, s0, n, d_err);
  return check_launch("csr_terms_check_s0");
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

} // namespace

size_t
csr_terms_dots_bytes(uint32_t K)
{
  return kDotsBytes + (size_t)K * dev::kCsrDotGrid * 8; // a multiple of 256
}

size_t
csr_terms_scratch_bytes(uint32_t n, uint32_t K)
{
  return csr_terms_dots_bytes(K) + (((size_t)n * 8 + 255) & ~(size_t)255);
}

const CsrTermsHandle*
as_csr_terms(const void* p, const CsrHandle* h, const char* what)
{
  const CsrTermsHandle* t = static_cast<const CsrTermsHandle*>(p);
  if (!t || t->magic != kCsrTermsMagic) {
    set_error("%s: not a terms object (st_csr_terms_create), or a destroyed one",
              what);
    return nullptr;
  }
  if (t->csr != h || t->n != h->n || t->dtype != h->dtype || t->device != h->device) {
    set_error("%s: the terms object belongs to another matrix handle (its own: n "
              "= %u, dtype %d, device %d; this one: n = %u, dtype %d, device %d)",
              what, t->n, t->dtype, t->device, h->n, h->dtype, h->device);
    return nullptr;
  }
  return t;
}

int
csr_terms_create(const CsrHandle* h, uint32_t K, const void* const* d_u,
                 const void* const* d_w, hipStream_t stream, CsrTermsHandle** out)
{
  ST_REQUIRE(out, "st_csr_terms_create: null output pointer");
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
  tmp.csr = h;
  for (uint32_t j = 0; j < K; j++) {
    ST_REQUIRE(d_u[j], "csr terms: null u_%u", j);
    ST_REQUIRE(d_w[j], "csr terms: null w_%u", j);
    ST_REQUIRE(((uintptr_t)d_u[j] & (elem - 1)) == 0 &&
                 ((uintptr_t)d_w[j] & (elem - 1)) == 0,
               "csr terms: a vector of term %u is not aligned to its element size", j);
    tmp.u[j] = d_u[j];
    tmp.w[j] = d_w[j];
  }
  Freed mem; // err (2 words) | dots + partial | s0 [n]
  const size_t dp = csr_terms_dots_bytes(K);
  ST_CHECK(hipMalloc(&mem.p, 256 + dp + elem * (size_t)h->n));
  unsigned long long* d_err = static_cast<unsigned long long*>(mem.p);
  void* dots_part = static_cast<char*>(mem.p) + 256;
  void* s0 = static_cast<char*>(mem.p) + 256 + dp;
  unsigned long long err[2];

  // 1. the vectors, one pass
  ST_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(err), stream));
  if (h->dtype ? terms_check<double>(&tmp, d_err, stream)
               : terms_check<float>(&tmp, d_err, stream))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[0] != ~0ull) {
    const uint32_t code = (uint32_t)(err[0] >> 32), i = (uint32_t)err[0];
    const uint32_t j = code >> 1;
    const int which = (int)(code & 1u);
    double x = 0;
    const char* at = static_cast<const char*>(which ? tmp.w[j] : tmp.u[j]) + elem * i;
    if (h->dtype) {
      ST_CHECK(hipMemcpy(&x, at, 8, hipMemcpyDeviceToHost));
    } else {
      float f = 0;
      ST_CHECK(hipMemcpy(&f, at, 4, hipMemcpyDeviceToHost));
      x = (double)f;
    }
    csr::describe_term_entry(j, which, i, x, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  // 2. s_0 of the operator: a row of M with a positive entry stays positive
  // for every positive x, so no round divides by zero
  if (h->dtype ? terms_rowsum<double>(h, &tmp, static_cast<double*>(s0), dots_part, stream)
               : terms_rowsum<float>(h, &tmp, static_cast<float*>(s0), dots_part, stream))
    return -1;
  if (h->dtype ? terms_check_s0<double>(static_cast<const double*>(s0), h->n, d_err, stream)
               : terms_check_s0<float>(static_cast<const float*>(s0), h->n, d_err, stream))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[1] != ~0ull) {
    const uint32_t r = (uint32_t)err[1];
    double x = 0;
    const char* at = static_cast<const char*>(s0) + elem * r;
    if (h->dtype) {
      ST_CHECK(hipMemcpy(&x, at, 8, hipMemcpyDeviceToHost));
    } else {
      float f = 0;
      ST_CHECK(hipMemcpy(&f, at, 4, hipMemcpyDeviceToHost));
      x = (double)f;
    }
    csr::describe_term_row(r, x, msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  CsrTermsHandle* t = new (std::nothrow) CsrTermsHandle(tmp);
  ST_REQUIRE(t, "st_csr_terms_create: out of memory");
  *out = t;
  return 0;
}

int
csr_terms_destroy(CsrTermsHandle* t)
{
  if (!t)
    return 0;
  ST_REQUIRE(t->magic == kCsrTermsMagic, "st_csr_terms_destroy: not a terms object");
  t->magic = 0;
  delete t;
  return 0;
}

int
launch_csr_terms_rowsum(const CsrHandle* h, const CsrTermsHandle* t, void* s,
                        void* dots_part, hipStream_t stream)
{
  ST_REQUIRE(s && dots_part, "csr_terms_rowsum: null pointer");
  ST_REQUIRE(((uintptr_t)dots_part & 255u) == 0,
             "csr_terms_rowsum: the scratch must be aligned to 256 bytes");
  if (h->dtype)
    return terms_rowsum<double>(h, t, static_cast<double*>(s), dots_part, stream);
  return terms_rowsum<float>(h, t, static_cast<float*>(s), dots_part, stream);
}

int
launch_csr_terms_round(const CsrHandle* h, const CsrTermsHandle* t,
                       const void* s_prev, void* s_next, const void* v_prev,
                       void* v_cur, void* x, void* dots_part, double eps,
                       uint32_t k, uint32_t max_itr, uint32_t semantics,
                       st_state* st, hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && x && dots_part && st,
             "csr_terms_round: null pointer");
  ST_REQUIRE(((uintptr_t)dots_part & 255u) == 0,
             "csr_terms_round: the scratch must be aligned to 256 bytes");
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_terms_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "csr_terms_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_terms_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_terms_round: s_prev and s_next must differ");
  ST_REQUIRE(x != s_prev && x != s_next && x != v_prev && x != v_cur,
             "csr_terms_round: x must be scratch of its own");
  if (h->dtype)
    return terms_round<double>(h, t, static_cast<const double*>(s_prev),
                               static_cast<double*>(s_next),
                               static_cast<const double*>(v_prev),
                               static_cast<double*>(v_cur), static_cast<double*>(x),
                               dots_part, eps, k, max_itr, semantics, st, stream);
  return terms_round<float>(h, t, static_cast<const float*>(s_prev),
                            static_cast<float*>(s_next),
                            static_cast<const float*>(v_prev),
                            static_cast<float*>(v_cur), static_cast<float*>(x),
                            dots_part, (float)eps, k, max_itr, semantics, st, stream);
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_csr_terms_destroy(void* terms)
{
  st::clear_error();
  return st::csr_terms_destroy(static_cast<st::CsrTermsHandle*>(terms));
}

uint64_t
st_csr_terms_scratch_bytes(uint32_t n, uint32_t K)
{
  if (n == 0 || n >= 0x80000000u || K < 1 || K > st::csr::kTermsMax)
    return 0;
  return st::csr_terms_scratch_bytes(n, K);
}

const char*
st_csr_terms_shape_desc(void)
{
  static_assert(st::dev::kCsrDotGrid == 2048 && st::csr::kTermsMax == 4 &&
                  st::kCheckGrid == 8192,
                "the description below");
  return "terms_max=4 dot_grid=2048 lanes=256 combine=one_workgroup "
         "launches_per_round=3 dots_offset=0 partial_offset=256 check_grid=8192";
}

int
st_csr_terms_rowsum(void* csr, void* terms, void* d_s, void* d_scratch, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_terms_rowsum");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = st::as_csr_terms(terms, h, "st_csr_terms_rowsum");
  if (!t)
    return -1;
  return st::launch_csr_terms_rowsum(h, t, d_s, d_scratch, ST_STREAM(stream));
}

int
st_csr_terms_round(void* csr, void* terms, const void* d_s_prev, void* d_s_next,
                   const void* d_v_prev, void* d_v_cur, void* d_scratch, double eps,
                   unsigned int k, unsigned int max_itr, unsigned int semantics,
                   st_state* d_state, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_terms_round");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = st::as_csr_terms(terms, h, "st_csr_terms_round");
  if (!t)
    return -1;
  ST_REQUIRE(d_scratch, "csr_terms_round: null pointer");
  void* x = static_cast<char*>(d_scratch) + st::csr_terms_dots_bytes(t->K);
  return st::launch_csr_terms_round(h, t, d_s_prev, d_s_next, d_v_prev, d_v_cur, x,
                                    d_scratch, eps, k, max_itr, semantics, d_state,
                                    ST_STREAM(stream));
}

} // extern "C"
