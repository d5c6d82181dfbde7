// st_csr_multi.hip — launchers of the kernels in st_csr_multi.h (the CSR round
// for up to 8 operators A + sum_j u_{c,j} w_{c,j}^T on one matrix), the multi
// terms object (validation and packing on the device) and the part of its
// C-ABI that needs no queue (similarity_transform.h section 3f:
// st_csr_multi_destroy, st_csr_multi_scratch_bytes, st_csr_multi_shape_desc,
// st_csr_multi_rowsum, st_csr_multi_round).  st_csr_multi_create,
// st_solve_csr_multi and max_eigen_value_csr_multi_ex live with the queue in
// st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <new>

#include "st_internal.h"
#include "st_csr_multi.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kCheckGrid = 8192; // workgroup cap of the create-time passes
constexpr size_t kDotsBytes = 256;    // dots [C][K] of either dtype, then partial

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

// the row pass's table: the handle's class starts in the plan, the object's
// own workgroup ranges (csr::multi_rows)
dev::CsrTab
tab_of(const CsrHandle* h, const CsrMultiHandle* t)
{
  dev::CsrTab tab;
  for (int c = 0; c <= csr::kClasses; c++) {
    tab.row_first[c] = h->row_first[c];
    tab.blk_first[c] = t->blk_first[c];
  }
  return tab;
}

// the vector pass's workgroups: st_csr_terms.hip's function of n alone
uint32_t
dot_grid(uint32_t n)
{
  const uint32_t want = (n + kBlock - 1) / kBlock;
  return want < dev::kCsrDotGrid ? want : dev::kCsrDotGrid;
}

uint32_t
pass_grid(uint32_t n)
{
  const uint32_t want = (n + kBlock - 1) / kBlock;
  return want < kCheckGrid ? want : kCheckGrid;
}

template <typename T>
T*
partial_of(void* scratch)
{
  return reinterpret_cast<T*>(static_cast<char*>(scratch) + kDotsBytes);
}

template <typename T, int CP>
int
multi_rowsum(const CsrHandle* h, const CsrMultiHandle* t, void* s, void* scratch,
             hipStream_t stream)
{
  const uint32_t pgrid = dot_grid(h->n);
  T* const partial = partial_of<T>(scratch);
  hipLaunchKernelGGL((dev::k_csrm_wsum<T, CP>), dim3(pgrid), dim3(kBlock), 0, stream,
                     h->n, t->C, t->K, static_cast<const T*>(t->w), partial);
  if (check_launch("csrm_wsum"))
    return -1;
  hipLaunchKernelGGL(dev::k_csrm_dots<T>, dim3(t->C), dim3(kBlock), 0, stream,
                     (const T*)partial, pgrid, t->K, static_cast<T*>(scratch), 0u,
                     (const st_state*)nullptr);
  if (check_launch("csrm_dots"))
    return -1;
  hipLaunchKernelGGL((dev::k_csrm_rowsum<T, CP>), dim3(t->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                     static_cast<const T*>(h->vals), h->d_order, tab_of(h, t),
                     static_cast<T*>(s), static_cast<const T*>(t->u),
                     static_cast<const T*>(scratch), h->n, t->C, t->K);
  return check_launch("csrm_rowsum");
}

template <typename T, int CP>
int
multi_round(const CsrHandle* h, const CsrMultiHandle* t, const void* s_prev,
            void* s_next, const void* v_prev, void* v_cur, void* scratch,
            double eps, uint32_t k, uint32_t max_itr, uint32_t semantics,
            st_state* states, uint32_t* finished, hipStream_t stream)
{
  const uint32_t pgrid = dot_grid(h->n);
  T* const partial = partial_of<T>(scratch);
  T* const x = reinterpret_cast<T*>(static_cast<char*>(scratch) +
                                    csr_multi_dots_bytes(t->C, t->K));
  hipLaunchKernelGGL((dev::k_csrm_prep<T, CP>), dim3(pgrid), dim3(kBlock), 0, stream,
                     static_cast<const T*>(s_prev), static_cast<const T*>(v_prev), x,
                     static_cast<const T*>(t->w), partial, h->n, t->C, t->K, (T)eps,
                     k, max_itr, semantics, states, finished);
  if (check_launch("csrm_prep"))
    return -1;
  hipLaunchKernelGGL(dev::k_csrm_dots<T>, dim3(t->C), dim3(kBlock), 0, stream,
                     (const T*)partial, pgrid, t->K, static_cast<T*>(scratch), k,
                     (const st_state*)states);
  if (check_launch("csrm_dots"))
    return -1;
  hipLaunchKernelGGL((dev::k_csrm_spmv<T, CP>), dim3(t->blk_first[csr::kClasses]),
                     dim3(kBlock), 0, stream, h->row_ptr, h->col_idx,
                     static_cast<const T*>(h->vals), h->d_order, tab_of(h, t),
                     (const T*)x, static_cast<const T*>(s_prev),
                     static_cast<const T*>(v_prev), static_cast<T*>(s_next),
                     static_cast<T*>(v_cur), static_cast<const T*>(t->u),
                     static_cast<const T*>(scratch), h->n, t->C, t->K, k,
                     (const st_state*)states);
  return check_launch("csrm_spmv");
}

template <typename T, int CP>
int
multi_collect(const CsrMultiHandle* t, const void* v0, const void* v1, void* out,
              const st_state* states, CsrBatchResult* res, hipStream_t stream)
{
  hipLaunchKernelGGL((dev::k_csrm_collect<T, CP>), dim3(pass_grid(t->n)),
                     dim3(kBlock), 0, stream, static_cast<const T*>(v0),
                     static_cast<const T*>(v1), static_cast<T*>(out), states, t->n,
                     t->C, res);
  return check_launch("csrm_collect");
}

// term j of every column -> dst [n][CP] (table: d_u or d_w, [c * K + j])
template <typename T, int CP>
int
multi_pack(const CsrMultiHandle* t, const void* const* table, uint32_t j, void* dst,
           hipStream_t stream)
{
  dev::CsrmSrc<T, CP> src;
  for (uint32_t c = 0; c < (uint32_t)CP; c++)
    src.p[c] = c < t->C ? static_cast<const T*>(table[(size_t)c * t->K + j]) : nullptr;
  hipLaunchKernelGGL((dev::k_csrm_pack<T, CP>), dim3(pass_grid(t->n)), dim3(kBlock), 0,
                     stream, src,
                     static_cast<T*>(dst) + (uint64_t)j * t->n * (uint64_t)CP, t->n);
  return check_launch("csrm_pack");
}

template <typename T, int CP>
int
multi_check_s0(const CsrMultiHandle* t, const void* s0, unsigned long long* d_err,
               hipStream_t stream)
{
  hipLaunchKernelGGL((dev::k_csrm_check_s0<T, CP>), dim3(pass_grid(t->n)),
                     dim3(kBlock), 0, stream, static_cast<const T*>(s0), t->n, t->C,
                     d_err);
  return check_launch("csrm_check_s0");
}

// column c's vectors by the single object's pass: d_err[0] = the lowest
// ((2 j + which) << 32 | i)
template <typename T>
int
multi_check_column(uint32_t n, uint32_t K, const void* const* d_u,
                   const void* const* d_w, unsigned long long* d_err,
                   hipStream_t stream)
{
  dev::CsrTermVecs<T> v;
  v.K = K;
  for (uint32_t j = 0; j < csr::kTermsMax; j++) {
    v.u[j] = j < K ? static_cast<const T*>(d_u[j]) : nullptr;
    v.w[j] = j < K ? static_cast<const T*>(d_w[j]) : nullptr;
  }
  hipLaunchKernelGGL(dev::k_csr_terms_check<T>, dim3(pass_grid(n)), dim3(kBlock), 0,
                     stream, v, n, d_err);
  return check_launch("csr_terms_check");
}

// F<T, CP>(args) for the object's dtype and packed width
#define ST_CSRM_CALL(F, t, ...)                                                    \
  ((t)->dtype ? ((t)->CP == 2   ? F<double, 2>(__VA_ARGS__)                        \
                 : (t)->CP == 4 ? F<double, 4>(__VA_ARGS__)                        \
                                : F<double, 8>(__VA_ARGS__))                       \
              : ((t)->CP == 2   ? F<float, 2>(__VA_ARGS__)                         \
                 : (t)->CP == 4 ? F<float, 4>(__VA_ARGS__)                         \
                                : F<float, 8>(__VA_ARGS__)))

struct Freed
{
  void* p = nullptr;
  ~Freed()
  {
    if (p)
      (void)hipFree(p);
  }
};

size_t
up256(size_t b)
{
  return (b + 255) & ~(size_t)255;
}

int
read_elem(int dtype, const void* at, double* x)
{
  if (dtype) {
    ST_CHECK(hipMemcpy(x, at, 8, hipMemcpyDeviceToHost));
  } else {
    float f = 0;
    ST_CHECK(hipMemcpy(&f, at, 4, hipMemcpyDeviceToHost));
    *x = (double)f;
  }
  return 0;
}

} // namespace

size_t
csr_multi_dots_bytes(uint32_t C, uint32_t K)
{
  // a multiple of 256: dots, then partial [CP][K][2048] of either dtype
  return kDotsBytes + (size_t)csr::multi_cp(C) * K * dev::kCsrDotGrid * 8;
}

size_t
csr_multi_scratch_bytes(uint32_t n, uint32_t C, uint32_t K)
{
  return csr_multi_dots_bytes(C, K) + up256((size_t)n * csr::multi_cp(C) * 8);
}

const CsrMultiHandle*
as_csr_multi(const void* p, const CsrHandle* h, const char* what)
{
  const CsrMultiHandle* t = static_cast<const CsrMultiHandle*>(p);
  if (!t || t->magic != kCsrMultiMagic) {
    set_error("%s: not a multi terms object (st_csr_multi_create), or a destroyed "
              "one", what);
    return nullptr;
  }
  if (t->csr != h || t->n != h->n || t->dtype != h->dtype || t->device != h->device) {
    set_error("%s: the multi terms object belongs to another matrix handle (its "
              "own: n = %u, dtype %d, device %d; this one: n = %u, dtype %d, device "
              "%d)", what, t->n, t->dtype, t->device, h->n, h->dtype, h->device);
    return nullptr;
  }
  return t;
}

int
csr_multi_create(const CsrHandle* h, uint32_t C, uint32_t K, const void* const* d_u,
                 const void* const* d_w, hipStream_t stream, CsrMultiHandle** out,
                 const void* h_pu, const void* h_pw)
{
  ST_REQUIRE(out, "st_csr_multi_create: null output pointer");
  *out = nullptr;
  char msg[448];
  if (csr::check_multi_count(C, K, msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  const bool packed = h_pu && h_pw;
  ST_REQUIRE(packed || (d_u && d_w), "csr multi: null vector table");
  const size_t elem = h->dtype ? 8 : 4;
  CsrMultiHandle tmp{};
  tmp.magic = kCsrMultiMagic;
  tmp.dtype = h->dtype;
  tmp.device = h->device;
  tmp.n = h->n;
  tmp.C = C;
  tmp.K = K;
  tmp.CP = csr::multi_cp(C);
  tmp.csr = h;
  if (!packed)
    for (uint32_t c = 0; c < C; c++)
      for (uint32_t j = 0; j < K; j++) {
        const void* pu = d_u[(size_t)c * K + j];
        const void* pw = d_w[(size_t)c * K + j];
        ST_REQUIRE(pu, "csr multi: column %u: null u_%u", c, j);
        ST_REQUIRE(pw, "csr multi: column %u: null w_%u", c, j);
        ST_REQUIRE(((uintptr_t)pu & (elem - 1)) == 0 && ((uintptr_t)pw & (elem - 1)) == 0,
                   "csr multi: column %u: a vector of term %u is not aligned to its "
                   "element size", c, j);
      }
  tmp.blk_first[0] = 0;
  for (int c = 0; c < csr::kClasses; c++) {
    const uint32_t rows = h->row_first[c + 1] - h->row_first[c];
    const uint32_t per = csr::multi_rows(c, (uint32_t)(tmp.CP * elem)) *
                         (csr::kBlock / csr::kLanes[c]);
    tmp.blk_first[c + 1] = tmp.blk_first[c] + (rows + per - 1) / per;
  }
  // err [2 C] | u | w | s0 | s1 | v0 | v1 | scratch
  const size_t b_vec = up256(elem * (size_t)h->n * tmp.CP);
  const size_t b_scr = csr_multi_scratch_bytes(h->n, C, K);
  Freed mem;
  ST_CHECK(hipMalloc(&mem.p, 256 + (2 * (size_t)K + 4) * b_vec + b_scr));
  char* at = static_cast<char*>(mem.p);
  unsigned long long* d_err = reinterpret_cast<unsigned long long*>(at);
  at += 256;
  tmp.u = at;
  at += K * b_vec;
  tmp.w = at;
  at += K * b_vec;
  for (int i = 0; i < 2; i++) {
    tmp.s[i] = at;
    at += b_vec;
  }
  for (int i = 0; i < 2; i++) {
    tmp.v[i] = at;
    at += b_vec;
  }
  tmp.scratch = at;
  unsigned long long err[2 * csr::kMultiMax];

  // 1. every column's vectors, one pass each, then the packing
  ST_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(err), stream));
  if (packed) {
    const size_t bytes = elem * (size_t)h->n * tmp.CP * K;
    ST_CHECK(hipMemcpyAsync(tmp.u, h_pu, bytes, hipMemcpyHostToDevice, stream));
    ST_CHECK(hipMemcpyAsync(tmp.w, h_pw, bytes, hipMemcpyHostToDevice, stream));
  } else {
    for (uint32_t c = 0; c < C; c++)
      if (h->dtype ? multi_check_column<double>(h->n, K, d_u + (size_t)c * K,
                                                d_w + (size_t)c * K, d_err + 2 * c, stream)
                   : multi_check_column<float>(h->n, K, d_u + (size_t)c * K,
                                               d_w + (size_t)c * K, d_err + 2 * c, stream))
        return -1;
    for (uint32_t j = 0; j < K; j++)
      if (ST_CSRM_CALL(multi_pack, &tmp, &tmp, d_u, j, tmp.u, stream) ||
          ST_CSRM_CALL(multi_pack, &tmp, &tmp, d_w, j, tmp.w, stream))
        return -1;
  }
  // 2. s_0 of every operator: a row of M_c with a positive entry stays
  // positive for every positive x, so no round divides by zero
  if (ST_CSRM_CALL(multi_rowsum, &tmp, h, &tmp, tmp.s[0], tmp.scratch, stream) ||
      ST_CSRM_CALL(multi_check_s0, &tmp, &tmp, tmp.s[0], d_err, stream))
    return -1;
  // the padding slots of everything a round reads before it writes hold 1
  const uint64_t cnt = (uint64_t)h->n * tmp.CP;
  void* const xbuf = static_cast<char*>(tmp.scratch) + csr_multi_dots_bytes(C, K);
  for (void* p : { tmp.s[1], tmp.v[0], tmp.v[1], xbuf })
    if (h->dtype ? launch_fill<double>(static_cast<double*>(p), cnt, 1.0, stream)
                 : launch_fill<float>(static_cast<float*>(p), cnt, 1.0f, stream))
      return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  for (uint32_t c = 0; c < C; c++) { // the lowest offender, column first
    if (err[2 * c] != ~0ull) {
      const uint32_t code = (uint32_t)(err[2 * c] >> 32), i = (uint32_t)err[2 * c];
      const uint32_t j = code >> 1;
      const int which = (int)(code & 1u);
      double x = 0;
      const void* vec = (which ? d_w : d_u)[(size_t)c * K + j];
      if (read_elem(h->dtype, static_cast<const char*>(vec) + elem * i, &x))
        return -1;
      csr::describe_multi_entry(c, j, which, i, x, msg, sizeof(msg));
      set_error("%s", msg);
      return -1;
    }
    if (err[2 * c + 1] != ~0ull) {
      const uint32_t r = (uint32_t)err[2 * c + 1];
      double x = 0;
      if (read_elem(h->dtype,
                    static_cast<const char*>(tmp.s[0]) + elem * ((size_t)r * tmp.CP + c),
                    &x))
        return -1;
      csr::describe_multi_row(c, r, x, msg, sizeof(msg));
      set_error("%s", msg);
      return -1;
    }
  }
  CsrMultiHandle* t = new (std::nothrow) CsrMultiHandle(tmp);
  ST_REQUIRE(t, "st_csr_multi_create: out of memory");
  t->mem = mem.p;
  mem.p = nullptr;
  *out = t;
  return 0;
}

int
csr_multi_destroy(CsrMultiHandle* t)
{
  if (!t)
    return 0;
  ST_REQUIRE(t->magic == kCsrMultiMagic, "st_csr_multi_destroy: not a multi terms object");
  t->magic = 0;
  if (t->mem)
    (void)hipFree(t->mem);
  delete t;
  return 0;
}

int
launch_csr_multi_rowsum(const CsrHandle* h, const CsrMultiHandle* t, void* s,
                        void* scratch, hipStream_t stream)
{
  ST_REQUIRE(s && scratch, "csr_multi_rowsum: null pointer");
  ST_REQUIRE(((uintptr_t)scratch & 255u) == 0,
             "csr_multi_rowsum: the scratch must be aligned to 256 bytes");
  const size_t row = (h->dtype ? 8 : 4) * (size_t)t->CP;
  ST_REQUIRE(((uintptr_t)s & (row - 1)) == 0,
             "csr_multi_rowsum: a packed vector must be aligned to its row of %zu "
             "bytes", row);
  return ST_CSRM_CALL(multi_rowsum, t, h, t, s, scratch, stream);
}

int
launch_csr_multi_round(const CsrHandle* h, const CsrMultiHandle* t, const void* s_prev,
                       void* s_next, const void* v_prev, void* v_cur, void* scratch,
                       double eps, uint32_t k, uint32_t max_itr, uint32_t semantics,
                       st_state* states, uint32_t* finished, hipStream_t stream)
{
  ST_REQUIRE(s_prev && s_next && v_prev && v_cur && scratch && states && finished,
             "csr_multi_round: null pointer");
  ST_REQUIRE(((uintptr_t)scratch & 255u) == 0,
             "csr_multi_round: the scratch must be aligned to 256 bytes");
  const size_t row = (h->dtype ? 8 : 4) * (size_t)t->CP;
  ST_REQUIRE((((uintptr_t)s_prev | (uintptr_t)s_next | (uintptr_t)v_prev |
               (uintptr_t)v_cur) & (row - 1)) == 0,
             "csr_multi_round: a packed vector must be aligned to its row of %zu "
             "bytes", row);
  ST_REQUIRE(semantics <= ST_SEM_MAINPY, "csr_multi_round: bad semantics %u",
             semantics);
  ST_REQUIRE(k >= 1 && max_itr > 0, "csr_multi_round: launch index k must be >= 1");
  ST_REQUIRE(v_prev != v_cur, "csr_multi_round: v_prev and v_cur must differ");
  ST_REQUIRE(s_prev != s_next, "csr_multi_round: s_prev and s_next must differ");
  return ST_CSRM_CALL(multi_round, t, h, t, s_prev, s_next, v_prev, v_cur, scratch,
                      eps, k, max_itr, semantics, states, finished, stream);
}

int
launch_csr_multi_collect(const CsrMultiHandle* t, const void* v0, const void* v1,
                         void* out, const st_state* states, CsrBatchResult* res,
                         hipStream_t stream)
{
  ST_REQUIRE(v0 && v1 && out && states && res, "csr_multi_collect: null pointer");
  return ST_CSRM_CALL(multi_collect, t, t, v0, v1, out, states, res, stream);
}

} // namespace st

#define ST_STREAM(p) (reinterpret_cast<hipStream_t>(p))

extern "C" {

int
st_csr_multi_destroy(void* multi)
{
  st::clear_error();
  return st::csr_multi_destroy(static_cast<st::CsrMultiHandle*>(multi));
}

uint64_t
st_csr_multi_scratch_bytes(uint32_t n, uint32_t C, uint32_t K)
{
  if (n == 0 || n >= 0x80000000u || C < 1 || C > st::csr::kMultiMax || K < 1 ||
      K > st::csr::kTermsMax)
    return 0;
  return st::csr_multi_scratch_bytes(n, C, K);
}

const char*
st_csr_multi_shape_desc(void)
{
  static_assert(st::dev::kCsrDotGrid == 2048 && st::csr::kTermsMax == 4 &&
                  st::csr::kMultiMax == 8 && st::csr::multi_cp(3) == 4 &&
                  st::csr::multi_rows(0, 64) == 2 && st::csr::multi_unroll(3, 32) == 4 &&
                  st::kCheckGrid == 8192,
                "the description below");
  return "multi_max=8 terms_max=4 widths=2,4,8 dot_grid=2048 lanes=256 "
         "combine=one_workgroup_per_column launches_per_round=3 dots_offset=0 "
         "partial_offset=256 rows16=8,4,2,1 unroll16=1,2,4,8 rows32=4,2,1,1 "
         "unroll32=1,2,4,4 rows64=2,2,1,1 unroll64=1,1,2,2 check_grid=8192";
}

int
st_csr_multi_rowsum(void* csr, void* multi, void* d_s, void* d_scratch, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_multi_rowsum");
  if (!h)
    return -1;
  const st::CsrMultiHandle* t = st::as_csr_multi(multi, h, "st_csr_multi_rowsum");
  if (!t)
    return -1;
  return st::launch_csr_multi_rowsum(h, t, d_s, d_scratch, ST_STREAM(stream));
}

int
st_csr_multi_round(void* csr, void* multi, const void* d_s_prev, void* d_s_next,
                   const void* d_v_prev, void* d_v_cur, void* d_scratch, double eps,
                   unsigned int k, unsigned int max_itr, unsigned int semantics,
                   st_state* d_states, uint32_t* d_finished, void* stream)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_multi_round");
  if (!h)
    return -1;
  const st::CsrMultiHandle* t = st::as_csr_multi(multi, h, "st_csr_multi_round");
  if (!t)
    return -1;
  return st::launch_csr_multi_round(h, t, d_s_prev, d_s_next, d_v_prev, d_v_cur,
                                    d_scratch, eps, k, max_itr, semantics, d_states,
                                    d_finished, ST_STREAM(stream));
}

} // extern "C"
