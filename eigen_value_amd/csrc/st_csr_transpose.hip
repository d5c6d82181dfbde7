// st_csr_transpose.hip — the stable device transposition of a CSR matrix
// (kernels in st_csr_transpose.h, the contract in st_csr_host.h) and the part
// of its C-ABI that needs no queue (similarity_transform.h section 3c,
// "Transposed CSR":
// st_csr_transpose_host, st_csr_transpose_scratch_bytes,
// st_csr_transpose_shape_desc).  st_csr_transpose and
// max_eigen_value_csr_left_ex live with the queue in st_solve.hip.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "st_csr_transpose.h"
#include "st_internal.h"

namespace st {
namespace {

using dev::kBlock;

constexpr uint32_t kTrGrid = 8192; // workgroup cap of the grid-stride kernels

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

// digit passes over the columns 0 .. n - 1: ceil(bits(n - 1) / kDigitBits)
uint32_t
passes_of(uint32_t n)
{
  uint32_t bits = 0;
  for (uint32_t x = n - 1; x; x >>= 1)
    bits++;
  return (bits + dev::kDigitBits - 1) / dev::kDigitBits;
}

// the one allocation of a transposition, every part at a multiple of 256 bytes
struct Layout
{
  uint32_t passes, ntiles, ncb, nblk, nidx, nkeys;
  size_t err, cnt, bsum, dtot, tab, idx[2], keys[2], plan_cnt, bytes;
  Layout(uint32_t n, uint64_t nnz)
  {
    passes = passes_of(n);
    ntiles = (uint32_t)((nnz + dev::kTile - 1) / dev::kTile);
    ncb = (n + dev::kColsPerBlock - 1) / dev::kColsPerBlock;
    nblk = (n + kBlock - 1) / kBlock;
    nidx = passes < 2 ? passes : 2;              // pass p writes idx[p & 1]
    nkeys = passes < 3 ? (passes ? passes - 1 : 0) : 2; // the last pass none
    size_t at = 0;
    auto take = [&at](size_t b) {
      const size_t was = at;
      at += (b + 255) & ~(size_t)255;
      return was;
    };
    err = take(2 * sizeof(unsigned long long) + 8 * sizeof(uint32_t));
    cnt = take(sizeof(uint32_t) * (size_t)n);
    bsum = take(sizeof(uint32_t) * (size_t)ncb);
    dtot = take(sizeof(uint32_t) * dev::kDigits * (passes ? passes : 1));
    tab = take(sizeof(uint32_t) * dev::kDigits * (size_t)ntiles);
    for (uint32_t i = 0; i < 2; i++)
      idx[i] = i < nidx ? take(sizeof(uint32_t) * nnz) : 0;
    for (uint32_t i = 0; i < 2; i++)
      keys[i] = i < nkeys ? take(sizeof(uint32_t) * nnz) : 0;
    plan_cnt = take(sizeof(uint32_t) * csr::kClasses * (size_t)nblk);
    bytes = at;
  }
};

struct Freed
{
  void* p = nullptr;
  ~Freed()
  {
    if (p)
      (void)hipFree(p);
  }
};

bool
overlap(const void* a, size_t na, const void* b, size_t nb)
{
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

} // namespace

int
csr_transpose_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                   const int32_t* col_idx, const void* vals, int64_t* t_row_ptr,
                   int32_t* t_col_idx, void* t_vals, uint32_t flags)
{
  char msg[384];
  if ((flags & ~csr::kEmptyRowsOk) != 0) {
    set_error("st_csr_transpose_host_ex: unknown flags %u", flags);
    return -1;
  }
  if (csr::transpose_host(dtype, n, nnz, row_ptr, col_idx, vals, t_row_ptr,
                          t_col_idx, t_vals, msg, sizeof(msg), flags)) {
    set_error("%s", msg);
    return -1;
  }
  return 0;
}

int
csr_transpose(const CsrHandle* a, int64_t* d_t_row_ptr, int32_t* d_t_col_idx,
              void* d_t_vals, hipStream_t stream, CsrHandle** out, uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_transpose: null output pointer");
  *out = nullptr;
  Freed order;
  uint32_t* d_order = nullptr;
  uint32_t cf[csr::kClasses + 1];
  uint32_t empty_rows = 0, first_empty = a->n;
  if (csr_transpose_arrays(a->dtype, a->n, a->nnz, a->row_ptr, a->col_idx, a->vals,
                           d_t_row_ptr, d_t_col_idx, d_t_vals, stream, flags, &d_order,
                           cf, &empty_rows, &first_empty))
    return -1;
  order.p = d_order;
  CsrHandle* h = nullptr;
  if (csr_make_handle(a->dtype, a->n, a->nnz, d_t_row_ptr, d_t_col_idx, d_t_vals,
                      d_order, cf, &h, empty_rows, first_empty))
    return -1;
  order.p = nullptr; // the handle's now
  *out = h;
  return 0;
}

// vals == nullptr (a pattern handle): two arrays in, two out, the final
// gather writes source rows only
int
csr_transpose_arrays(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                     const int32_t* col_idx, const void* vals, int64_t* d_t_row_ptr,
                     int32_t* d_t_col_idx, void* d_t_vals, hipStream_t stream,
                     uint32_t flags, uint32_t** d_order_out, uint32_t* cf,
                     uint32_t* empty_rows_out, uint32_t* first_empty_out)
{
  *d_order_out = nullptr;
  const bool pattern = vals == nullptr;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "st_csr_transpose_ex: unknown flags %u", flags);
  const bool empty_ok = (flags & csr::kEmptyRowsOk) != 0;
  char msg[384];
  if (csr::check_transpose_nnz(nnz, msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  if (pattern)
    ST_REQUIRE(d_t_row_ptr && d_t_col_idx, "csr transpose: null t_row_ptr / t_col_idx");
  else
    ST_REQUIRE(d_t_row_ptr && d_t_col_idx && d_t_vals,
               "csr transpose: null t_row_ptr / t_col_idx / t_vals");
  const size_t elem = dtype ? 8 : 4;
  ST_REQUIRE(((uintptr_t)d_t_row_ptr & 7u) == 0 && ((uintptr_t)d_t_col_idx & 3u) == 0 &&
               (pattern || ((uintptr_t)d_t_vals & (elem - 1)) == 0),
             "csr: an array is not aligned to its element size");
  {
    const int na = pattern ? 2 : 3; // the arrays on each side
    const void* in[3] = { row_ptr, col_idx, vals };
    const void* o[3] = { d_t_row_ptr, d_t_col_idx, d_t_vals };
    const size_t sz[3] = { 8 * ((size_t)n + 1), 4 * (size_t)nnz, elem * (size_t)nnz };
    static const char* const name[3] = { "row_ptr", "col_idx", "vals" };
    for (int i = 0; i < na; i++) {
      for (int j = 0; j < na; j++)
        ST_REQUIRE(!overlap(o[i], sz[i], in[j], sz[j]),
                   "csr transpose: the output t_%s overlaps the input %s: the "
                   "transposition is not done in place", name[i], name[j]);
      for (int j = 0; j < i; j++)
        ST_REQUIRE(!overlap(o[i], sz[i], o[j], sz[j]),
                   "csr transpose: the outputs t_%s and t_%s overlap", name[i],
                   name[j]);
    }
  }

  const Layout lay(n, nnz);
  Freed mem, order;
  ST_CHECK(hipMalloc(&mem.p, lay.bytes));
  ST_CHECK(hipMalloc(&order.p, sizeof(uint32_t) * (size_t)n));
  char* base = static_cast<char*>(mem.p);
  unsigned long long* d_err = reinterpret_cast<unsigned long long*>(base + lay.err);
  uint32_t* d_cf = reinterpret_cast<uint32_t*>(d_err + 2);
  uint32_t* d_empty = d_cf + 5; // the result's empty rows (ST_CSR_EMPTY_ROWS_OK)
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + lay.cnt);
  uint32_t* d_bsum = reinterpret_cast<uint32_t*>(base + lay.bsum);
  uint32_t* d_dtot = reinterpret_cast<uint32_t*>(base + lay.dtot);
  uint32_t* d_tab = reinterpret_cast<uint32_t*>(base + lay.tab);
  uint32_t* d_idx[2] = { reinterpret_cast<uint32_t*>(base + lay.idx[0]),
                         reinterpret_cast<uint32_t*>(base + lay.idx[1]) };
  uint32_t* d_keys[2] = { reinterpret_cast<uint32_t*>(base + lay.keys[0]),
                          reinterpret_cast<uint32_t*>(base + lay.keys[1]) };
  uint32_t* d_pcnt = reinterpret_cast<uint32_t*>(base + lay.plan_cnt);
  uint32_t* d_order = static_cast<uint32_t*>(order.p);
  const uint64_t want = (nnz + kBlock - 1) / kBlock;
  const uint32_t egrid = want < kTrGrid ? (uint32_t)want : kTrGrid;
  unsigned long long err[2];

  // 1. the column histogram, its scan = t_row_ptr, and the empty-column check
  // before anything is scattered
  ST_CHECK(hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), stream));
  ST_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * (size_t)n, stream));
  ST_CHECK(hipMemsetAsync(d_dtot, 0, sizeof(uint32_t) * dev::kDigits *
                                       (lay.passes ? lay.passes : 1), stream));
  hipLaunchKernelGGL(dev::k_tr_count, dim3(egrid), dim3(kBlock), 0, stream,
                     col_idx, n, nnz, d_cnt);
  if (check_launch("tr_count"))
    return -1;
  hipLaunchKernelGGL(dev::k_tr_colsum, dim3(lay.ncb), dim3(kBlock), 0, stream,
                     (const uint32_t*)d_cnt, n, d_bsum, d_err);
  if (check_launch("tr_colsum"))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[0] != ~0ull && !empty_ok) {
    csr::describe_empty_col((uint32_t)err[0], msg, sizeof(msg));
    set_error("%s", msg);
    return -1;
  }
  if (err[0] != ~0ull) // an empty column is legal here: the plan's check is next
    ST_CHECK(hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(dev::k_tr_top, dim3(1), dim3(kBlock), 0, stream, d_bsum,
                     lay.ncb);
  if (check_launch("tr_top"))
    return -1;
  hipLaunchKernelGGL(dev::k_tr_rowptr, dim3(lay.ncb), dim3(kBlock), 0, stream,
                     (const uint32_t*)d_cnt, n, (const uint32_t*)d_bsum,
                     d_t_row_ptr);
  if (check_launch("tr_rowptr"))
    return -1;

  // 2. the digit passes: pass p sorts by bits [8 p, 8 p + 8) of the column
  const uint32_t* keys_in = reinterpret_cast<const uint32_t*>(col_idx);
  const uint32_t* idx_in = nullptr;
  for (uint32_t p = 0; p < lay.passes; p++) {
    const uint32_t shift = p * dev::kDigitBits;
    uint32_t* dt = d_dtot + (size_t)p * dev::kDigits;
    uint32_t* keys_out = p + 1 < lay.passes ? d_keys[p & 1] : nullptr;
    hipLaunchKernelGGL(dev::k_tr_hist, dim3(lay.ntiles), dim3(kBlock), 0, stream,
                       keys_in, nnz, shift, lay.ntiles, d_tab, dt);
    if (check_launch("tr_hist"))
      return -1;
    hipLaunchKernelGGL(dev::k_tr_scan, dim3(dev::kDigits), dim3(kBlock), 0,
                       stream, d_tab, lay.ntiles, (const uint32_t*)dt);
    if (check_launch("tr_scan"))
      return -1;
    hipLaunchKernelGGL(dev::k_tr_scatter, dim3(lay.ntiles), dim3(kBlock), 0,
                       stream, keys_in, idx_in, nnz, shift, lay.ntiles,
                       (const uint32_t*)d_tab, keys_out, d_idx[p & 1]);
    if (check_launch("tr_scatter"))
      return -1;
    keys_in = keys_out;
    idx_in = d_idx[p & 1];
  }

  // 3. the values and the source rows through the permutation
  if (pattern)
    hipLaunchKernelGGL(dev::k_tr_gather_rows, dim3(egrid), dim3(kBlock), 0, stream,
                       row_ptr, idx_in, n, nnz, d_t_col_idx);
  else if (dtype)
    hipLaunchKernelGGL(dev::k_tr_gather<double>, dim3(egrid), dim3(kBlock), 0,
                       stream, row_ptr, static_cast<const double*>(vals),
                       idx_in, n, nnz, d_t_col_idx, static_cast<double*>(d_t_vals));
  else
    hipLaunchKernelGGL(dev::k_tr_gather<float>, dim3(egrid), dim3(kBlock), 0,
                       stream, row_ptr, static_cast<const float*>(vals),
                       idx_in, n, nnz, d_t_col_idx, static_cast<float*>(d_t_vals));
  if (check_launch("tr_gather"))
    return -1;

  // 4. the plan of t_row_ptr, as csr_create builds it (the predicate again:
  // it fails only if the matrix changed under the handle)
  ST_CHECK(hipMemsetAsync(d_empty, 0, sizeof(uint32_t), stream));
  if (launch_csr_check_ptr(d_t_row_ptr, n, nnz, d_pcnt, d_err, stream,
                           empty_ok ? d_empty : nullptr))
    return -1;
  ST_CHECK(hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  if (err[0] != ~0ull) {
    const uint32_t r = (uint32_t)err[0];
    int64_t w[2];
    ST_CHECK(hipMemcpy(w, d_t_row_ptr + r, sizeof(w), hipMemcpyDeviceToHost));
    csr::describe_row(r, w[0], w[1], n, nnz, msg, sizeof(msg), empty_ok);
    set_error("csr transpose: the matrix changed under its handle (%s)", msg);
    return -1;
  }
  const uint32_t first_empty = err[1] != ~0ull ? (uint32_t)err[1] : n;
  uint32_t empty_rows = 0;
  if (empty_ok)
    ST_CHECK(hipMemcpy(&empty_rows, d_empty, sizeof(uint32_t), hipMemcpyDeviceToHost));
  ST_CHECK(hipMemsetAsync(d_order, 0, sizeof(uint32_t) * (size_t)n, stream));
  if (launch_csr_plan(d_t_row_ptr, n, d_pcnt, d_cf, d_order, stream))
    return -1;
  ST_CHECK(hipMemcpyAsync(cf, d_cf, sizeof(uint32_t) * (csr::kClasses + 1),
                          hipMemcpyDeviceToHost, stream));
  ST_CHECK(hipStreamSynchronize(stream));
  order.p = nullptr; // the caller's now
  *d_order_out = d_order;
  *empty_rows_out = empty_rows;
  *first_empty_out = first_empty;
  return 0;
}

} // namespace st

extern "C" {

int
st_csr_transpose_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                      const int32_t* col_idx, const void* vals,
                      int64_t* t_row_ptr, int32_t* t_col_idx, void* t_vals)
{
  st::clear_error();
  return st::csr_transpose_host(dtype, n, nnz, row_ptr, col_idx, vals, t_row_ptr,
                                t_col_idx, t_vals);
}

int
st_csr_transpose_host_ex(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                         const int32_t* col_idx, const void* vals,
                         int64_t* t_row_ptr, int32_t* t_col_idx, void* t_vals,
                         unsigned int flags)
{
  st::clear_error();
  return st::csr_transpose_host(dtype, n, nnz, row_ptr, col_idx, vals, t_row_ptr,
                                t_col_idx, t_vals, flags);
}

uint64_t
st_csr_transpose_scratch_bytes(uint32_t n, uint64_t nnz)
{
  if (n == 0 || n >= 0x80000000u || nnz >= (1ull << 32))
    return 0;
  return st::Layout(n, nnz).bytes;
}

const char*
st_csr_transpose_shape_desc(void)
{
  static_assert(st::dev::kDigitBits == 8 && st::dev::kTile == 2048 &&
                  st::dev::kTileRounds == 8 && st::dev::kColsPerBlock == 2048 &&
                  st::kTrGrid == 8192,
                "the description below");
  return "digit_bits=8 tile=2048 rounds=8 lanes=256 col_block=2048 payload=index "
         "grid=8192";
}

} // extern "C"
