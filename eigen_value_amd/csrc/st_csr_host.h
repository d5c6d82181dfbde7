// st_csr_host.h — the host side of the sparse (CSR) solve that needs no GPU:
// the row-class table, the plan (rows sorted by class) and the validation of
// a host CSR matrix.  Plain C++ without any HIP, so that it also compiles
// into a stand-alone program (tests/cpp/csr_sanitize.cpp and, for the empty
// rows flag and the low-rank terms, tests/cpp/csr_terms_sanitize.cpp, for the
// multi-column packing and validation tests/cpp/csr_multi_sanitize.cpp, for
// the product operator tests/cpp/csr_product_sanitize.cpp, for the pattern-only
// operator tests/cpp/csr_pattern_sanitize.cpp, run under the host sanitizers).
// Included by st_csr.hip; not a public header.
//
// Every function returns 0 (or a count) on success and -1 on failure with
// the reason written to msg[cap].
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace st {
namespace csr {

// Row classes: a row of nnz entries belongs to the first class c with
// nnz <= kNnzMax[c], and kLanes[c] lanes share it (4 and 16: part of a wave,
// 64: one wave, 256: one workgroup).  The kernels (st_csr.h), the plan and
// st_csr_class_limits all read this one table.
constexpr int kClasses = 4;
constexpr uint32_t kLanes[kClasses] = { 4u, 16u, 64u, 256u };
constexpr uint32_t kNnzMax[kClasses] = { 16u, 128u, 2048u, 0xffffffffu };
constexpr uint32_t kBlock = 256; // lanes of a workgroup
// launch shape (no effect on any result): rows the lanes of a row take side by
// side, and entries of each row in flight per lane; a workgroup of class c
// holds kRows[c] * 256 / kLanes[c] rows
constexpr uint32_t kRows[kClasses] = { 8u, 4u, 2u, 1u };
constexpr uint32_t kUnroll[kClasses] = { 1u, 2u, 4u, 8u };
// flags of the _ex calls (ST_CSR_EMPTY_ROWS_OK) and the most rank-one terms
// of one operator (ST_CSR_TERMS_MAX)
constexpr uint32_t kEmptyRowsOk = 1u;
constexpr uint32_t kTermsMax = 4;

// the class of a row of `len` entries (an empty row, where a handle allows
// one, is class 0)
inline int
row_class(uint64_t len)
{
  for (int c = 0; c < kClasses - 1; c++)
    if (len <= kNnzMax[c])
      return c;
  return kClasses - 1;
}

// row_ptr on its own, row by row: row_ptr[0] == 0, strictly increasing (an
// empty row would divide by zero), row_ptr[n] == nnz when check_nnz.  The
// device check (k_csr_check_ptr) applies the same predicate per row and
// reports the lowest offending row through describe_row.  empty_ok
// (kEmptyRowsOk): b == a is legal, row_ptr only must not decrease.
inline bool
row_bad(uint32_t r, int64_t a, int64_t b, uint32_t n, bool check_nnz,
        uint64_t nnz, bool empty_ok = false)
{
  return (r == 0 && a != 0) || (empty_ok ? b < a : b <= a) ||
         (check_nnz && r == n - 1 && (uint64_t)b != nnz);
}

// the message for row r with row_ptr[r] = a, row_ptr[r + 1] = b
inline void
describe_row(uint32_t r, int64_t a, int64_t b, uint32_t n, uint64_t nnz,
             char* msg, size_t cap, bool empty_ok = false)
{
  if (r == 0 && a != 0)
    snprintf(msg, cap, "csr: row_ptr[0] must be 0, got %lld (row 0)",
             (long long)a);
  else if (b < a)
    snprintf(msg, cap,
             "csr: row_ptr decreases at row %u (row_ptr[%u] = %lld, "
             "row_ptr[%u] = %lld)", r, r, (long long)a, r + 1, (long long)b);
  else if (b == a && !empty_ok)
    snprintf(msg, cap,
             "csr: row %u is empty (row_ptr[%u] = row_ptr[%u] = %lld): its "
             "row sum would be divided by zero", r, r, r + 1, (long long)a);
  else
    snprintf(msg, cap, "csr: row_ptr[n] must be nnz = %llu, got %lld (row %u)",
             (unsigned long long)nnz, (long long)b, n - 1);
}

inline int
check_row_ptr(const int64_t* row_ptr, uint32_t n, bool check_nnz, uint64_t nnz,
              char* msg, size_t cap, bool empty_ok = false)
{
  for (uint32_t r = 0; r < n; r++)
    if (row_bad(r, row_ptr[r], row_ptr[r + 1], n, check_nnz, nnz, empty_ok)) {
      describe_row(r, row_ptr[r], row_ptr[r + 1], n, nnz, msg, cap, empty_ok);
      return -1;
    }
  return 0;
}

// the empty rows of a checked row_ptr: their number, *lowest = the first one
// (n when there is none)
inline uint32_t
count_empty_rows(const int64_t* row_ptr, uint32_t n, uint32_t* lowest)
{
  uint32_t k = 0;
  *lowest = n;
  for (uint32_t r = 0; r < n; r++)
    if (row_ptr[r + 1] == row_ptr[r]) {
      if (k == 0)
        *lowest = r;
      k++;
    }
  return k;
}

// what a call that divides by a row sum of A alone says to an empty-rows
// handle (st_solve_csr without terms, st_csr_mfree_round,
// max_eigen_value_csr_ex)
inline void
describe_needs_terms(const char* what, uint32_t r, uint32_t count, char* msg,
                     size_t cap)
{
  snprintf(msg, cap,
           "%s: row %u is empty (%u empty rows, ST_CSR_EMPTY_ROWS_OK): its row "
           "sum would be divided by zero; such a matrix is solved with "
           "low-rank terms (st_solve_csr_terms)", what, r, count);
}

// the flagged create needs one entry: redirected loads read entry 0
inline int
check_nnz_min(uint64_t nnz, char* msg, size_t cap)
{
  if (nnz == 0) {
    snprintf(msg, cap, "csr: nnz must be >= 1, got 0: loads past a row's end "
                       "are redirected to entry 0");
    return -1;
  }
  return 0;
}

// every col_idx[e], e in [0, nnz), inside [0, n); call only after
// check_row_ptr passed (the row of the offending entry is looked up in it)
inline int
check_col_idx(const int64_t* row_ptr, const int32_t* col_idx, uint32_t n,
              uint64_t nnz, char* msg, size_t cap)
{
  for (uint64_t e = 0; e < nnz; e++) {
    const int32_t c = col_idx[e];
    if (c < 0 || (uint32_t)c >= n) {
      uint32_t lo = 0, hi = n; // the row r with row_ptr[r] <= e < row_ptr[r+1]
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)row_ptr[mid] <= e)
          lo = mid;
        else
          hi = mid;
      }
      snprintf(msg, cap,
               "csr: column index %d of entry %llu (row %u) is outside [0, %u)",
               c, (unsigned long long)e, lo, n);
      return -1;
    }
  }
  return 0;
}

// The plan: order_out[n] = the row indices sorted by class, row order kept
// within a class; class_first[kClasses + 1] = where each class starts.
// Returns the number of non-empty classes.
inline int
plan(const int64_t* row_ptr, uint32_t n, uint32_t* order_out,
     uint32_t* class_first, char* msg, size_t cap, bool empty_ok = false)
{
  if (check_row_ptr(row_ptr, n, false, 0, msg, cap, empty_ok))
    return -1;
  uint32_t count[kClasses] = { 0, 0, 0, 0 };
  for (uint32_t r = 0; r < n; r++)
    count[row_class((uint64_t)(row_ptr[r + 1] - row_ptr[r]))]++;
  uint32_t at[kClasses];
  int used = 0;
  class_first[0] = 0;
  for (int c = 0; c < kClasses; c++) {
    at[c] = class_first[c];
    class_first[c + 1] = class_first[c] + count[c];
    used += count[c] != 0;
  }
  for (uint32_t r = 0; r < n; r++)
    order_out[at[row_class((uint64_t)(row_ptr[r + 1] - row_ptr[r]))]++] = r;
  return used;
}

// a whole host matrix, in the order the device check runs: the arguments,
// row_ptr on its own, then the column indices
inline int
check_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
           const int32_t* col_idx, const void* vals, char* msg, size_t cap,
           bool empty_ok = false)
{
  if (dtype != 0 && dtype != 1) {
    snprintf(msg, cap, "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
    return -1;
  }
  if (n == 0 || n >= 0x80000000u) {
    snprintf(msg, cap, "csr: n must be in [1, 2^31), got %u", n);
    return -1;
  }
  if (empty_ok && check_nnz_min(nnz, msg, cap)) // arrays of no entry may be null
    return -1;
  if (!row_ptr || !col_idx || !vals) {
    snprintf(msg, cap, "csr: null row_ptr / col_idx / vals");
    return -1;
  }
  if (check_row_ptr(row_ptr, n, true, nnz, msg, cap, empty_ok))
    return -1;
  return check_col_idx(row_ptr, col_idx, n, nnz, msg, cap);
}

// ---------------------------------------------------------------------------
// Low-rank terms (st_csr_terms.hip): M = A + sum_j u_j w_j^T, j < K.  The
// device check applies the same predicates in the same order - the lowest
// (term, vector, index) with u before w - and prints through the same
// describe_* functions.
// ---------------------------------------------------------------------------
inline int
check_terms_count(uint32_t K, char* msg, size_t cap)
{
  if (K < 1 || K > kTermsMax) {
    snprintf(msg, cap, "csr terms: K must be in [1, %u], got %u", kTermsMax, K);
    return -1;
  }
  return 0;
}

// finite and >= 0 (NaN fails every comparison)
template <typename T>
inline bool
term_entry_bad(T x)
{
  return !(x >= (T)0) || x - x != (T)0; // inf - inf is NaN
}

// which: 0 = u, 1 = w
inline void
describe_term_entry(uint32_t j, int which, uint32_t i, double x, char* msg,
                    size_t cap)
{
  snprintf(msg, cap,
           "csr terms: %s_%u[%u] = %g: every entry of a term vector must be "
           "finite and >= 0", which ? "w" : "u", j, i, x);
}

inline void
describe_term_row(uint32_t r, double s0, char* msg, size_t cap)
{
  snprintf(msg, cap,
           "csr terms: row %u of A + Σ u wᵀ has no positive entry "
           "(its sum is %g): it would be divided by zero", r, s0);
}

template <typename T>
inline int
check_terms_vectors(uint32_t n, uint32_t K, const T* const* u, const T* const* w,
                    char* msg, size_t cap)
{
  for (uint32_t j = 0; j < K; j++)
    for (int which = 0; which < 2; which++) {
      const T* p = which ? w[j] : u[j];
      if (!p) {
        snprintf(msg, cap, "csr terms: null %s_%u", which ? "w" : "u", j);
        return -1;
      }
      for (uint32_t i = 0; i < n; i++)
        if (term_entry_bad<T>(p[i])) {
          describe_term_entry(j, which, i, (double)p[i], msg, cap);
          return -1;
        }
    }
  return 0;
}

// every row of M needs a positive entry: s_0[r] = the row sum of A plus
// sum_j u_j[r] (w_j . 1), finite and > 0 (summed in double here; the device
// judges the s_0 its own K0 computes)
template <typename T>
inline int
check_terms_rows(uint32_t n, const int64_t* row_ptr, const T* vals, uint32_t K,
                 const T* const* u, const T* const* w, char* msg, size_t cap)
{
  double d[kTermsMax] = { 0, 0, 0, 0 };
  for (uint32_t j = 0; j < K; j++)
    for (uint32_t i = 0; i < n; i++)
      d[j] += (double)w[j][i];
  for (uint32_t r = 0; r < n; r++) {
    double s = 0;
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++)
      s += (double)vals[e];
    for (uint32_t j = 0; j < K; j++)
      s += (double)u[j][r] * d[j];
    const T st = (T)s;
    if (!(st > (T)0) || st - st != (T)0) {
      describe_term_row(r, (double)st, msg, cap);
      return -1;
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The product operator M = B A (st_csr_product.hip), both factors n x n of one
// dtype; no entry of M is formed.  Every row of M needs a positive entry.  The
// device judges the s_0 its own K0 computes (finite and > 0); the host twin
// below asks whether row r of B has an entry b > 0 whose column is a row of A
// holding a value > 0.  For finite nonnegative factors the two predicates can
// differ only where a product or a sum under- or overflows: b * (row sum of
// A) may round to 0 or to inf on the device where the host sees a positive
// entry.  Both print through describe_product_row.
// ---------------------------------------------------------------------------
inline void
describe_product_row(uint32_t r, char* msg, size_t cap)
{
  snprintf(msg, cap,
           "csr product: row %u of B·A has no positive entry: it would be "
           "divided by zero", r);
}

// "csr: <text>" -> "csr product: factor B: <text>"
inline void
put_factor(const char* which, char* msg, size_t cap)
{
  char tmp[384];
  snprintf(tmp, sizeof(tmp), "%s", msg);
  const char* head = "csr: ";
  size_t skip = 0;
  while (head[skip] && tmp[skip] == head[skip])
    skip++;
  if (head[skip])
    skip = 0;
  snprintf(msg, cap, "csr product: factor %s: %s", which, tmp + skip);
}

// the rows of B A in ascending order; call only after both triples passed
// check_host.  a_pos [n] is scratch of the caller: a_pos[c] = row c of A
// holds a value > 0
template <typename T>
inline int
check_product_rows(uint32_t n, const int64_t* b_row_ptr, const int32_t* b_col_idx,
                   const T* b_vals, const int64_t* a_row_ptr, const T* a_vals,
                   unsigned char* a_pos, char* msg, size_t cap)
{
  for (uint32_t c = 0; c < n; c++) {
    a_pos[c] = 0;
    for (int64_t e = a_row_ptr[c]; e < a_row_ptr[c + 1]; e++)
      if (a_vals[e] > (T)0) {
        a_pos[c] = 1;
        break;
      }
  }
  for (uint32_t r = 0; r < n; r++) {
    bool any = false;
    for (int64_t e = b_row_ptr[r]; e < b_row_ptr[r + 1] && !any; e++)
      any = b_vals[e] > (T)0 && a_pos[(uint32_t)b_col_idx[e]] != 0;
    if (!any) {
      describe_product_row(r, msg, cap);
      return -1;
    }
  }
  return 0;
}

// a whole host product, in its fixed order: dtype and n (shared), B's triple
// (no empty row: it would be an empty row of M), A's triple (empty rows legal
// under a_flags & kEmptyRowsOk), then the rows of B A
inline int
check_product_host(int dtype, uint32_t n, uint64_t b_nnz, const int64_t* b_row_ptr,
                   const int32_t* b_col_idx, const void* b_vals, uint64_t a_nnz,
                   const int64_t* a_row_ptr, const int32_t* a_col_idx,
                   const void* a_vals, uint32_t a_flags, unsigned char* a_pos,
                   char* msg, size_t cap)
{
  if (check_host(dtype, n, b_nnz, b_row_ptr, b_col_idx, b_vals, msg, cap)) {
    put_factor("B", msg, cap);
    return -1;
  }
  if (check_host(dtype, n, a_nnz, a_row_ptr, a_col_idx, a_vals, msg, cap,
                 (a_flags & kEmptyRowsOk) != 0)) {
    put_factor("A", msg, cap);
    return -1;
  }
  if (!a_pos) {
    snprintf(msg, cap, "csr product: null scratch");
    return -1;
  }
  return dtype ? check_product_rows<double>(
                   n, b_row_ptr, b_col_idx, static_cast<const double*>(b_vals),
                   a_row_ptr, static_cast<const double*>(a_vals), a_pos, msg, cap)
               : check_product_rows<float>(
                   n, b_row_ptr, b_col_idx, static_cast<const float*>(b_vals),
                   a_row_ptr, static_cast<const float*>(a_vals), a_pos, msg, cap);
}

// the Gram operators of one matrix: side 0 = A^T A ("ata"), 1 = A A^T ("aat")
inline int
check_gram_side(int side, char* msg, size_t cap)
{
  if (side != 0 && side != 1) {
    snprintf(msg, cap, "csr gram: side must be 0 (A^T A) or 1 (A A^T), got %d", side);
    return -1;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Many term sets on one matrix (st_csr_multi.hip): M_c = A + sum_j u_{c,j}
// w_{c,j}^T, c < C <= kMultiMax, the same K for every column; the tables are
// indexed [c * K + j].  Vectors are packed [n][CP], the column fastest, CP =
// multi_cp(C); padding columns hold 1.  The device check applies the
// predicates above per column and reports the lowest offender by (column,
// then term, u before w, index; then the column's rows), the message the
// single one with the column in front.
// ---------------------------------------------------------------------------
constexpr uint32_t kMultiMax = 8;

// the packed width: the smallest of 2, 4, 8 that is >= C
constexpr uint32_t
multi_cp(uint32_t C)
{
  return C <= 2 ? 2u : C <= 4 ? 4u : 8u;
}

// launch shape of the multi row pass (no effect on any result): rows side by
// side and entries in flight per lane for class c when a packed row of x is
// row_bytes = CP * b bytes.  Up to 16 bytes the single pass's table (R * U =
// 8); 32 bytes R * U = 4; 64 bytes R * U = 2 - the x rows in flight stay at 32
// registers per lane.
constexpr uint32_t
multi_rows(int c, uint32_t row_bytes)
{
  return row_bytes <= 16 ? kRows[c]
         : row_bytes == 32 ? (c == 0 ? 4u : c == 1 ? 2u : 1u)
                           : (c <= 1 ? 2u : 1u);
}
constexpr uint32_t
multi_unroll(int c, uint32_t row_bytes)
{
  return row_bytes <= 16 ? kUnroll[c]
         : row_bytes == 32 ? (c == 0 ? 1u : c == 1 ? 2u : 4u)
                           : (c <= 1 ? 1u : 2u);
}

inline int
check_multi_count(uint32_t C, uint32_t K, char* msg, size_t cap)
{
  if (C < 1 || C > kMultiMax) {
    snprintf(msg, cap, "csr multi: C must be in [1, %u], got %u", kMultiMax, C);
    return -1;
  }
  if (K < 1 || K > kTermsMax) {
    snprintf(msg, cap,
             "csr multi: K must be in [1, %u], got %u%s", kTermsMax, K,
             K == 0 ? ": without terms every column is the same solve" : "");
    return -1;
  }
  return 0;
}

// "csr terms: <text>" -> "csr terms: column c: <text>"
inline void
put_column(uint32_t c, char* msg, size_t cap)
{
  char tmp[384];
  snprintf(tmp, sizeof(tmp), "%s", msg);
  const char* head = "csr terms: ";
  size_t skip = 0;
  while (head[skip] && tmp[skip] == head[skip])
    skip++;
  if (head[skip])
    skip = 0;
  snprintf(msg, cap, "csr terms: column %u: %s", c, tmp + skip);
}

inline void
describe_multi_entry(uint32_t c, uint32_t j, int which, uint32_t i, double x,
                     char* msg, size_t cap)
{
  describe_term_entry(j, which, i, x, msg, cap);
  put_column(c, msg, cap);
}

inline void
describe_multi_row(uint32_t c, uint32_t r, double s0, char* msg, size_t cap)
{
  describe_term_row(r, s0, msg, cap);
  put_column(c, msg, cap);
}

// the whole validation in its fixed order: column after column, the
// column's vectors (term, u before w, index), then its rows
template <typename T>
inline int
check_multi_terms(uint32_t n, const int64_t* row_ptr, const T* vals, uint32_t C,
                  uint32_t K, const T* const* u, const T* const* w, char* msg,
                  size_t cap)
{
  for (uint32_t c = 0; c < C; c++)
    if (check_terms_vectors<T>(n, K, u + (size_t)c * K, w + (size_t)c * K, msg, cap) ||
        check_terms_rows<T>(n, row_ptr, vals, K, u + (size_t)c * K,
                            w + (size_t)c * K, msg, cap)) {
      put_column(c, msg, cap);
      return -1;
    }
  return 0;
}

// dst [n][CP] <- the C dense vectors src[c * stride] (c < C), padding columns
// filled with 1: the packed form of term j when src = table + j, stride = K
template <typename T>
inline void
pack_columns(uint32_t n, uint32_t C, uint32_t CP, const T* const* src,
             size_t stride, T* dst)
{
  for (uint64_t i = 0; i < n; i++)
    for (uint32_t c = 0; c < CP; c++)
      dst[i * CP + c] = c < C ? src[(size_t)c * stride][i] : (T)1;
}

// ---------------------------------------------------------------------------
// The transposition T(A) (st_csr_transpose.hip): t_row_ptr[c] = the entries
// with column < c; transposed row c holds A's entries of column c in
// ascending storage position (so ascending source row, duplicates of a row in
// their order), t_col_idx their source rows, t_vals their values - a stable
// sort of the entries by column.  The device path applies the same
// predicates and prints through the same describe_* functions.
// ---------------------------------------------------------------------------
// the device sort carries 32-bit entry indices
inline int
check_transpose_nnz(uint64_t nnz, char* msg, size_t cap)
{
  if (nnz >= (1ull << 32)) {
    snprintf(msg, cap,
             "csr transpose: nnz must be below 2^32, got %llu: the sort "
             "carries 32-bit entry indices", (unsigned long long)nnz);
    return -1;
  }
  return 0;
}

inline void
describe_empty_col(uint32_t c, char* msg, size_t cap)
{
  snprintf(msg, cap,
           "csr transpose: column %u has no entry: row %u of the transposed "
           "matrix would be empty and its row sum divided by zero", c, c);
}

// a counting sort; the outputs must not overlap the inputs
// flags & kEmptyRowsOk: the source may have empty rows and empty columns (the
// result then has empty rows)
inline int
transpose_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
               const int32_t* col_idx, const void* vals, int64_t* t_row_ptr,
               int32_t* t_col_idx, void* t_vals, char* msg, size_t cap,
               uint32_t flags = 0)
{
  const bool empty_ok = (flags & kEmptyRowsOk) != 0;
  if (check_transpose_nnz(nnz, msg, cap)) // before any array is read
    return -1;
  if (check_host(dtype, n, nnz, row_ptr, col_idx, vals, msg, cap, empty_ok))
    return -1;
  if (!t_row_ptr || !t_col_idx || !t_vals) {
    snprintf(msg, cap, "csr transpose: null t_row_ptr / t_col_idx / t_vals");
    return -1;
  }
  for (uint32_t c = 0; c <= n; c++)
    t_row_ptr[c] = 0;
  for (uint64_t e = 0; e < nnz; e++)
    t_row_ptr[(uint32_t)col_idx[e] + 1]++;
  for (uint32_t c = 0; c < n; c++) {
    if (t_row_ptr[c + 1] == 0 && !empty_ok) { // the lowest: nothing added up yet
      describe_empty_col(c, msg, cap);
      return -1;
    }
    t_row_ptr[c + 1] += t_row_ptr[c];
  }
  // t_row_ptr[c] serves as column c's cursor and is put back afterwards
  for (uint32_t r = 0; r < n; r++)
    for (uint64_t e = (uint64_t)row_ptr[r]; e < (uint64_t)row_ptr[r + 1]; e++) {
      const uint64_t at = (uint64_t)t_row_ptr[(uint32_t)col_idx[e]]++;
      t_col_idx[at] = (int32_t)r;
      if (dtype)
        static_cast<double*>(t_vals)[at] = static_cast<const double*>(vals)[e];
      else
        static_cast<float*>(t_vals)[at] = static_cast<const float*>(vals)[e];
    }
  for (uint32_t c = n; c > 0; c--)
    t_row_ptr[c] = t_row_ptr[c - 1];
  t_row_ptr[0] = 0;
  return 0;
}

// ---------------------------------------------------------------------------
// A batch in stacked CSR storage (st_csr_batch.hip): `batch` matrices, matrix
// b of n_b = mat_first[b + 1] - mat_first[b] rows from stacked row
// mat_first[b]; row_ptr [N + 1] over the concatenated entries; col_idx local
// to its matrix.  The device check (st_csr_batch_create) applies the same
// predicates and prints through the same describe_* functions.
// ---------------------------------------------------------------------------
// mat_first (always a host array): [0] == 0, strictly increasing (every
// matrix has a row), N = mat_first[batch] < 2^31
inline int
check_mat_first(uint32_t batch, const uint32_t* mat_first, char* msg, size_t cap)
{
  if (batch == 0) {
    snprintf(msg, cap, "csr batch: batch must be >= 1, got 0");
    return -1;
  }
  if (!mat_first) {
    snprintf(msg, cap, "csr batch: null mat_first");
    return -1;
  }
  if (mat_first[0] != 0) {
    snprintf(msg, cap, "csr batch: mat_first[0] must be 0, got %u", mat_first[0]);
    return -1;
  }
  for (uint32_t b = 0; b < batch; b++)
    if (mat_first[b + 1] <= mat_first[b]) {
      snprintf(msg, cap,
               "csr batch: mat_first does not increase at matrix %u "
               "(mat_first[%u] = %u, mat_first[%u] = %u): every matrix has at "
               "least one row", b, b, mat_first[b], b + 1, mat_first[b + 1]);
      return -1;
    }
  if (mat_first[batch] >= 0x80000000u) {
    snprintf(msg, cap,
             "csr batch: N = mat_first[batch] must be below 2^31, got %u",
             mat_first[batch]);
    return -1;
  }
  return 0;
}

// the matrix b with mat_first[b] <= r < mat_first[b + 1] (r < N)
inline uint32_t
mat_of_row(const uint32_t* mat_first, uint32_t batch, uint32_t r)
{
  uint32_t lo = 0, hi = batch;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (mat_first[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// the message for stacked row r (row_ptr[r] = a, row_ptr[r + 1] = b): the
// matrix and its local row, then describe_row's text on the stacked arrays
inline void
describe_batch_row(const uint32_t* mat_first, uint32_t batch, uint32_t r,
                   int64_t a, int64_t b, uint64_t nnz, char* msg, size_t cap)
{
  const uint32_t m = mat_of_row(mat_first, batch, r);
  const int at = snprintf(msg, cap, "csr batch: matrix %u, local row %u: ", m,
                          r - mat_first[m]);
  if (at > 0 && (size_t)at < cap)
    describe_row(r, a, b, mat_first[batch], nnz, msg + at, cap - (size_t)at);
}

// the message for entry e of stacked row r holding column c
inline void
describe_batch_col(const uint32_t* mat_first, uint32_t batch, uint32_t r,
                   uint64_t e, int32_t c, char* msg, size_t cap)
{
  const uint32_t m = mat_of_row(mat_first, batch, r);
  snprintf(msg, cap,
           "csr batch: column index %d of entry %llu (matrix %u, local row %u) "
           "is outside [0, %u): columns are local to their matrix", c,
           (unsigned long long)e, m, r - mat_first[m],
           mat_first[m + 1] - mat_first[m]);
}

// every column of matrix b inside [0, n_b) - which also proves that no entry
// couples two matrices; call only after row_ptr passed
inline int
check_batch_col_idx(const uint32_t* mat_first, uint32_t batch,
                    const int64_t* row_ptr, const int32_t* col_idx, char* msg,
                    size_t cap)
{
  for (uint32_t m = 0; m < batch; m++) {
    const uint32_t nb = mat_first[m + 1] - mat_first[m];
    for (uint32_t r = mat_first[m]; r < mat_first[m + 1]; r++)
      for (uint64_t e = (uint64_t)row_ptr[r]; e < (uint64_t)row_ptr[r + 1]; e++) {
        const int32_t c = col_idx[e];
        if (c < 0 || (uint32_t)c >= nb) {
          describe_batch_col(mat_first, batch, r, e, c, msg, cap);
          return -1;
        }
      }
  }
  return 0;
}

// a whole host batch, in the order the device check runs: dtype, mat_first,
// the pointers, row_ptr over the N stacked rows, then the columns
inline int
check_batch_host(int dtype, uint32_t batch, const uint32_t* mat_first,
                 uint64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
                 const void* vals, char* msg, size_t cap)
{
  if (dtype != 0 && dtype != 1) {
    snprintf(msg, cap, "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
    return -1;
  }
  if (check_mat_first(batch, mat_first, msg, cap))
    return -1;
  if (!row_ptr || !col_idx || !vals) {
    snprintf(msg, cap, "csr: null row_ptr / col_idx / vals");
    return -1;
  }
  const uint32_t n = mat_first[batch];
  for (uint32_t r = 0; r < n; r++)
    if (row_bad(r, row_ptr[r], row_ptr[r + 1], n, true, nnz)) {
      describe_batch_row(mat_first, batch, r, row_ptr[r], row_ptr[r + 1], nnz,
                         msg, cap);
      return -1;
    }
  return check_batch_col_idx(mat_first, batch, row_ptr, col_idx, msg, cap);
}

// the participants (workgroups) of matrix b in the batch's vector pass
// (k_csrb_prep): one per kBlock rows, at most prep_cap
inline uint32_t
batch_prep_wgs(uint32_t n_b, uint32_t prep_cap)
{
  const uint32_t want = (n_b + kBlock - 1) / kBlock;
  return want < prep_cap ? want : prep_cap;
}

// ---------------------------------------------------------------------------
// The pattern-only operator M = diag(r) P diag(c) (st_csr_pattern.hip): P the
// 0/1 pattern of row_ptr / col_idx (duplicates count), r and c dense vectors
// [n], each null (all ones) or finite and > 0.  The device check applies the
// same predicates in the same order - row_ptr, the columns, then the scales,
// row_scale before col_scale, the lowest index - and prints through the same
// describe_* functions (tests/cpp/csr_pattern_sanitize.cpp runs these under
// the host sanitizers).
// ---------------------------------------------------------------------------
// finite and > 0 (NaN fails every comparison)
template <typename T>
inline bool
scale_entry_bad(T x)
{
  return !(x > (T)0) || x - x != (T)0; // inf - inf is NaN
}

// which: 0 = row_scale, 1 = col_scale
inline void
describe_scale_entry(int which, uint32_t i, double x, char* msg, size_t cap)
{
  snprintf(msg, cap, "csr pattern: %s[%u] = %g is not finite and positive",
           which ? "col_scale" : "row_scale", i, x);
}

// either vector may be null
template <typename T>
inline int
check_pattern_scales(uint32_t n, const T* r, const T* c, char* msg, size_t cap)
{
  for (int which = 0; which < 2; which++) {
    const T* p = which ? c : r;
    if (!p)
      continue;
    for (uint32_t i = 0; i < n; i++)
      if (scale_entry_bad<T>(p[i])) {
        describe_scale_entry(which, i, (double)p[i], msg, cap);
        return -1;
      }
  }
  return 0;
}

// check_host without values
inline int
check_pattern_host(int dtype, uint32_t n, uint64_t nnz, const int64_t* row_ptr,
                   const int32_t* col_idx, char* msg, size_t cap, bool empty_ok = false)
{
  if (dtype != 0 && dtype != 1) {
    snprintf(msg, cap, "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
    return -1;
  }
  if (n == 0 || n >= 0x80000000u) {
    snprintf(msg, cap, "csr: n must be in [1, 2^31), got %u", n);
    return -1;
  }
  if (empty_ok && check_nnz_min(nnz, msg, cap))
    return -1;
  if (!row_ptr || !col_idx) {
    snprintf(msg, cap, "csr: null row_ptr / col_idx");
    return -1;
  }
  if (check_row_ptr(row_ptr, n, true, nnz, msg, cap, empty_ok))
    return -1;
  return check_col_idx(row_ptr, col_idx, n, nnz, msg, cap);
}

// the terms of a pattern operator: none (K = 0) is legal
inline int
check_pattern_terms_count(uint32_t K, char* msg, size_t cap)
{
  if (K > kTermsMax) {
    snprintf(msg, cap, "csr pattern: K must be in [0, %u], got %u", kTermsMax, K);
    return -1;
  }
  return 0;
}

// what a pattern solve without terms says to an empty-rows handle
inline void
describe_pattern_needs_terms(const char* what, uint32_t r, uint32_t count, char* msg,
                             size_t cap)
{
  snprintf(msg, cap,
           "%s: row %u is empty (%u empty rows, ST_CSR_EMPTY_ROWS_OK): its row "
           "sum would be divided by zero; such a pattern is solved with "
           "low-rank terms (st_csr_pattern_terms_create)", what, r, count);
}

// check_terms_rows on the pattern operator: s_0[i] = r[i] * sum_e c[col[e]] +
// sum_j u_j[i] (w_j . 1), finite and > 0 (summed in double here; the device
// judges the s_0 its own launch 0 computes)
template <typename T>
inline int
check_pattern_terms_rows(uint32_t n, const int64_t* row_ptr, const int32_t* col_idx,
                         const T* r, const T* c, uint32_t K, const T* const* u,
                         const T* const* w, char* msg, size_t cap)
{
  double d[kTermsMax] = { 0, 0, 0, 0 };
  for (uint32_t j = 0; j < K; j++)
    for (uint32_t i = 0; i < n; i++)
      d[j] += (double)w[j][i];
  for (uint32_t i = 0; i < n; i++) {
    double s = 0;
    for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; e++)
      s += c ? (double)c[(uint32_t)col_idx[e]] : 1.0;
    if (r)
      s *= (double)r[i];
    for (uint32_t j = 0; j < K; j++)
      s += (double)u[j][i] * d[j];
    const T st = (T)s;
    if (!(st > (T)0) || st - st != (T)0) {
      describe_term_row(i, (double)st, msg, cap);
      return -1;
    }
  }
  return 0;
}

} // namespace csr
} // namespace st
