// The host side of the CSR solve with low-rank terms and empty rows - the
// flagged checks, the plan, the flagged transposition and the terms
// validation of eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program
// for the host sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   make csr_terms_sanitize                 # builds with
//       -fsanitize=address,undefined and runs it on those files
// or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_terms_sanitize.cpp
//       -o csr_terms_sanitize
//   ./csr_terms_sanitize DIR/table0.bin DIR/table1.bin DIR/table2.bin
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz];
// the value of entry e is e + 1.  Every matrix is taken as it is and with
// rows emptied at both ends and in the middle (rows 0, 1, n / 2, n / 2 + 1,
// n - 1), in both dtypes: the unflagged checks refuse the lowest empty row
// with the text they always had, the flagged ones pass; the plan puts the
// empty rows into class 0 in row order; the flagged transposition is checked
// against its definition entry by entry (empty columns become empty rows) and
// T(T(A)) == A; the terms validation names the lowest (term, vector, index)
// and the lowest row of A + sum u w^T without a positive entry.  Exit 0 and
// "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "st_csr_host.h"

using namespace st::csr;

static int g_fail = 0;
#define EXPECT(cond)                                                           \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__,   \
                   #cond);                                                     \
      g_fail++;                                                                \
    }                                                                          \
  } while (0)

static bool
refused(int rc, const char* msg, const std::string& want)
{
  if (rc >= 0 || !std::strstr(msg, want.c_str())) {
    std::fprintf(stderr, "expected an error holding \"%s\", got rc=%d \"%s\"\n",
                 want.c_str(), rc, msg);
    return false;
  }
  return true;
}

struct Csr
{
  uint32_t n;
  std::vector<int64_t> rp;
  std::vector<int32_t> ci;
  uint64_t nnz() const { return ci.size(); }
};

static Csr
emptied(const Csr& a, const std::vector<uint32_t>& rows)
{
  std::vector<bool> drop(a.n, false);
  for (uint32_t r : rows)
    if (r < a.n)
      drop[r] = true;
  Csr b;
  b.n = a.n;
  b.rp.assign(1, 0);
  for (uint32_t r = 0; r < a.n; r++) {
    if (!drop[r])
      for (int64_t e = a.rp[r]; e < a.rp[r + 1]; e++)
        b.ci.push_back(a.ci[e]);
    b.rp.push_back((int64_t)b.ci.size());
  }
  return b;
}

template <typename T>
static void
check_transpose(int dtype, const Csr& a)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  const uint64_t nnz = a.nnz();
  std::vector<T> va(nnz);
  for (uint64_t e = 0; e < nnz; e++)
    va[e] = (T)(e + 1);
  std::vector<int64_t> tp(n + 1, -1);
  std::vector<int32_t> tc(nnz, -1);
  std::vector<T> tv(nnz, (T)-1);
  EXPECT(transpose_host(dtype, n, nnz, a.rp.data(), a.ci.data(), va.data(), tp.data(),
                        tc.data(), tv.data(), msg, sizeof(msg), kEmptyRowsOk) == 0);
  std::vector<uint64_t> count(n, 0);
  for (uint64_t e = 0; e < nnz; e++)
    count[(uint32_t)a.ci[e]]++;
  EXPECT(tp[0] == 0 && (uint64_t)tp[n] == nnz);
  for (uint32_t c = 0; c < n; c++)
    EXPECT((uint64_t)(tp[c + 1] - tp[c]) == count[c]);
  std::vector<uint32_t> row_of(nnz);
  for (uint32_t r = 0; r < n; r++)
    for (int64_t e = a.rp[r]; e < a.rp[r + 1]; e++)
      row_of[e] = r;
  int bad = 0;
  for (uint32_t c = 0; c < n; c++)
    for (int64_t i = tp[c]; i < tp[c + 1]; i++) {
      const uint64_t e = (uint64_t)tv[i] - 1; // its source
      bad += !(e < nnz && (uint32_t)a.ci[e] == c && (uint32_t)tc[i] == row_of[e]);
      if (i > tp[c]) // ascending storage position within the column
        bad += !(tv[i - 1] < tv[i]);
    }
  EXPECT(bad == 0);
  // twice: A again (the table's rows are sorted and free of duplicates)
  std::vector<int64_t> bp(n + 1);
  std::vector<int32_t> bc(nnz);
  std::vector<T> bv(nnz);
  EXPECT(transpose_host(dtype, n, nnz, tp.data(), tc.data(), tv.data(), bp.data(),
                        bc.data(), bv.data(), msg, sizeof(msg), kEmptyRowsOk) == 0);
  EXPECT(bp == a.rp && bc == a.ci && bv == va);
  // the plan of the transposed matrix, empty rows included
  std::vector<uint32_t> order(n, 0xffffffffu);
  uint32_t cf[kClasses + 1];
  EXPECT(plan(tp.data(), n, order.data(), cf, msg, sizeof(msg), true) >= 1);
  EXPECT(cf[0] == 0 && cf[kClasses] == n);
}

template <typename T>
static void
check_terms(const Csr& a, bool has_empty)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  std::vector<T> va(a.nnz(), (T)0.5);
  std::vector<std::vector<T>> u(kTermsMax, std::vector<T>(n, (T)0.25)),
    w(kTermsMax, std::vector<T>(n, (T)0.125));
  const T* up[kTermsMax];
  const T* wp[kTermsMax];
  for (uint32_t j = 0; j < kTermsMax; j++) {
    up[j] = u[j].data();
    wp[j] = w[j].data();
  }
  EXPECT(refused(check_terms_count(0, msg, sizeof(msg)), msg, "K must be in [1, 4], got 0"));
  EXPECT(refused(check_terms_count(kTermsMax + 1, msg, sizeof(msg)), msg, "got 5"));
  for (uint32_t K = 1; K <= kTermsMax; K++) {
    EXPECT(check_terms_count(K, msg, sizeof(msg)) == 0);
    EXPECT(check_terms_vectors<T>(n, K, up, wp, msg, sizeof(msg)) == 0);
    EXPECT(check_terms_rows<T>(n, a.rp.data(), va.data(), K, up, wp, msg, sizeof(msg)) == 0);
  }
  // the lowest (term, u before w, index)
  const uint32_t at = n - 1;
  const T bads[3] = { (T)-1, std::numeric_limits<T>::quiet_NaN(),
                      std::numeric_limits<T>::infinity() };
  for (T b : bads) {
    w[1][at] = b;
    u[2][0] = b;
    EXPECT(refused(check_terms_vectors<T>(n, 3, up, wp, msg, sizeof(msg)), msg,
                   "w_1[" + std::to_string(at) + "]"));
    EXPECT(check_terms_vectors<T>(n, 1, up, wp, msg, sizeof(msg)) == 0);
    u[1][at] = b;
    EXPECT(refused(check_terms_vectors<T>(n, 3, up, wp, msg, sizeof(msg)), msg,
                   "u_1[" + std::to_string(at) + "]"));
    w[1][at] = (T)0.125;
    u[2][0] = u[1][at] = (T)0.25;
  }
  const T* nul[kTermsMax] = { up[0], nullptr, up[2], up[3] };
  EXPECT(refused(check_terms_vectors<T>(n, 2, nul, wp, msg, sizeof(msg)), msg, "null u_1"));
  // rows of the operator: u = 0 at an empty row leaves it without an entry
  if (has_empty) {
    u[0][n / 2] = (T)0;
    EXPECT(refused(check_terms_rows<T>(n, a.rp.data(), va.data(), 1, up, wp, msg, sizeof(msg)),
                   msg, "row " + std::to_string(n / 2) + " of A + "));
    u[0][0] = (T)0;
    EXPECT(refused(check_terms_rows<T>(n, a.rp.data(), va.data(), 1, up, wp, msg, sizeof(msg)),
                   msg, "row 0 of A + "));
    EXPECT(check_terms_rows<T>(n, a.rp.data(), va.data(), 2, up, wp, msg, sizeof(msg)) == 0);
  }
}

static void
check_matrix(const Csr& a, bool has_empty)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  const uint64_t nnz = a.nnz();
  std::vector<float> vf(nnz, 1.0f);
  uint32_t lowest = 0;
  const uint32_t k = count_empty_rows(a.rp.data(), n, &lowest);
  EXPECT((k != 0) == has_empty && lowest == (has_empty ? 0u : n));
  if (has_empty) {
    EXPECT(refused(check_host(0, n, nnz, a.rp.data(), a.ci.data(), vf.data(), msg, sizeof(msg)),
                   msg, "row 0 is empty"));
    EXPECT(refused(plan(a.rp.data(), n, nullptr, nullptr, msg, sizeof(msg)), msg,
                   "row 0 is empty"));
    describe_needs_terms("st_solve_csr", lowest, k, msg, sizeof(msg));
    EXPECT(std::strstr(msg, "row 0 is empty") && std::strstr(msg, "low-rank terms"));
  } else {
    EXPECT(check_host(0, n, nnz, a.rp.data(), a.ci.data(), vf.data(), msg, sizeof(msg)) == 0);
  }
  EXPECT(check_host(0, n, nnz, a.rp.data(), a.ci.data(), vf.data(), msg, sizeof(msg), true) == 0);
  // the flag does not let row_ptr decrease, start off 0 or end off nnz
  std::vector<int64_t> badp = a.rp;
  badp[n / 2 + 1] = badp[n / 2] - 1;
  EXPECT(refused(check_host(0, n, nnz, badp.data(), a.ci.data(), vf.data(), msg, sizeof(msg), true),
                 msg, "decreases at row " + std::to_string(n / 2)));
  badp = a.rp;
  badp[0] = 1;
  EXPECT(refused(check_host(0, n, nnz, badp.data(), a.ci.data(), vf.data(), msg, sizeof(msg), true),
                 msg, "row_ptr[0] must be 0"));
  EXPECT(refused(check_host(0, n, nnz + 1, a.rp.data(), a.ci.data(), vf.data(), msg, sizeof(msg),
                            true),
                 msg, "row_ptr[n] must be nnz"));
  std::vector<int64_t> zero(n + 1, 0);
  EXPECT(refused(check_host(0, n, 0, zero.data(), a.ci.data(), vf.data(), msg, sizeof(msg), true),
                 msg, "nnz must be >= 1"));
  // the plan: stable within a class, an empty row in class 0
  std::vector<uint32_t> order(n, 0xffffffffu);
  uint32_t cf[kClasses + 1];
  EXPECT(plan(a.rp.data(), n, order.data(), cf, msg, sizeof(msg), true) >= 1);
  EXPECT(cf[0] == 0 && cf[kClasses] == n);
  std::vector<bool> seen(n, false);
  for (int c = 0; c < kClasses; c++)
    for (uint32_t i = cf[c]; i < cf[c + 1]; i++) {
      const uint32_t r = order[i];
      EXPECT(r < n && !seen[r]);
      if (r >= n)
        continue;
      seen[r] = true;
      EXPECT(row_class((uint64_t)(a.rp[r + 1] - a.rp[r])) == c);
      EXPECT(i == cf[c] || order[i - 1] < r);
    }
  if (has_empty)
    EXPECT(order[0] == 0 && row_class(0) == 0);
  check_transpose<float>(0, a);
  check_transpose<double>(1, a);
  check_terms<float>(a, has_empty);
  check_terms<double>(a, has_empty);
}

static void
one(const char* path)
{
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    g_fail++;
    return;
  }
  int64_t hdr[2];
  EXPECT(std::fread(hdr, 8, 2, f) == 2);
  Csr a;
  a.n = (uint32_t)hdr[0];
  const uint64_t nnz = (uint64_t)hdr[1];
  a.rp.resize(a.n + 1);
  a.ci.resize(nnz);
  EXPECT(std::fread(a.rp.data(), 8, a.n + 1, f) == a.n + 1);
  EXPECT(std::fread(a.ci.data(), 4, nnz, f) == nnz);
  std::fclose(f);
  check_matrix(a, false);
  const Csr b = emptied(a, { 0, 1, a.n / 2, a.n / 2 + 1, a.n - 1 });
  check_matrix(b, true);
  std::printf("%s: n = %u, nnz = %llu / %llu checked\n", path, a.n,
              (unsigned long long)nnz, (unsigned long long)b.nnz());
}

int
main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s MATRIX.bin ...\n", argv[0]);
    return 2;
  }
  for (int i = 1; i < argc; i++)
    one(argv[i]);
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("ok");
  return 0;
}
