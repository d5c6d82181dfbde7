// The host side of the CSR solve on a product operator B A - the validation
// of two triples and of the rows of the product in
// eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program for the host
// sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   make csr_product_sanitize               # builds with
//       -fsanitize=address,undefined and runs it on those files
// or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_product_sanitize.cpp
//       -o csr_product_sanitize
//   ./csr_product_sanitize DIR/table0.bin DIR/table1.bin DIR/table2.bin
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz];
// every value is 0.5.  Each matrix A is paired with itself (A^2) and with its
// host transposition (A^T A and A A^T), in both dtypes, and then with its
// malformed variants: a factor with a bad column, a decreasing row_ptr or a
// wrong nnz (the factor is named, B before A); B with an empty row; A with
// rows emptied with and without the flag; a row of B whose columns all hit
// emptied rows of A, and one whose values there are all zero (the lowest such
// row is named); the Gram side.  Exit 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static int
product(int dtype, const Csr& b, const std::vector<T>& vb, const Csr& a,
        const std::vector<T>& va, uint32_t flags, char* msg, size_t cap)
{
  std::vector<unsigned char> pos(a.n);
  return check_product_host(dtype, a.n, b.nnz(), b.rp.data(), b.ci.data(), vb.data(),
                            a.nnz(), a.rp.data(), a.ci.data(), va.data(), flags,
                            pos.data(), msg, cap);
}

template <typename T>
static void
check_pair(int dtype, const Csr& a)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  const std::vector<T> va(a.nnz(), (T)0.5);
  // A^2
  EXPECT(product<T>(dtype, a, va, a, va, 0, msg, sizeof(msg)) == 0);
  // A^T A and A A^T on the host transposition
  Csr t;
  t.n = n;
  t.rp.resize(n + 1);
  t.ci.resize(a.nnz());
  std::vector<T> vt(a.nnz());
  EXPECT(transpose_host(dtype, n, a.nnz(), a.rp.data(), a.ci.data(), va.data(),
                        t.rp.data(), t.ci.data(), vt.data(), msg, sizeof(msg),
                        kEmptyRowsOk) == 0);
  uint32_t lowest = 0;
  if (count_empty_rows(t.rp.data(), n, &lowest) == 0) {
    EXPECT(product<T>(dtype, t, vt, a, va, 0, msg, sizeof(msg)) == 0);
  } else { // an empty column of A: an empty row of the left factor
    EXPECT(refused(product<T>(dtype, t, vt, a, va, 0, msg, sizeof(msg)), msg,
                   "factor B: row " + std::to_string(lowest) + " is empty"));
  }
  EXPECT(product<T>(dtype, a, va, t, vt, kEmptyRowsOk, msg, sizeof(msg)) == 0);

  // malformed factors: B is judged before A
  Csr bad = a;
  bad.ci[a.nnz() / 2] = (int32_t)n;
  EXPECT(refused(product<T>(dtype, bad, va, a, va, 0, msg, sizeof(msg)), msg,
                 "csr product: factor B: column index " + std::to_string(n)));
  EXPECT(refused(product<T>(dtype, a, va, bad, va, 0, msg, sizeof(msg)), msg,
                 "csr product: factor A: column index " + std::to_string(n)));
  Csr down = a;
  down.rp[n / 2 + 1] = down.rp[n / 2] - 1;
  EXPECT(refused(product<T>(dtype, down, va, bad, va, 0, msg, sizeof(msg)), msg,
                 "factor B: row_ptr decreases at row " + std::to_string(n / 2)));
  EXPECT(refused(product<T>(dtype, a, va, down, va, kEmptyRowsOk, msg, sizeof(msg)), msg,
                 "factor A: row_ptr decreases at row " + std::to_string(n / 2)));
  {
    std::vector<unsigned char> pos(n);
    EXPECT(refused(check_product_host(dtype, n, a.nnz() + 1, a.rp.data(), a.ci.data(),
                                      va.data(), a.nnz(), a.rp.data(), a.ci.data(),
                                      va.data(), 0, pos.data(), msg, sizeof(msg)),
                   msg, "factor B: row_ptr[n] must be nnz"));
    EXPECT(refused(check_product_host(2, n, a.nnz(), a.rp.data(), a.ci.data(), va.data(),
                                      a.nnz(), a.rp.data(), a.ci.data(), va.data(), 0,
                                      pos.data(), msg, sizeof(msg)),
                   msg, "dtype must be 0 (f32) or 1 (f64)"));
    EXPECT(refused(check_product_host(dtype, n, a.nnz(), a.rp.data(), a.ci.data(),
                                      va.data(), a.nnz(), a.rp.data(), a.ci.data(),
                                      nullptr, 0, pos.data(), msg, sizeof(msg)),
                   msg, "factor A: null row_ptr / col_idx / vals"));
    EXPECT(refused(check_product_host(dtype, n, a.nnz(), a.rp.data(), a.ci.data(),
                                      va.data(), a.nnz(), a.rp.data(), a.ci.data(),
                                      va.data(), 0, nullptr, msg, sizeof(msg)),
                   msg, "null scratch"));
  }

  // empty rows: never in B; in A only under the flag
  const Csr e = emptied(a, { 0, 1, n / 2, n / 2 + 1, n - 1 });
  const std::vector<T> ve(e.nnz(), (T)0.5);
  EXPECT(refused(product<T>(dtype, e, ve, a, va, kEmptyRowsOk, msg, sizeof(msg)), msg,
                 "factor B: row 0 is empty"));
  EXPECT(refused(product<T>(dtype, a, va, e, ve, 0, msg, sizeof(msg)), msg,
                 "factor A: row 0 is empty"));
  EXPECT(product<T>(dtype, a, va, e, ve, kEmptyRowsOk, msg, sizeof(msg)) == 0 ||
         std::strstr(msg, "has no positive entry"));

  // a row of B whose columns all hit emptied rows of A: rows r1 < r2 of B,
  // every row of A they point at emptied; the lowest is named
  const uint32_t r1 = n / 3, r2 = n - 1;
  std::vector<uint32_t> hit;
  for (uint32_t r : { r1, r2 })
    for (int64_t k = a.rp[r]; k < a.rp[r + 1]; k++)
      hit.push_back((uint32_t)a.ci[k]);
  if (hit.size() < n) { // the full row of the heavy table would empty all of A
    const Csr h = emptied(a, hit);
    const std::vector<T> vh(h.nnz(), (T)0.5);
    if (h.nnz() >= 1) {
      EXPECT(refused(product<T>(dtype, a, va, h, vh, kEmptyRowsOk, msg, sizeof(msg)), msg,
                     "csr product: row "));
      // the lowest row of B all of whose columns are emptied rows of A
      std::vector<bool> gone(n, false);
      for (uint32_t c : hit)
        gone[c] = true;
      uint32_t low = n;
      for (uint32_t r = 0; r < n && low == n; r++) {
        bool any = false;
        for (int64_t k = a.rp[r]; k < a.rp[r + 1]; k++)
          any |= !gone[(uint32_t)a.ci[k]];
        if (!any)
          low = r;
      }
      EXPECT(low <= r1);
      EXPECT(refused(product<T>(dtype, a, va, h, vh, kEmptyRowsOk, msg, sizeof(msg)), msg,
                     "row " + std::to_string(low) + " of B·A has no positive entry"));
    }
  }
  // zeros count as no entry: row r1 of B all zero, then only its hits in A zero
  {
    std::vector<T> vz = va;
    for (int64_t k = a.rp[r1]; k < a.rp[r1 + 1]; k++)
      vz[k] = (T)0;
    const int rc = product<T>(dtype, a, vz, a, va, 0, msg, sizeof(msg));
    EXPECT(refused(rc, msg, "row " + std::to_string(r1) + " of B·A has no positive entry"));
    // a zero row of A alone is no offence: every row of the tables holds two
    // distinct columns at the least
    EXPECT(product<T>(dtype, a, va, a, vz, 0, msg, sizeof(msg)) == 0);
  }
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
  check_pair<float>(0, a);
  check_pair<double>(1, a);
  std::printf("%s: n = %u, nnz = %llu checked\n", path, a.n, (unsigned long long)nnz);
}

int
main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s MATRIX.bin ...\n", argv[0]);
    return 2;
  }
  char msg[384] = "";
  EXPECT(check_gram_side(0, msg, sizeof(msg)) == 0 && check_gram_side(1, msg, sizeof(msg)) == 0);
  EXPECT(refused(check_gram_side(2, msg, sizeof(msg)), msg, "side must be 0"));
  describe_product_row(17, msg, sizeof(msg));
  EXPECT(std::strstr(msg, "row 17 of B·A has no positive entry"));
  for (int i = 1; i < argc; i++)
    one(argv[i]);
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("ok");
  return 0;
}
