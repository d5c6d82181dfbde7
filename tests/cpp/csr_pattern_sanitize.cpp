// The host side of the pattern-only operator diag(r) P diag(c) - the scales'
// predicate and messages, the host check of a pattern, the terms count and
// the rows of the operator with terms, all of
// eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program for the host
// sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   make csr_pattern_sanitize               # builds with
//       -fsanitize=address,undefined and runs it on those files
// or by hand:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_pattern_sanitize.cpp
//       -o csr_pattern_sanitize
//   ./csr_pattern_sanitize DIR/table0.bin DIR/table1.bin DIR/table2.bin
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz].
// Every matrix is taken as it is and with rows emptied at both ends and in
// the middle, in both dtypes: check_pattern_host agrees with check_host on
// the same arrays with values, the scales are refused at the lowest index,
// row_scale before col_scale, with the value printed; null scales pass; the
// rows of the operator with terms name the lowest row without a positive
// entry.  Exit 0 and "ok" on success.
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
check_scales(const Csr& a)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  std::vector<T> r(n, (T)0.5), c(n, (T)2);
  EXPECT(check_pattern_scales<T>(n, nullptr, nullptr, msg, sizeof(msg)) == 0);
  EXPECT(check_pattern_scales<T>(n, r.data(), nullptr, msg, sizeof(msg)) == 0);
  EXPECT(check_pattern_scales<T>(n, nullptr, c.data(), msg, sizeof(msg)) == 0);
  EXPECT(check_pattern_scales<T>(n, r.data(), c.data(), msg, sizeof(msg)) == 0);
  // the smallest subnormal and the largest finite value are positive and finite
  r[0] = std::numeric_limits<T>::denorm_min();
  c[n - 1] = std::numeric_limits<T>::max();
  EXPECT(check_pattern_scales<T>(n, r.data(), c.data(), msg, sizeof(msg)) == 0);
  const uint32_t at = n / 2;
  const T bads[5] = { (T)0, (T)-0.5, std::numeric_limits<T>::quiet_NaN(),
                      std::numeric_limits<T>::infinity(),
                      -std::numeric_limits<T>::infinity() };
  const char* shown[5] = { "= 0 ", "= -0.5 ", "= nan ", "= inf ", "= -inf " };
  for (int i = 0; i < 5; i++) {
    EXPECT(scale_entry_bad<T>(bads[i]));
    // col_scale alone, the lowest of two
    c[at] = bads[i];
    c[n - 1] = bads[i];
    EXPECT(refused(check_pattern_scales<T>(n, r.data(), c.data(), msg, sizeof(msg)), msg,
                   "col_scale[" + std::to_string(at) + "] " + shown[i]));
    EXPECT(std::strstr(msg, "is not finite and positive") != nullptr);
    // row_scale before col_scale, whatever the index
    r[n - 1] = bads[i];
    EXPECT(refused(check_pattern_scales<T>(n, r.data(), c.data(), msg, sizeof(msg)), msg,
                   "row_scale[" + std::to_string(n - 1) + "] " + shown[i]));
    // a null row_scale is not looked at
    EXPECT(refused(check_pattern_scales<T>(n, nullptr, c.data(), msg, sizeof(msg)), msg,
                   "col_scale[" + std::to_string(at) + "]"));
    r[n - 1] = (T)0.5;
    c[at] = (T)2;
    c[n - 1] = (T)2;
  }
  EXPECT(!scale_entry_bad<T>((T)1) && !scale_entry_bad<T>(std::numeric_limits<T>::min()));
}

template <typename T>
static void
check_rows(const Csr& a, bool has_empty)
{
  char msg[384] = "";
  const uint32_t n = a.n;
  std::vector<T> r(n, (T)0.5), c(n, (T)2);
  std::vector<std::vector<T>> u(kTermsMax, std::vector<T>(n, (T)0.25)),
    w(kTermsMax, std::vector<T>(n, (T)0.125));
  const T* up[kTermsMax];
  const T* wp[kTermsMax];
  for (uint32_t j = 0; j < kTermsMax; j++) {
    up[j] = u[j].data();
    wp[j] = w[j].data();
  }
  EXPECT(check_pattern_terms_count(0, msg, sizeof(msg)) == 0);
  EXPECT(check_pattern_terms_count(kTermsMax, msg, sizeof(msg)) == 0);
  EXPECT(refused(check_pattern_terms_count(kTermsMax + 1, msg, sizeof(msg)), msg,
                 "K must be in [0, 4], got 5"));
  for (uint32_t K = 1; K <= kTermsMax; K++)
    for (int sc = 0; sc < 4; sc++)
      EXPECT(check_pattern_terms_rows<T>(n, a.rp.data(), a.ci.data(),
                                         (sc & 1) ? r.data() : nullptr,
                                         (sc & 2) ? c.data() : nullptr, K, up, wp, msg,
                                         sizeof(msg)) == 0);
  // without terms (K = 0) an empty row has no positive entry
  const int rc0 = check_pattern_terms_rows<T>(n, a.rp.data(), a.ci.data(), r.data(), c.data(),
                                              0, up, wp, msg, sizeof(msg));
  if (has_empty)
    EXPECT(refused(rc0, msg, "row 0 of A + "));
  else
    EXPECT(rc0 == 0);
  if (has_empty) {
    u[0][n / 2] = (T)0;
    EXPECT(refused(check_pattern_terms_rows<T>(n, a.rp.data(), a.ci.data(), r.data(), c.data(),
                                               1, up, wp, msg, sizeof(msg)),
                   msg, "row " + std::to_string(n / 2) + " of A + "));
    u[0][0] = (T)0;
    EXPECT(refused(check_pattern_terms_rows<T>(n, a.rp.data(), a.ci.data(), nullptr, nullptr,
                                               1, up, wp, msg, sizeof(msg)),
                   msg, "row 0 of A + "));
    EXPECT(check_pattern_terms_rows<T>(n, a.rp.data(), a.ci.data(), r.data(), c.data(), 2, up,
                                       wp, msg, sizeof(msg)) == 0);
    uint32_t lowest = 0;
    const uint32_t k = count_empty_rows(a.rp.data(), n, &lowest);
    describe_pattern_needs_terms("st_solve_csr_pattern", lowest, k, msg, sizeof(msg));
    EXPECT(std::strstr(msg, "st_solve_csr_pattern: row 0 is empty") &&
           std::strstr(msg, "st_csr_pattern_terms_create"));
  }
}

static void
check_matrix(const Csr& a, bool has_empty)
{
  char msg[384] = "", ref[384] = "";
  const uint32_t n = a.n;
  const uint64_t nnz = a.nnz();
  std::vector<float> vf(nnz, 1.0f);
  // check_pattern_host is check_host without the values: same verdict, same text
  for (int flag = 0; flag < 2; flag++) {
    const int want = check_host(0, n, nnz, a.rp.data(), a.ci.data(), vf.data(), ref,
                                sizeof(ref), flag != 0);
    const int got = check_pattern_host(0, n, nnz, a.rp.data(), a.ci.data(), msg, sizeof(msg),
                                       flag != 0);
    EXPECT(got == want && (got == 0 || std::strcmp(msg, ref) == 0));
    EXPECT((got == 0) == (!has_empty || flag != 0));
  }
  EXPECT(refused(check_pattern_host(2, n, nnz, a.rp.data(), a.ci.data(), msg, sizeof(msg)), msg,
                 "dtype must be 0 (f32) or 1 (f64), got 2"));
  EXPECT(refused(check_pattern_host(0, 0, nnz, a.rp.data(), a.ci.data(), msg, sizeof(msg)), msg,
                 "n must be in [1, 2^31)"));
  EXPECT(refused(check_pattern_host(0, n, nnz, nullptr, a.ci.data(), msg, sizeof(msg)), msg,
                 "null row_ptr / col_idx"));
  EXPECT(refused(check_pattern_host(1, n, nnz, a.rp.data(), nullptr, msg, sizeof(msg)), msg,
                 "null row_ptr / col_idx"));
  std::vector<int64_t> badp = a.rp;
  badp[n / 2 + 1] = badp[n / 2] - 1;
  EXPECT(refused(check_pattern_host(0, n, nnz, badp.data(), a.ci.data(), msg, sizeof(msg), true),
                 msg, "decreases at row " + std::to_string(n / 2)));
  EXPECT(refused(check_pattern_host(0, n, nnz + 1, a.rp.data(), a.ci.data(), msg, sizeof(msg),
                                    true),
                 msg, "row_ptr[n] must be nnz"));
  std::vector<int64_t> zero(n + 1, 0);
  EXPECT(refused(check_pattern_host(0, n, 0, zero.data(), a.ci.data(), msg, sizeof(msg), true),
                 msg, "nnz must be >= 1"));
  std::vector<int32_t> badc = a.ci;
  badc[nnz - 1] = (int32_t)n;
  EXPECT(refused(check_pattern_host(0, n, nnz, a.rp.data(), badc.data(), msg, sizeof(msg), true),
                 msg, "column index " + std::to_string(n) + " of entry " +
                        std::to_string(nnz - 1)));
  badc[nnz - 1] = -1;
  EXPECT(refused(check_pattern_host(0, n, nnz, a.rp.data(), badc.data(), msg, sizeof(msg), true),
                 msg, "column index -1"));
  check_scales<float>(a);
  check_scales<double>(a);
  check_rows<float>(a, has_empty);
  check_rows<double>(a, has_empty);
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
