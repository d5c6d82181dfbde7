// The host twin of the CSR transposition - transpose_host of
// eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program for the host
// sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_transpose_sanitize.cpp
//       -o csr_transpose_sanitize
//   ./csr_transpose_sanitize DIR/table0.bin DIR/table1.bin DIR/table2.bin
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz];
// the value of entry e is e (fp32) or e + 0.5 (fp64), so a value names its
// source entry.  For every matrix and both dtypes: T(A) is checked against the
// definition (t_row_ptr counts the columns below; a transposed row holds its
// column's entries in ascending storage position; t_col_idx is the source
// row), and T(T(A)) == A when A has sorted, duplicate-free rows.  Then the
// malformed variants: everything check_host refuses (same messages), a column
// without an entry (the lowest is named), nnz = 2^32 with null arrays (refused
// before any array is read), null outputs.  Exit 0 and "ok" on success.
#include <algorithm>
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
refused(int rc, const char* msg, const char* want)
{
  if (rc >= 0 || !std::strstr(msg, want)) {
    std::fprintf(stderr, "expected an error holding \"%s\", got rc=%d \"%s\"\n",
                 want, rc, msg);
    return false;
  }
  return true;
}

template <typename T>
static void
check_one(int dtype, uint32_t n, uint64_t nnz, const std::vector<int64_t>& rp,
          const std::vector<int32_t>& ci)
{
  char msg[384] = "";
  std::vector<T> va(nnz);
  for (uint64_t e = 0; e < nnz; e++)
    va[e] = (T)e + (dtype ? (T)0.5 : (T)0);
  std::vector<int64_t> tp(n + 1, -1);
  std::vector<int32_t> tc(nnz, -1);
  std::vector<T> tv(nnz, (T)-1);
  EXPECT(transpose_host(dtype, n, nnz, rp.data(), ci.data(), va.data(), tp.data(),
                        tc.data(), tv.data(), msg, sizeof(msg)) == 0);
  // the definition, entry by entry
  std::vector<uint64_t> count(n, 0);
  for (uint64_t e = 0; e < nnz; e++)
    count[(uint32_t)ci[e]]++;
  EXPECT(tp[0] == 0 && (uint64_t)tp[n] == nnz);
  for (uint32_t c = 0; c < n; c++)
    EXPECT((uint64_t)(tp[c + 1] - tp[c]) == count[c]);
  std::vector<uint32_t> row_of(nnz);
  for (uint32_t r = 0; r < n; r++)
    for (int64_t e = rp[r]; e < rp[r + 1]; e++)
      row_of[e] = r;
  int bad = 0;
  for (uint32_t c = 0; c < n; c++)
    for (int64_t i = tp[c]; i < tp[c + 1]; i++) {
      const uint64_t e = (uint64_t)(tv[i] - (dtype ? (T)0.5 : (T)0)); // its source
      bad += !(e < nnz && (uint32_t)ci[e] == c && (uint32_t)tc[i] == row_of[e]);
      if (i > tp[c]) // ascending storage position within the column
        bad += !(tv[i - 1] < tv[i]);
    }
  EXPECT(bad == 0);

  // twice: A again, when every row of A is sorted and free of duplicates
  bool sorted = true;
  for (uint32_t r = 0; r < n && sorted; r++)
    for (int64_t e = rp[r] + 1; e < rp[r + 1]; e++)
      sorted = sorted && ci[e - 1] < ci[e];
  if (sorted) { // T(A) has no empty column, as A has no empty row
    std::vector<int64_t> bp(n + 1);
    std::vector<int32_t> bc(nnz);
    std::vector<T> bv(nnz);
    EXPECT(transpose_host(dtype, n, nnz, tp.data(), tc.data(), tv.data(), bp.data(),
                          bc.data(), bv.data(), msg, sizeof(msg)) == 0);
    EXPECT(bp == rp && bc == ci && bv == va);
  }

  // malformed variants: check_host's messages, unchanged
  std::vector<int64_t> badp = rp;
  badp[0] = 1;
  EXPECT(refused(transpose_host(dtype, n, nnz, badp.data(), ci.data(), va.data(), tp.data(),
                                tc.data(), tv.data(), msg, sizeof(msg)),
                 msg, "row_ptr[0] must be 0"));
  if (n >= 3) {
    const uint32_t r = n / 2;
    const std::string row = "row " + std::to_string(r);
    badp = rp;
    badp[r + 1] = badp[r];
    EXPECT(refused(transpose_host(dtype, n, nnz, badp.data(), ci.data(), va.data(), tp.data(),
                                  tc.data(), tv.data(), msg, sizeof(msg)),
                   msg, (row + " is empty").c_str()));
    badp[r + 1] = badp[r] - 1;
    EXPECT(refused(transpose_host(dtype, n, nnz, badp.data(), ci.data(), va.data(), tp.data(),
                                  tc.data(), tv.data(), msg, sizeof(msg)),
                   msg, ("decreases at " + row).c_str()));
  }
  EXPECT(refused(transpose_host(dtype, n, nnz - 1, rp.data(), ci.data(), va.data(), tp.data(),
                                tc.data(), tv.data(), msg, sizeof(msg)),
                 msg, "row_ptr[n] must be nnz"));
  for (int32_t c : { (int32_t)n, -1 }) {
    std::vector<int32_t> badc = ci;
    badc[nnz - 1] = c;
    EXPECT(refused(transpose_host(dtype, n, nnz, rp.data(), badc.data(), va.data(), tp.data(),
                                  tc.data(), tv.data(), msg, sizeof(msg)),
                   msg, ("of entry " + std::to_string(nnz - 1) + " (row " +
                         std::to_string(n - 1) + ")").c_str()));
  }
  EXPECT(refused(transpose_host(2, n, nnz, rp.data(), ci.data(), va.data(), tp.data(),
                                tc.data(), tv.data(), msg, sizeof(msg)), msg, "dtype"));
  EXPECT(refused(transpose_host(dtype, 0, nnz, rp.data(), ci.data(), va.data(), tp.data(),
                                tc.data(), tv.data(), msg, sizeof(msg)), msg, "n must be"));
  EXPECT(refused(transpose_host(dtype, n, nnz, nullptr, ci.data(), va.data(), tp.data(),
                                tc.data(), tv.data(), msg, sizeof(msg)), msg, "null"));
  EXPECT(refused(transpose_host(dtype, n, nnz, rp.data(), ci.data(), va.data(), nullptr,
                                tc.data(), tv.data(), msg, sizeof(msg)), msg, "null t_row_ptr"));
  // nnz = 2^32: refused by name before any array is read (there is none)
  EXPECT(refused(transpose_host(dtype, n, 1ull << 32, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, msg, sizeof(msg)), msg, "below 2^32"));
  // empty columns: every entry of columns lo and hi moves to another column
  // that exists; the LOWEST empty column is named
  if (n >= 4) {
    const int32_t lo = (int32_t)(n / 3), hi = (int32_t)(n - 1);
    std::vector<int32_t> badc = ci;
    for (auto& c : badc)
      if (c == lo || c == hi)
        c = 0;
    EXPECT(refused(transpose_host(dtype, n, nnz, rp.data(), badc.data(), va.data(), tp.data(),
                                  tc.data(), tv.data(), msg, sizeof(msg)),
                   msg, ("column " + std::to_string(lo) + " has no entry").c_str()));
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
  const uint32_t n = (uint32_t)hdr[0];
  const uint64_t nnz = (uint64_t)hdr[1];
  std::vector<int64_t> rp(n + 1);
  std::vector<int32_t> ci(nnz);
  EXPECT(std::fread(rp.data(), 8, n + 1, f) == n + 1);
  EXPECT(std::fread(ci.data(), 4, nnz, f) == nnz);
  std::fclose(f);
  check_one<float>(0, n, nnz, rp, ci);
  check_one<double>(1, n, nnz, rp, ci);
  std::printf("%s: n = %u, nnz = %llu transposed\n", path, n, (unsigned long long)nnz);
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
