// Host code of the sparse (CSR) solve - the plan and the host validation of
// eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program for the host
// sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_sanitize.cpp -o csr_sanitize
//   ./csr_sanitize DIR/table0.bin DIR/table1.bin DIR/table2.bin
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz].
// For every matrix: the validation passes, the plan is a stable partition by
// class; then the malformed variants (row_ptr[0] != 0, an empty row, a
// decreasing row_ptr, row_ptr[n] != nnz, a column of n and of -1, a bad dtype,
// n = 0) are each refused with the row or entry named.  Exit 0 and "ok" on
// success.
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
  std::vector<float> va(nnz, 1.f);
  EXPECT(std::fread(rp.data(), 8, n + 1, f) == n + 1);
  EXPECT(std::fread(ci.data(), 4, nnz, f) == nnz);
  std::fclose(f);
  char msg[384] = "";

  EXPECT(check_host(0, n, nnz, rp.data(), ci.data(), va.data(), msg, sizeof(msg)) == 0);
  std::vector<uint32_t> order(n);
  uint32_t first[kClasses + 1];
  const int used = plan(rp.data(), n, order.data(), first, msg, sizeof(msg));
  EXPECT(used >= 1 && first[0] == 0 && first[kClasses] == n);
  std::vector<char> seen(n, 0);
  for (int c = 0; c < kClasses; c++)
    for (uint32_t i = first[c]; i < first[c + 1]; i++) {
      const uint32_t r = order[i];
      EXPECT(r < n && !seen[r]);
      seen[r] = 1;
      EXPECT(row_class((uint64_t)(rp[r + 1] - rp[r])) == c);
      EXPECT(i == first[c] || order[i - 1] < r); // row order kept
    }

  // malformed variants of this matrix
  std::vector<int64_t> bad = rp;
  bad[0] = 1;
  EXPECT(refused(check_host(0, n, nnz, bad.data(), ci.data(), va.data(), msg, sizeof(msg)),
                 msg, "row_ptr[0] must be 0"));
  EXPECT(refused(plan(bad.data(), n, order.data(), first, msg, sizeof(msg)), msg,
                 "row_ptr[0] must be 0"));
  if (n >= 3) {
    const uint32_t r = n / 2;
    const std::string row = "row " + std::to_string(r);
    bad = rp;
    bad[r + 1] = bad[r];
    EXPECT(refused(check_host(0, n, nnz, bad.data(), ci.data(), va.data(), msg, sizeof(msg)),
                   msg, (row + " is empty").c_str()));
    EXPECT(refused(plan(bad.data(), n, order.data(), first, msg, sizeof(msg)), msg,
                   (row + " is empty").c_str()));
    bad[r + 1] = bad[r] - 1;
    EXPECT(refused(check_host(0, n, nnz, bad.data(), ci.data(), va.data(), msg, sizeof(msg)),
                   msg, ("decreases at " + row).c_str()));
    EXPECT(refused(plan(bad.data(), n, order.data(), first, msg, sizeof(msg)), msg,
                   ("decreases at " + row).c_str()));
  }
  EXPECT(refused(check_host(0, n, nnz - 1, rp.data(), ci.data(), va.data(), msg, sizeof(msg)),
                 msg, "row_ptr[n] must be nnz"));
  for (int32_t c : { (int32_t)n, -1 }) {
    std::vector<int32_t> badc = ci;
    const uint64_t e = nnz - 1; // the last entry: the lookup ends in the last row
    badc[e] = c;
    EXPECT(refused(check_host(1, n, nnz, rp.data(), badc.data(), va.data(), msg, sizeof(msg)),
                   msg, ("of entry " + std::to_string(e) + " (row " + std::to_string(n - 1) + ")").c_str()));
    badc = ci;
    badc[0] = c;
    EXPECT(refused(check_host(1, n, nnz, rp.data(), badc.data(), va.data(), msg, sizeof(msg)),
                   msg, "of entry 0 (row 0)"));
  }
  EXPECT(refused(check_host(2, n, nnz, rp.data(), ci.data(), va.data(), msg, sizeof(msg)), msg,
                 "dtype"));
  EXPECT(refused(check_host(0, 0, nnz, rp.data(), ci.data(), va.data(), msg, sizeof(msg)), msg,
                 "n must be"));
  EXPECT(refused(check_host(0, n, nnz, nullptr, ci.data(), va.data(), msg, sizeof(msg)), msg,
                 "null"));
  std::printf("%s: n = %u, nnz = %llu, %d classes in use\n", path, n,
              (unsigned long long)nnz, used);
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
