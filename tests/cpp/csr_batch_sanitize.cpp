// Host validation of a batch in stacked CSR storage - check_batch_host and
// its parts in eigen_value_amd/csrc/st_csr_host.h - as a stand-alone program
// for the host sanitizers (no HIP, no Python, no input file):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/csr_batch_sanitize.cpp
//       -o csr_batch_sanitize
//   ./csr_batch_sanitize
//
// It stacks matrices of n = 1, 2, 5, 64, 257, 300 and 1 rows (row lengths
// from a small generator, columns local to each matrix, the largest legal
// column in every matrix's last row), checks that the batch passes and that
// the plan of the stacked row_ptr is a stable partition by class, and then
// that each malformed variant is refused with its matrix and local row or
// entry named: bad dtype, batch = 0, null mat_first, mat_first[0] != 0, a
// non-increasing mat_first, N >= 2^31, a wrong mat_first[batch] (seen as
// row_ptr[N] != nnz), row_ptr[0] != 0, an empty row, a decreasing row_ptr, a
// wrong nnz, a column equal to n_b that is still below N (the cross-matrix
// case), a column of -1, null arrays.  Exit 0 and "ok" on success.
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

int
main()
{
  const uint32_t dims[] = { 1, 2, 5, 64, 257, 300, 1 };
  const uint32_t batch = sizeof(dims) / sizeof(dims[0]);
  std::vector<uint32_t> mf(batch + 1, 0);
  std::vector<int64_t> rp(1, 0);
  std::vector<int32_t> ci;
  uint32_t seed = 12345u;
  auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
  for (uint32_t b = 0; b < batch; b++) {
    const uint32_t n = dims[b];
    mf[b + 1] = mf[b] + n;
    for (uint32_t r = 0; r < n; r++) {
      uint32_t len = 1 + (next() >> 8) % (r == 3 ? 400u : 20u); // a long row too
      for (uint32_t j = 0; j < len; j++)
        ci.push_back((int32_t)((next() >> 8) % n)); // unsorted, duplicates legal
      if (r == n - 1)
        ci.back() = (int32_t)(n - 1); // the largest legal column
      rp.push_back((int64_t)ci.size());
    }
  }
  const uint32_t N = mf[batch];
  const uint64_t nnz = ci.size();
  std::vector<double> va(nnz, 1.0);
  char msg[448] = "";
  auto check = [&](int dtype, uint32_t bt, const uint32_t* m, uint64_t z,
                   const int64_t* p, const int32_t* c, const void* v) {
    msg[0] = '\0';
    return check_batch_host(dtype, bt, m, z, p, c, v, msg, sizeof(msg));
  };

  EXPECT(check(1, batch, mf.data(), nnz, rp.data(), ci.data(), va.data()) == 0);
  EXPECT(check(0, batch, mf.data(), nnz, rp.data(), ci.data(), va.data()) == 0);
  for (uint32_t r = 0; r < N; r++) {
    const uint32_t b = mat_of_row(mf.data(), batch, r);
    EXPECT(b < batch && mf[b] <= r && r < mf[b + 1]);
  }
  { // the batch's plan is st_csr_plan of the stacked row_ptr
    std::vector<uint32_t> order(N);
    uint32_t first[kClasses + 1];
    const int used = plan(rp.data(), N, order.data(), first, msg, sizeof(msg));
    EXPECT(used >= 2 && first[0] == 0 && first[kClasses] == N);
    std::vector<char> seen(N, 0);
    for (int c = 0; c < kClasses; c++)
      for (uint32_t i = first[c]; i < first[c + 1]; i++) {
        const uint32_t r = order[i];
        EXPECT(r < N && !seen[r]);
        seen[r] = 1;
        EXPECT(row_class((uint64_t)(rp[r + 1] - rp[r])) == c);
        EXPECT(i == first[c] || order[i - 1] < r);
      }
  }
  { // participants of the vector pass
    EXPECT(batch_prep_wgs(1, 2048) == 1 && batch_prep_wgs(256, 2048) == 1 &&
           batch_prep_wgs(257, 2048) == 2 && batch_prep_wgs(0x7fffffffu, 2048) == 2048);
  }

  // the arguments
  EXPECT(refused(check(2, batch, mf.data(), nnz, rp.data(), ci.data(), va.data()), msg, "dtype"));
  EXPECT(refused(check(0, 0, mf.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                 "batch must be >= 1"));
  EXPECT(refused(check(0, batch, nullptr, nnz, rp.data(), ci.data(), va.data()), msg,
                 "null mat_first"));
  EXPECT(refused(check(0, batch, mf.data(), nnz, nullptr, ci.data(), va.data()), msg, "null"));
  EXPECT(refused(check(0, batch, mf.data(), nnz, rp.data(), nullptr, va.data()), msg, "null"));
  EXPECT(refused(check(0, batch, mf.data(), nnz, rp.data(), ci.data(), nullptr), msg, "null"));
  // mat_first
  std::vector<uint32_t> badm = mf;
  badm[0] = 1;
  EXPECT(refused(check(0, batch, badm.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                 "mat_first[0] must be 0, got 1"));
  for (uint32_t b : { 0u, 3u, batch - 1 }) {
    badm = mf;
    badm[b + 1] = badm[b]; // matrix b without a row
    EXPECT(refused(check(0, batch, badm.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                   "does not increase at matrix " + std::to_string(b)));
  }
  badm = mf;
  badm[4] = badm[3] - 1;
  EXPECT(refused(check(0, batch, badm.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                 "does not increase at matrix 3"));
  badm = mf;
  badm[batch] = 0x80000000u;
  EXPECT(refused(check(0, batch, badm.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                 "below 2^31"));
  badm = mf;
  badm[batch] = N - 1; // mat_first[batch] != N: one matrix short of the arrays
  EXPECT(refused(check(0, batch - 1, badm.data(), nnz, rp.data(), ci.data(), va.data()), msg,
                 "row_ptr[n] must be nnz"));
  // row_ptr, with the matrix and the local row named
  std::vector<int64_t> bad = rp;
  bad[0] = 1;
  EXPECT(refused(check(0, batch, mf.data(), nnz, bad.data(), ci.data(), va.data()), msg,
                 "matrix 0, local row 0: csr: row_ptr[0] must be 0"));
  for (uint32_t b = 1; b < batch; b++)
    for (uint32_t lr : { 0u, dims[b] / 2, dims[b] - 1 }) {
      const uint32_t r = mf[b] + lr;
      if (r + 1 == N)
        continue; // the last stacked row's end is the nnz check's
      const std::string where =
        "matrix " + std::to_string(b) + ", local row " + std::to_string(lr) + ": ";
      bad = rp;
      bad[r + 1] = bad[r];
      EXPECT(refused(check(0, batch, mf.data(), nnz, bad.data(), ci.data(), va.data()), msg,
                     where + "csr: row " + std::to_string(r) + " is empty"));
      bad[r + 1] = bad[r] - 1;
      EXPECT(refused(check(0, batch, mf.data(), nnz, bad.data(), ci.data(), va.data()), msg,
                     where + "csr: row_ptr decreases at row " + std::to_string(r)));
    }
  EXPECT(refused(check(0, batch, mf.data(), nnz - 1, rp.data(), ci.data(), va.data()), msg,
                 "matrix " + std::to_string(batch - 1) + ", local row 0: csr: row_ptr[n] must be nnz"));
  // columns: n_b itself - below N for every matrix but a batch of one, so the
  // entry would couple two matrices - and -1, in the first and the last entry
  for (uint32_t b = 0; b < batch; b++)
    for (int32_t c : { (int32_t)dims[b], -1 })
      for (int last = 0; last < 2; last++) {
        const uint32_t lr = last ? dims[b] - 1 : 0;
        const uint64_t e = last ? (uint64_t)rp[mf[b + 1]] - 1 : (uint64_t)rp[mf[b]];
        std::vector<int32_t> badc = ci;
        badc[e] = c;
        EXPECT(refused(check(1, batch, mf.data(), nnz, rp.data(), badc.data(), va.data()), msg,
                       "column index " + std::to_string(c) + " of entry " + std::to_string(e) +
                         " (matrix " + std::to_string(b) + ", local row " + std::to_string(lr) +
                         ") is outside [0, " + std::to_string(dims[b]) + ")"));
      }
  // row_ptr is judged on its own first: a bad column is not even looked at
  {
    std::vector<int32_t> badc = ci;
    badc[0] = 99;
    bad = rp;
    bad[mf[3] + 1] = bad[mf[3]];
    EXPECT(refused(check(0, batch, mf.data(), nnz, bad.data(), badc.data(), va.data()), msg,
                   "matrix 3, local row 0"));
  }
  std::printf("batch = %u, N = %u, nnz = %llu\n", batch, N, (unsigned long long)nnz);
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("ok");
  return 0;
}
