// The host side of the multi-column CSR solve - the counts, the packed width,
// the launch-shape tables, the packing and the per-column validation in its
// fixed order, of eigen_value_amd/csrc/st_csr_host.h - as a stand-alone
// program for the host sanitizers (no HIP, no Python):
//
//   python tests/csr_cases.py DIR           # writes DIR/table{0,1,2}.bin
//   make csr_multi_sanitize                 # builds with
//       -fsanitize=address,undefined and runs it on those files
//
// A file holds int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz];
// the value of entry e is 1.  Every matrix is taken as it is and with rows
// emptied (0, 1, n / 2, n / 2 + 1, n - 1), in both dtypes, for C = 1, 2, 3, 5,
// 8 and K = 1, 4: the packing is checked slot by slot (padding columns hold
// 1, exactly n * CP slots are written); the validation passes on good terms
// and names the lowest offender by (column, then term, u before w, index;
// then the column's rows).  Exit 0 and "ok" on success.
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

static void
check_tables()
{
  char msg[384] = "";
  EXPECT(multi_cp(1) == 2 && multi_cp(2) == 2 && multi_cp(3) == 4 && multi_cp(4) == 4 &&
         multi_cp(5) == 8 && multi_cp(8) == 8);
  EXPECT(check_multi_count(1, 1, msg, sizeof(msg)) == 0);
  EXPECT(check_multi_count(8, 4, msg, sizeof(msg)) == 0);
  EXPECT(refused(check_multi_count(0, 1, msg, sizeof(msg)), msg, "C must be in [1, 8], got 0"));
  EXPECT(refused(check_multi_count(9, 1, msg, sizeof(msg)), msg, "C must be in [1, 8], got 9"));
  EXPECT(refused(check_multi_count(2, 0, msg, sizeof(msg)), msg, "K must be in [1, 4], got 0"));
  EXPECT(refused(check_multi_count(2, 5, msg, sizeof(msg)), msg, "K must be in [1, 4], got 5"));
  for (uint32_t rb : { 8u, 16u, 32u, 64u })
    for (int c = 0; c < kClasses; c++) {
      const uint32_t r = multi_rows(c, rb), u = multi_unroll(c, rb);
      EXPECT(r >= 1 && u >= 1 && r * u <= 8);
      EXPECT(kLanes[c] <= 64 || r == 1); // a workgroup-wide row stands alone
      EXPECT(r * u * rb <= 128 || rb <= 16);
    }
}

template <typename T>
static void
check_multi(const Csr& a, bool has_empty, uint32_t C, uint32_t K)
{
  char msg[448] = "";
  const uint32_t n = a.n, CP = multi_cp(C);
  std::vector<T> vals(a.nnz(), (T)1);
  // u_{c,j}[i], w_{c,j}[i]: positive, all different
  std::vector<std::vector<T>> store(2 * (size_t)C * K, std::vector<T>(n));
  std::vector<const T*> u(C * K), w(C * K);
  for (uint32_t c = 0; c < C; c++)
    for (uint32_t j = 0; j < K; j++) {
      std::vector<T>& uu = store[2 * ((size_t)c * K + j)];
      std::vector<T>& ww = store[2 * ((size_t)c * K + j) + 1];
      for (uint32_t i = 0; i < n; i++) {
        uu[i] = (T)(1 + c + 10 * j) + (T)i / (T)n;
        ww[i] = (T)(100 + c + 10 * j) + (T)i / (T)n;
      }
      u[c * K + j] = uu.data();
      w[c * K + j] = ww.data();
    }
  EXPECT(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(), w.data(), msg,
                              sizeof(msg)) == 0);
  // the packing of every term: exactly n * CP slots, a guard slot behind them
  for (uint32_t j = 0; j < K; j++) {
    std::vector<T> dst((size_t)n * CP + 1, (T)-7);
    pack_columns<T>(n, C, CP, u.data() + j, K, dst.data());
    int bad = 0;
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t c = 0; c < CP; c++)
        bad += !(dst[(size_t)i * CP + c] == (c < C ? u[c * K + j][i] : (T)1));
    EXPECT(bad == 0);
    EXPECT(dst[(size_t)n * CP] == (T)-7);
  }
  // the lowest offender: column first, then (term, u before w, index)
  const uint32_t cb = C - 1, jb = K - 1, at = n / 3;
  {
    std::vector<T>& ww = store[2 * ((size_t)cb * K + jb) + 1];
    const T keep = ww[at];
    ww[at] = (T)-0.5;
    char want[96];
    std::snprintf(want, sizeof(want), "column %u: w_%u[%u] = -0.5", cb, jb, at);
    EXPECT(refused(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(), w.data(),
                                        msg, sizeof(msg)), msg, want));
    // a NaN in column 0's last u wins over it; u before w inside a term
    std::vector<T>& u0 = store[2 * (size_t)jb];
    const T keep0 = u0[n - 1];
    u0[n - 1] = std::numeric_limits<T>::quiet_NaN();
    std::snprintf(want, sizeof(want), "column 0: u_%u[%u] = ", jb, n - 1);
    EXPECT(refused(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(), w.data(),
                                        msg, sizeof(msg)), msg, want));
    u0[n - 1] = keep0;
    ww[at] = keep;
  }
  // a row of M_c without a positive entry: empty in A and every u_{c,j} = 0
  // there; a column's rows come after its vectors and before the next column
  if (has_empty) {
    const uint32_t r = n / 2;
    std::vector<T> kept(K);
    for (uint32_t j = 0; j < K; j++) {
      kept[j] = store[2 * ((size_t)cb * K + j)][r];
      store[2 * ((size_t)cb * K + j)][r] = (T)0;
    }
    char want[96];
    std::snprintf(want, sizeof(want), "column %u: row %u of A", cb, r);
    EXPECT(refused(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(), w.data(),
                                        msg, sizeof(msg)), msg, want));
    if (C > 1) { // an earlier column's entry wins over a later column's row
      std::vector<T>& w0 = store[1];
      const T keep = w0[0];
      w0[0] = (T)-1;
      EXPECT(refused(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(),
                                          w.data(), msg, sizeof(msg)), msg,
                     "column 0: w_0[0] = -1"));
      w0[0] = keep;
    }
    for (uint32_t j = 0; j < K; j++)
      store[2 * ((size_t)cb * K + j)][r] = kept[j];
  }
  // a null vector is named with its column
  {
    const T* keep = u[cb * K + jb];
    u[cb * K + jb] = nullptr;
    char want[64];
    std::snprintf(want, sizeof(want), "column %u: null u_%u", cb, jb);
    EXPECT(refused(check_multi_terms<T>(n, a.rp.data(), vals.data(), C, K, u.data(), w.data(),
                                        msg, sizeof(msg)), msg, want));
    u[cb * K + jb] = keep;
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
  const Csr b = emptied(a, { 0, 1, a.n / 2, a.n / 2 + 1, a.n - 1 });
  for (uint32_t C : { 1u, 2u, 3u, 5u, 8u })
    for (uint32_t K : { 1u, 4u }) {
      check_multi<float>(a, false, C, K);
      check_multi<double>(a, false, C, K);
      check_multi<float>(b, true, C, K);
      check_multi<double>(b, true, C, K);
    }
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
  check_tables();
  for (int i = 1; i < argc; i++)
    one(argv[i]);
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("ok");
  return 0;
}
