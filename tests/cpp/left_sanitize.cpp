// left_sanitize.cpp — the host arithmetic of the dense left-vector solve
// (eigen_value_amd/csrc/st_left_host.h: the rows per block of the order
// contract, the scratch layout, the launch grid and the staging of
// max_eigen_value_left_ex) as a stand-alone program for the host sanitizers
// (no HIP, no Python, no input files):
//
//   make left_sanitize          # builds with -fsanitize=address,undefined
//                               # and runs it
// or by hand
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/left_sanitize.cpp -o left_sanitize
//   ./left_sanitize
//
// It walks n over every table boundary, the small sizes, powers of two and
// their neighbours up to 2^31 - 1, for both element sizes and every vector
// width, and lays the staging and the scratch out in real buffers for the
// small ones: each tile of the sweep must read inside the matrix, write
// inside the partials, and the tiles together must cover every element once.
// Exit code 0 and "left_sanitize ok" when every check holds.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "st_left_host.h"

namespace L = st::left;

static int g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                \
      std::fprintf(stderr, __VA_ARGS__);                                       \
      std::fprintf(stderr, "\n");                                              \
      g_fail++;                                                                \
    }                                                                          \
  } while (0)

// the arithmetic alone, for any n in [1, 2^31)
static void
check_arith(uint32_t n)
{
  for (int dtype = 0; dtype < 2; dtype++) {
    const size_t elem = dtype ? 8 : 4;
    const uint32_t rb = L::rows(dtype, n);
    CHECK(rb >= 1 && rb <= 65536, "rows(%d, %u) = %u", dtype, n, rb);
    if (n > 1)
      CHECK(L::rows(dtype, n - 1) <= rb, "rows not monotone at %u", n);
    const uint64_t nrb = L::blocks(n, rb);
    CHECK(nrb >= 1 && (nrb - 1) * rb < n && nrb * rb >= n, "blocks(%u, %u)", n, rb);
    const uint64_t xe = L::x_elems(n), pe = L::part_elems(n, rb);
    CHECK(xe >= n && xe % 64 == 0 && xe - n < 64, "x_elems(%u) = %" PRIu64, n, xe);
    CHECK(pe == nrb * n && pe / n == nrb, "part_elems(%u) = %" PRIu64, n, pe);
    CHECK((xe + pe) * elem / elem == xe + pe, "scratch bytes wrap at %u", n);
    for (uint32_t w : { 1u, (uint32_t)(16 / elem) }) {
      L::Grid g{};
      uint64_t want = 0;
      const bool ok = L::grid(n, rb, w, elem, &g, &want);
      const uint64_t strip = (uint64_t)L::kBlockLanes * w;
      CHECK(want == nrb * ((n + strip - 1) / strip), "grid want at %u", n);
      CHECK(ok == (want <= L::kGridMax), "grid refusal at %u", n);
      if (ok) {
        CHECK(g.grid == want && g.nrb == nrb && (uint64_t)g.nstrips * strip >= n &&
                (uint64_t)(g.nstrips - 1) * strip < n,
              "grid fields at %u", n);
        CHECK(g.nt == ((long double)n * n * elem >= (long double)L::kNtBytes), "nt at %u", n);
      }
    }
    const bool fits = L::stage_fits(n, elem);
    CHECK(fits == ((long double)n * n * elem + 255 < 18446744073709551616.0L),
          "stage_fits(%u, %zu)", n, elem);
    if (fits) {
      const uint64_t b = L::stage_bytes(n, elem);
      CHECK(b % 256 == 0 && b >= (uint64_t)n * n * elem && b - (uint64_t)n * n * elem < 256,
            "stage_bytes(%u)", n);
    }
  }
}

// the layout in real buffers: stage the matrix as the twin does, then walk
// every tile of the sweep as the kernel's lanes do (rows [tile * rb, ...),
// W columns from (strip * 256 + lane) * W), counting every read and write
static void
check_layout(uint32_t n, int dtype, uint32_t w)
{
  const size_t elem = dtype ? 8 : 4;
  if (n % w != 0)
    return; // the launcher takes W = 1 then
  const uint32_t rb = L::rows(dtype, n);
  L::Grid g{};
  uint64_t want = 0;
  if (!L::grid(n, rb, w, elem, &g, &want)) {
    CHECK(false, "small n refused: %u", n);
    return;
  }
  std::vector<unsigned char> stage(L::stage_bytes(n, elem)); // the twin's slot
  CHECK(stage.size() >= (size_t)n * n * elem, "stage too small");
  std::vector<uint8_t> reads((size_t)n * n, 0);
  std::vector<uint8_t> scratch(L::x_elems(n) + L::part_elems(n, rb), 0);
  uint8_t* part = scratch.data() + L::x_elems(n);
  for (uint32_t blk = 0; blk < g.grid; blk++) {
    const uint32_t strip = blk % g.nstrips, tile = blk / g.nstrips;
    for (uint32_t lane = 0; lane < L::kBlockLanes; lane++) {
      const uint64_t c0 = ((uint64_t)strip * L::kBlockLanes + lane) * w;
      if (c0 >= n)
        continue;
      const uint64_t r0 = (uint64_t)tile * rb;
      const uint64_t r1 = r0 + rb < n ? r0 + rb : n;
      for (uint64_t r = r0; r < r1; r++)
        for (uint32_t i = 0; i < w; i++) {
          stage.at((r * n + c0 + i) * elem + elem - 1) = 1; // inside the staged matrix
          reads.at(r * n + c0 + i)++;
        }
      for (uint32_t i = 0; i < w; i++)
        part[(uint64_t)tile * n + c0 + i]++; // ASan: inside the scratch
    }
  }
  for (size_t i = 0; i < reads.size(); i++)
    if (reads[i] != 1) {
      CHECK(false, "n = %u w = %u: element %zu read %u times", n, w, i, reads[i]);
      break;
    }
  for (uint64_t i = 0; i < L::part_elems(n, rb); i++)
    if (part[i] != 1) {
      CHECK(false, "n = %u w = %u: partial %" PRIu64 " written %u times", n, w, i, part[i]);
      break;
    }
  for (uint64_t i = 0; i < L::x_elems(n); i++)
    CHECK(scratch[i] == 0, "n = %u: the sweep wrote into x", n);
}

int
main()
{
  std::vector<uint32_t> ns;
  for (uint32_t n = 1; n <= 70; n++)
    ns.push_back(n);
  for (uint32_t b : { 255u, 256u, 257u, 511u, 512u, 513u, 1023u, 1024u, 1025u, 2047u, 2048u,
                      2049u, 2051u, 4095u, 4096u, 4097u, 16383u, 16384u, 16385u, 32768u,
                      65536u, 131072u })
    ns.push_back(b);
  for (int e = 18; e <= 31; e++)
    for (int64_t d = -1; d <= 1; d++) {
      const int64_t n = ((int64_t)1 << e) + d;
      if (n >= 1 && n <= (int64_t)L::kNMax)
        ns.push_back((uint32_t)n);
    }
  for (uint32_t n : ns)
    check_arith(n);
  for (uint32_t n : ns)
    if (n <= 2051)
      for (int dtype = 0; dtype < 2; dtype++)
        for (uint32_t w : { 1u, (uint32_t)(dtype ? 2 : 4) })
          check_layout(n, dtype, w);
  if (g_fail) {
    std::fprintf(stderr, "left_sanitize: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("left_sanitize ok: %zu sizes\n", ns.size());
  return 0;
}
