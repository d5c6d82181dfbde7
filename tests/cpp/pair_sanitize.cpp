// pair_sanitize.cpp — the host arithmetic of the dense Perron pair solve
// (eigen_value_amd/csrc/st_pair_host.h: the strip of the right side's order,
// the scratch layout and the launch grid) as a stand-alone program for the
// host sanitizers (no HIP, no Python, no input files):
//
//   make pair_sanitize          # builds with -fsanitize=address,undefined
//                               # and runs it
// or by hand
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -Ieigen_value_amd/csrc tests/cpp/pair_sanitize.cpp -o pair_sanitize
//   ./pair_sanitize
//
// It walks n over every table boundary, the small sizes, powers of two and
// their neighbours up to 2^31 - 1, for both element sizes, and lays the
// scratch out in a real buffer for the small ones: every tile of the sweep is
// walked as the kernel's lanes walk it (pair_tile, st_pair.h) - a lane's
// columns below n, the rows of the tile in LDS chunks, the flush of the four
// wave slots - in both kinds of load.  Each element must be read exactly once
// per side, each partial written exactly once, the LDS slots written before
// they are read and inside their array, and x never written by the sweep.
// Exit code 0 and "pair_sanitize ok" when every check holds.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "st_pair_host.h"

namespace L = st::left;
namespace P = st::pair;

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
    const uint32_t S = P::strip_cols(elem);
    CHECK(S == (dtype ? 512u : 1024u) && P::lane_cols(elem) * elem == 16, "strip");
    const uint64_t ns = P::strips(n, elem);
    CHECK(ns >= 1 && (ns - 1) * S < n && ns * S >= n, "strips(%u)", n);
    const P::Layout l = P::layout(n, rb, elem);
    CHECK(l.x_right == 0 && l.x_left == L::x_elems(n) && l.colpart == 2 * L::x_elems(n),
          "layout x at %u", n);
    CHECK(l.rowpart >= l.colpart + L::part_elems(n, rb) &&
            l.rowpart - l.colpart - L::part_elems(n, rb) < 64,
          "layout colpart at %u", n);
    CHECK(l.total == l.rowpart + ns * n, "layout total at %u", n);
    for (uint64_t off : { l.x_left, l.colpart, l.rowpart })
      CHECK(off % 64 == 0, "part not 256-byte aligned at %u", n);
    CHECK(l.total * elem / elem == l.total, "scratch bytes wrap at %u", n);
    L::Grid g{};
    uint64_t want = 0;
    const bool ok = P::grid(n, rb, elem, &g, &want);
    CHECK(want == L::blocks(n, rb) * ns, "grid want at %u", n);
    CHECK(ok == (want <= L::kGridMax), "grid refusal at %u", n);
    if (ok) {
      CHECK(g.grid == want && g.nrb == L::blocks(n, rb) && g.nstrips == ns && g.rb == rb,
            "grid fields at %u", n);
      CHECK(g.nt == ((long double)n * n * elem >= (long double)L::kNtBytes), "nt at %u", n);
    }
  }
}

// the layout in real buffers: every tile as pair_tile's lanes walk it.  vec:
// one 16-byte access per lane and row (only when n is a multiple of the lane's
// columns), else element-wide
static void
check_layout(uint32_t n, int dtype, bool vec, uint32_t rb)
{
  const size_t elem = dtype ? 8 : 4;
  const uint32_t w = P::lane_cols(elem);
  if (vec && n % w != 0)
    return; // the launcher takes the element-wide loads then
  L::Grid g{};
  uint64_t want = 0;
  if (!P::grid(n, rb, elem, &g, &want)) {
    CHECK(false, "small n refused: %u", n);
    return;
  }
  const P::Layout l = P::layout(n, rb, elem);
  std::vector<uint8_t> mat((size_t)n * n, 0);       // the matrix, one byte per element
  std::vector<uint8_t> reads_left((size_t)n * n, 0), reads_right((size_t)n * n, 0);
  std::vector<uint8_t> scratch(l.total, 0);
  uint8_t* colpart = scratch.data() + l.colpart;
  uint8_t* rowpart = scratch.data() + l.rowpart;
  const uint32_t waves = L::kBlockLanes / 64;
  for (uint32_t blk = 0; blk < g.grid; blk++) {
    const uint32_t strip = blk % g.nstrips, tile = blk / g.nstrips;
    const uint64_t r0 = (uint64_t)tile * rb;
    const uint64_t r1 = r0 + rb < n ? r0 + rb : n;
    for (uint64_t lo = r0; lo < r1; lo += P::kChunkRows) {
      const uint64_t hi = lo + P::kChunkRows < r1 ? lo + P::kChunkRows : r1;
      std::vector<uint8_t> red((size_t)waves * P::kChunkRows, 0); // LDS: [wave][row]
      for (uint32_t lane = 0; lane < L::kBlockLanes; lane++) {
        const uint64_t c0 = ((uint64_t)strip * L::kBlockLanes + lane) * w;
        const uint32_t nc = c0 >= n ? 0 : (n - c0 < w ? (uint32_t)(n - c0) : w);
        if (vec)
          CHECK(nc == 0 || nc == w, "n = %u: a vector lane straddles n", n);
        for (uint64_t r = lo; r < hi; r++) {
          for (uint32_t i = 0; i < nc; i++) {
            (void)mat.at(r * n + c0 + i); // inside the matrix
            reads_left.at(r * n + c0 + i)++;
            reads_right.at(r * n + c0 + i)++;
          }
          if (lane % 64 == 63) // lane 63 of each wave leaves the row's wave sum
            red.at((size_t)(lane / 64) * P::kChunkRows + (r - lo))++;
        }
        if (lo + P::kChunkRows >= r1) // the tile's end: the lane's column partials
          for (uint32_t i = 0; i < nc; i++)
            colpart[(uint64_t)tile * n + c0 + i]++; // ASan: inside the scratch
      }
      // the flush: lane t < rows of the chunk adds the four slots of row t
      for (uint32_t t = 0; t < L::kBlockLanes; t++)
        if (t < hi - lo) {
          for (uint32_t wv = 0; wv < waves; wv++)
            CHECK(red.at((size_t)wv * P::kChunkRows + t) == 1,
                  "n = %u: LDS slot [%u][%u] read before it was written", n, wv, t);
          rowpart[(uint64_t)strip * n + lo + t]++;
        }
    }
  }
  for (size_t i = 0; i < reads_left.size(); i++)
    if (reads_left[i] != 1 || reads_right[i] != 1) {
      CHECK(false, "n = %u vec = %d: element %zu read %u / %u times", n, (int)vec, i,
            reads_left[i], reads_right[i]);
      break;
    }
  for (uint64_t i = 0; i < L::part_elems(n, rb); i++)
    if (colpart[i] != 1) {
      CHECK(false, "n = %u: column partial %" PRIu64 " written %u times", n, i, colpart[i]);
      break;
    }
  for (uint64_t i = 0; i < P::strips(n, elem) * n; i++)
    if (rowpart[i] != 1) {
      CHECK(false, "n = %u: row partial %" PRIu64 " written %u times", n, i, rowpart[i]);
      break;
    }
  for (uint64_t i = 0; i < l.colpart; i++)
    CHECK(scratch[i] == 0, "n = %u: the sweep wrote into x", n);
  for (uint64_t i = l.colpart + L::part_elems(n, rb); i < l.rowpart; i++)
    CHECK(scratch[i] == 0, "n = %u: the sweep wrote into the padding", n);
}

int
main()
{
  std::vector<uint32_t> ns;
  for (uint32_t n = 1; n <= 70; n++)
    ns.push_back(n);
  for (uint32_t b : { 255u, 256u, 257u, 511u, 512u, 513u, 1023u, 1024u, 1025u, 1027u, 2047u,
                      2048u, 2049u, 2051u, 4095u, 4096u, 4097u, 16383u, 16384u, 16385u, 32768u,
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
  size_t walked = 0;
  for (uint32_t n : ns)
    if (n <= 2051)
      for (int dtype = 0; dtype < 2; dtype++)
        for (bool vec : { false, true }) {
          check_layout(n, dtype, vec, L::rows(dtype, n));
          walked++;
        }
  // rows per block above the LDS chunk (a tuning override): two flushes per tile
  for (uint32_t n : { 300u, 513u, 600u })
    for (int dtype = 0; dtype < 2; dtype++)
      check_layout(n, dtype, false, 2 * P::kChunkRows + 8);
  if (g_fail) {
    std::fprintf(stderr, "pair_sanitize: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("pair_sanitize ok: %zu sizes, %zu layouts walked\n", ns.size(), walked);
  return 0;
}
