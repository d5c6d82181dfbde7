// st_solve.hip — host orchestration of the similarity-transform round loop
// and the drop-in C-ABI (similarity_transform.h layers 1-3).
//
// Replaces, in the reference (itzmeanjan/eigen_value):
//   wrapper/similarity_transform.cpp:3-37   make_queue / max_eigen_value
//   similarity_transform.cpp:5-75           similarity_transform() host loop
//
// Round loop (one device stream, no per-round host sync):
//   K0  s_0 = rowsum(A_0)                                  N^2 b read, once
//       (k_flat_sum + k_parts where the flat round pays, else k_fused)
//   per round k, ONE launch (k_round, st_device.h; matrices of >= 144 MiB
//   take the flat round, k_flat + k_parts, instead, storing the matrix
//   every defer_rounds() rounds; N <= 128 fp64 / 256 fp32 run the whole
//   loop in one k_solve_small launch):
//     from s_k: max, v *= s/m, stop test, lambda = s_k[0] (every workgroup
//     derives m_k/stop_k from its own sweep of s_k; workgroup 0 records)
//     A_{k+1} = D_k^-1 A_k D_k in place, s_{k+1} = rowsum(A_{k+1})
//     (launches after the stop round return at once)
// What the loop works on is one Operator value: the dense matrix (transformed
// in place as above, or only read with ST_FLAG_MATRIX_FREE), a 16-bit matrix,
// a CSR handle, CSR plus terms, the product of two handles, a pattern handle
// with optional terms, or a dense matrix swept by columns (the left vector).  Every read-only kind runs the matrix-free
// loop; op_rowsum and op_round are the only places that tell the kinds apart.
// A batch of matrices runs k_solve_batched (one launch, a workgroup per
// matrix) or, with ST_FLAG_BATCH_ROUNDS, this loop with every launch
// covering the whole batch (k_round_batched, solve_batched_rounds).  The
// batched forms that enqueue rounds (solve_batched_rounds, the batched and
// the multi-column CSR solves) share counted_rounds; all five batched forms
// share report_entries; the dense pair solve (solve_pair_t: two sides of one
// matrix) uses both.  The host-pointer twins lay their workspace out with
// CsrSlots / VecSlots and end in finish_twin.
// The reference blocks on a host_accessor every round
// (similarity_transform.cpp:45-50).  Here rounds are enqueued in batches;
// the host checks the device `done` flag of batch b while batch b+1 is
// already queued, and rounds after convergence are device-gated no-ops, so
// the observable results (lambda, v, iter_count) are exactly those of the
// sequential loop.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "st_csr_host.h"
#include "st_internal.h"
#include "st_left_host.h"
#include "st_pair_host.h"

namespace st {

static thread_local char g_err[512];

void
set_error(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void
clear_error()
{
  g_err[0] = '\0';
}

namespace {

constexpr uint32_t kDefaultBatch = 8;
constexpr uint32_t kFlatBatch = 2;

constexpr size_t
up256(size_t b)
{
  return (b + 255) & ~(size_t)255;
}

// a device allocation that only grows: ensure() keeps what is large enough,
// else waits for the stream's work on the old one, frees it and allocates
struct DeviceBuf
{
  void* p = nullptr;
  size_t cap = 0; // bytes
  int ensure(hipStream_t stream, size_t bytes)
  {
    if (p && cap >= bytes)
      return 0;
    if (p) {
      ST_CHECK(hipStreamSynchronize(stream));
      ST_CHECK(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    ST_CHECK(hipMalloc(&p, bytes));
    cap = bytes;
    return 0;
  }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// slots of Context::vec and of Context::bsum
constexpr size_t kVecSlots = 4 + 2 * (kDeferRoundsMax + 1);
constexpr size_t kBsumSlots = 3;

struct Context
{
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr; // own_stream or a caller stream
  // cached device workspaces (grown on demand, freed by destroy_queue)
  DeviceBuf mat; // the host twins' copy of their matrix
  // [s0 | s1 | v | v' | s ring (kDeferRoundsMax + 1) | 1/s ring (same)],
  // each vec_bytes
  DeviceBuf vec;
  size_t vec_bytes = 0;
  DeviceBuf part; // flat-round partial sums (large matrices)
  st_state* d_state = nullptr;
  st_state* h_state = nullptr; // pinned, 2 slots
  std::vector<float> round_ms; // per-round kernel time of the last timed solve
  // ST_FLAG_TRACE_SUMS: the row sums s_k every round of the last traced
  // solve evaluated (device staging, then the host copy st_last_round_sums
  // returns)
  DeviceBuf trace;
  std::vector<unsigned char> trace_sums;
  uint32_t trace_rounds = 0;
  hipEvent_t ev_flag[2] = { nullptr, nullptr };
  // batched solve: one st_state per matrix (device array and its host copy)
  DeviceBuf bstate;
  std::vector<st_state> h_bstate;
  // batched round loop: [s0 | s1 | v], each bsum_bytes ([batch][n]); the
  // count of finished matrices and its pinned host mirror (2 slots)
  DeviceBuf bsum;
  size_t bsum_bytes = 0;
  uint32_t* d_bcount = nullptr;
  uint32_t* h_bcount = nullptr;
  // variable-size batch: the descriptor table (plan order) for vb_cap
  // matrices, staged in pinned memory and copied to the device once per call
  // (every call ends in a stream sync, so the staging is free again when the
  // next one fills it)
  void* h_vb = nullptr;
  void* d_vb = nullptr;
  size_t vb_cap = 0; // matrices

  template <typename T>
  T* vec_slot(size_t i) const
  {
    return reinterpret_cast<T*>(static_cast<char*>(vec.p) + i * vec_bytes);
  }
  template <typename T>
  T* bsum_slot(size_t i) const
  {
    return reinterpret_cast<T*>(static_cast<char*>(bsum.p) + i * bsum_bytes);
  }
  st_state* d_bstate() const { return static_cast<st_state*>(bstate.p); }
};

// bytes of the descriptor table for `count` matrices
constexpr size_t
vb_bytes(size_t count)
{
  return count * sizeof(VBatchDesc);
}

double
ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(
           std::chrono::steady_clock::now() - t0)
    .count();
}

int
ensure_device(Context* c)
{
  ST_CHECK(hipSetDevice(c->device));
  return 0;
}

int
ensure_vectors(Context* c, size_t vec_bytes)
{
  if (c->vec.ensure(c->stream, kVecSlots * up256(vec_bytes)))
    return -1;
  c->vec_bytes = c->vec.cap / kVecSlots;
  return 0;
}

int
ensure_bstate(Context* c, size_t count)
{
  return c->bstate.ensure(c->stream, count * sizeof(st_state));
}

// a traced solve records every evaluated round's n row sums: at most
// kTraceMaxBytes of them (tests and diagnostics, not a production mode)
constexpr size_t kTraceMaxBytes = (size_t)1 << 30;

int
ensure_vbatch(Context* c, size_t count)
{
  if (c->h_vb && c->d_vb && c->vb_cap >= count)
    return 0;
  if (c->h_vb || c->d_vb) {
    ST_CHECK(hipStreamSynchronize(c->stream));
    if (c->h_vb)
      ST_CHECK(hipHostFree(c->h_vb));
    c->h_vb = nullptr;
    if (c->d_vb)
      ST_CHECK(hipFree(c->d_vb));
    c->d_vb = nullptr;
    c->vb_cap = 0;
  }
  ST_CHECK(hipHostMalloc(&c->h_vb, vb_bytes(count), hipHostMallocDefault));
  ST_CHECK(hipMalloc(&c->d_vb, vb_bytes(count)));
  c->vb_cap = count;
  return 0;
}

int
ensure_bsum(Context* c, size_t bytes)
{
  if (!c->d_bcount)
    ST_CHECK(hipMalloc((void**)&c->d_bcount, sizeof(uint32_t)));
  if (!c->h_bcount)
    ST_CHECK(hipHostMalloc((void**)&c->h_bcount, 2 * sizeof(uint32_t),
                           hipHostMallocCoherent | hipHostMallocMapped));
  if (c->bsum.ensure(c->stream, kBsumSlots * up256(bytes)))
    return -1;
  c->bsum_bytes = c->bsum.cap / kBsumSlots;
  return 0;
}

// the largest n whose single solve takes the k_round path: the last n below
// the flat threshold (round_flat_pays is monotone in n)
uint32_t
batched_rounds_max_n(size_t elem)
{
  uint32_t lo = 0, hi = 1u << 20; // pays(hi), !pays(lo)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (round_flat_pays(mid, mid, elem))
      hi = mid;
    else
      lo = mid;
  }
  return lo;
}

template <typename T>
T
default_eps();
template <>
float
default_eps<float>()
{
  return ST_EPS_F32; // include/similarity_transform.hpp:4 (float)
}
template <>
double
default_eps<double>()
{
  return ST_EPS_F64; // main.py:6
}

struct Resolved
{
  double eps;
  uint32_t max_itr, semantics, batch, flags;
};

template <typename T>
int
resolve(const st_options* opt, Resolved* r)
{
  r->eps = (opt && opt->eps >= 0.0) ? opt->eps : (double)default_eps<T>();
  r->max_itr = (opt && opt->max_itr) ? opt->max_itr : ST_MAX_ITR;
  r->semantics = opt ? opt->semantics : ST_SEM_SYCL;
  r->batch = (opt && opt->batch) ? opt->batch : 0; // 0: per round form
  r->flags = opt ? opt->flags : 0u;
  ST_REQUIRE(r->semantics <= ST_SEM_MAINPY, "unknown semantics %u",
             r->semantics);
  return 0;
}

// What a solve_device loop works on.  A dense matrix is transformed in place
// (k_round, flat, deferred, single launch) or, with ST_FLAG_MATRIX_FREE, only
// read; every other kind is read only and runs the matrix-free loop with its
// own launch 0 (op_rowsum) and round (op_round).  The named constructors are
// the only way to make one, so no other combination of handles exists.
struct Operator
{
  enum Kind { kDense, kHalf, kCsr, kCsrTerms, kProduct, kPattern, kDenseLeft };
  Kind kind;
  uint32_t n;
  void* mat;                   // kDense, kDenseLeft: n x n of the vectors' type; kHalf: 16-bit elements
  int storage;                 // kHalf: ST_STORE_F16 / ST_STORE_BF16
  const CsrHandle* a;          // kCsr, kCsrTerms; kProduct: the right factor
  const CsrHandle* b;          // kProduct: the left factor of B A
  const CsrTermsHandle* terms; // kCsrTerms; kPattern: its terms object or null
  const CsrPatternHandle* pat; // kPattern

  static Operator dense(void* d_mat, uint32_t n)
  {
    return { kDense, n, d_mat, 0, nullptr, nullptr, nullptr, nullptr };
  }
  // fp32 vectors only; the loop never writes through d_mat
  static Operator half(int storage, const void* d_mat, uint32_t n)
  {
    return { kHalf, n, const_cast<void*>(d_mat), storage,
             nullptr, nullptr, nullptr, nullptr };
  }
  static Operator csr(const CsrHandle* h)
  {
    return { kCsr, h->n, nullptr, 0, h, nullptr, nullptr, nullptr };
  }
  // A + sum_j u_j w_j^T
  static Operator csr_terms(const CsrHandle* h, const CsrTermsHandle* t)
  {
    return { kCsrTerms, h->n, nullptr, 0, h, nullptr, t, nullptr };
  }
  // B A, never formed
  static Operator product(const CsrHandle* b, const CsrHandle* a)
  {
    return { kProduct, a->n, nullptr, 0, a, b, nullptr, nullptr };
  }
  // diag(r) P diag(c) [+ sum_j u_j w_j^T]
  static Operator pattern(const CsrPatternHandle* p, const CsrTermsHandle* t)
  {
    return { kPattern, p->n, nullptr, 0, nullptr, nullptr, t, p };
  }
  // u A = lambda u on the dense matrix where it lies: the loop never writes
  // through d_mat and makes no copy of it
  static Operator dense_left(const void* d_mat, uint32_t n)
  {
    return { kDenseLeft, n, const_cast<void*>(d_mat), 0,
             nullptr, nullptr, nullptr, nullptr };
  }
  bool read_only() const { return kind != kDense; }
};

// the loop's buffers a read-only operator works in besides s and v: x (the
// pattern's z) in the first slot of the deferred ring, the product's y in its
// second, dots and partials (terms; the flat K0's partials; the left round's
// row-block partials) in the flat scratch
template <typename T>
struct OpScratch
{
  T* x;
  T* y;
  T* part;
};

// launch 0: s0 = the row sums of the operator (`flat`: the dense K0 in its
// flat form, w.part sized for it)
template <typename T>
int
op_rowsum(const Operator& op, T* s0, const OpScratch<T>& w, bool flat, hipStream_t s)
{
  switch (op.kind) {
    case Operator::kDenseLeft: // the column sums
      return launch_colsum<T>(static_cast<const T*>(op.mat), s0, w.part, op.n, s);
    case Operator::kPattern:
      return launch_csr_pattern_rowsum(op.pat, op.terms, s0, w.part, s);
    case Operator::kProduct:
      return launch_csr_product_rowsum(op.b, op.a, s0, w.y, s);
    case Operator::kCsrTerms:
      return launch_csr_terms_rowsum(op.a, op.terms, s0, w.part, s);
    case Operator::kCsr:
      return launch_csr_rowsum(op.a, s0, s);
    case Operator::kHalf:
      if constexpr (std::is_same<T, float>::value)
        return launch_rowsum_half(op.storage, op.mat, s0, op.n, op.n, s);
      else
        return 0;
    case Operator::kDense: {
      const T* a = static_cast<const T*>(op.mat);
      return flat ? launch_rowsum_flat<T>(a, s0, w.part, op.n, op.n, s)
                  : launch_rowsum<T>(a, s0, op.n, op.n, s);
    }
  }
  return 0;
}

// the matrix-free round: launch number `launch` = k + 1 evaluates round k
template <typename T>
int
op_round(const Operator& op, const T* s_prev, T* s_next, const T* v_prev, T* v_cur,
         const OpScratch<T>& w, const Resolved& o, uint32_t launch, st_state* st,
         hipStream_t s)
{
  switch (op.kind) {
    case Operator::kDenseLeft:
      return launch_left_round<T>(static_cast<const T*>(op.mat), s_prev, s_next, v_prev,
                                  v_cur, w.x, w.part, op.n, (T)o.eps, launch, o.max_itr,
                                  o.semantics, st, s);
    case Operator::kPattern:
      return launch_csr_pattern_round(op.pat, op.terms, s_prev, s_next, v_prev, v_cur, w.x,
                                      w.part, o.eps, launch, o.max_itr, o.semantics, st, s);
    case Operator::kProduct:
      return launch_csr_product_round(op.b, op.a, s_prev, s_next, v_prev, v_cur, w.x, w.y,
                                      o.eps, launch, o.max_itr, o.semantics, st, s);
    case Operator::kCsrTerms:
      return launch_csr_terms_round(op.a, op.terms, s_prev, s_next, v_prev, v_cur, w.x,
                                    w.part, o.eps, launch, o.max_itr, o.semantics, st, s);
    case Operator::kCsr:
      return launch_csr_round(op.a, s_prev, s_next, v_prev, v_cur, w.x, o.eps, launch,
                              o.max_itr, o.semantics, st, s);
    case Operator::kHalf:
      if constexpr (std::is_same<T, float>::value)
        return launch_mfree_half(op.storage, op.mat, s_prev, s_next, v_prev, v_cur, op.n,
                                 op.n, 0, (T)o.eps, launch, o.max_itr, o.semantics, st, s);
      else
        return 0;
    case Operator::kDense:
      return launch_mfree<T>(static_cast<const T*>(op.mat), s_prev, s_next, v_prev, v_cur,
                             op.n, op.n, 0, (T)o.eps, launch, o.max_itr, o.semantics, st, s);
  }
  return 0;
}

// The round loop on a device-resident operator.
// flush_matrix (a dense matrix transformed in place): leave the matrix as the
// every-round loop would (the caller sees it); a private copy (solve_host)
// skips the deferred loop's last store.
template <typename T>
int64_t
solve_device(Context* c, const Operator& op, T* d_v_out, T* v_host, T* eigen_val,
             uint32_t* iter_cnt, const st_options* opt, st_stats* stats,
             bool flush_matrix = true)
{
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value,
                "fp32 / fp64 vectors");
  const uint32_t n = op.n;
  T* const d_mat = static_cast<T*>(op.mat); // kDense only
  ST_REQUIRE(c, "null queue");
  if (op.kind == Operator::kDense || op.kind == Operator::kHalf ||
      op.kind == Operator::kDenseLeft)
    ST_REQUIRE(op.mat, "null matrix");
  ST_REQUIRE(n > 0, "dim must be > 0");
  ST_REQUIRE(eigen_val && iter_cnt, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  Resolved o;
  if (resolve<T>(opt, &o))
    return -1;
  if (ensure_device(c) || ensure_vectors(c, sizeof(T) * (size_t)n))
    return -1;
  hipStream_t s = c->stream;
  T* s_buf[2] = { c->vec_slot<T>(0), c->vec_slot<T>(1) };
  T* d_v = d_v_out ? d_v_out : c->vec_slot<T>(2);
  // matrix-free ping-pong partner of d_v
  T* d_v2 = c->vec_slot<T>(3);
  T* vb[2] = { d_v, d_v2 };
  const bool timed = (o.flags & ST_FLAG_TIME_KERNELS) != 0;
  const bool traced = (o.flags & ST_FLAG_TRACE_SUMS) != 0;
  const size_t row_bytes = sizeof(T) * (size_t)n;
  c->trace_sums.clear();
  c->trace_rounds = 0;
  if (traced) {
    ST_REQUIRE(row_bytes * o.max_itr <= kTraceMaxBytes,
               "ST_FLAG_TRACE_SUMS: %u rounds x %u row sums exceed the %zu MiB "
               "trace; lower max_itr", o.max_itr, n, kTraceMaxBytes >> 20);
    if (c->trace.ensure(s, row_bytes * o.max_itr))
      return -1;
  }
  const bool mfree = op.read_only() || (o.flags & ST_FLAG_MATRIX_FREE) != 0;
  // large matrices: the flat round (k_flat + k_parts)
  const bool flat = !mfree && round_flat_pays(n, n, sizeof(T));
  // the flat round stores the matrix every kDefer rounds (bit-identical
  // results; ST_FLAG_WRITE_EVERY_ROUND stores every round)
  const bool defer = flat && (o.flags & ST_FLAG_WRITE_EVERY_ROUND) == 0;
  const uint32_t kDefer = defer_rounds(n, n, sizeof(T));
  const uint32_t kR = kDefer + 1; // ring slots: pending + s_k + s_{k+1}
  T* ring_s[kDeferRoundsMax + 1];
  T* ring_inv[kDeferRoundsMax + 1];
  for (uint32_t i = 0; i < kR; i++) {
    ring_s[i] = c->vec_slot<T>(4 + i);
    ring_inv[i] = c->vec_slot<T>(4 + kDeferRoundsMax + 1 + i);
  }
  // K0 takes the flat form wherever the flat round pays (the matrix-free
  // loop's too)
  const bool flat_k0 = !op.read_only() && round_flat_pays(n, n, sizeof(T));
  if (flat_k0 && c->part.ensure(s, sizeof(T) * round_flat_scratch(n, n)))
    return -1;
  if (op.terms && c->part.ensure(s, csr_terms_dots_bytes(op.terms->K)))
    return -1;
  if (op.kind == Operator::kDenseLeft &&
      c->part.ensure(s, sizeof(T) * left_part_elems(sizeof(T) == 8, n)))
    return -1;
  T* d_part = reinterpret_cast<T*>(c->part.p);
  // (the deferred ring is the dense loop's: free in every read-only one)
  const OpScratch<T> scratch{ c->vec_slot<T>(4), c->vec_slot<T>(5), d_part };
  // rounds per host flag check: the launches queued behind the stopping
  // round still run as gated no-ops, and a gated flat round is two launches
  // of up to millions of workgroups (~10 us each), so the flat form checks
  // every 2 rounds (>= 0.16 ms of work each) and the one-launch form every 8
  if (o.batch == 0)
    o.batch = flat ? kFlatBatch : kDefaultBatch;
  // timing events [rowsum_a, rowsum_b, (round_a, round_b)*], destroyed on
  // every exit path
  struct Events
  {
    std::vector<hipEvent_t> e;
    ~Events()
    {
      for (hipEvent_t x : e)
        if (x)
          (void)hipEventDestroy(x);
    }
  } events;
  std::vector<hipEvent_t>& ev = events.e;
  auto mk = [&](hipEvent_t* e) -> int {
    ST_CHECK(hipEventCreate(e));
    return 0;
  };
  int rc = 0;

  // a matrix that fits one workgroup's registers runs the whole solve in a
  // single launch, bit-identical to the round loop below; per-round timing,
  // tracing and ST_FLAG_ROUND_LOOP keep the loop
  const bool single = !mfree && !timed && !traced && (o.flags & ST_FLAG_ROUND_LOOP) == 0 &&
                      solve_small_fits<T>(d_mat, n);
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->d_state, 0, sizeof(st_state), s));
  if (!single && launch_fill<T>(d_v, n, (T)1, s)) // initialise_eigen_vector, cpp:34
    return -1;
  if (timed) { // (never single: k_solve_small does v = 1 and s_0 itself)
    ev.resize(2, nullptr);
    if (mk(&ev[0]) || mk(&ev[1]))
      return -1;
    (void)hipEventRecord(ev[0], s);
  }
  T* const s0 = defer ? ring_s[0] : s_buf[0];
  if (!single && op_rowsum<T>(op, s0, scratch, flat_k0, s)) // K0
    return -1;
  if (defer && launch_recip<T>(ring_s[0], ring_inv[0], n, s))
    return -1;
  if (timed)
    (void)hipEventRecord(ev[1], s);

  const T eps = (T)o.eps;
  uint32_t enqueued = 0, cur = 0, batch_no = 0;
  bool done = false;
  if (single) { // the whole loop in one launch (k_solve_small)
    if (launch_solve_small<T>(d_mat, d_v, n, eps, o.max_itr, o.semantics,
                              c->d_state, s))
      return -1;
    done = true;
  }
  while (!done && enqueued < o.max_itr) {
    const uint32_t b = (o.max_itr - enqueued) < o.batch ? (o.max_itr - enqueued)
                                                        : o.batch;
    for (uint32_t j = 0; j < b; j++) {
      const uint32_t k = enqueued + j;
      hipEvent_t ea = nullptr, eb = nullptr;
      if (traced) // s_k, the row sums round k evaluates (no-op copies past the stop)
        rc |= hipMemcpyAsync((char*)c->trace.p + (size_t)k * row_bytes,
                             defer ? ring_s[k % kR] : s_buf[cur], row_bytes,
                             hipMemcpyDeviceToDevice, s) != hipSuccess;
      if (timed) {
        rc |= mk(&ea) | mk(&eb);
        ev.push_back(ea);
        ev.push_back(eb);
        (void)hipEventRecord(ea, s);
      }
      if (mfree) // launch k+1 evaluates round k
        rc |= op_round<T>(op, s_buf[cur], s_buf[cur ^ 1], vb[k & 1], vb[(k + 1) & 1],
                          scratch, o, k + 1, c->d_state, s);
      else if (defer) {
        // stored: A_j, j = the last multiple of kDefer <= k
        const uint32_t j0 = k - k % kDefer, np = k - j0;
        const T* ps[kDeferRoundsMax];
        const T* pi[kDeferRoundsMax];
        for (uint32_t i = 0; i < np; i++) {
          ps[i] = ring_s[(j0 + i) % kR];
          pi[i] = ring_inv[(j0 + i) % kR];
        }
        rc |= launch_round_flat_deferred<T>(
          d_mat, ring_s[k % kR], ring_inv[k % kR], ring_s[(k + 1) % kR],
          ring_inv[(k + 1) % kR], d_part, d_v, n, n, 0, eps, k, o.max_itr,
          o.semantics, c->d_state, ps, pi, np, np + 1 == kDefer, false, s);
      } else if (flat)
        rc |= launch_round_flat<T>(d_mat, s_buf[cur], s_buf[cur ^ 1], d_part,
                                   d_v, n, n, 0, eps, k, o.max_itr,
                                   o.semantics, c->d_state, s);
      else
        rc |= launch_round<T>(d_mat, s_buf[cur], s_buf[cur ^ 1], d_v, n, n, 0,
                              eps, k, o.max_itr, o.semantics, c->d_state, s);
      if (timed)
        (void)hipEventRecord(eb, s);
      cur ^= 1;
      if (rc)
        return -1;
    }
    enqueued += b;
    const int slot = batch_no & 1;
    if (launch_state_mirror(c->d_state, &c->h_state[slot], s))
      return -1;
    ST_CHECK(hipEventRecord(c->ev_flag[slot], s));
    // wait for the previous batch's flag while this batch runs
    if (batch_no > 0) {
      ST_CHECK(hipEventSynchronize(c->ev_flag[slot ^ 1]));
      done = c->h_state[slot ^ 1].done != 0;
    }
    batch_no++;
  }
  ST_CHECK(hipStreamSynchronize(s));
  st_state fin;
  ST_CHECK(hipMemcpy(&fin, c->d_state, sizeof(st_state), hipMemcpyDeviceToHost));
  ST_REQUIRE(fin.done, "internal: loop ended without done flag");
  if (defer && flush_matrix && fin.end % kDefer != 0) {
    // the matrix stands at A_J (J = the last store); apply rounds J .. end-1
    // and store A_end, exactly what storing every round leaves
    const uint32_t kl = fin.end - 1, j0 = kl - kl % kDefer, np = kl - j0;
    const T* ps[kDeferRoundsMax];
    const T* pi[kDeferRoundsMax];
    for (uint32_t i = 0; i < np; i++) {
      ps[i] = ring_s[(j0 + i) % kR];
      pi[i] = ring_inv[(j0 + i) % kR];
    }
    if (launch_round_flat_deferred<T>(
          d_mat, ring_s[kl % kR], ring_inv[kl % kR], nullptr, nullptr, d_part,
          d_v, n, n, 0, eps, kl, o.max_itr, o.semantics, c->d_state, ps, pi,
          np, true, true, s))
      return -1;
    ST_CHECK(hipStreamSynchronize(s));
  }
  if (mfree && (fin.end & 1u)) { // the final v_{end-1} landed in the partner
    ST_CHECK(hipMemcpyAsync(d_v, d_v2, sizeof(T) * (size_t)n,
                            hipMemcpyDeviceToDevice, s));
    ST_CHECK(hipStreamSynchronize(s));
  }
  const double loop_ms = ms_since(t0);

  const auto t1 = std::chrono::steady_clock::now();
  *eigen_val = (T)fin.lambda;
  *iter_cnt = fin.iters;
  if (v_host)
    ST_CHECK(hipMemcpy(v_host, d_v, sizeof(T) * (size_t)n,
                       hipMemcpyDeviceToHost));
  const double d2h_ms = ms_since(t1);
  if (traced) { // rounds 0 .. end-1 were evaluated
    c->trace_sums.resize(row_bytes * fin.end);
    ST_CHECK(hipMemcpy(c->trace_sums.data(), c->trace.p, c->trace_sums.size(),
                       hipMemcpyDeviceToHost));
    c->trace_rounds = fin.end;
  }

  // per-round kernel times (rounds 0 .. end-1 did work; the stop round's
  // launch also streams the matrix), kept for st_last_round_times
  c->round_ms.clear();
  float rowsum_ms = 0.f;
  double tot = 0.0;
  if (timed) {
    (void)hipEventElapsedTime(&rowsum_ms, ev[0], ev[1]);
    for (uint32_t k = 0; k < fin.end && 2 + 2 * k + 1 < ev.size(); k++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ev[2 + 2 * k], ev[2 + 2 * k + 1]);
      c->round_ms.push_back(ms);
      tot += ms;
    }
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->loop_ms = loop_ms;
    stats->d2h_ms = d2h_ms;
    stats->rounds = fin.end;
    stats->converged = fin.stop;
    if (timed) {
      stats->rowsum_ms = rowsum_ms;
      stats->fused_ms_total = tot;
      stats->fused_launches = (uint32_t)c->round_ms.size();
    }
  }
  return (int64_t)loop_ms;
}

// solve_device on a handle's operator, in the handle's dtype
int64_t
solve_operator(Context* c, const Operator& op, int dtype, void* d_v_out, void* v_host,
               void* eigen_val, uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  if (dtype)
    return solve_device<double>(c, op, static_cast<double*>(d_v_out),
                                static_cast<double*>(v_host),
                                static_cast<double*>(eigen_val), iter_cnt, opt, stats);
  return solve_device<float>(c, op, static_cast<float*>(d_v_out),
                             static_cast<float*>(v_host), static_cast<float*>(eigen_val),
                             iter_cnt, opt, stats);
}

// What every host-pointer twin ends with: the copy-in's milliseconds (and the
// device transposition's, tr_ms >= 0, in microseconds clamped to the field)
// into the solve's stats, those to the caller; returns the call's milliseconds
int64_t
finish_twin(st_stats local, double h2d, st_stats* stats, double tr_ms = -1.0)
{
  local.h2d_ms = h2d;
  if (tr_ms >= 0.0) {
    const double us = tr_ms * 1000.0;
    local.transpose_us = us < 4294967295.0 ? (uint32_t)us : 0xffffffffu;
    h2d += tr_ms;
  }
  if (stats)
    *stats = local;
  return (int64_t)(h2d + local.loop_ms);
}

// The solve on a device-resident matrix stored in 16 bits (read only):
// solve_device<float>'s matrix-free loop - gated batches, pinned state
// mirror, v ping-pong, timing and tracing - with the 16-bit launchers.
// Everything is checked before anything is enqueued.
int64_t
solve_device_half(Context* c, int storage, const void* d_mat, uint32_t n,
                  float* d_v_out, float* v_host, float* eigen_val,
                  uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  if (check_storage("half solve", storage))
    return -1;
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNoHalf =
    ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND | ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNoHalf) == 0,
             "half solve: ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix "
             "is read only and every round is one launch", flags);
  ST_REQUIRE(((uintptr_t)d_mat & 1u) == 0, "half solve: matrix not 2-byte aligned");
  return solve_device<float>(c, Operator::half(storage, d_mat, n), d_v_out, v_host,
                             eigen_val, iter_cnt, opt, stats);
}

// The LEFT Perron vector of a device-resident dense matrix (u A = lambda u):
// solve_device's matrix-free loop with the column-sum launchers (st_left.hip).
// The matrix is only read and never copied.  Everything is checked before
// anything is enqueued.
int
left_check_flags(const st_options* opt)
{
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNoLeft =
    ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND | ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNoLeft) == 0,
             "dense left solve: ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix "
             "is read only and every round is the same three launches", flags);
  return 0;
}

template <typename T>
int64_t
solve_device_left(Context* c, const T* d_mat, uint32_t n, T* d_v_out, T* v_host,
                  T* eigen_val, uint32_t* iter_cnt, const st_options* opt,
                  st_stats* stats)
{
  if (left_check_flags(opt))
    return -1;
  ST_REQUIRE(d_mat, "dense left solve: null matrix");
  ST_REQUIRE(n > 0, "dense left solve: dim must be > 0");
  ST_REQUIRE(((uintptr_t)d_mat & (sizeof(T) - 1)) == 0,
             "dense left solve: matrix not aligned to its element size");
  return solve_device<T>(c, Operator::dense_left(d_mat, n), d_v_out, v_host, eigen_val,
                         iter_cnt, opt, stats);
}

// the host twin: the workspace holds the matrix as the caller has it (one
// slot, copied in once and only read)
template <typename T>
int64_t
solve_host_left(Context* c, const T* mat, uint32_t n, T* eigen_val, T* eigen_vec,
                uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  if (left_check_flags(opt))
    return -1;
  {
    Resolved o;
    if (resolve<T>(opt, &o))
      return -1;
  }
  ST_REQUIRE(mat, "max_eigen_value_left_ex: null matrix");
  ST_REQUIRE(n > 0, "max_eigen_value_left_ex: dim must be > 0");
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(n <= left::kNMax && left::stage_fits(n, sizeof(T)),
             "max_eigen_value_left_ex: dim = %u is too large", n);
  if (c->mat.ensure(c->stream, (size_t)left::stage_bytes(n, sizeof(T))))
    return -1;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mat, sizeof(T) * (size_t)n * n, hipMemcpyHostToDevice,
                          c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  st_stats local{};
  if (solve_device_left<T>(c, static_cast<const T*>(c->mat.p), n, nullptr, eigen_vec,
                           eigen_val, iter_cnt, opt, &local) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

int64_t
solve_host_half(Context* c, int storage, const void* mat, uint32_t n,
                float* eigen_val, float* eigen_vec, uint32_t* iter_cnt,
                const st_options* opt, st_stats* stats)
{
  if (check_storage("half solve", storage))
    return -1;
  {
    const uint32_t flags = opt ? opt->flags : 0u;
    ST_REQUIRE((flags & (ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND |
                         ST_FLAG_BATCH_ROUNDS)) == 0,
               "half solve: ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
               "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix "
               "is read only and every round is one launch", flags);
    Resolved o;
    if (resolve<float>(opt, &o))
      return -1;
  }
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(mat && eigen_val && eigen_vec && iter_cnt, "null pointer");
  ST_REQUIRE(n > 0, "dim must be > 0");
  if (ensure_device(c))
    return -1;
  const size_t bytes = 2 * (size_t)n * n;
  if (c->mat.ensure(c->stream, bytes))
    return -1;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mat, bytes, hipMemcpyHostToDevice,
                          c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  st_stats local{};
  if (solve_device_half(c, storage, c->mat.p, n, nullptr, eigen_vec, eigen_val,
                        iter_cnt, opt, &local) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

// The solve on a validated CSR matrix (st_csr_create): solve_device's
// matrix-free loop with the CSR launchers.  Everything is checked before
// anything is enqueued.
int64_t
solve_csr(Context* c, const CsrHandle* h, void* d_v_out, void* v_host,
          void* eigen_val, uint32_t* iter_cnt, const st_options* opt,
          st_stats* stats, const CsrTermsHandle* terms = nullptr)
{
  if (csr_check_flags(opt))
    return -1;
  if (!terms && csr_refuse_empty(h, "st_solve_csr"))
    return -1;
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(c->device == h->device,
             "csr solve: the matrix lives on device %d, the queue on %d",
             h->device, c->device);
  return solve_operator(c, terms ? Operator::csr_terms(h, terms) : Operator::csr(h),
                        h->dtype, d_v_out, v_host, eigen_val, iter_cnt, opt, stats);
}

// The solve on a validated pattern handle (st_csr_pattern_create): solve_csr
// with the pattern launchers.  Everything is checked before anything is
// enqueued.
int64_t
solve_csr_pattern(Context* c, const CsrPatternHandle* h, void* d_v_out, void* v_host,
                  void* eigen_val, uint32_t* iter_cnt, const st_options* opt,
                  st_stats* stats, const CsrTermsHandle* terms = nullptr)
{
  if (csr_check_flags(opt))
    return -1;
  if (!terms && csr_pattern_refuse_empty(h, "st_solve_csr_pattern"))
    return -1;
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(c->device == h->device,
             "csr pattern solve: the pattern lives on device %d, the queue on %d",
             h->device, c->device);
  return solve_operator(c, Operator::pattern(h, terms), h->dtype, d_v_out, v_host,
                        eigen_val, iter_cnt, opt, stats);
}

// one host triple in the workspace at `base`: [row_ptr | vals | col_idx], each
// at a 256-byte aligned offset (a pattern has no vals: b_val = 0)
struct CsrSlots
{
  size_t b_ptr, b_val, b_col;
  size_t bytes() const { return b_ptr + b_val + b_col; }
  int64_t* ptr(char* base) const { return reinterpret_cast<int64_t*>(base); }
  void* val(char* base) const { return base + b_ptr; }
  int32_t* col(char* base) const { return reinterpret_cast<int32_t*>(base + b_ptr + b_val); }
};

CsrSlots
csr_slots(int dtype, uint32_t n, uint64_t nnz, bool with_vals = true)
{
  const size_t elem = dtype ? 8 : 4;
  return CsrSlots{ up256(8 * ((size_t)n + 1)), with_vals ? up256(elem * nnz) : 0,
                   up256(4 * nnz) };
}

int
csr_copy_in(Context* c, const CsrSlots& sl, char* base, int dtype, uint32_t n,
            uint64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
            const void* vals)
{
  const size_t elem = dtype ? 8 : 4;
  ST_CHECK(hipMemcpyAsync(sl.ptr(base), row_ptr, 8 * ((size_t)n + 1),
                          hipMemcpyHostToDevice, c->stream));
  if (sl.b_val)
    ST_CHECK(hipMemcpyAsync(sl.val(base), vals, elem * nnz, hipMemcpyHostToDevice,
                            c->stream));
  ST_CHECK(hipMemcpyAsync(sl.col(base), col_idx, 4 * nnz, hipMemcpyHostToDevice,
                          c->stream));
  return 0;
}

// one host triple into its slots at `base` and, once every copy queued so far
// has landed, the validated handle over it (flags: csr_create's)
int
csr_stage(Context* c, const CsrSlots& sl, char* base, int dtype, uint32_t n,
          uint64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
          const void* vals, uint32_t flags, CsrHandle** out)
{
  if (csr_copy_in(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals))
    return -1;
  ST_CHECK(hipStreamSynchronize(c->stream));
  return csr_create(dtype, n, nnz, sl.ptr(base), sl.col(base), sl.val(base), c->stream,
                    out, flags);
}

// n-vectors behind one another at `base`: vector i at the 256-byte aligned
// slot base + i * stride
struct VecSlots
{
  char* base;
  size_t stride, bytes; // up256(bytes); one vector's elem * n
  static size_t stride_of(int dtype, uint32_t n) { return up256((dtype ? 8 : 4) * (size_t)n); }
  VecSlots(char* at, int dtype, uint32_t n)
    : base(at), stride(stride_of(dtype, n)), bytes((dtype ? 8 : 4) * (size_t)n)
  {
  }
  // the host vector `src` into slot i, *d_out <- its device address (a null
  // src: no copy, a null address)
  int copy_in(Context* c, size_t i, const void* src, const void** d_out) const
  {
    *d_out = nullptr;
    if (!src)
      return 0;
    ST_CHECK(hipMemcpyAsync(base + i * stride, src, bytes, hipMemcpyHostToDevice,
                            c->stream));
    *d_out = base + i * stride;
    return 0;
  }
  // K term pairs into slots first, first + 1, ...: [u_0 | w_0 | u_1 | ...]
  int terms_in(Context* c, size_t first, uint32_t K, const void* const* u,
               const void* const* w, const void** d_u, const void** d_w) const
  {
    for (uint32_t j = 0; j < K; j++)
      if (copy_in(c, first + 2 * j, u[j], &d_u[j]) ||
          copy_in(c, first + 2 * j + 1, w[j], &d_w[j]))
        return -1;
    return 0;
  }
};

// The host-pointer solve of diag(r) P diag(c) + sum_j u_j w_j^T: everything
// validated on the host first (dtype, opt's flags, flags, n, row_ptr, the
// columns, the scales row before column, K, the vectors, then the rows of the
// operator or - without terms - the empty rows); the workspace holds
// [row_ptr | col_idx | r | c | u_0 | w_0 | u_1 | ...]
template <typename T>
int
check_pattern_host_t(uint32_t n, const int64_t* row_ptr, const int32_t* col_idx,
                     const void* r, const void* c, uint32_t K, const void* const* u,
                     const void* const* w, bool scales_only)
{
  char msg[384];
  if (scales_only) {
    if (csr::check_pattern_scales<T>(n, static_cast<const T*>(r),
                                     static_cast<const T*>(c), msg, sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
    return 0;
  }
  const T* uu[csr::kTermsMax] = {};
  const T* ww[csr::kTermsMax] = {};
  for (uint32_t j = 0; j < K; j++) {
    uu[j] = static_cast<const T*>(u[j]);
    ww[j] = static_cast<const T*>(w[j]);
  }
  if (csr::check_terms_vectors<T>(n, K, uu, ww, msg, sizeof(msg)) ||
      csr::check_pattern_terms_rows<T>(n, row_ptr, col_idx, static_cast<const T*>(r),
                                       static_cast<const T*>(c), K, uu, ww, msg,
                                       sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  return 0;
}

int64_t
solve_host_csr_pattern(Context* c, int dtype, uint32_t n, uint64_t nnz,
                       const int64_t* row_ptr, const int32_t* col_idx,
                       const void* row_scale, const void* col_scale, uint32_t K,
                       const void* const* u, const void* const* w, uint32_t flags,
                       void* eigen_val, void* eigen_vec, uint32_t* iter_cnt,
                       const st_options* opt, st_stats* stats)
{
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "max_eigen_value_csr_pattern_ex: unknown flags %u", flags);
  {
    char msg[384];
    if (csr::check_pattern_host(dtype, n, nnz, row_ptr, col_idx, msg, sizeof(msg),
                                (flags & csr::kEmptyRowsOk) != 0)) {
      set_error("%s", msg);
      return -1;
    }
  }
  if (dtype ? check_pattern_host_t<double>(n, row_ptr, col_idx, row_scale, col_scale, 0,
                                           nullptr, nullptr, true)
            : check_pattern_host_t<float>(n, row_ptr, col_idx, row_scale, col_scale, 0,
                                          nullptr, nullptr, true))
    return -1;
  {
    char msg[384];
    if (csr::check_pattern_terms_count(K, msg, sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
  }
  if (K) {
    ST_REQUIRE(u && w, "csr terms: null vector table");
    if (dtype ? check_pattern_host_t<double>(n, row_ptr, col_idx, row_scale, col_scale,
                                             K, u, w, false)
              : check_pattern_host_t<float>(n, row_ptr, col_idx, row_scale, col_scale, K,
                                            u, w, false))
      return -1;
  } else {
    uint32_t lowest = n;
    const uint32_t empty = csr::count_empty_rows(row_ptr, n, &lowest);
    if (empty) {
      char msg[384];
      csr::describe_pattern_needs_terms("max_eigen_value_csr_pattern_ex", lowest, empty,
                                        msg, sizeof(msg));
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz, false);
  if (c->mat.ensure(c->stream,
                    sl.bytes() + (2 + 2 * (size_t)K) * VecSlots::stride_of(dtype, n)))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  const VecSlots vs(base + sl.bytes(), dtype, n);
  const void* d_rs = nullptr;
  const void* d_cs = nullptr;
  const void* d_u[csr::kTermsMax] = {};
  const void* d_w[csr::kTermsMax] = {};
  const auto t0 = std::chrono::steady_clock::now();
  if (csr_copy_in(c, sl, base, dtype, n, nnz, row_ptr, col_idx, nullptr) ||
      vs.copy_in(c, 0, row_scale, &d_rs) || vs.copy_in(c, 1, col_scale, &d_cs) ||
      vs.terms_in(c, 2, K, u, w, d_u, d_w))
    return -1;
  ST_CHECK(hipStreamSynchronize(c->stream));
  CsrPatternHandle* h = nullptr;
  if (csr_pattern_create(dtype, n, nnz, sl.ptr(base), sl.col(base), d_rs, d_cs, c->stream,
                         &h, flags))
    return -1;
  CsrTermsHandle* t = nullptr;
  if (K && csr_pattern_terms_create(h, K, d_u, d_w, c->stream, &t)) {
    (void)csr_pattern_destroy(h);
    return -1;
  }
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc =
    solve_csr_pattern(c, h, nullptr, eigen_vec, eigen_val, iter_cnt, opt, &local, t);
  (void)csr_terms_destroy(t);
  (void)csr_pattern_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

// The host-pointer solve of A + sum_j u_j w_j^T: everything validated on the
// host first (dtype, flags, the matrix, K, the vectors u before w term by
// term, then the rows of the operator); the workspace holds
// [row_ptr | vals | col_idx | u_0 | w_0 | u_1 | ...]
template <typename T>
int
check_terms_host_t(uint32_t n, const int64_t* row_ptr, const void* vals, uint32_t K,
                   const void* const* u, const void* const* w)
{
  char msg[384];
  const T* uu[csr::kTermsMax] = {};
  const T* ww[csr::kTermsMax] = {};
  for (uint32_t j = 0; j < K; j++) {
    uu[j] = static_cast<const T*>(u[j]);
    ww[j] = static_cast<const T*>(w[j]);
  }
  if (csr::check_terms_vectors<T>(n, K, uu, ww, msg, sizeof(msg)) ||
      csr::check_terms_rows<T>(n, row_ptr, static_cast<const T*>(vals), K, uu, ww,
                               msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  return 0;
}

int64_t
solve_host_csr_terms(Context* c, int dtype, uint32_t n, uint64_t nnz,
                     const int64_t* row_ptr, const int32_t* col_idx,
                     const void* vals, uint32_t K, const void* const* u,
                     const void* const* w, uint32_t flags, void* eigen_val,
                     void* eigen_vec, uint32_t* iter_cnt, const st_options* opt,
                     st_stats* stats)
{
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "max_eigen_value_csr_terms_ex: unknown flags %u", flags);
  if (csr_check_host(dtype, n, nnz, row_ptr, col_idx, vals, flags))
    return -1;
  {
    char msg[384];
    if (csr::check_terms_count(K, msg, sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(u && w, "csr terms: null vector table");
  if (dtype ? check_terms_host_t<double>(n, row_ptr, vals, K, u, w)
            : check_terms_host_t<float>(n, row_ptr, vals, K, u, w))
    return -1;
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, sl.bytes() + 2 * K * VecSlots::stride_of(dtype, n)))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  const VecSlots vs(base + sl.bytes(), dtype, n);
  const void* d_u[csr::kTermsMax] = {};
  const void* d_w[csr::kTermsMax] = {};
  const auto t0 = std::chrono::steady_clock::now();
  CsrHandle* h = nullptr; // (the vectors first: csr_stage waits for every copy)
  if (vs.terms_in(c, 0, K, u, w, d_u, d_w) ||
      csr_stage(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals, flags, &h))
    return -1;
  CsrTermsHandle* t = nullptr;
  if (csr_terms_create(h, K, d_u, d_w, c->stream, &t)) {
    (void)csr_destroy(h);
    return -1;
  }
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc =
    solve_csr(c, h, nullptr, eigen_vec, eigen_val, iter_cnt, opt, &local, t);
  (void)csr_terms_destroy(t);
  (void)csr_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

// the context's cached device workspace holds the three arrays of a host
// matrix: [row_ptr | vals | col_idx], each at a 256-byte aligned offset
int64_t
solve_host_csr(Context* c, int dtype, uint32_t n, uint64_t nnz,
               const int64_t* row_ptr, const int32_t* col_idx, const void* vals,
               void* eigen_val, void* eigen_vec, uint32_t* iter_cnt,
               const st_options* opt, st_stats* stats)
{
  // host validation first: dtype, flags, then the matrix (row_ptr, col_idx)
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  if (csr_check_host(dtype, n, nnz, row_ptr, col_idx, vals))
    return -1;
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, sl.bytes()))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  const auto t0 = std::chrono::steady_clock::now();
  CsrHandle* h = nullptr;
  if (csr_stage(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals, 0, &h))
    return -1;
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc =
    solve_csr(c, h, nullptr, eigen_vec, eigen_val, iter_cnt, opt, &local);
  (void)csr_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

// The LEFT Perron vector of a host matrix: solve_host_csr on T(A), which is
// made on the device.  The workspace holds A's three arrays, then T(A)'s:
// [row_ptr | vals | col_idx | t_row_ptr | t_vals | t_col_idx].
int64_t
solve_host_csr_left(Context* c, int dtype, uint32_t n, uint64_t nnz,
                    const int64_t* row_ptr, const int32_t* col_idx,
                    const void* vals, void* eigen_val, void* eigen_vec,
                    uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  ST_REQUIRE(nnz < (1ull << 32),
             "csr transpose: nnz must be below 2^32, got %llu: the sort "
             "carries 32-bit entry indices", (unsigned long long)nnz);
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  if (csr_check_host(dtype, n, nnz, row_ptr, col_idx, vals))
    return -1;
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, 2 * sl.bytes()))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  char* base_t = base + sl.bytes();
  const auto t0 = std::chrono::steady_clock::now();
  CsrHandle* h = nullptr;
  if (csr_stage(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals, 0, &h))
    return -1;
  const double h2d = ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  CsrHandle* ht = nullptr;
  const int trc =
    csr_transpose(h, sl.ptr(base_t), sl.col(base_t), sl.val(base_t), c->stream, &ht);
  (void)csr_destroy(h);
  if (trc)
    return -1;
  const double tr_ms = ms_since(t1);
  st_stats local{};
  const int64_t rc =
    solve_csr(c, ht, nullptr, eigen_vec, eigen_val, iter_cnt, opt, &local);
  (void)csr_destroy(ht);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats, tr_ms);
}

// The solve on the product operator B A of two validated handles (never
// formed): solve_csr's loop with st_csr_product.hip's launchers.  Checked
// before any round, in this order: the flags, the pair (n, dtype, device), the
// queue's device, then s_0 of the operator on the device - every row finite
// and > 0, the lowest offender named (a row of M with a positive entry stays
// positive for every positive x, so no round divides by zero).
int64_t
solve_csr_product(Context* c, const CsrHandle* b, const CsrHandle* a, void* d_v_out,
                  void* v_host, void* eigen_val, uint32_t* iter_cnt,
                  const st_options* opt, st_stats* stats)
{
  if (csr_product_check_pair(b, a, "st_solve_csr_product"))
    return -1;
  if (csr_check_flags(opt))
    return -1;
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(c->device == a->device,
             "csr product solve: the matrices live on device %d, the queue on %d",
             a->device, c->device);
  ST_REQUIRE(eigen_val && iter_cnt, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  const size_t elem = a->dtype ? 8 : 4;
  if (ensure_device(c) || ensure_vectors(c, elem * (size_t)a->n) ||
      c->part.ensure(c->stream, 256))
    return -1;
  {
    // s_0 into the loop's own first buffer, y in the ring's second slot; the
    // solve computes both again
    void* s0 = c->vec_slot<char>(0);
    void* y = c->vec_slot<char>(5);
    unsigned long long* d_err = static_cast<unsigned long long*>(c->part.p);
    unsigned long long err = 0;
    ST_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(err), c->stream));
    if (launch_csr_product_rowsum(b, a, s0, y, c->stream) ||
        launch_csr_product_check_s0(a->dtype, s0, a->n, d_err, c->stream))
      return -1;
    ST_CHECK(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    ST_CHECK(hipStreamSynchronize(c->stream));
    if (err != ~0ull) {
      char msg[384];
      csr::describe_product_row((uint32_t)err, msg, sizeof(msg));
      set_error("%s", msg);
      return -1;
    }
  }
  return solve_operator(c, Operator::product(b, a), a->dtype, d_v_out, v_host, eigen_val,
                        iter_cnt, opt, stats);
}

// The host-pointer solve of B A: everything validated on the host first
// (dtype, opt's flags, `flags`, B's triple, A's triple, the rows of B A); the
// workspace holds B's three arrays, then A's
int64_t
solve_host_csr_product(Context* c, int dtype, uint32_t n, uint64_t b_nnz,
                       const int64_t* b_row_ptr, const int32_t* b_col_idx,
                       const void* b_vals, uint64_t a_nnz, const int64_t* a_row_ptr,
                       const int32_t* a_col_idx, const void* a_vals, uint32_t flags,
                       void* eigen_val, void* eigen_vec, uint32_t* iter_cnt,
                       const st_options* opt, st_stats* stats)
{
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "max_eigen_value_csr_product_ex: unknown flags %u", flags);
  {
    char msg[384];
    std::vector<unsigned char> a_pos(n && n < 0x80000000u ? n : 1);
    if (csr::check_product_host(dtype, n, b_nnz, b_row_ptr, b_col_idx, b_vals, a_nnz,
                                a_row_ptr, a_col_idx, a_vals, flags, a_pos.data(), msg,
                                sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sb = csr_slots(dtype, n, b_nnz), sa = csr_slots(dtype, n, a_nnz);
  if (c->mat.ensure(c->stream, sb.bytes() + sa.bytes()))
    return -1;
  char* base_b = static_cast<char*>(c->mat.p);
  char* base_a = base_b + sb.bytes();
  const auto t0 = std::chrono::steady_clock::now();
  if (csr_copy_in(c, sb, base_b, dtype, n, b_nnz, b_row_ptr, b_col_idx, b_vals) ||
      csr_copy_in(c, sa, base_a, dtype, n, a_nnz, a_row_ptr, a_col_idx, a_vals))
    return -1;
  ST_CHECK(hipStreamSynchronize(c->stream));
  CsrHandle* hb = nullptr;
  if (csr_create(dtype, n, b_nnz, sb.ptr(base_b), sb.col(base_b), sb.val(base_b),
                 c->stream, &hb))
    return -1;
  CsrHandle* ha = nullptr;
  if (csr_create(dtype, n, a_nnz, sa.ptr(base_a), sa.col(base_a), sa.val(base_a),
                 c->stream, &ha, flags)) {
    (void)csr_destroy(hb);
    return -1;
  }
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc = solve_csr_product(c, hb, ha, nullptr, eigen_vec, eigen_val,
                                       iter_cnt, opt, &local);
  (void)csr_destroy(ha);
  (void)csr_destroy(hb);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

// The Gram operators of ONE host matrix: side 0 = A^T A, 1 = A A^T.  Validated
// on the host (nnz < 2^32, the side, dtype, flags, the triple, then the product
// on a host transposition), A copied in and transposed on the device
// (st_csr_transpose_ex, empty rows and columns legal there: what the product
// cannot take the host check has refused)
int64_t
solve_host_csr_gram(Context* c, int dtype, uint32_t n, uint64_t nnz,
                    const int64_t* row_ptr, const int32_t* col_idx, const void* vals,
                    int side, uint32_t flags, void* eigen_val, void* eigen_vec,
                    uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  char msg[384];
  if (csr::check_transpose_nnz(nnz, msg, sizeof(msg)) ||
      csr::check_gram_side(side, msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_check_flags(opt))
    return -1;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "max_eigen_value_csr_gram_ex: unknown flags %u", flags);
  if (csr_check_host(dtype, n, nnz, row_ptr, col_idx, vals, flags))
    return -1;
  {
    const size_t elem = dtype ? 8 : 4;
    std::vector<int64_t> t_ptr((size_t)n + 1);
    std::vector<int32_t> t_col(nnz);
    std::vector<unsigned char> t_val(elem * nnz), a_pos(n);
    if (csr::transpose_host(dtype, n, nnz, row_ptr, col_idx, vals, t_ptr.data(),
                            t_col.data(), t_val.data(), msg, sizeof(msg),
                            csr::kEmptyRowsOk) ||
        (side == 0 ? csr::check_product_host(dtype, n, nnz, t_ptr.data(), t_col.data(),
                                             t_val.data(), nnz, row_ptr, col_idx, vals,
                                             csr::kEmptyRowsOk, a_pos.data(), msg,
                                             sizeof(msg))
                   : csr::check_product_host(dtype, n, nnz, row_ptr, col_idx, vals, nnz,
                                             t_ptr.data(), t_col.data(), t_val.data(),
                                             csr::kEmptyRowsOk, a_pos.data(), msg,
                                             sizeof(msg)))) {
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(eigen_val && eigen_vec && iter_cnt, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, 2 * sl.bytes()))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  char* base_t = base + sl.bytes();
  const auto t0 = std::chrono::steady_clock::now();
  CsrHandle* h = nullptr;
  if (csr_stage(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals, csr::kEmptyRowsOk, &h))
    return -1;
  const double h2d = ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  CsrHandle* ht = nullptr;
  if (csr_transpose(h, sl.ptr(base_t), sl.col(base_t), sl.val(base_t), c->stream, &ht,
                    csr::kEmptyRowsOk)) {
    (void)csr_destroy(h);
    return -1;
  }
  const double tr_ms = ms_since(t1);
  st_stats local{};
  const int64_t rc =
    side == 0 ? solve_csr_product(c, ht, h, nullptr, eigen_vec, eigen_val, iter_cnt, opt,
                                  &local)
              : solve_csr_product(c, h, ht, nullptr, eigen_vec, eigen_val, iter_cnt, opt,
                                  &local);
  (void)csr_destroy(ht);
  (void)csr_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats, tr_ms);
}

// The counted round loop of the batched forms: round(k), k = 0, 1, ..., is
// enqueued `per_check` at a time (the last batch cut at max_itr), then the
// device's count of finished entries is mirrored into one of two pinned words
// and an event recorded.  While that batch runs the host waits for the batch
// before it and stops enqueuing once its count has reached `target`.  Returns
// the rounds enqueued, -1 on an error.  round is a lambda: this loop is the
// latency of a small batched call.
template <typename Round>
int64_t
counted_rounds(Context* c, uint32_t per_check, uint32_t max_itr, uint32_t target,
               Round&& round)
{
  hipStream_t s = c->stream;
  uint32_t enqueued = 0, batch_no = 0;
  bool done = false;
  while (!done && enqueued < max_itr) {
    const uint32_t b = (max_itr - enqueued) < per_check ? (max_itr - enqueued)
                                                        : per_check;
    for (uint32_t j = 0; j < b; j++)
      if (round(enqueued + j))
        return -1;
    enqueued += b;
    const int slot = batch_no & 1;
    if (launch_count_mirror(c->d_bcount, &c->h_bcount[slot], s))
      return -1;
    ST_CHECK(hipEventRecord(c->ev_flag[slot], s));
    // wait for the previous batch's count while this batch runs
    if (batch_no > 0) {
      ST_CHECK(hipEventSynchronize(c->ev_flag[slot ^ 1]));
      done = c->h_bcount[slot ^ 1] >= target;
    }
    batch_no++;
  }
  return enqueued;
}

// What every batched form ends with, its states read back into res [count]
// (Rec: st_state or CsrBatchResult) after loop_ms: per entry the done flag
// (`noun` names the entry in the message), lambda, count and converged flag;
// the eigenvectors to the host; the call's stats, `launches` in
// fused_launches.  Returns the call's milliseconds.
template <typename T, typename Rec>
int64_t
report_entries(const Rec* res, uint32_t count, const char* noun, T* eigen_vals,
               uint32_t* iter_cnts, uint32_t* converged, T* v_host, const T* d_v,
               size_t v_bytes, double loop_ms, uint32_t launches, st_stats* stats)
{
  const auto t1 = std::chrono::steady_clock::now();
  uint32_t rounds = 0, all = 1;
  for (uint32_t b = 0; b < count; b++) {
    const Rec& fin = res[b];
    ST_REQUIRE(fin.done, "internal: %s %u ended without done flag", noun, b);
    eigen_vals[b] = (T)fin.lambda;
    iter_cnts[b] = fin.iters;
    if (converged)
      converged[b] = fin.stop;
    rounds = fin.end > rounds ? fin.end : rounds;
    all &= fin.stop;
  }
  if (v_host)
    ST_CHECK(hipMemcpy(v_host, d_v, v_bytes, hipMemcpyDeviceToHost));
  const double d2h_ms = ms_since(t1);
  if (stats) {
    stats->loop_ms = loop_ms;
    stats->d2h_ms = d2h_ms;
    stats->rounds = rounds;
    stats->converged = all;
    stats->fused_launches = launches;
  }
  return (int64_t)loop_ms;
}

// the dense batched forms: the state array into the context's host copy first
template <typename T>
int64_t
report_bstates(Context* c, uint32_t batch, T* eigen_vals, uint32_t* iter_cnts,
               uint32_t* converged, T* v_host, const T* d_v, size_t v_bytes,
               std::chrono::steady_clock::time_point t0, uint32_t launches,
               st_stats* stats)
{
  ST_CHECK(hipStreamSynchronize(c->stream));
  c->h_bstate.resize(batch);
  ST_CHECK(hipMemcpy(c->h_bstate.data(), c->bstate.p, sizeof(st_state) * (size_t)batch,
                     hipMemcpyDeviceToHost));
  return report_entries<T>(c->h_bstate.data(), batch, "matrix", eigen_vals, iter_cnts,
                           converged, v_host, d_v, v_bytes, ms_since(t0), launches, stats);
}

// The solve of a validated batch in stacked CSR storage
// (st_csr_batch_create): solve_batched_rounds' host loop - one memset of the
// states and the finished counter, one fill of v, K0, then opt->batch rounds
// per look at the mirrored counter - with st_csr_batch.hip's two launches per
// round for the whole batch.  Every matrix keeps its own state and stops in
// its own round; k_csrb_collect picks each eigenvector from the ping-pong
// buffer its end's parity names.  Everything is checked before anything is
// enqueued.  Workspace: [s0 | s1 | v0 | v1 | x | out] in the vector buffer.
template <typename T>
int64_t
solve_csr_batched_t(Context* c, const CsrBatchHandle* h, T* d_v_out, T* v_host,
                    T* eigen_vals, uint32_t* iter_cnts, uint32_t* converged,
                    const Resolved& o, st_stats* stats)
{
  const uint32_t batch = h->batch;
  const size_t v_bytes = sizeof(T) * (size_t)h->n;
  if (ensure_device(c) || ensure_vectors(c, v_bytes) || ensure_bstate(c, batch) ||
      ensure_bsum(c, 256) ||
      c->part.ensure(c->stream, sizeof(CsrBatchResult) * (size_t)batch))
    return -1;
  T* s_buf[2] = { c->vec_slot<T>(0), c->vec_slot<T>(1) };
  T* vb[2] = { c->vec_slot<T>(2), c->vec_slot<T>(3) };
  T* d_x = c->vec_slot<T>(4);
  T* d_v = d_v_out ? d_v_out : c->vec_slot<T>(5);
  CsrBatchResult* d_res = static_cast<CsrBatchResult*>(c->part.p);
  hipStream_t s = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * (size_t)batch, s));
  ST_CHECK(hipMemsetAsync(c->d_bcount, 0, sizeof(uint32_t), s));
  if (launch_fill<T>(vb[0], h->n, (T)1, s))
    return -1;
  if (launch_csrb_rowsum(h, s_buf[0], s)) // K0
    return -1;
  const int64_t enqueued = counted_rounds(
    c, o.batch ? o.batch : kDefaultBatch, o.max_itr, batch,
    [&](uint32_t k) { // launch k+1 evaluates round k
      return launch_csrb_round(h, s_buf[k & 1], s_buf[(k + 1) & 1], vb[k & 1],
                               vb[(k + 1) & 1], d_x, o.eps, k + 1, o.max_itr, o.semantics,
                               c->d_bstate(), c->d_bcount, s);
    });
  if (enqueued < 0)
    return -1;
  if (launch_csrb_collect(h, vb[0], vb[1], d_v, c->d_bstate(), d_res, s))
    return -1;
  ST_CHECK(hipStreamSynchronize(s));
  std::vector<CsrBatchResult> res(batch);
  ST_CHECK(hipMemcpy(res.data(), d_res, sizeof(CsrBatchResult) * (size_t)batch,
                     hipMemcpyDeviceToHost));
  const double loop_ms = ms_since(t0);
  if (stats)
    std::memset(stats, 0, sizeof(*stats));
  return report_entries<T>(res.data(), batch, "matrix", eigen_vals, iter_cnts, converged,
                           v_host, d_v, v_bytes, loop_ms, (uint32_t)enqueued, stats);
}

int64_t
solve_csr_batched(Context* c, const CsrBatchHandle* h, void* d_v_out,
                  void* v_host, void* eigen_vals, uint32_t* iter_cnts,
                  uint32_t* converged, const st_options* opt, st_stats* stats)
{
  if (csr_batch_check_flags(opt))
    return -1;
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(c->device == h->device,
             "csr batched solve: the batch lives on device %d, the queue on %d",
             h->device, c->device);
  ST_REQUIRE(eigen_vals && iter_cnts, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  Resolved o;
  if (h->dtype ? resolve<double>(opt, &o) : resolve<float>(opt, &o))
    return -1;
  if (h->dtype)
    return solve_csr_batched_t<double>(
      c, h, static_cast<double*>(d_v_out), static_cast<double*>(v_host),
      static_cast<double*>(eigen_vals), iter_cnts, converged, o, stats);
  return solve_csr_batched_t<float>(
    c, h, static_cast<float*>(d_v_out), static_cast<float*>(v_host),
    static_cast<float*>(eigen_vals), iter_cnts, converged, o, stats);
}

// the host twin: [row_ptr | vals | col_idx] of the stacked batch in the
// context's cached device workspace, as solve_host_csr
int64_t
solve_host_csr_batched(Context* c, int dtype, uint32_t batch,
                       const uint32_t* mat_first, uint64_t nnz,
                       const int64_t* row_ptr, const int32_t* col_idx,
                       const void* vals, void* eigen_vals, void* eigen_vecs,
                       uint32_t* iter_cnts, uint32_t* converged,
                       const st_options* opt, st_stats* stats)
{
  // host validation first: dtype, flags, then the batch (mat_first, row_ptr,
  // col_idx)
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_batch_check_flags(opt))
    return -1;
  if (csr_batch_check_host(dtype, batch, mat_first, nnz, row_ptr, col_idx, vals))
    return -1;
  ST_REQUIRE(eigen_vals && eigen_vecs && iter_cnts, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const uint32_t n = mat_first[batch];
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, sl.bytes()))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  const auto t0 = std::chrono::steady_clock::now();
  if (csr_copy_in(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals))
    return -1;
  ST_CHECK(hipStreamSynchronize(c->stream));
  CsrBatchHandle* h = nullptr;
  if (csr_batch_create(dtype, batch, mat_first, nnz, sl.ptr(base), sl.col(base),
                       sl.val(base), c->stream, &h))
    return -1;
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc = solve_csr_batched(c, h, nullptr, eigen_vecs, eigen_vals,
                                       iter_cnts, converged, opt, &local);
  (void)csr_batch_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

// The solve of up to 8 operators A + sum_j u_{c,j} w_{c,j}^T on one matrix
// (st_csr_multi_create): solve_csr_batched's host loop - one memset of the C
// states and the finished counter, one fill of v, K0, then opt->batch rounds
// per look at the mirrored counter - with st_csr_multi.hip's three launches
// per round for all columns.  Every column keeps its own state and stops in
// its own round; the collect kernel picks each eigenvector from the ping-pong
// buffer its end's parity names.  The packed vectors are the object's own.
template <typename T>
int64_t
solve_csr_multi_t(Context* c, const CsrHandle* h, const CsrMultiHandle* t, T* d_v_out,
                  T* v_host, T* eigen_vals, uint32_t* iter_cnts, uint32_t* converged,
                  const Resolved& o, st_stats* stats)
{
  const uint32_t C = t->C;
  const size_t out_bytes = sizeof(T) * (size_t)h->n * C;
  if (ensure_device(c) || ensure_bstate(c, C) || ensure_bsum(c, 256) ||
      c->part.ensure(c->stream, sizeof(CsrBatchResult) * (size_t)C))
    return -1;
  DeviceBuf tmp_out; // host output only: the collected [C][n] lives for this call
  struct Release
  {
    DeviceBuf& b;
    ~Release() { b.release(); }
  } release_tmp{ tmp_out };
  hipStream_t s = c->stream;
  if (!d_v_out) {
    if (tmp_out.ensure(s, out_bytes))
      return -1;
    d_v_out = static_cast<T*>(tmp_out.p);
  }
  CsrBatchResult* d_res = static_cast<CsrBatchResult*>(c->part.p);
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * (size_t)C, s));
  ST_CHECK(hipMemsetAsync(c->d_bcount, 0, sizeof(uint32_t), s));
  if (launch_fill<T>(static_cast<T*>(t->v[0]), (uint64_t)h->n * t->CP, (T)1, s))
    return -1;
  if (launch_csr_multi_rowsum(h, t, t->s[0], t->scratch, s)) // K0
    return -1;
  const int64_t enqueued = counted_rounds(
    c, o.batch ? o.batch : kDefaultBatch, o.max_itr, C,
    [&](uint32_t k) { // launch k+1 evaluates round k
      return launch_csr_multi_round(h, t, t->s[k & 1], t->s[(k + 1) & 1], t->v[k & 1],
                                    t->v[(k + 1) & 1], t->scratch, o.eps, k + 1, o.max_itr,
                                    o.semantics, c->d_bstate(), c->d_bcount, s);
    });
  if (enqueued < 0)
    return -1;
  if (launch_csr_multi_collect(t, t->v[0], t->v[1], d_v_out, c->d_bstate(), d_res, s))
    return -1;
  ST_CHECK(hipStreamSynchronize(s));
  CsrBatchResult res[csr::kMultiMax];
  ST_CHECK(hipMemcpy(res, d_res, sizeof(CsrBatchResult) * (size_t)C,
                     hipMemcpyDeviceToHost));
  const double loop_ms = ms_since(t0);
  if (stats)
    std::memset(stats, 0, sizeof(*stats));
  return report_entries<T>(res, C, "column", eigen_vals, iter_cnts, converged, v_host,
                           d_v_out, out_bytes, loop_ms, (uint32_t)enqueued, stats);
}

int
csr_multi_check_flags(const st_options* opt)
{
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNo = ST_FLAG_TIME_KERNELS | ST_FLAG_TRACE_SUMS |
                           ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND |
                           ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNo) == 0,
             "csr multi solve: ST_FLAG_TIME_KERNELS, ST_FLAG_TRACE_SUMS, "
             "ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix is "
             "read only and every round is the same three launches for all "
             "columns", flags);
  ST_REQUIRE(!opt || opt->semantics <= ST_SEM_MAINPY, "unknown semantics %u",
             opt->semantics);
  return 0;
}

int64_t
solve_csr_multi(Context* c, const CsrHandle* h, const CsrMultiHandle* t, void* d_v_out,
                void* v_host, void* eigen_vals, uint32_t* iter_cnts,
                uint32_t* converged, const st_options* opt, st_stats* stats)
{
  if (csr_multi_check_flags(opt))
    return -1;
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(c->device == h->device,
             "csr multi solve: the matrix lives on device %d, the queue on %d",
             h->device, c->device);
  ST_REQUIRE(eigen_vals && iter_cnts, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  Resolved o;
  if (h->dtype ? resolve<double>(opt, &o) : resolve<float>(opt, &o))
    return -1;
  if (h->dtype)
    return solve_csr_multi_t<double>(
      c, h, t, static_cast<double*>(d_v_out), static_cast<double*>(v_host),
      static_cast<double*>(eigen_vals), iter_cnts, converged, o, stats);
  return solve_csr_multi_t<float>(
    c, h, t, static_cast<float*>(d_v_out), static_cast<float*>(v_host),
    static_cast<float*>(eigen_vals), iter_cnts, converged, o, stats);
}

// The Perron pair of a device-resident dense matrix (A v = lambda v and
// u A = lambda u): solve_csr_multi_t's host loop - one memset of the two
// states and the finished counter, one fill of both v, launch 0, then
// opt->batch rounds per look at the mirrored counter - with st_pair.hip's five
// launches per round, whose sweep reads the matrix once for both sides.  Each
// side keeps its own state and stops in its own round; its eigenvector lies in
// the ping-pong buffer its end's parity names.  The matrix is only read and
// never copied.  Workspace: [s_R0 | s_R1 | s_L0 | s_L1 | v_R0 | v_L0 | v_R1 |
// v_L1] in the vector buffer, the round's scratch in the partials' buffer.
// Everything is checked before anything is enqueued.
int
pair_check_flags(const st_options* opt)
{
  const uint32_t flags = opt ? opt->flags : 0u;
  constexpr uint32_t kNo = ST_FLAG_TIME_KERNELS | ST_FLAG_TRACE_SUMS |
                           ST_FLAG_ROUND_LOOP | ST_FLAG_WRITE_EVERY_ROUND |
                           ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((flags & kNo) == 0,
             "dense pair solve: ST_FLAG_TIME_KERNELS, ST_FLAG_TRACE_SUMS, "
             "ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and "
             "ST_FLAG_BATCH_ROUNDS are not supported (flags = %u): the matrix is "
             "read only and every round is the same five launches for both sides",
             flags);
  return 0;
}

template <typename T>
int64_t
solve_pair_t(Context* c, const T* d_mat, uint32_t n, T* d_v_out, T* v_host, T* eigen_vals,
             uint32_t* iter_cnts, uint32_t* converged, const Resolved& o, st_stats* stats)
{
  {
    left::Grid g;
    uint64_t want = 0;
    ST_REQUIRE(pair::grid(n, left_rows(sizeof(T) == 8, n), sizeof(T), &g, &want),
               "dense pair: dim = %u needs %llu workgroups per launch, above %llu", n,
               (unsigned long long)want, (unsigned long long)left::kGridMax);
  }
  const size_t v_bytes = sizeof(T) * (size_t)n;
  if (ensure_device(c) || ensure_vectors(c, v_bytes) || ensure_bstate(c, 2) ||
      ensure_bsum(c, 256) ||
      c->part.ensure(c->stream, sizeof(T) * pair_scratch_elems(sizeof(T) == 8, n)))
    return -1;
  T* sb[2][2] = { { c->vec_slot<T>(0), c->vec_slot<T>(1) },   // [side][parity]
                  { c->vec_slot<T>(2), c->vec_slot<T>(3) } };
  T* vb[2][2] = { { c->vec_slot<T>(4), c->vec_slot<T>(6) },   // both v_0 adjacent
                  { c->vec_slot<T>(5), c->vec_slot<T>(7) } };
  T* scratch = static_cast<T*>(c->part.p);
  hipStream_t s = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * 2, s));
  ST_CHECK(hipMemsetAsync(c->d_bcount, 0, sizeof(uint32_t), s));
  if (launch_fill<T>(vb[0][0], (uint64_t)(c->vec_bytes / sizeof(T)) + n, (T)1, s))
    return -1;
  if (launch_pair_sum<T>(d_mat, sb[pair::kRight][0], sb[pair::kLeft][0], scratch, n, s))
    return -1;
  const int64_t enqueued = counted_rounds(
    c, o.batch ? o.batch : kDefaultBatch, o.max_itr, 2,
    [&](uint32_t k) { // launch k+1 evaluates round k
      const uint32_t a = k & 1, b = (k + 1) & 1;
      const PairVectors<T> v = { { sb[0][a], sb[1][a] },
                                 { sb[0][b], sb[1][b] },
                                 { vb[0][a], vb[1][a] },
                                 { vb[0][b], vb[1][b] } };
      return launch_pair_round<T>(d_mat, v, scratch, n, (T)o.eps, k + 1, o.max_itr,
                                  o.semantics, c->d_bstate(), c->d_bcount, s);
    });
  if (enqueued < 0)
    return -1;
  ST_CHECK(hipStreamSynchronize(s));
  st_state res[2];
  ST_CHECK(hipMemcpy(res, c->bstate.p, sizeof(res), hipMemcpyDeviceToHost));
  const double loop_ms = ms_since(t0);
  st_stats local{};
  const int64_t rc =
    report_entries<T>(res, 2, "side", eigen_vals, iter_cnts, converged, (T*)nullptr,
                      (const T*)nullptr, 0, loop_ms, (uint32_t)enqueued, &local);
  if (rc < 0)
    return -1;
  const auto t1 = std::chrono::steady_clock::now();
  for (uint32_t side = 0; side < 2; side++) { // launch `end` wrote v into buffer end & 1
    const T* fin = vb[side][res[side].end & 1u];
    if (d_v_out)
      ST_CHECK(hipMemcpyAsync(d_v_out + (size_t)side * n, fin, v_bytes,
                              hipMemcpyDeviceToDevice, s));
    if (v_host)
      ST_CHECK(hipMemcpyAsync(v_host + (size_t)side * n, fin, v_bytes,
                              hipMemcpyDeviceToHost, s));
  }
  ST_CHECK(hipStreamSynchronize(s));
  local.d2h_ms = ms_since(t1);
  if (stats)
    *stats = local;
  return rc;
}

template <typename T>
int64_t
solve_device_pair(Context* c, const T* d_mat, uint32_t n, T* d_v_out, T* v_host,
                  T* eigen_vals, uint32_t* iter_cnts, uint32_t* converged,
                  const st_options* opt, st_stats* stats)
{
  if (pair_check_flags(opt))
    return -1;
  Resolved o;
  if (resolve<T>(opt, &o))
    return -1;
  ST_REQUIRE(d_mat, "dense pair solve: null matrix");
  ST_REQUIRE(n > 0, "dense pair solve: dim must be > 0");
  ST_REQUIRE(((uintptr_t)d_mat & (sizeof(T) - 1)) == 0,
             "dense pair solve: matrix not aligned to its element size");
  ST_REQUIRE(eigen_vals && iter_cnts, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  ST_REQUIRE(c, "null queue");
  return solve_pair_t<T>(c, d_mat, n, d_v_out, v_host, eigen_vals, iter_cnts, converged, o,
                         stats);
}

// the host twin: max_eigen_value_left_ex's check order and staging (one
// slot, copied in once and only read; no transposed copy)
template <typename T>
int64_t
solve_host_pair(Context* c, const T* mat, uint32_t n, T* eigen_vals, T* eigen_vecs,
                uint32_t* iter_cnts, uint32_t* converged, const st_options* opt,
                st_stats* stats)
{
  if (pair_check_flags(opt))
    return -1;
  {
    Resolved o;
    if (resolve<T>(opt, &o))
      return -1;
  }
  ST_REQUIRE(mat, "max_eigen_value_pair_ex: null matrix");
  ST_REQUIRE(n > 0, "max_eigen_value_pair_ex: dim must be > 0");
  ST_REQUIRE(eigen_vals && eigen_vecs && iter_cnts, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(n <= left::kNMax && left::stage_fits(n, sizeof(T)),
             "max_eigen_value_pair_ex: dim = %u is too large", n);
  if (c->mat.ensure(c->stream, (size_t)left::stage_bytes(n, sizeof(T))))
    return -1;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mat, sizeof(T) * (size_t)n * n, hipMemcpyHostToDevice,
                          c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  st_stats local{};
  if (solve_device_pair<T>(c, static_cast<const T*>(c->mat.p), n, nullptr, eigen_vecs,
                           eigen_vals, iter_cnts, converged, opt, &local) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

// The host-pointer twin: everything validated on the host first (dtype,
// flags, the matrix, C and K, then column after column the vectors and the
// rows of M_c), the terms packed on the host (csr::pack_columns) and copied
// in packed; the workspace holds [row_ptr | vals | col_idx].
template <typename T>
int
multi_host_pack_t(uint32_t n, const int64_t* row_ptr, const void* vals, uint32_t C,
                  uint32_t K, const void* const* u, const void* const* w,
                  std::vector<unsigned char>* pu, std::vector<unsigned char>* pw)
{
  char msg[448];
  const T* uu[csr::kMultiMax * csr::kTermsMax] = {};
  const T* ww[csr::kMultiMax * csr::kTermsMax] = {};
  for (uint32_t i = 0; i < C * K; i++) {
    uu[i] = static_cast<const T*>(u[i]);
    ww[i] = static_cast<const T*>(w[i]);
  }
  if (csr::check_multi_terms<T>(n, row_ptr, static_cast<const T*>(vals), C, K, uu, ww,
                                msg, sizeof(msg))) {
    set_error("%s", msg);
    return -1;
  }
  const uint32_t CP = csr::multi_cp(C);
  const size_t per = (size_t)n * CP;
  pu->resize(sizeof(T) * per * K);
  pw->resize(sizeof(T) * per * K);
  for (uint32_t j = 0; j < K; j++) {
    csr::pack_columns<T>(n, C, CP, uu + j, K, reinterpret_cast<T*>(pu->data()) + per * j);
    csr::pack_columns<T>(n, C, CP, ww + j, K, reinterpret_cast<T*>(pw->data()) + per * j);
  }
  return 0;
}

int64_t
solve_host_csr_multi(Context* c, int dtype, uint32_t n, uint64_t nnz,
                     const int64_t* row_ptr, const int32_t* col_idx, const void* vals,
                     uint32_t C, uint32_t K, const void* const* u,
                     const void* const* w, uint32_t flags, void* eigen_vals,
                     void* eigen_vecs, uint32_t* iter_cnts, uint32_t* converged,
                     const st_options* opt, st_stats* stats)
{
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "csr: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  if (csr_multi_check_flags(opt))
    return -1;
  ST_REQUIRE((flags & ~csr::kEmptyRowsOk) == 0,
             "max_eigen_value_csr_multi_ex: unknown flags %u", flags);
  if (csr_check_host(dtype, n, nnz, row_ptr, col_idx, vals, flags))
    return -1;
  {
    char msg[384];
    if (csr::check_multi_count(C, K, msg, sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(u && w, "csr multi: null vector table");
  std::vector<unsigned char> pu, pw;
  if (dtype ? multi_host_pack_t<double>(n, row_ptr, vals, C, K, u, w, &pu, &pw)
            : multi_host_pack_t<float>(n, row_ptr, vals, C, K, u, w, &pu, &pw))
    return -1;
  ST_REQUIRE(eigen_vals && eigen_vecs && iter_cnts, "null output pointer");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  const CsrSlots sl = csr_slots(dtype, n, nnz);
  if (c->mat.ensure(c->stream, sl.bytes()))
    return -1;
  char* base = static_cast<char*>(c->mat.p);
  const auto t0 = std::chrono::steady_clock::now();
  CsrHandle* h = nullptr;
  if (csr_stage(c, sl, base, dtype, n, nnz, row_ptr, col_idx, vals, flags, &h))
    return -1;
  CsrMultiHandle* t = nullptr;
  if (csr_multi_create(h, C, K, nullptr, nullptr, c->stream, &t, pu.data(), pw.data())) {
    (void)csr_destroy(h);
    return -1;
  }
  const double h2d = ms_since(t0);
  st_stats local{};
  const int64_t rc = solve_csr_multi(c, h, t, nullptr, eigen_vecs, eigen_vals,
                                     iter_cnts, converged, opt, &local);
  (void)csr_multi_destroy(t);
  (void)csr_destroy(h);
  return rc < 0 ? -1 : finish_twin(local, h2d, stats);
}

template <typename T>
int64_t
solve_host(Context* c, const T* mat, uint32_t n, T* eigen_val, T* eigen_vec,
           uint32_t* iter_cnt, const st_options* opt, st_stats* stats)
{
  ST_REQUIRE(c, "null queue");
  ST_REQUIRE(mat && eigen_val && eigen_vec && iter_cnt, "null pointer");
  ST_REQUIRE(n > 0, "dim must be > 0");
  if (ensure_device(c))
    return -1;
  const size_t bytes = sizeof(T) * (size_t)n * n;
  if (c->mat.ensure(c->stream, bytes))
    return -1;
  // the reference's timed region starts before the first kernel, which
  // performs the lazy host->device copy (similarity_transform.cpp:36-40)
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mat, bytes, hipMemcpyHostToDevice,
                          c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  st_stats local{};
  if (solve_device<T>(c, Operator::dense(c->mat.p, n), nullptr, eigen_vec, eigen_val,
                      iter_cnt, opt, &local, false) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

// what both batched entry points reject before touching the device
template <typename T>
int
batched_args(Context* c, uint32_t batch, uint32_t n, const st_options* opt,
             Resolved* o)
{
  ST_REQUIRE(c, "null queue");
  if (resolve<T>(opt, o))
    return -1;
  constexpr uint32_t kNoBatch = ST_FLAG_MATRIX_FREE | ST_FLAG_TIME_KERNELS |
                                ST_FLAG_TRACE_SUMS | ST_FLAG_ROUND_LOOP;
  ST_REQUIRE((o->flags & kNoBatch) == 0,
             "batched solve: ST_FLAG_MATRIX_FREE, ST_FLAG_TIME_KERNELS, "
             "ST_FLAG_TRACE_SUMS and ST_FLAG_ROUND_LOOP are not supported "
             "(flags = %u)", o->flags);
  ST_REQUIRE(n > 0, "dim must be > 0");
  if (o->flags & ST_FLAG_BATCH_ROUNDS)
    ST_REQUIRE(n <= batched_rounds_max_n(sizeof(T)),
               "batched solve: dim = %u exceeds the round-loop limit %u "
               "(st_solve_batched_rounds_max_dim)", n,
               batched_rounds_max_n(sizeof(T)));
  else
    ST_REQUIRE(n <= solve_batched_max_n<T>(),
               "batched solve: dim = %u exceeds the one-workgroup limit %u "
               "(st_solve_batched_max_dim)", n, solve_batched_max_n<T>());
  ST_REQUIRE(batch <= 0x7fffffffu,
             "batched solve: batch = %u exceeds the grid limit 2^31 - 1", batch);
  return 0;
}

// The batched solve for matrices beyond one workgroup's registers
// (ST_FLAG_BATCH_ROUNDS): solve_device's round loop with every launch
// covering the whole batch (k_round_batched, blockIdx.y / .z = the matrix).
// Once per call: one memset of the states and the finished counter, one fill
// of v, one K0 pass over the batch seen as a tall (batch n) x n matrix (a
// row's sum does not depend on the rows around it).  Per host check
// (opt->batch rounds, default 8) one word, the count of finished matrices,
// is mirrored to pinned memory; the loop stops enqueuing once it reaches
// `batch`.  The caller (solve_batched) has checked the arguments and cleared
// the stats.
template <typename T>
int64_t
solve_batched_rounds(Context* c, T* d_mats, uint32_t batch, uint32_t n,
                     T* d_v_out, T* v_host, T* eigen_vals, uint32_t* iter_cnts,
                     uint32_t* converged, const Resolved& o, st_stats* stats)
{
  const size_t v_bytes = sizeof(T) * (size_t)batch * n;
  if (ensure_device(c) || ensure_bstate(c, batch) || ensure_bsum(c, v_bytes))
    return -1;
  T* s_buf[2] = { c->bsum_slot<T>(0), c->bsum_slot<T>(1) };
  T* d_v = d_v_out ? d_v_out : c->bsum_slot<T>(2);
  hipStream_t s = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * (size_t)batch, s));
  ST_CHECK(hipMemsetAsync(c->d_bcount, 0, sizeof(uint32_t), s));
  if (launch_fill<T>(d_v, (uint64_t)batch * n, (T)1, s))
    return -1;
  // K0, in passes of whole matrices whose rows fit the launcher's uint32_t
  const uint32_t per_pass = 0x7fffffffu / n;
  for (uint32_t b0 = 0; b0 < batch; b0 += per_pass) {
    const uint32_t nb = batch - b0 < per_pass ? batch - b0 : per_pass;
    if (launch_rowsum<T>(d_mats + (size_t)b0 * n * n, s_buf[0] + (size_t)b0 * n,
                         nb * n, n, s))
      return -1;
  }
  const T eps = (T)o.eps;
  const int64_t enqueued = counted_rounds(
    c, o.batch ? o.batch : kDefaultBatch, o.max_itr, batch, [&](uint32_t k) {
      return launch_round_batched<T>(d_mats, s_buf[k & 1], s_buf[(k + 1) & 1], d_v, batch,
                                     n, eps, k, o.max_itr, o.semantics, c->d_bstate(),
                                     c->d_bcount, s);
    });
  if (enqueued < 0)
    return -1;
  return report_bstates<T>(c, batch, eigen_vals, iter_cnts, converged, v_host, d_v,
                           v_bytes, t0, (uint32_t)enqueued, stats);
}

// Many small solves in one launch (k_solve_batched: a workgroup per matrix
// of the device-resident [batch][n][n] array, each transformed in place).
// One memset of the state array, one launch, one stream sync, one read-back.
template <typename T>
int64_t
solve_batched(Context* c, T* d_mats, uint32_t batch, uint32_t n, T* d_v_out,
              T* v_host, T* eigen_vals, uint32_t* iter_cnts,
              uint32_t* converged, const st_options* opt, st_stats* stats)
{
  Resolved o;
  if (batched_args<T>(c, batch, n, opt, &o))
    return -1;
  if (stats)
    std::memset(stats, 0, sizeof(*stats));
  if (batch == 0) { // nothing to solve
    if (stats)
      stats->converged = 1;
    return 0;
  }
  ST_REQUIRE(d_mats, "null matrix");
  ST_REQUIRE(eigen_vals && iter_cnts, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  if (o.flags & ST_FLAG_BATCH_ROUNDS) // one launch per round for the batch
    return solve_batched_rounds<T>(c, d_mats, batch, n, d_v_out, v_host,
                                   eigen_vals, iter_cnts, converged, o, stats);
  const size_t v_bytes = sizeof(T) * (size_t)batch * n;
  if (ensure_device(c) || ensure_bstate(c, batch) ||
      (!d_v_out && c->part.ensure(c->stream, v_bytes))) // part: free outside flat rounds
    return -1;
  T* d_v = d_v_out ? d_v_out : reinterpret_cast<T*>(c->part.p);
  hipStream_t s = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * (size_t)batch, s));
  if (launch_solve_batched<T>(d_mats, d_v, batch, n, (T)o.eps, o.max_itr,
                              o.semantics, c->d_bstate(), s))
    return -1;
  return report_bstates<T>(c, batch, eigen_vals, iter_cnts, converged, v_host, d_v,
                           v_bytes, t0, 0, stats);
}

// host-pointer twin: [mats | v] staged in the context's matrix buffer
template <typename T>
int64_t
solve_batched_host(Context* c, const T* mats, uint32_t batch, uint32_t n,
                   T* eigen_vals, T* eigen_vecs, uint32_t* iter_cnts,
                   const st_options* opt, st_stats* stats)
{
  Resolved o;
  if (batched_args<T>(c, batch, n, opt, &o))
    return -1;
  if (batch == 0) // the no-op, with its stats
    return solve_batched<T>(c, nullptr, 0, n, nullptr, nullptr, nullptr,
                            nullptr, nullptr, opt, stats);
  ST_REQUIRE(mats && eigen_vals && eigen_vecs && iter_cnts, "null pointer");
  const size_t bytes = up256(sizeof(T) * (size_t)batch * n * n); // v stays aligned
  if (ensure_device(c) ||
      c->mat.ensure(c->stream, bytes + sizeof(T) * (size_t)batch * n))
    return -1;
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mats, sizeof(T) * (size_t)batch * n * n,
                          hipMemcpyHostToDevice, c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  T* d_mats = reinterpret_cast<T*>(c->mat.p);
  T* d_v = reinterpret_cast<T*>((char*)c->mat.p + bytes);
  st_stats local{};
  if (solve_batched<T>(c, d_mats, batch, n, d_v, eigen_vecs, eigen_vals,
                       iter_cnts, nullptr, opt, &local) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

// The size-class plan of a variable-size batch (pure host code): a stable
// counting sort of the indices by solve_shape_class(dims[b]).  order[batch],
// class_first[kSolveShapeClasses + 1].  Returns the number of non-empty
// classes or -1 (a dim of 0 or above max_n, named with its index).
int
vbatched_plan(uint32_t max_n, const uint32_t* dims, uint32_t batch,
              uint32_t* order, uint32_t* class_first)
{
  uint32_t count[kSolveShapeClasses] = {};
  for (uint32_t b = 0; b < batch; b++) {
    ST_REQUIRE(dims[b] > 0, "vbatched solve: dims[%u] = 0, dim must be > 0", b);
    ST_REQUIRE(dims[b] <= max_n,
               "vbatched solve: dims[%u] = %u exceeds the one-workgroup limit "
               "%u (st_solve_batched_max_dim)", b, dims[b], max_n);
    count[solve_shape_class(dims[b])]++;
  }
  uint32_t next[kSolveShapeClasses];
  int used = 0;
  class_first[0] = 0;
  for (uint32_t k = 0; k < kSolveShapeClasses; k++) {
    next[k] = class_first[k];
    class_first[k + 1] = class_first[k] + count[k];
    used += count[k] ? 1 : 0;
  }
  for (uint32_t b = 0; b < batch; b++)
    order[next[solve_shape_class(dims[b])]++] = b;
  return used;
}

// what both variable-size entry points reject before touching the device
template <typename T>
int
vbatched_args(Context* c, uint32_t batch, const st_options* opt, Resolved* o)
{
  ST_REQUIRE(c, "null queue");
  if (resolve<T>(opt, o))
    return -1;
  constexpr uint32_t kNoVBatch = ST_FLAG_MATRIX_FREE | ST_FLAG_TIME_KERNELS |
                                 ST_FLAG_TRACE_SUMS | ST_FLAG_ROUND_LOOP |
                                 ST_FLAG_BATCH_ROUNDS;
  ST_REQUIRE((o->flags & kNoVBatch) == 0,
             "vbatched solve: ST_FLAG_MATRIX_FREE, ST_FLAG_TIME_KERNELS, "
             "ST_FLAG_TRACE_SUMS, ST_FLAG_ROUND_LOOP and ST_FLAG_BATCH_ROUNDS "
             "are not supported (flags = %u)", o->flags);
  ST_REQUIRE(batch <= 0x7fffffffu,
             "vbatched solve: batch = %u exceeds the grid limit 2^31 - 1", batch);
  return 0;
}

// Many small solves of different sizes: one k_solve_vbatched launch per
// non-empty shape class, largest class first, back to back on the stream.
// Per call: the plan, the descriptor table filled in plan order in pinned
// staging, one copy of it to the device, one memset of the states, the
// class launches, one stream sync, one state read-back.
template <typename T>
int64_t
solve_vbatched(Context* c, T* const* mat_ptrs, const uint32_t* dims,
               uint32_t batch, T* d_v_out, T* v_host, T* eigen_vals,
               uint32_t* iter_cnts, uint32_t* converged, const st_options* opt,
               st_stats* stats)
{
  Resolved o;
  if (vbatched_args<T>(c, batch, opt, &o))
    return -1;
  if (stats)
    std::memset(stats, 0, sizeof(*stats));
  if (batch == 0) { // nothing to solve
    if (stats)
      stats->converged = 1;
    return 0;
  }
  ST_REQUIRE(mat_ptrs && dims, "null matrix pointer array or dims");
  ST_REQUIRE(eigen_vals && iter_cnts, "null output pointer");
  ST_REQUIRE(d_v_out || v_host, "need a device or host eigenvector output");
  // everything that can be refused is refused here, before the first enqueue
  std::vector<uint32_t> order(batch);
  uint32_t class_first[kSolveShapeClasses + 1];
  const int used = vbatched_plan(solve_batched_max_n<T>(), dims, batch,
                                 order.data(), class_first);
  if (used < 0)
    return -1;
  for (uint32_t b = 0; b < batch; b++)
    ST_REQUIRE(mat_ptrs[b], "vbatched solve: d_mat_ptrs[%u] is NULL", b);
  size_t v_elems = 0;
  for (uint32_t b = 0; b < batch; b++)
    v_elems += dims[b];
  const size_t v_bytes = sizeof(T) * v_elems;
  if (ensure_device(c) || ensure_bstate(c, batch) || ensure_vbatch(c, batch) ||
      (!d_v_out && c->part.ensure(c->stream, v_bytes))) // part: free outside flat rounds
    return -1;
  T* d_v = d_v_out ? d_v_out : reinterpret_cast<T*>(c->part.p);
  hipStream_t s = c->stream;
  const auto t0 = std::chrono::steady_clock::now();
  // the table in plan order: entry j describes matrix order[j] (the
  // eigenvector offsets follow the input order)
  VBatchDesc* h_desc = reinterpret_cast<VBatchDesc*>(c->h_vb);
  std::vector<uint64_t> v_off(batch);
  size_t off = 0;
  for (uint32_t b = 0; b < batch; b++) {
    v_off[b] = off;
    off += dims[b];
  }
  for (uint32_t j = 0; j < batch; j++) {
    const uint32_t b = order[j];
    h_desc[j] = VBatchDesc{ (uint64_t) reinterpret_cast<uintptr_t>(mat_ptrs[b]),
                            v_off[b], dims[b], b };
  }
  ST_CHECK(hipMemcpyAsync(c->d_vb, c->h_vb, vb_bytes(batch),
                          hipMemcpyHostToDevice, s));
  const VBatchDesc* d_desc = reinterpret_cast<const VBatchDesc*>(c->d_vb);
  ST_CHECK(hipMemsetAsync(c->bstate.p, 0, sizeof(st_state) * (size_t)batch, s));
  uint32_t launches = 0;
  for (uint32_t k = kSolveShapeClasses; k-- > 0;) {
    const uint32_t count = class_first[k + 1] - class_first[k];
    if (!count)
      continue;
    if (launch_solve_vbatched<T>(d_desc, class_first[k], count, k, d_v,
                                 (T)o.eps, o.max_itr, o.semantics, c->d_bstate(),
                                 s))
      return -1;
    launches++;
  }
  return report_bstates<T>(c, batch, eigen_vals, iter_cnts, converged, v_host, d_v,
                           v_bytes, t0, launches, stats);
}

// host-pointer twin: [tightly packed mats | v] staged in the context's matrix
// buffer, matrix b at element offset sum_{j<b} dims[j]^2
template <typename T>
int64_t
solve_vbatched_host(Context* c, const T* mats, const uint32_t* dims,
                    uint32_t batch, T* eigen_vals, T* eigen_vecs,
                    uint32_t* iter_cnts, const st_options* opt, st_stats* stats)
{
  Resolved o;
  if (vbatched_args<T>(c, batch, opt, &o))
    return -1;
  if (batch == 0) // the no-op, with its stats
    return solve_vbatched<T>(c, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                             nullptr, nullptr, opt, stats);
  ST_REQUIRE(mats && dims && eigen_vals && eigen_vecs && iter_cnts,
             "null pointer");
  // the dims, before they size anything (the solve checks them again)
  {
    std::vector<uint32_t> order(batch);
    uint32_t class_first[kSolveShapeClasses + 1];
    if (vbatched_plan(solve_batched_max_n<T>(), dims, batch, order.data(),
                      class_first) < 0)
      return -1;
  }
  size_t m_elems = 0, v_elems = 0;
  for (uint32_t b = 0; b < batch; b++) {
    m_elems += (size_t)dims[b] * dims[b];
    v_elems += dims[b];
  }
  const size_t bytes = up256(sizeof(T) * m_elems); // v stays aligned
  if (ensure_device(c) || c->mat.ensure(c->stream, bytes + sizeof(T) * v_elems))
    return -1;
  T* d_mats = reinterpret_cast<T*>(c->mat.p);
  T* d_v = reinterpret_cast<T*>((char*)c->mat.p + bytes);
  std::vector<T*> ptrs(batch);
  size_t off = 0;
  for (uint32_t b = 0; b < batch; b++) {
    ptrs[b] = d_mats + off;
    off += (size_t)dims[b] * dims[b];
  }
  const auto t0 = std::chrono::steady_clock::now();
  ST_CHECK(hipMemcpyAsync(c->mat.p, mats, sizeof(T) * m_elems,
                          hipMemcpyHostToDevice, c->stream));
  ST_CHECK(hipStreamSynchronize(c->stream));
  const double h2d = ms_since(t0);
  st_stats local{};
  if (solve_vbatched<T>(c, ptrs.data(), dims, batch, d_v, eigen_vecs,
                        eigen_vals, iter_cnts, nullptr, opt, &local) < 0)
    return -1;
  return finish_twin(local, h2d, stats);
}

int
csr_create_on(Context* c, int dtype, uint32_t n, uint64_t nnz,
              const int64_t* d_row_ptr, const int32_t* d_col_idx,
              const void* d_vals, void** out, uint32_t flags = 0)
{
  ST_REQUIRE(out, "st_csr_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  CsrHandle* h = nullptr;
  if (csr_create(dtype, n, nnz, d_row_ptr, d_col_idx, d_vals, c->stream, &h, flags))
    return -1;
  *out = h;
  return 0;
}

int
csr_terms_create_on(Context* c, const CsrHandle* h, uint32_t K,
                    const void* const* d_u, const void* const* d_w, void** out)
{
  ST_REQUIRE(out, "st_csr_terms_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(c->device == h->device,
             "csr terms: the matrix lives on device %d, the queue on %d",
             h->device, c->device);
  CsrTermsHandle* t = nullptr;
  if (csr_terms_create(h, K, d_u, d_w, c->stream, &t))
    return -1;
  *out = t;
  return 0;
}

int
csr_multi_create_on(Context* c, const CsrHandle* h, uint32_t C, uint32_t K,
                    const void* const* d_u, const void* const* d_w, void** out)
{
  ST_REQUIRE(out, "st_csr_multi_create: null output pointer");
  *out = nullptr;
  {
    char msg[384];
    if (csr::check_multi_count(C, K, msg, sizeof(msg))) {
      set_error("%s", msg);
      return -1;
    }
  }
  ST_REQUIRE(d_u && d_w, "csr multi: null vector table");
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(c->device == h->device,
             "csr multi: the matrix lives on device %d, the queue on %d",
             h->device, c->device);
  CsrMultiHandle* t = nullptr;
  if (csr_multi_create(h, C, K, d_u, d_w, c->stream, &t))
    return -1;
  *out = t;
  return 0;
}

int
csr_transpose_on(Context* c, const CsrHandle* a, int64_t* d_t_row_ptr,
                 int32_t* d_t_col_idx, void* d_t_vals, void** out,
                 uint32_t flags = 0)
{
  ST_REQUIRE(out, "st_csr_transpose: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(c->device == a->device,
             "csr transpose: the matrix lives on device %d, the queue on %d",
             a->device, c->device);
  CsrHandle* h = nullptr;
  if (csr_transpose(a, d_t_row_ptr, d_t_col_idx, d_t_vals, c->stream, &h, flags))
    return -1;
  *out = h;
  return 0;
}

int
csr_pattern_create_on(Context* c, int dtype, uint32_t n, uint64_t nnz,
                      const int64_t* d_row_ptr, const int32_t* d_col_idx,
                      const void* d_row_scale, const void* d_col_scale, void** out,
                      uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_pattern_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  CsrPatternHandle* h = nullptr;
  if (csr_pattern_create(dtype, n, nnz, d_row_ptr, d_col_idx, d_row_scale, d_col_scale,
                         c->stream, &h, flags))
    return -1;
  *out = h;
  return 0;
}

int
csr_pattern_transpose_on(Context* c, const CsrPatternHandle* p, int64_t* d_t_row_ptr,
                         int32_t* d_t_col_idx, void** out, uint32_t flags)
{
  ST_REQUIRE(out, "st_csr_pattern_transpose: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(c->device == p->device,
             "csr transpose: the matrix lives on device %d, the queue on %d",
             p->device, c->device);
  CsrPatternHandle* h = nullptr;
  if (csr_pattern_transpose(p, d_t_row_ptr, d_t_col_idx, c->stream, &h, flags))
    return -1;
  *out = h;
  return 0;
}

int
csr_pattern_terms_create_on(Context* c, const CsrPatternHandle* h, uint32_t K,
                            const void* const* d_u, const void* const* d_w, void** out)
{
  ST_REQUIRE(out, "st_csr_pattern_terms_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  ST_REQUIRE(c->device == h->device,
             "csr terms: the matrix lives on device %d, the queue on %d",
             h->device, c->device);
  CsrTermsHandle* t = nullptr;
  if (csr_pattern_terms_create(h, K, d_u, d_w, c->stream, &t))
    return -1;
  *out = t;
  return 0;
}

int
csr_batch_create_on(Context* c, int dtype, uint32_t batch,
                    const uint32_t* mat_first, uint64_t nnz,
                    const int64_t* d_row_ptr, const int32_t* d_col_idx,
                    const void* d_vals, void** out)
{
  ST_REQUIRE(out, "st_csr_batch_create: null output pointer");
  *out = nullptr;
  ST_REQUIRE(c, "null queue");
  if (ensure_device(c))
    return -1;
  CsrBatchHandle* h = nullptr;
  if (csr_batch_create(dtype, batch, mat_first, nnz, d_row_ptr, d_col_idx, d_vals,
                       c->stream, &h))
    return -1;
  *out = h;
  return 0;
}

Context*
as_ctx(void* wq)
{
  return reinterpret_cast<Context*>(wq);
}

} // namespace
} // namespace st

using st::Context;

extern "C" {

const char*
eigen_last_error(void)
{
  return st::g_err;
}

const char*
st_version(void)
{
  // the A/B probe switches the kernels were built with (st_kernels.hip):
  // "defaults" in every library build, the values in a probe build
  static const std::string v =
    std::string("eigen_value_amd 0.6.0 (gfx950; probe switches: ") +
    st_probe_switches() + "; " + st::rccl_desc() + ")";
  return v.c_str();
}

int
st_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

void
make_queue(void** wq)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (!wq)
    return;
  *wq = nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    st::set_error("make_queue: no HIP device");
    return;
  }
  if (const char* e = std::getenv("EIGEN_VALUE_DEVICE"))
    dev = std::atoi(e);
  Context* c = new (std::nothrow) Context();
  if (!c) {
    st::set_error("make_queue: out of host memory");
    return;
  }
  c->device = dev;
  bool ok = hipSetDevice(dev) == hipSuccess &&
            hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) ==
              hipSuccess &&
            hipMalloc(&c->d_state, sizeof(st_state)) == hipSuccess &&
            hipHostMalloc(&c->h_state, 2 * sizeof(st_state),
                          hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_flag[0], hipEventDisableTiming) ==
              hipSuccess &&
            hipEventCreateWithFlags(&c->ev_flag[1], hipEventDisableTiming) ==
              hipSuccess;
  if (!ok) {
    st::set_error("make_queue: HIP initialisation failed: %s",
                  hipGetErrorString(hipGetLastError()));
    destroy_queue(c);
    return;
  }
  c->stream = c->own_stream;
  *wq = c;
}

void
destroy_queue(void* wq)
{
  st::DeviceGuard guard;
  Context* c = st::as_ctx(wq);
  if (!c)
    return;
  (void)hipSetDevice(c->device);
  if (c->stream)
    (void)hipStreamSynchronize(c->stream);
  for (st::DeviceBuf* b : { &c->mat, &c->vec, &c->part, &c->trace, &c->bstate, &c->bsum })
    b->release();
  for (void* p : { (void*)c->d_state, (void*)c->d_bcount, c->d_vb })
    if (p)
      (void)hipFree(p);
  for (void* p : { (void*)c->h_state, (void*)c->h_bcount, c->h_vb })
    if (p)
      (void)hipHostFree(p);
  for (hipEvent_t e : c->ev_flag)
    if (e)
      (void)hipEventDestroy(e);
  if (c->own_stream)
    (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int
st_last_round_times(void* wq, float* ms, unsigned int cap)
{
  st::clear_error();
  Context* c = st::as_ctx(wq);
  ST_REQUIRE(c, "st_last_round_times: null queue");
  ST_REQUIRE(ms || cap == 0, "st_last_round_times: null buffer");
  const size_t n = c->round_ms.size();
  for (size_t i = 0; i < n && i < cap; i++)
    ms[i] = c->round_ms[i];
  return (int)n;
}

int
st_last_round_sums(void* wq, void* sums, unsigned int cap_rounds)
{
  st::clear_error();
  Context* c = st::as_ctx(wq);
  ST_REQUIRE(c, "st_last_round_sums: null queue");
  ST_REQUIRE(sums || cap_rounds == 0, "st_last_round_sums: null buffer");
  const uint32_t r = c->trace_rounds;
  if (r && cap_rounds) {
    const size_t row = c->trace_sums.size() / r;
    std::memcpy(sums, c->trace_sums.data(), row * (cap_rounds < r ? cap_rounds : r));
  }
  return (int)r;
}

int
st_set_stream(void* wq, void* stream)
{
  st::clear_error();
  Context* c = st::as_ctx(wq);
  ST_REQUIRE(c, "st_set_stream: null queue");
  // NULL is HIP's null stream (torch's default stream handle is 0), not
  // "no stream": the context must order itself after the caller's work
  c->stream = reinterpret_cast<hipStream_t>(stream);
  return 0;
}

int
st_use_own_stream(void* wq)
{
  st::clear_error();
  Context* c = st::as_ctx(wq);
  ST_REQUIRE(c, "st_use_own_stream: null queue");
  c->stream = c->own_stream;
  return 0;
}

int64_t
max_eigen_value(void* wq, float* mat, float* eigen_val, float* eigen_vec,
                unsigned int dim, unsigned int* iter_cnt)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host<float>(st::as_ctx(wq), mat, dim, eigen_val, eigen_vec,
                               iter_cnt, nullptr, nullptr);
}

int64_t
max_eigen_value_f64(void* wq, double* mat, double* eigen_val,
                    double* eigen_vec, unsigned int dim,
                    unsigned int* iter_cnt)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host<double>(st::as_ctx(wq), mat, dim, eigen_val,
                                eigen_vec, iter_cnt, nullptr, nullptr);
}

int64_t
max_eigen_value_ex(void* wq, int dtype, const void* mat, void* eigen_val,
                   void* eigen_vec, unsigned int dim, unsigned int* iter_cnt,
                   const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (dtype == 0)
    return st::solve_host<float>(st::as_ctx(wq), (const float*)mat, dim,
                                 (float*)eigen_val, (float*)eigen_vec,
                                 iter_cnt, opt, stats);
  if (dtype == 1)
    return st::solve_host<double>(st::as_ctx(wq), (const double*)mat, dim,
                                  (double*)eigen_val, (double*)eigen_vec,
                                  iter_cnt, opt, stats);
  st::set_error("max_eigen_value_ex: dtype must be 0 (f32) or 1 (f64)");
  return -1;
}

int64_t
st_solve_device_f32(void* wq, float* d_mat, unsigned int dim,
                    float* d_eigen_vec, float* eigen_vec_host,
                    float* eigen_val, unsigned int* iter_cnt,
                    const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_device<float>(st::as_ctx(wq), st::Operator::dense(d_mat, dim),
                                 d_eigen_vec, eigen_vec_host, eigen_val, iter_cnt,
                                 opt, stats);
}

int64_t
st_solve_device_left_f32(void* wq, const float* d_mat, unsigned int dim,
                         float* d_eigen_vec, float* eigen_vec_host, float* eigen_val,
                         unsigned int* iter_cnt, const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_device_left<float>(st::as_ctx(wq), d_mat, dim, d_eigen_vec,
                                      eigen_vec_host, eigen_val, iter_cnt, opt, stats);
}

int64_t
st_solve_device_left_f64(void* wq, const double* d_mat, unsigned int dim,
                         double* d_eigen_vec, double* eigen_vec_host, double* eigen_val,
                         unsigned int* iter_cnt, const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_device_left<double>(st::as_ctx(wq), d_mat, dim, d_eigen_vec,
                                       eigen_vec_host, eigen_val, iter_cnt, opt, stats);
}

int64_t
max_eigen_value_left_ex(void* wq, int dtype, const void* mat, void* eigen_val,
                        void* eigen_vec, unsigned int dim, unsigned int* iter_cnt,
                        const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (dtype == 0)
    return st::solve_host_left<float>(st::as_ctx(wq), (const float*)mat, dim,
                                      (float*)eigen_val, (float*)eigen_vec, iter_cnt,
                                      opt, stats);
  if (dtype == 1)
    return st::solve_host_left<double>(st::as_ctx(wq), (const double*)mat, dim,
                                       (double*)eigen_val, (double*)eigen_vec, iter_cnt,
                                       opt, stats);
  st::set_error("max_eigen_value_left_ex: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  return -1;
}

#define ST_PAIR_SOLVE(T, SFX)                                                           \
  int64_t st_solve_device_pair_##SFX(void* wq, const T* d_mat, unsigned int dim,        \
                                     T* d_eigen_vecs, T* eigen_vecs_host, T* eigen_vals, \
                                     unsigned int* iter_cnts, unsigned int* converged,   \
                                     const st_options* opt, st_stats* stats)             \
  {                                                                                     \
    st::clear_error();                                                                  \
    st::DeviceGuard guard;                                                              \
    return st::solve_device_pair<T>(st::as_ctx(wq), d_mat, dim, d_eigen_vecs,           \
                                    eigen_vecs_host, eigen_vals, iter_cnts, converged,  \
                                    opt, stats);                                        \
  }
ST_PAIR_SOLVE(float, f32)
ST_PAIR_SOLVE(double, f64)
#undef ST_PAIR_SOLVE

int64_t
max_eigen_value_pair_ex(void* wq, int dtype, const void* mat, void* eigen_vals,
                        void* eigen_vecs, unsigned int dim, unsigned int* iter_cnts,
                        unsigned int* converged, const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (dtype == 0)
    return st::solve_host_pair<float>(st::as_ctx(wq), (const float*)mat, dim,
                                      (float*)eigen_vals, (float*)eigen_vecs, iter_cnts,
                                      converged, opt, stats);
  if (dtype == 1)
    return st::solve_host_pair<double>(st::as_ctx(wq), (const double*)mat, dim,
                                       (double*)eigen_vals, (double*)eigen_vecs, iter_cnts,
                                       converged, opt, stats);
  st::set_error("max_eigen_value_pair_ex: dtype must be 0 (f32) or 1 (f64), got %d", dtype);
  return -1;
}

int64_t
st_solve_device_half(void* wq, int storage, const void* d_mat, unsigned int dim,
                     float* d_eigen_vec, float* eigen_vec_host,
                     float* eigen_val, unsigned int* iter_cnt,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_device_half(st::as_ctx(wq), storage, d_mat, dim, d_eigen_vec,
                               eigen_vec_host, eigen_val, iter_cnt, opt, stats);
}

int64_t
max_eigen_value_half_ex(void* wq, int storage, const void* mat,
                        float* eigen_val, float* eigen_vec, unsigned int dim,
                        unsigned int* iter_cnt, const st_options* opt,
                        st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_half(st::as_ctx(wq), storage, mat, dim, eigen_val,
                             eigen_vec, iter_cnt, opt, stats);
}

int
st_csr_create(void* wq, int dtype, uint32_t n, uint64_t nnz,
              const int64_t* d_row_ptr, const int32_t* d_col_idx,
              const void* d_vals, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::csr_create_on(st::as_ctx(wq), dtype, n, nnz, d_row_ptr, d_col_idx,
                           d_vals, out);
}

int
st_csr_create_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                 const int64_t* d_row_ptr, const int32_t* d_col_idx,
                 const void* d_vals, unsigned int flags, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::csr_create_on(st::as_ctx(wq), dtype, n, nnz, d_row_ptr, d_col_idx,
                           d_vals, out, flags);
}

int
st_csr_empty_rows(void* csr, uint32_t* count, uint32_t* lowest)
{
  st::clear_error();
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_empty_rows");
  if (!h)
    return -1;
  if (count)
    *count = h->empty_rows;
  if (lowest)
    *lowest = h->first_empty;
  return 0;
}

int
st_csr_terms_create(void* wq, void* csr, uint32_t K, const void* const* d_u,
                    const void* const* d_w, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_terms_create");
  if (!h)
    return -1;
  return st::csr_terms_create_on(st::as_ctx(wq), h, K, d_u, d_w, out);
}

int64_t
st_solve_csr_terms(void* wq, void* csr, void* terms, void* d_eigen_vec,
                   void* eigen_vec_host, void* eigen_val, unsigned int* iter_cnt,
                   const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrHandle* h = st::as_csr(csr, "st_solve_csr_terms");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = st::as_csr_terms(terms, h, "st_solve_csr_terms");
  if (!t)
    return -1;
  return st::solve_csr(st::as_ctx(wq), h, d_eigen_vec, eigen_vec_host, eigen_val,
                       iter_cnt, opt, stats, t);
}

int64_t
max_eigen_value_csr_terms_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                             const int64_t* row_ptr, const int32_t* col_idx,
                             const void* vals, uint32_t K, const void* const* u,
                             const void* const* w, unsigned int flags,
                             void* eigen_val, void* eigen_vec,
                             unsigned int* iter_cnt, const st_options* opt,
                             st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_terms(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx,
                                  vals, K, u, w, flags, eigen_val, eigen_vec,
                                  iter_cnt, opt, stats);
}

int
st_csr_multi_create(void* wq, void* csr, uint32_t C, uint32_t K,
                    const void* const* d_u, const void* const* d_w, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrHandle* h = st::as_csr(csr, "st_csr_multi_create");
  if (!h)
    return -1;
  return st::csr_multi_create_on(st::as_ctx(wq), h, C, K, d_u, d_w, out);
}

int64_t
st_solve_csr_multi(void* wq, void* csr, void* multi, void* d_eigen_vecs,
                   void* eigen_vecs_host, void* eigen_vals, unsigned int* iter_cnts,
                   unsigned int* converged, const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrHandle* h = st::as_csr(csr, "st_solve_csr_multi");
  if (!h)
    return -1;
  const st::CsrMultiHandle* t = st::as_csr_multi(multi, h, "st_solve_csr_multi");
  if (!t)
    return -1;
  return st::solve_csr_multi(st::as_ctx(wq), h, t, d_eigen_vecs, eigen_vecs_host,
                             eigen_vals, iter_cnts, converged, opt, stats);
}

int64_t
max_eigen_value_csr_multi_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                             const int64_t* row_ptr, const int32_t* col_idx,
                             const void* vals, uint32_t C, uint32_t K,
                             const void* const* u, const void* const* w,
                             unsigned int flags, void* eigen_vals, void* eigen_vecs,
                             unsigned int* iter_cnts, unsigned int* converged,
                             const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_multi(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx,
                                  vals, C, K, u, w, flags, eigen_vals, eigen_vecs,
                                  iter_cnts, converged, opt, stats);
}

int
st_csr_transpose_ex(void* wq, void* csr, int64_t* d_t_row_ptr,
                    int32_t* d_t_col_idx, void* d_t_vals, unsigned int flags,
                    void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrHandle* a = st::as_csr(csr, "st_csr_transpose_ex");
  if (!a)
    return -1;
  return st::csr_transpose_on(st::as_ctx(wq), a, d_t_row_ptr, d_t_col_idx,
                              d_t_vals, out, flags);
}

int64_t
st_solve_csr(void* wq, void* csr, void* d_eigen_vec, void* eigen_vec_host,
             void* eigen_val, unsigned int* iter_cnt, const st_options* opt,
             st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrHandle* h = st::as_csr(csr, "st_solve_csr");
  if (!h)
    return -1;
  return st::solve_csr(st::as_ctx(wq), h, d_eigen_vec, eigen_vec_host,
                       eigen_val, iter_cnt, opt, stats);
}

int64_t
max_eigen_value_csr_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                       const int64_t* row_ptr, const int32_t* col_idx,
                       const void* vals, void* eigen_val, void* eigen_vec,
                       unsigned int* iter_cnt, const st_options* opt,
                       st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx,
                            vals, eigen_val, eigen_vec, iter_cnt, opt, stats);
}

int
st_csr_transpose(void* wq, void* csr, int64_t* d_t_row_ptr, int32_t* d_t_col_idx,
                 void* d_t_vals, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrHandle* a = st::as_csr(csr, "st_csr_transpose");
  if (!a)
    return -1;
  return st::csr_transpose_on(st::as_ctx(wq), a, d_t_row_ptr, d_t_col_idx,
                              d_t_vals, out);
}

int64_t
max_eigen_value_csr_left_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                            const int64_t* row_ptr, const int32_t* col_idx,
                            const void* vals, void* eigen_val, void* eigen_vec,
                            unsigned int* iter_cnt, const st_options* opt,
                            st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_left(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx,
                                 vals, eigen_val, eigen_vec, iter_cnt, opt, stats);
}

int
st_csr_pattern_create(void* wq, int dtype, uint32_t n, uint64_t nnz,
                      const int64_t* d_row_ptr, const int32_t* d_col_idx,
                      const void* d_row_scale, const void* d_col_scale,
                      unsigned int flags, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::csr_pattern_create_on(st::as_ctx(wq), dtype, n, nnz, d_row_ptr, d_col_idx,
                                   d_row_scale, d_col_scale, out, flags);
}

int
st_csr_pattern_transpose(void* wq, void* pat, int64_t* d_t_row_ptr,
                         int32_t* d_t_col_idx, unsigned int flags, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrPatternHandle* p = st::as_csr_pattern(pat, "st_csr_pattern_transpose");
  if (!p)
    return -1;
  return st::csr_pattern_transpose_on(st::as_ctx(wq), p, d_t_row_ptr, d_t_col_idx, out,
                                      flags);
}

int
st_csr_pattern_terms_create(void* wq, void* pat, uint32_t K, const void* const* d_u,
                            const void* const* d_w, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (out)
    *out = nullptr;
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_csr_pattern_terms_create");
  if (!h)
    return -1;
  return st::csr_pattern_terms_create_on(st::as_ctx(wq), h, K, d_u, d_w, out);
}

int64_t
st_solve_csr_pattern(void* wq, void* pat, void* terms, void* d_eigen_vec,
                     void* eigen_vec_host, void* eigen_val, unsigned int* iter_cnt,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrPatternHandle* h = st::as_csr_pattern(pat, "st_solve_csr_pattern");
  if (!h)
    return -1;
  const st::CsrTermsHandle* t = nullptr;
  if (terms && !(t = st::as_csr_pattern_terms(terms, h, "st_solve_csr_pattern")))
    return -1;
  return st::solve_csr_pattern(st::as_ctx(wq), h, d_eigen_vec, eigen_vec_host, eigen_val,
                               iter_cnt, opt, stats, t);
}

int64_t
max_eigen_value_csr_pattern_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                               const int64_t* row_ptr, const int32_t* col_idx,
                               const void* row_scale, const void* col_scale, uint32_t K,
                               const void* const* u, const void* const* w,
                               unsigned int flags, void* eigen_val, void* eigen_vec,
                               unsigned int* iter_cnt, const st_options* opt,
                               st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_pattern(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx,
                                    row_scale, col_scale, K, u, w, flags, eigen_val,
                                    eigen_vec, iter_cnt, opt, stats);
}

int64_t
st_solve_csr_product(void* wq, void* csr_b, void* csr_a, void* d_eigen_vec,
                     void* eigen_vec_host, void* eigen_val, unsigned int* iter_cnt,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrHandle* b = st::as_csr(csr_b, "st_solve_csr_product (B)");
  if (!b)
    return -1;
  const st::CsrHandle* a = st::as_csr(csr_a, "st_solve_csr_product (A)");
  if (!a)
    return -1;
  return st::solve_csr_product(st::as_ctx(wq), b, a, d_eigen_vec, eigen_vec_host,
                               eigen_val, iter_cnt, opt, stats);
}

int64_t
max_eigen_value_csr_product_ex(void* wq, int dtype, uint32_t n, uint64_t b_nnz,
                               const int64_t* b_row_ptr, const int32_t* b_col_idx,
                               const void* b_vals, uint64_t a_nnz,
                               const int64_t* a_row_ptr, const int32_t* a_col_idx,
                               const void* a_vals, unsigned int flags, void* eigen_val,
                               void* eigen_vec, unsigned int* iter_cnt,
                               const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_product(st::as_ctx(wq), dtype, n, b_nnz, b_row_ptr,
                                    b_col_idx, b_vals, a_nnz, a_row_ptr, a_col_idx,
                                    a_vals, flags, eigen_val, eigen_vec, iter_cnt, opt,
                                    stats);
}

int64_t
max_eigen_value_csr_gram_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                            const int64_t* row_ptr, const int32_t* col_idx,
                            const void* vals, int side, unsigned int flags,
                            void* eigen_val, void* eigen_vec, unsigned int* iter_cnt,
                            const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_gram(st::as_ctx(wq), dtype, n, nnz, row_ptr, col_idx, vals,
                                 side, flags, eigen_val, eigen_vec, iter_cnt, opt,
                                 stats);
}

int
st_csr_batch_create(void* wq, int dtype, uint32_t batch,
                    const uint32_t* mat_first, uint64_t nnz,
                    const int64_t* d_row_ptr, const int32_t* d_col_idx,
                    const void* d_vals, void** out)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::csr_batch_create_on(st::as_ctx(wq), dtype, batch, mat_first, nnz,
                                 d_row_ptr, d_col_idx, d_vals, out);
}

int64_t
st_solve_csr_batched(void* wq, void* hp, void* d_eigen_vecs,
                     void* eigen_vecs_host, void* eigen_vals,
                     unsigned int* iter_cnts, unsigned int* converged,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  const st::CsrBatchHandle* h = st::as_csr_batch(hp, "st_solve_csr_batched");
  if (!h)
    return -1;
  return st::solve_csr_batched(st::as_ctx(wq), h, d_eigen_vecs, eigen_vecs_host,
                               eigen_vals, iter_cnts, converged, opt, stats);
}

int64_t
max_eigen_value_csr_batched_ex(void* wq, int dtype, uint32_t batch,
                               const uint32_t* mat_first, uint64_t nnz,
                               const int64_t* row_ptr, const int32_t* col_idx,
                               const void* vals, void* eigen_vals,
                               void* eigen_vecs, unsigned int* iter_cnts,
                               unsigned int* converged, const st_options* opt,
                               st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_host_csr_batched(st::as_ctx(wq), dtype, batch, mat_first, nnz,
                                    row_ptr, col_idx, vals, eigen_vals,
                                    eigen_vecs, iter_cnts, converged, opt, stats);
}

int64_t
st_solve_device_f64(void* wq, double* d_mat, unsigned int dim,
                    double* d_eigen_vec, double* eigen_vec_host,
                    double* eigen_val, unsigned int* iter_cnt,
                    const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_device<double>(st::as_ctx(wq), st::Operator::dense(d_mat, dim),
                                  d_eigen_vec, eigen_vec_host, eigen_val, iter_cnt,
                                  opt, stats);
}

int64_t
st_solve_batched_f32(void* wq, float* d_mats, unsigned int batch,
                     unsigned int dim, float* d_eigen_vecs,
                     float* eigen_vecs_host, float* eigen_vals,
                     unsigned int* iter_cnts, unsigned int* converged,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_batched<float>(st::as_ctx(wq), d_mats, batch, dim,
                                  d_eigen_vecs, eigen_vecs_host, eigen_vals,
                                  iter_cnts, converged, opt, stats);
}

int64_t
st_solve_batched_f64(void* wq, double* d_mats, unsigned int batch,
                     unsigned int dim, double* d_eigen_vecs,
                     double* eigen_vecs_host, double* eigen_vals,
                     unsigned int* iter_cnts, unsigned int* converged,
                     const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_batched<double>(st::as_ctx(wq), d_mats, batch, dim,
                                   d_eigen_vecs, eigen_vecs_host, eigen_vals,
                                   iter_cnts, converged, opt, stats);
}

int64_t
max_eigen_value_batched_ex(void* wq, int dtype, const void* mats,
                           void* eigen_vals, void* eigen_vecs,
                           unsigned int batch, unsigned int dim,
                           unsigned int* iter_cnts, const st_options* opt,
                           st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (dtype == 0)
    return st::solve_batched_host<float>(
      st::as_ctx(wq), (const float*)mats, batch, dim, (float*)eigen_vals,
      (float*)eigen_vecs, iter_cnts, opt, stats);
  if (dtype == 1)
    return st::solve_batched_host<double>(
      st::as_ctx(wq), (const double*)mats, batch, dim, (double*)eigen_vals,
      (double*)eigen_vecs, iter_cnts, opt, stats);
  st::set_error("max_eigen_value_batched_ex: dtype must be 0 (f32) or 1 (f64)");
  return -1;
}

int64_t
st_solve_vbatched_f32(void* wq, float* const* d_mat_ptrs, const uint32_t* dims,
                      unsigned int batch, float* d_eigen_vecs,
                      float* eigen_vecs_host, float* eigen_vals,
                      unsigned int* iter_cnts, unsigned int* converged,
                      const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_vbatched<float>(st::as_ctx(wq), d_mat_ptrs, dims, batch,
                                   d_eigen_vecs, eigen_vecs_host, eigen_vals,
                                   iter_cnts, converged, opt, stats);
}

int64_t
st_solve_vbatched_f64(void* wq, double* const* d_mat_ptrs, const uint32_t* dims,
                      unsigned int batch, double* d_eigen_vecs,
                      double* eigen_vecs_host, double* eigen_vals,
                      unsigned int* iter_cnts, unsigned int* converged,
                      const st_options* opt, st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  return st::solve_vbatched<double>(st::as_ctx(wq), d_mat_ptrs, dims, batch,
                                    d_eigen_vecs, eigen_vecs_host, eigen_vals,
                                    iter_cnts, converged, opt, stats);
}

int64_t
max_eigen_value_vbatched_ex(void* wq, int dtype, const void* mats,
                            const uint32_t* dims, unsigned int batch,
                            void* eigen_vals, void* eigen_vecs,
                            unsigned int* iter_cnts, const st_options* opt,
                            st_stats* stats)
{
  st::clear_error();
  st::DeviceGuard guard;
  if (dtype == 0)
    return st::solve_vbatched_host<float>(
      st::as_ctx(wq), (const float*)mats, dims, batch, (float*)eigen_vals,
      (float*)eigen_vecs, iter_cnts, opt, stats);
  if (dtype == 1)
    return st::solve_vbatched_host<double>(
      st::as_ctx(wq), (const double*)mats, dims, batch, (double*)eigen_vals,
      (double*)eigen_vecs, iter_cnts, opt, stats);
  st::set_error("max_eigen_value_vbatched_ex: dtype must be 0 (f32) or 1 (f64)");
  return -1;
}

int
st_vbatched_plan(int dtype, const uint32_t* dims, unsigned int batch,
                 uint32_t* order_out, uint32_t* class_first)
{
  st::clear_error();
  ST_REQUIRE(dtype == 0 || dtype == 1,
             "st_vbatched_plan: dtype must be 0 (f32) or 1 (f64)");
  ST_REQUIRE(class_first && ((dims && order_out) || batch == 0),
             "st_vbatched_plan: null pointer");
  return st::vbatched_plan(st_solve_batched_max_dim(dtype), dims, batch,
                           order_out, class_first);
}

unsigned int
st_solve_batched_max_dim(int dtype)
{
  return dtype == 0   ? st::solve_batched_max_n<float>()
         : dtype == 1 ? st::solve_batched_max_n<double>()
                      : 0u;
}

unsigned int
st_solve_batched_rounds_max_dim(int dtype)
{
  return dtype == 0   ? st::batched_rounds_max_n(sizeof(float))
         : dtype == 1 ? st::batched_rounds_max_n(sizeof(double))
                      : 0u;
}

} // extern "C"
