/*
 * similarity_transform.h — C-ABI of libsimilarity_transform.so, the
 * MI355X (gfx950) implementation of the similarity-transform maximum
 * eigenvalue iteration.
 *
 * Plain C: pointers, sizes, no torch or HIP types in any signature
 * (streams are passed as `void*` = hipStream_t).  Citations refer to the
 * reference tree (itzmeanjan/eigen_value), path:line.
 *
 * Layers
 *   1. Drop-in exports: exactly the two symbols the reference's Python
 *      wrapper binds (wrapper/python/similarity_transform.py:33-37,63-69).
 *   2. Additions at the same level (fp64 twin, queue teardown, last error,
 *      an extended call with options and statistics).
 *   3. Device-resident solve (input already in HBM; bench and torch users);
 *      3a-3j: batched (3a), multi-GPU (3b), sparse CSR (3c-3h), dense
 *      left-vector (3i) and dense pair (3j: both Perron vectors from one
 *      pass over the matrix per round) solves.
 *   4. Step-level kernels on a caller stream: what the row-block sharded
 *      driver (eigen_value_amd/sharded.py) and the kernel unit tests call.
 *
 * Errors: nothing throws across this ABI.  Functions returning int64_t /
 * int return a negative value on error and record a message readable with
 * eigen_last_error() (thread-local).  make_queue writes NULL on failure.
 *
 * Threading: a queue (context) is used by one host thread at a time.
 */
#ifndef EIGEN_VALUE_AMD_SIMILARITY_TRANSFORM_H
#define EIGEN_VALUE_AMD_SIMILARITY_TRANSFORM_H

#include <stdint.h>

/* the library is built with -fvisibility=hidden: what this header declares
 * is its whole dynamic ABI */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* include/similarity_transform.hpp:4-5 */
#define ST_EPS_F32 1e-3f
#define ST_EPS_F64 1e-3
#define ST_MAX_ITR 1000u

/* semantics of the round loop */
#define ST_SEM_SYCL 0u   /* similarity_transform.cpp: cyclic stop (413-417),   */
                         /* A *= (1/s_r)*s_c (324-325), count = break idx (54) */
#define ST_SEM_MAINPY 1u /* main.py: non-cyclic stop (25-27),                 */
                         /* ((1/s_r)*A)*s_c (13-16), count = itr + 1 (47)     */

/* ---------------------------------------------------------------------- */
/* 1. drop-in exports                                                      */
/* ---------------------------------------------------------------------- */

/* replaces wrapper/similarity_transform.cpp:3-12 (sycl::default_selector
 * queue).  Creates a context on the current HIP device (env
 * EIGEN_VALUE_DEVICE overrides) with its own non-blocking stream.
 * *wq = NULL on failure. */
void make_queue(void** wq);

/* replaces wrapper/similarity_transform.cpp:14-37 and, behind it,
 * similarity_transform.cpp:5-75.  fp32, reference semantics (ST_SEM_SYCL,
 * EPS = 1e-3f, MAX_ITR = 1000).  `mat` (dim x dim, row-major) is read only.
 * Writes eigen_val[0], eigen_vec[0..dim), *iter_cnt.  Returns elapsed ms
 * (steady clock, host->device copy of `mat` included, as the reference's
 * lazily-copied buffer is) or a negative value on error.  Any dim >= 1 is
 * accepted (the reference required dim % work-group-size == 0). */
int64_t max_eigen_value(void* wq, float* mat, float* eigen_val,
                        float* eigen_vec, unsigned int dim,
                        unsigned int* iter_cnt);

/* ---------------------------------------------------------------------- */
/* 2. additions                                                            */
/* ---------------------------------------------------------------------- */

/* fp64 twin of max_eigen_value (EPS = 1e-3). */
int64_t max_eigen_value_f64(void* wq, double* mat, double* eigen_val,
                            double* eigen_vec, unsigned int dim,
                            unsigned int* iter_cnt);

/* Frees a context from make_queue (the reference leaks its queue). */
void destroy_queue(void* wq);

/* Message of the last error on this thread ("" if none). */
const char* eigen_last_error(void);

typedef struct st_options
{
  double eps;         /* stop tolerance; < 0 selects the dtype default     */
  uint32_t max_itr;   /* 0 selects ST_MAX_ITR                               */
  uint32_t semantics; /* ST_SEM_SYCL or ST_SEM_MAINPY                       */
  uint32_t batch;     /* rounds enqueued per host flag check; 0 = default   */
  uint32_t flags;     /* ST_FLAG_* below                                    */
} st_options;

#define ST_FLAG_TIME_KERNELS 1u /* hipEvents around every fused launch     */
#define ST_FLAG_MATRIX_FREE 2u  /* st_mfree_round_* instead of the in-place */
                                /* transform (input never written)         */
#define ST_FLAG_WRITE_EVERY_ROUND 8u /* store the matrix every round; by    */
                                /* default the flat round (>= 144 MiB)      */
                                /* stores it every 6th round (st_defer_     */
                                /* rounds) and re-applies                   */
                                /* the pending scalings in registers:       */
                                /* identical results, fewer bytes           */
#define ST_FLAG_ROUND_LOOP 4u   /* one launch per round even where the whole */
                                /* solve fits one workgroup (n <= 128 fp64, */
                                /* 256 fp32): results are identical        */
#define ST_FLAG_TRACE_SUMS 16u  /* record every evaluated round's row sums  */
                                /* s_k (st_last_round_sums; max_itr * dim   */
                                /* elements <= 1 GiB): identical results    */
#define ST_FLAG_BATCH_ROUNDS 32u /* batched entry points only: one launch   */
                                /* per round for the whole batch            */
                                /* (k_round_batched), dim up to             */
                                /* st_solve_batched_rounds_max_dim          */

typedef struct st_stats
{
  double h2d_ms;          /* host->device copy of the input               */
  double loop_ms;         /* first kernel .. convergence observed on host */
  double d2h_ms;          /* eigenvector / eigenvalue copy back           */
  double fused_ms_total;  /* sum of fused scale+rowsum kernel times       */
  double rowsum_ms;       /* the initial row-sum pass                     */
  uint32_t fused_launches;/* fused launches timed                         */
  uint32_t rounds;        /* row-sum evaluations performed                */
  uint32_t converged;     /* 1 if the stop test passed before max_itr     */
  uint32_t transpose_us;  /* max_eigen_value_csr_left_ex: the device        */
                          /* transposition, microseconds; 0 elsewhere      */
} st_stats;

/* Extended host-pointer solve.  dtype: 0 = float32, 1 = float64.
 * opt / stats may be NULL. */
int64_t max_eigen_value_ex(void* wq, int dtype, const void* mat,
                           void* eigen_val, void* eigen_vec,
                           unsigned int dim, unsigned int* iter_cnt,
                           const st_options* opt, st_stats* stats);

/* Per-round kernel times (ms) of the last solve on this queue that ran
 * with ST_FLAG_TIME_KERNELS: copies min(cap, n) values into ms and returns
 * n, the number of rounds that did work (0 if the last solve was not
 * timed), or a negative value on error. */
int st_last_round_times(void* wq, float* ms, unsigned int cap);

/* Row sums of the last solve on this queue that ran with ST_FLAG_TRACE_SUMS:
 * s_k for the evaluated rounds k = 0 .. n-1 (the vectors the stop test of
 * similarity_transform.cpp:413-421 compared), copied as min(cap_rounds, n)
 * rows of dim elements of the solve's dtype into `sums`.  Returns n (0 if the
 * last solve was not traced) or a negative value on error. */
int st_last_round_sums(void* wq, void* sums, unsigned int cap_rounds);

/* Make the context launch on a caller stream (a hipStream_t; NULL is the
 * HIP null stream, which is torch's default stream).  Returns 0 or
 * negative.  st_use_own_stream restores the context's own non-blocking
 * stream (the make_queue default). */
int st_set_stream(void* wq, void* stream);
int st_use_own_stream(void* wq);

/* ---------------------------------------------------------------------- */
/* 3. device-resident solve                                                */
/* ---------------------------------------------------------------------- */

/* d_mat: device pointer, dim x dim row-major; TRANSFORMED IN PLACE (it is
 * the private working copy the reference makes at
 * similarity_transform.cpp:14,19).  On return d_mat holds A_end, where end =
 * st_stats.rounds = the rounds evaluated: the launch that evaluates the
 * stopping round still applies its transform, so a converged solve leaves
 * one transform more than the reference's working copy, whose loop breaks
 * before compute_next_matrix (similarity_transform.cpp:45-52); an
 * exhausted solve (MAX_ITR rounds) leaves A_MAX_ITR like the reference.
 * lambda, the eigenvector and iter_cnt do not depend on it.  d_eigen_vec:
 * device pointer [dim] or
 * NULL (then eigen_vec_host must be non-NULL and receives it).
 * eigen_val / iter_cnt: host pointers.  Returns loop ms or negative. */
int64_t st_solve_device_f32(void* wq, float* d_mat, unsigned int dim,
                            float* d_eigen_vec, float* eigen_vec_host,
                            float* eigen_val, unsigned int* iter_cnt,
                            const st_options* opt, st_stats* stats);
int64_t st_solve_device_f64(void* wq, double* d_mat, unsigned int dim,
                            double* d_eigen_vec, double* eigen_vec_host,
                            double* eigen_val, unsigned int* iter_cnt,
                            const st_options* opt, st_stats* stats);

/* Half-precision STORAGE: the matrix-free solve on a matrix held in 16 bits
 * per element (N^2 * 2 bytes read per round), widened to fp32 in registers -
 * exactly, for both formats - with every vector, the stop test, lambda and
 * all arithmetic in fp32, as st_solve_device_f32 with ST_FLAG_MATRIX_FREE
 * runs them.  The only difference from solving the widened fp32 matrix is the
 * association of the row sums (8 columns per lane and load instead of 4).
 * `storage` codes (the `dtype` parameters of the other calls keep accepting
 * 0 and 1 only): */
#define ST_STORE_F16  2   /* IEEE binary16 */
#define ST_STORE_BF16 3   /* bfloat16      */
/* d_mat: device pointer, dim x dim row-major 16-bit elements, READ ONLY
 * (never written, no copy made).  d_eigen_vec / eigen_vec_host / eigen_val /
 * iter_cnt as st_solve_device_f32 (fp32).  opt: eps < 0 selects ST_EPS_F32;
 * max_itr, semantics and batch as in st_solve_device_f32;
 * ST_FLAG_MATRIX_FREE is accepted and implied, ST_FLAG_TIME_KERNELS and
 * ST_FLAG_TRACE_SUMS work (st_last_round_times; st_last_round_sums returns
 * float elements); ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and
 * ST_FLAG_BATCH_ROUNDS are errors ("not supported"), as is a storage code
 * other than 2 or 3 (the message names it) - checked before anything is
 * enqueued, never a fallback.  Returns loop ms or negative. */
int64_t st_solve_device_half(void* wq, int storage, const void* d_mat,
                             unsigned int dim, float* d_eigen_vec,
                             float* eigen_vec_host, float* eigen_val,
                             unsigned int* iter_cnt, const st_options* opt,
                             st_stats* stats);
/* The host-pointer twin: copies the dim * dim * 2 bytes of `mat` in, solves,
 * copies out.  Returns h2d + loop ms or negative. */
int64_t max_eigen_value_half_ex(void* wq, int storage, const void* mat,
                                float* eigen_val, float* eigen_vec,
                                unsigned int dim, unsigned int* iter_cnt,
                                const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3a. batched solve (many small matrices, one launch)                     */
/* ---------------------------------------------------------------------- */

/* `batch` independent solves of dim x dim matrices in ONE launch, a
 * workgroup per matrix (k_solve_batched): dim from 1 to
 * st_solve_batched_max_dim (the matrix stays in one workgroup's registers).
 * d_mats: device pointer [batch][dim][dim], contiguous, row-major; every
 * matrix is TRANSFORMED IN PLACE like st_solve_device_*'s and ends at its
 * own A_end.  For dim % (16 / sizeof(element)) == 0 and a 16-byte aligned
 * d_mats every entry's eigen_val, eigenvector, iter_cnt, converged flag and
 * final matrix are bit-identical to st_solve_device_* on that matrix alone;
 * other dims sum a row in the same lane layout (the single solve sums them
 * element-wide), so they agree to rounding.  d_eigen_vecs: device pointer
 * [batch][dim] or NULL (then eigen_vecs_host must be non-NULL and receives
 * them; both may be given).  eigen_vals, iter_cnts, converged (1 where the
 * stop test passed before max_itr; may be NULL): host pointers [batch].
 * opt->eps, max_itr and semantics as in st_solve_device_*; opt->batch is
 * ignored; ST_FLAG_MATRIX_FREE, ST_FLAG_TIME_KERNELS, ST_FLAG_TRACE_SUMS
 * and ST_FLAG_ROUND_LOOP are errors, as are dim == 0, dim above the limit
 * and batch > 2^31 - 1 (never a fallback to another path).  batch == 0 is a
 * no-op returning 0.  stats->rounds is the largest number of rounds any
 * matrix evaluated, stats->converged 1 only if every matrix converged.
 * Returns loop ms or negative. */
int64_t st_solve_batched_f32(void* wq, float* d_mats, unsigned int batch,
                             unsigned int dim, float* d_eigen_vecs,
                             float* eigen_vecs_host, float* eigen_vals,
                             unsigned int* iter_cnts, unsigned int* converged,
                             const st_options* opt, st_stats* stats);
int64_t st_solve_batched_f64(void* wq, double* d_mats, unsigned int batch,
                             unsigned int dim, double* d_eigen_vecs,
                             double* eigen_vecs_host, double* eigen_vals,
                             unsigned int* iter_cnts, unsigned int* converged,
                             const st_options* opt, st_stats* stats);
/* The host-pointer twin (copies in, solves, copies out; mats is read only).
 * dtype: 0 = float32, 1 = float64.  mats [batch][dim][dim], eigen_vals
 * [batch], eigen_vecs [batch][dim], iter_cnts [batch]: host pointers.
 * Returns h2d + loop ms or negative. */
int64_t max_eigen_value_batched_ex(void* wq, int dtype, const void* mats,
                                   void* eigen_vals, void* eigen_vecs,
                                   unsigned int batch, unsigned int dim,
                                   unsigned int* iter_cnts,
                                   const st_options* opt, st_stats* stats);
/* Largest dim the batched solve accepts for dtype (0 = f32: 256,
 * 1 = f64: 128; anything else: 0).  No GPU needed. */
unsigned int st_solve_batched_max_dim(int dtype);

/* ST_FLAG_BATCH_ROUNDS in opt->flags of the three calls above selects the
 * round-loop form of the batched solve, for matrices beyond one workgroup's
 * registers: dim from 1 to st_solve_batched_rounds_max_dim, the sizes whose
 * single solve runs one k_round launch per round (dim * dim elements below
 * the 144 MiB flat threshold, st_round_flat_pays).  One launch per round
 * covers the whole batch (k_round_batched: the grid's y / z select the
 * matrix, its row sums, its eigenvector and its own state); a matrix that
 * has stopped costs workgroups that return at once while the others carry
 * on.  Rounds are enqueued opt->batch at a time (0 = 8) and the host looks
 * at one word, the count of finished matrices, per check.  Every matrix is
 * transformed in place to its own A_end.  For a 16-byte aligned d_mats every
 * entry's eigen_val, eigenvector, iter_cnt, converged flag and final matrix
 * are bit-identical to st_solve_device_* on that matrix alone AT EVERY DIM:
 * each matrix runs the kernel instantiation of its single solve on the same
 * lane layout (dims with dim % (16 / sizeof(element)) != 0 included: both
 * sides take the element-wide path there).  stats->fused_launches is the
 * number of rounds enqueued.  Without the flag the calls behave exactly as
 * documented above.  ST_FLAG_MATRIX_FREE, ST_FLAG_TIME_KERNELS,
 * ST_FLAG_TRACE_SUMS and ST_FLAG_ROUND_LOOP stay errors; a dim above the
 * limit is an error ("exceeds the round-loop limit"), never a fallback. */
/* Largest dim of the round-loop form for dtype (0 = f32: 6143, 1 = f64:
 * 4344; anything else: 0), derived from st_round_flat_pays.  No GPU needed. */
unsigned int st_solve_batched_rounds_max_dim(int dtype);

/* Variable-size batch ("vbatched"): `batch` independent solves of matrices of
 * DIFFERENT dims in one call.  The batch is split into at most
 * ST_VBATCH_CLASSES workgroup-shape classes (dim <= 4, 8, 16, 32, 64, 128,
 * 256; the last fp32 only), the classes st_solve_batched_* chooses from, and
 * each non-empty class is one launch (k_solve_vbatched), a workgroup per
 * matrix, largest class first.
 * d_mat_ptrs: HOST array [batch] of device pointers, matrix b is dims[b] x
 * dims[b], row-major, contiguous, TRANSFORMED IN PLACE to its own A_end; the
 * matrices must not overlap.  dims: HOST array [batch], each 1 ..
 * st_solve_batched_max_dim.  Eigenvectors are packed: matrix b's at element
 * offset sum_{j<b} dims[j] of d_eigen_vecs (device) and/or eigen_vecs_host.
 * eigen_vals / iter_cnts / converged (may be NULL): host [batch], input
 * order.  Every entry's eigen_val, eigenvector, iter_cnt, converged flag and
 * final matrix are bit-identical to st_solve_batched_* on that matrix alone
 * (batch = 1), whatever its alignment: a matrix whose dim is a multiple of
 * 16 / sizeof(element) and whose pointer is 16-byte aligned is loaded and
 * stored 16 bytes at a time, any other element-wide, into the same lanes.
 * opt as for st_solve_batched_*; ST_FLAG_BATCH_ROUNDS is an error here as are
 * the four flags that are errors there; a dim of 0 or above the limit and a
 * NULL matrix pointer are errors naming the index, never a fallback and never
 * a partial solve (checked before anything is enqueued).  batch == 0: no-op
 * returning 0.  stats->fused_launches = the number of class launches.
 * Returns loop ms or negative. */
int64_t st_solve_vbatched_f32(void* wq, float* const* d_mat_ptrs,
                              const uint32_t* dims, unsigned int batch,
                              float* d_eigen_vecs, float* eigen_vecs_host,
                              float* eigen_vals, unsigned int* iter_cnts,
                              unsigned int* converged, const st_options* opt,
                              st_stats* stats);
int64_t st_solve_vbatched_f64(void* wq, double* const* d_mat_ptrs,
                              const uint32_t* dims, unsigned int batch,
                              double* d_eigen_vecs, double* eigen_vecs_host,
                              double* eigen_vals, unsigned int* iter_cnts,
                              unsigned int* converged, const st_options* opt,
                              st_stats* stats);
/* Host twin: mats = ONE host buffer holding the matrices tightly packed in
 * input order (matrix b at element offset sum_{j<b} dims[j]^2), read only;
 * one H2D copy.  dtype: 0 = float32, 1 = float64.  eigen_vals [batch],
 * eigen_vecs (packed as above), iter_cnts [batch]: host pointers.  The tight
 * packing leaves some matrices off 16-byte alignment on the device; those
 * take the element-wide path (same bits, see above).  Returns h2d + loop ms
 * or negative. */
int64_t max_eigen_value_vbatched_ex(void* wq, int dtype, const void* mats,
                                    const uint32_t* dims, unsigned int batch,
                                    void* eigen_vals, void* eigen_vecs,
                                    unsigned int* iter_cnts,
                                    const st_options* opt, st_stats* stats);
#define ST_VBATCH_CLASSES 7
/* Size-class plan of a variable-size batch for dtype (0 f32, 1 f64):
 * order_out[batch] = the matrix indices sorted by class, input order kept
 * within a class; class_first[ST_VBATCH_CLASSES + 1] = where each class
 * starts in order_out (empty classes have equal neighbours).  Returns the
 * number of non-empty classes, or negative (dim 0 or above
 * st_solve_batched_max_dim: the message names the index and the dim; bad
 * dtype; null pointer).  No GPU needed. */
int st_vbatched_plan(int dtype, const uint32_t* dims, unsigned int batch,
                     uint32_t* order_out, uint32_t* class_first);

/* ---------------------------------------------------------------------- */
/* 3b. native multi-GPU solve (one process, ngpus devices, RCCL)           */
/* ---------------------------------------------------------------------- */

/* Row-block sharded solve over `ngpus` devices (`devices` = list of HIP
 * device ids, or NULL for 0..ngpus-1) with ONE ncclAllGather of the row-sum
 * vector per round.  Input: gen_kind 0 = host matrix `mat`
 * (dim x dim, row-major; each device copies its rows), 1 = Hilbert,
 * 2 = seeded random (generated on each device for its rows; `mat` unused).
 * Outputs on the host.  opt may select ST_FLAG_MATRIX_FREE.  stats->h2d_ms
 * reports the setup (allocation, input, communicator, first row sums),
 * stats->loop_ms the round loop.  Returns total ms or negative. */
int64_t st_solve_multi_f32(const float* mat, unsigned int dim, int ngpus,
                           const int* devices, int gen_kind, uint64_t seed,
                           float* eigen_val, float* eigen_vec,
                           unsigned int* iter_cnt, const st_options* opt,
                           st_stats* stats);
int64_t st_solve_multi_f64(const double* mat, unsigned int dim, int ngpus,
                           const int* devices, int gen_kind, uint64_t seed,
                           double* eigen_val, double* eigen_vec,
                           unsigned int* iter_cnt, const st_options* opt,
                           st_stats* stats);

/* One-process-per-GPU RCCL communicator for the sharded step API: one
 * process calls st_comm_unique_id (ST_COMM_ID_BYTES), the caller
 * distributes the id, every rank calls st_comm_init (nranks, its rank, its
 * HIP device); the process that made the id must join too.  st_allgather is
 * ncclAllGather on `stream` (in place when send = recv + rank*count).
 *
 * Presence before RCCL: the id is a rendezvous id, not an RCCL one - the
 * maker listens on a TCP port of the address it advertises (ST_COMM_ADDR,
 * else the first IPv4 address of NCCL_SOCKET_IFNAME's or of the first up
 * non-loopback interface, else 127.0.0.1).  st_comm_init on every rank
 * first joins it; only when all nranks are present (and still connected)
 * does the maker create the RCCL id and hand it to all, every rank
 * acknowledges it, and only on the maker's final "go" does any rank enter
 * ncclCommInitRankConfig (all ranks enter RCCL or none does).  A rank that
 * does not arrive within the deadline makes st_comm_init return -1 on every
 * present rank, eigen_last_error() naming the missing ranks, with no RCCL
 * state created (the process exits normally).  Connections that present no
 * hello within 5 s are dropped without delaying the others.
 *
 * Deadline: every communicator is non-blocking (ncclConfig_t.blocking = 0)
 * and each step that waits for peers - the rendezvous, st_comm_init's RCCL
 * init, a collective's connection setup, st_comm_destroy, and the
 * communicator setup and all-gathers of st_solve_multi_* - waits at most
 * st_set_comm_timeout() seconds (default: the environment variable
 * ST_COMM_TIMEOUT_S, else 120).  Past it the call returns -1 naming the RCCL
 * rank and HIP device still in progress; a communicator whose init has
 * returned is aborted (ncclCommAbort), one whose init has not is left to
 * the init thread, which aborts it if the init ever returns (the error then
 * says to end the process with _exit: a peer died after the rendezvous). */
#define ST_COMM_ID_BYTES 128
int st_comm_unique_id(char* id_out);
/* The same, advertising `addr` (dotted IPv4, e.g. "127.0.0.1" when every
 * rank runs on this host; NULL = the choice above). */
int st_comm_unique_id_addr(char* id_out, const char* addr);
int st_comm_init(void** comm, int nranks, int rank, const char* id_in,
                 int device);
/* Close the listener of an id this process made and will not join (e.g. its
 * maker failed before st_comm_init): 0, or 1 if there is none (already
 * joined or released, or made elsewhere).  An id never joined nor released
 * is closed by a later st_comm_unique_id once 2 x the deadline + 30 s have
 * passed. */
int st_comm_id_release(const char* id);
int st_comm_destroy(void* comm);
/* Set the RCCL deadline in seconds (<= 0: back to ST_COMM_TIMEOUT_S / 120);
 * returns the previous effective value.  Process-wide. */
double st_set_comm_timeout(double seconds);
/* The effective RCCL deadline in seconds (the setter's, ST_COMM_TIMEOUT_S or
 * 120). */
double st_get_comm_timeout(void);
/* The RCCL the library's calls are bound to: *version_code = ncclGetVersion
 * (X*10000 + Y*100 + Z) and `path` = the file holding the bound
 * ncclAllGather (dladdr); inside a torch process that is torch's bundled
 * librccl, for a C caller the /opt/rocm one the library links.  Either
 * output may be NULL.  Returns 0 or -1.  No GPU needed. */
int st_rccl_version(int* version_code, char* path, int path_len);
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice): the ranks RCCL joined, this rank, its HIP device.
 * Any output pointer may be NULL.  Returns 0 or negative. */
int st_comm_info(void* comm, int* nranks, int* rank, int* device);
int st_allgather_f32(void* comm, const float* send, float* recv,
                     uint64_t count, void* stream);
int st_allgather_f64(void* comm, const double* send, double* recv,
                     uint64_t count, void* stream);

/* ---------------------------------------------------------------------- */
/* 3c. sparse (CSR) solve                                                  */
/* ---------------------------------------------------------------------- */

/* The matrix-free solve on a nonnegative SPARSE matrix in CSR storage: the
 * iteration, stop test, v, lambda, counts and semantics of
 * st_solve_device_f32 / _f64 with ST_FLAG_MATRIX_FREE, with the sweep over a
 * dense row replaced by a CSR row product - nnz * (b + 4) bytes per round.
 * Storage: square n x n, 1 <= n < 2^31; row_ptr int64 [n + 1], col_idx int32
 * [nnz], vals fp32 / fp64 [nnz] (dtype 0 / 1).  Column indices within a row
 * need not be sorted; duplicates are legal and add up; no alignment beyond
 * the element's own.  The sign of the values is not checked (as in the dense
 * paths).
 *
 * Row classes: a row is shared by 4, 16, 64 (one wave) or 256 (one
 * workgroup) lanes according to its OWN nnz (<= 16, <= 128, <= 2048, above);
 * st_csr_class_limits returns the table.  The plan - built once per matrix -
 * is the row indices sorted by class, row order kept within a class, and the
 * class starts; a round's row products are ONE launch over all classes.
 * Summation order of a row (fixed, no atomics): with L lanes, lane t takes
 * the entries start + t, start + t + L, ... in storage order, one fused
 * multiply-add each, then the L lanes combine by a fixed halving tree (L =
 * 256: each wave's tree, then the 4 wave partials added in wave order).  A
 * row's result depends only on its own entries and on x - not on the other
 * rows of the matrix nor on where the row stands. */
#define ST_CSR_CLASSES 4
/* The class table for dtype (0 f32, 1 f64; the same for both today): the
 * first min(cap, ST_CSR_CLASSES) entries of nnz_max (the largest nnz of a
 * row of the class; 0xffffffff for the last) and lanes (either may be
 * NULL).  Returns ST_CSR_CLASSES, or negative (bad dtype).  No GPU needed. */
int st_csr_class_limits(int dtype, uint32_t* nnz_max, uint32_t* lanes, int cap);
/* The plan of a HOST row_ptr [n + 1]: order_out[n] = the row indices sorted
 * by class, row order kept within a class; class_first[ST_CSR_CLASSES + 1] =
 * where each class starts in order_out.  Returns the number of non-empty
 * classes, or negative: row_ptr[0] != 0, an empty row or a decreasing
 * row_ptr (the message names the row), n outside [1, 2^31), null pointer.
 * No GPU needed. */
int st_csr_plan(const int64_t* row_ptr, uint32_t n, uint32_t* order_out,
                uint32_t* class_first);
/* The shape the CSR kernels were built with ("lanes=4,16,64,256
 * nnz_max=16,128,2048,inf rows=8,4,2,1 unroll=1,2,4,8 prep_grid=2048
 * check_grid=8192": lanes per row and nnz limit of each class, rows the lanes
 * of a row take side by side and entries of each in flight, the workgroup cap
 * of the vector pass and of the create-time column check);
 * tools record it next to their numbers.  On MI355X (tools/bench_csr.py,
 * profiles/csr_solve.json, one interleaved run, n = 4194304): 0.633 / 1.981 /
 * 7.702 ms per fp32 round at 8 / 32 / 128 random columns per row (715 / 635 /
 * 582 GB/s: bound by the gathers of x), 0.639 ms (1968 GB/s) at 32 columns
 * within 2048 of the diagonal; torch.mv on the same arrays took 13.5 - 19.9
 * ms.  No GPU needed. */
const char* st_csr_shape_desc(void);
/* A matrix handle over DEVICE arrays, which are read only, not copied, and
 * must stay alive and unchanged until st_csr_destroy.  Validation comes
 * before any gather: first row_ptr on its own (row_ptr[0] == 0, strictly
 * increasing - an empty row would divide by zero -, row_ptr[n] == nnz);
 * only if that passes every col_idx[e], e in [0, nnz), against [0, n).
 * The first offending row or entry is named in eigen_last_error() and no
 * handle is made.  Then the plan is built on the device.  Runs on wq's
 * stream and device and returns after it completed.  0 or negative. */
int st_csr_create(void* wq, int dtype, uint32_t n, uint64_t nnz,
                  const int64_t* d_row_ptr, const int32_t* d_col_idx,
                  const void* d_vals, void** out);
int st_csr_destroy(void* csr);
/* The handle's plan (built on the device), copied to the host: order_out [n]
 * and class_first [ST_CSR_CLASSES + 1], either may be NULL - what st_csr_plan
 * gives for the same row_ptr.  Returns the number of non-empty classes, or
 * negative. */
int st_csr_get_plan(void* csr, uint32_t* order_out, uint32_t* class_first);
/* The solve.  Output conventions of st_solve_device_*, in the handle's dtype
 * (d_eigen_vec device [n] or NULL, then eigen_vec_host receives it;
 * eigen_val one element; iter_cnt).  opt: eps < 0 selects the dtype's
 * default; max_itr, semantics and batch as in st_solve_device_*;
 * ST_FLAG_MATRIX_FREE is accepted and implied, ST_FLAG_TIME_KERNELS and
 * ST_FLAG_TRACE_SUMS work; ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and
 * ST_FLAG_BATCH_ROUNDS are errors ("not supported") - checked before
 * anything is enqueued, never a fallback.  A reducible matrix (e.g. a row
 * whose only entry is its diagonal) may never meet the stop test: the solve
 * then ends at max_itr with converged = 0.  Returns loop ms or negative. */
int64_t st_solve_csr(void* wq, void* csr, void* d_eigen_vec,
                     void* eigen_vec_host, void* eigen_val,
                     unsigned int* iter_cnt, const st_options* opt,
                     st_stats* stats);
/* The host-pointer twin: validates dtype, flags and the matrix ON THE HOST
 * (same order and messages, before the queue is even looked at), copies the
 * three arrays in, solves, copies out.  Returns h2d + loop ms or negative. */
int64_t max_eigen_value_csr_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                               const int64_t* row_ptr, const int32_t* col_idx,
                               const void* vals, void* eigen_val,
                               void* eigen_vec, unsigned int* iter_cnt,
                               const st_options* opt, st_stats* stats);

/* Transposed CSR: the LEFT Perron vector (u A = lambda u; the stationary
 * distribution of a row-stochastic P is u / sum(u)) is the right one of the
 * transposed matrix.  T(A) is DEFINED as the stable sort of A's entries by
 * column: t_row_ptr[c] = the number of entries with column < c; transposed
 * row c holds A's entries of column c in ascending storage position (so in
 * ascending source row, duplicates within a row in their order); t_col_idx
 * is each entry's source row, t_vals its value - numpy's
 * p = argsort(col_idx, kind="stable"), rows[p], vals[p].  The order in which a
 * transposed row is summed is therefore a property of A alone, and every bit
 * of a solve on the device's T(A) is that of a solve on a host-transposed
 * copy.
 *
 * st_csr_transpose_host: the host twin, a counting sort.  Refuses nnz >= 2^32
 * before any array is read (the device sort carries 32-bit entry indices),
 * then everything max_eigen_value_csr_ex refuses with the same messages, then
 * a column without any entry (the transposed matrix would have an empty row,
 * which divides by zero; the message names the LOWEST such column).  The
 * outputs ([n + 1] / [nnz] / [nnz]) must not overlap the inputs.  0 or
 * negative.  No GPU needed. */
int st_csr_transpose_host(int dtype, uint32_t n, uint64_t nnz,
                          const int64_t* row_ptr, const int32_t* col_idx,
                          const void* vals, int64_t* t_row_ptr,
                          int32_t* t_col_idx, void* t_vals);
/* The device transposition of a st_csr_create handle into the CALLER's device
 * arrays d_t_row_ptr [n + 1], d_t_col_idx [nnz], d_t_vals [nnz] (aligned to
 * their elements; refused when one overlaps an array of `csr` or another
 * output - checked by address range), and *out = a handle over them with its
 * plan built, of the same grade as st_csr_create's: a view, the arrays stay
 * the caller's and must outlive it; destroyed with st_csr_destroy; accepted
 * by every call of 3c and refused by those of 3d.  A hand-written stable LSD
 * radix sort by column, digit_bits bits per pass, ceil(bits(n - 1) /
 * digit_bits) passes of three launches (per-tile digit counts; a digit-major
 * scan of the tile x digit table; the stable scatter, ranks from ballots of
 * the digit's bits), then one gather of values and source rows through the
 * permutation.  No float atomics, no workgroup waits on another, every
 * computed destination is bounded.  t_row_ptr is the scan of the column
 * histogram; the lowest empty column is reported before anything is
 * scattered and no handle is made.  Runs on wq's stream and returns after it
 * completed.  0 or negative. */
int st_csr_transpose(void* wq, void* csr, int64_t* d_t_row_ptr,
                     int32_t* d_t_col_idx, void* d_t_vals, void** out);
/* Bytes of device scratch st_csr_transpose allocates and frees inside (the
 * handle's plan, 4 n bytes, not counted); 0 for an n outside [1, 2^31) or
 * nnz >= 2^32.  No GPU needed. */
uint64_t st_csr_transpose_scratch_bytes(uint32_t n, uint64_t nnz);
/* The shape the transposition was built with ("digit_bits=8 tile=2048
 * rounds=8 lanes=256 col_block=2048 payload=index grid=8192": bits per pass,
 * entries per workgroup = rounds x lanes, columns per workgroup of the
 * t_row_ptr scan, what travels with the key, the workgroup cap of the count
 * and the gather).  What tools/bench_csr_transpose.py
 * measured with it is in DESIGN.md, "Transposed CSR".  No GPU needed. */
const char* st_csr_transpose_shape_desc(void);
/* max_eigen_value_csr_ex for the LEFT vector: validates on the host (nnz <
 * 2^32, then as max_eigen_value_csr_ex), copies in, st_csr_transpose,
 * st_solve_csr on the result, copies out.  stats->h2d_ms is the copy and A's
 * check, stats->transpose_us the transposition, stats->loop_ms the solve.
 * Returns h2d + transposition + loop ms or negative.  A function of its own
 * and not a flag: the dense entry points ignore unknown flag bits. */
int64_t max_eigen_value_csr_left_ex(void* wq, int dtype, uint32_t n,
                                    uint64_t nnz, const int64_t* row_ptr,
                                    const int32_t* col_idx, const void* vals,
                                    void* eigen_val, void* eigen_vec,
                                    unsigned int* iter_cnt,
                                    const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3d. batched sparse (CSR) solve                                          */
/* ---------------------------------------------------------------------- */

/* Many sparse matrices in one call: every round is ONE pair of launches over
 * the stacked rows of all matrices, every matrix keeps its own st_state and
 * stops in its own round, and lambda, iterations, converged flag and
 * eigenvector of each are bit for bit what st_solve_csr gives it alone with
 * the same options (a row's product depends on its own entries and x only,
 * its lane class on its own nnz, and max / stop test fold exactly under any
 * partition).
 *
 * Stacked CSR: `batch` >= 1 matrices, matrix b square of n_b >= 1 rows,
 * N = sum n_b < 2^31.
 *   mat_first  HOST uint32 [batch + 1]: the first stacked row of each matrix;
 *              mat_first[0] == 0, strictly increasing, mat_first[batch] == N
 *              (N is read from here: a wrong last element shows as
 *              row_ptr[N] != nnz)
 *   row_ptr    int64 [N + 1] over the concatenated entries: row_ptr[0] == 0,
 *              strictly increasing, row_ptr[N] == nnz
 *   col_idx    int32 [nnz], LOCAL to its matrix: in [0, n_b)
 *   vals       fp32 / fp64 [nnz] (dtype 0 / 1)
 * i.e. the single-matrix arrays concatenated with row_ptr rebased.  Unsorted
 * and duplicate columns stay legal.  Eigenvectors are stacked likewise:
 * matrix b's at element mat_first[b].
 *
 * st_csr_batch_create: a handle over DEVICE arrays (read only, not copied,
 * alive and unchanged until st_csr_batch_destroy); mat_first is copied.
 * Validation before any gather: mat_first on the host, row_ptr's predicate
 * over the N stacked rows, then every column against its OWN matrix's n_b (a
 * column >= n_b but < N is refused: no entry couples two matrices).  The
 * lowest offender is named in eigen_last_error() with its matrix and local
 * row or entry, and no handle is made.  Then the plan over the N stacked
 * rows - st_csr_plan of the stacked row_ptr - is built on the device.  A
 * st_csr_create handle is refused by every call here, and a batch handle by
 * every call of 3c. */
int st_csr_batch_create(void* wq, int dtype, uint32_t batch,
                        const uint32_t* mat_first, uint64_t nnz,
                        const int64_t* d_row_ptr, const int32_t* d_col_idx,
                        const void* d_vals, void** out);
int st_csr_batch_destroy(void* h);
/* The handle's plan: order_out [N] and class_first [ST_CSR_CLASSES + 1],
 * either may be NULL, as st_csr_get_plan. */
int st_csr_batch_get_plan(void* h, uint32_t* order_out, uint32_t* class_first);
/* The launch shape of the batch kernels, for tools to record
 * (tools/bench_csr_batched.py; what it measured is in DESIGN.md, "Batched
 * sparse solve"); it ends with the caps of the create-time column check (16
 * lanes per row, at most 8192 workgroups) and of the collect pass
 * (collect_grid=2048).  No GPU needed. */
const char* st_csr_batch_shape_desc(void);
/* The solve.  d_eigen_vecs device [N] or NULL, then eigen_vecs_host receives
 * the stacked eigenvectors; eigen_vals (the handle's dtype), iter_cnts and
 * converged (may be NULL) are HOST arrays [batch].  opt: eps, max_itr,
 * semantics and batch (rounds per host check, 0 = 8) as in st_solve_csr;
 * ST_FLAG_MATRIX_FREE is accepted and implied; ST_FLAG_TIME_KERNELS,
 * ST_FLAG_TRACE_SUMS, ST_FLAG_ROUND_LOOP, ST_FLAG_WRITE_EVERY_ROUND and
 * ST_FLAG_BATCH_ROUNDS are errors ("not supported"), checked before anything
 * is enqueued.  stats->rounds = the largest count of rounds any matrix
 * evaluated, converged = 1 only if every matrix converged, fused_launches =
 * the rounds enqueued.  For ONE matrix st_solve_csr is the call to use (see
 * DESIGN.md, "Batched sparse solve").  Returns loop ms or negative. */
int64_t st_solve_csr_batched(void* wq, void* h, void* d_eigen_vecs,
                             void* eigen_vecs_host, void* eigen_vals,
                             unsigned int* iter_cnts, unsigned int* converged,
                             const st_options* opt, st_stats* stats);
/* The host-pointer twin: validates dtype, flags, mat_first, row_ptr and the
 * columns ON THE HOST (same predicates and messages, before the queue is
 * even looked at), copies the arrays in, solves, copies out. */
int64_t max_eigen_value_csr_batched_ex(void* wq, int dtype, uint32_t batch,
                                       const uint32_t* mat_first, uint64_t nnz,
                                       const int64_t* row_ptr,
                                       const int32_t* col_idx, const void* vals,
                                       void* eigen_vals, void* eigen_vecs,
                                       unsigned int* iter_cnts,
                                       unsigned int* converged,
                                       const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3e. sparse (CSR) solve with low-rank terms and empty rows               */
/* ---------------------------------------------------------------------- */

/* The operator M = A + sum_{j < K} u_j w_j^T, 1 <= K <= ST_CSR_TERMS_MAX: A a
 * st_csr_create / st_csr_create_ex handle, u_j and w_j dense DEVICE vectors
 * [n] in the handle's dtype, nonnegative and finite.  No entry of M is
 * stored: a round of st_solve_csr becomes
 *   x      = v_prev * s_prev                      (k_csr_prep's pass)
 *   d_j    = w_j . x                    j < K     (the same pass + k_csr_dots)
 *   tot_r  = row r of A times x, in st_solve_csr's order (0 for an empty row)
 *   tot_r  = fma(u_j[r], d_j, tot_r)    j = 0 .. K-1, in that order
 *   s_next = tot_r / x[r];  v_cur[r] = v_prev[r] * (s_prev[r] / m)
 * and launch 0 the same with x = 1.  Three launches per round, all gated on
 * the state as st_csr_mfree_round's two; stop test, m, lambda, counts, both
 * semantics, batches, tracing, timing as st_solve_csr.  With u_j = 0 every
 * bit is st_solve_csr's.  This is how a reducible or periodic matrix (a link
 * graph) is made primitive - the Google matrix alpha P^T + t ((1 - alpha) 1 +
 * alpha [row of P empty])^T is one term.
 *
 * The order of a dot d_j is a function of n alone (not of K, the other terms,
 * the matrix or timing): G = min(ceil(n / 256), 2048) workgroups of 256
 * lanes; lane t of workgroup b takes i = b 256 + t + g G 256, g ascending, by
 * fma from 0; wave_sum's tree over the 64 lanes of a wave; the four wave
 * sums in wave order -> partial[j][b]; then one workgroup: lane t adds
 * partial[j][t + 256 g], g ascending, from 0, the same tree, the same four
 * adds -> dots[j].  No float atomics, no workgroup waits on another.
 *
 * Empty rows.  ST_CSR_EMPTY_ROWS_OK makes st_csr_create_ex accept rows without
 * an entry (row_ptr must not decrease; nnz >= 1 stays required; such a row is
 * of class 0) and st_csr_transpose_ex / st_csr_transpose_host_ex accept
 * columns without one (the result then has empty rows).  Without the flag the
 * _ex calls are the plain ones.  A handle with empty rows is refused, the
 * lowest such row named, by whatever divides by a row sum of A alone:
 * st_solve_csr, st_csr_mfree_round (and max_eigen_value_csr_ex refuses the
 * arrays as before); the calls of this section take it. */
#define ST_CSR_TERMS_MAX 4
#define ST_CSR_EMPTY_ROWS_OK 1u
int st_csr_create_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                     const int64_t* d_row_ptr, const int32_t* d_col_idx,
                     const void* d_vals, unsigned int flags, void** out);
/* The handle's rows without an entry and the lowest one (n when none);
 * either pointer may be NULL.  0 or negative. */
int st_csr_empty_rows(void* csr, uint32_t* count, uint32_t* lowest);
int st_csr_transpose_ex(void* wq, void* csr, int64_t* d_t_row_ptr,
                        int32_t* d_t_col_idx, void* d_t_vals,
                        unsigned int flags, void** out);
int st_csr_transpose_host_ex(int dtype, uint32_t n, uint64_t nnz,
                             const int64_t* row_ptr, const int32_t* col_idx,
                             const void* vals, int64_t* t_row_ptr,
                             int32_t* t_col_idx, void* t_vals,
                             unsigned int flags);
/* A terms object over K pairs of device vectors (d_u[j], d_w[j]: host arrays
 * of K device pointers), which stay the caller's and must outlive it.
 * Validation on the device, before anything else: one pass over the vectors
 * - every entry finite and >= 0, the lowest offender in the order (term, u
 * before w, index) named as "u_1[17]" - then launch 0 of the operator: every
 * s_0[r] finite and > 0, else "row r of A + Σ u wᵀ has no positive entry" (a
 * row of M with a positive entry stays positive for every positive x, so no
 * round divides by zero).  The object is bound to `csr`: every call refuses
 * it with another handle.  Runs on wq's stream; returns after it completed. */
int st_csr_terms_create(void* wq, void* csr, uint32_t K,
                        const void* const* d_u, const void* const* d_w,
                        void** terms);
int st_csr_terms_destroy(void* terms);
/* Bytes of the scratch st_csr_terms_rowsum / st_csr_terms_round take (256-byte
 * aligned): dots [K] at offset 0, the workgroup partials [K][2048] at 256, x
 * [n] behind them; 0 for a bad n or K.  No GPU needed. */
uint64_t st_csr_terms_scratch_bytes(uint32_t n, uint32_t K);
/* "terms_max=4 dot_grid=2048 lanes=256 combine=one_workgroup
 * launches_per_round=3 dots_offset=0 partial_offset=256 check_grid=8192"
 * (check_grid: the workgroup cap of the create-time checks).  What
 * tools/bench_csr_terms.py measured with it is in DESIGN.md, "Low-rank terms
 * and empty rows".  No GPU needed. */
const char* st_csr_terms_shape_desc(void);
/* st_solve_csr on the operator; the same arguments and conventions. */
int64_t st_solve_csr_terms(void* wq, void* csr, void* terms, void* d_eigen_vec,
                           void* eigen_vec_host, void* eigen_val,
                           unsigned int* iter_cnt, const st_options* opt,
                           st_stats* stats);
/* The host-pointer twin (u, w: K host vectors each): validates ON THE HOST -
 * dtype, opt's flags, `flags` (ST_CSR_EMPTY_ROWS_OK), the matrix, K, the
 * vectors, the rows of the operator, same order and messages - copies in,
 * solves, copies out.  Returns h2d + loop ms or negative. */
int64_t max_eigen_value_csr_terms_ex(void* wq, int dtype, uint32_t n,
                                     uint64_t nnz, const int64_t* row_ptr,
                                     const int32_t* col_idx, const void* vals,
                                     uint32_t K, const void* const* u,
                                     const void* const* w, unsigned int flags,
                                     void* eigen_val, void* eigen_vec,
                                     unsigned int* iter_cnt,
                                     const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3f. many term sets on one sparse matrix                                  */
/* ---------------------------------------------------------------------- */

/* C operators on ONE handle, M_c = A + sum_{j < K} u_{c,j} w_{c,j}^T, c < C,
 * 1 <= C <= ST_CSR_MULTI_MAX, 1 <= K <= ST_CSR_TERMS_MAX terms for every
 * column (a column that needs fewer pads with u = 0, which changes no bit; K
 * = 0 is refused: every column would be the same solve) - personalised
 * PageRank, one link graph under many teleport vectors.  One pass over the
 * matrix per round serves all columns: the library keeps packed copies
 * [n][CP] of s, v, x and [K][n][CP] of u, w, the column index fastest, CP =
 * the smallest of 2, 4, 8 that is >= C, so one gather brings x[col] for every
 * column.  Every column has its own st_state and stops in its own round, and
 * its eigenvalue, eigenvector, count, converged flag and final state are bit
 * for bit st_solve_csr_terms' on (A, u_{c,.}, w_{c,.}) alone, for both
 * semantics, both dtypes and any max_itr.  No float atomics, no workgroup
 * waits on another.  Not offered here: tracing and kernel timing, a left
 * solve, batches, sharded or 16-bit storage, C > 8 in one call.
 *
 * st_csr_multi_create: d_u / d_w are host arrays of C * K device pointers,
 * [c * K + j] = a dense vector [n] in the handle's dtype; they are read
 * during the call only.  Validation on the device per column, the single
 * object's predicates, the lowest offender by (column, then term, u before w,
 * index; then the column's rows), the single message with the column in
 * front: "column 2: u_1[17] = -0.5 ...", "column 2: row 9 of A + Σ u wᵀ has
 * no positive entry".  The object is bound to `csr` (every call refuses it
 * with another handle) and owns its packed vectors: one solve at a time. */
#define ST_CSR_MULTI_MAX 8
int st_csr_multi_create(void* wq, void* csr, uint32_t C, uint32_t K,
                        const void* const* d_u, const void* const* d_w,
                        void** multi);
int st_csr_multi_destroy(void* multi);
/* Bytes of the scratch st_csr_multi_rowsum / st_csr_multi_round take (256-byte
 * aligned): dots [C][K] at offset 0, the workgroup partials [CP][K][2048] at
 * 256, x [n][CP] behind them; 0 for a bad n, C or K.  No GPU needed. */
uint64_t st_csr_multi_scratch_bytes(uint32_t n, uint32_t C, uint32_t K);
/* "multi_max=8 terms_max=4 widths=2,4,8 dot_grid=2048 lanes=256
 * combine=one_workgroup_per_column launches_per_round=3 dots_offset=0
 * partial_offset=256 rows16=... unroll16=... rows32=... unroll32=... rows64=...
 * unroll64=... check_grid=8192": check_grid is the workgroup cap of the
 * create-time passes (pack, checks, collect); rowsB / unrollB are the rows side by side and the entries in
 * flight per lane of the four row classes when a packed row is B = CP * b
 * bytes.  What tools/bench_csr_multi.py measured with it is in DESIGN.md,
 * "Many term sets on one matrix".  No GPU needed. */
const char* st_csr_multi_shape_desc(void);
/* st_solve_csr_batched's conventions: d_eigen_vecs device [C][n] (each column
 * contiguous) and / or eigen_vecs_host, eigen_vals [C] in the handle's dtype,
 * iter_cnts [C], converged [C] (may be NULL); opt->batch rounds (default 8)
 * per host check of the count of finished columns. */
int64_t st_solve_csr_multi(void* wq, void* csr, void* multi, void* d_eigen_vecs,
                           void* eigen_vecs_host, void* eigen_vals,
                           unsigned int* iter_cnts, unsigned int* converged,
                           const st_options* opt, st_stats* stats);
/* The host-pointer twin (u, w: C * K host vectors, [c * K + j]): validates ON
 * THE HOST - dtype, opt's flags, `flags` (ST_CSR_EMPTY_ROWS_OK), the matrix, C
 * and K, then column after column the vectors and the rows of M_c, same
 * messages - packs on the host, copies in, solves, copies out. */
int64_t max_eigen_value_csr_multi_ex(void* wq, int dtype, uint32_t n,
                                     uint64_t nnz, const int64_t* row_ptr,
                                     const int32_t* col_idx, const void* vals,
                                     uint32_t C, uint32_t K,
                                     const void* const* u, const void* const* w,
                                     unsigned int flags, void* eigen_vals,
                                     void* eigen_vecs, unsigned int* iter_cnts,
                                     unsigned int* converged,
                                     const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3g. sparse (CSR) solve on a product operator B A                        */
/* ---------------------------------------------------------------------- */

/* The operator M = B A: A and B two st_csr_create / st_csr_create_ex handles
 * of the same n, dtype and device; the same handle twice gives A^2.  No entry
 * of M is stored or formed (it would hold about d^2 entries per row where the
 * factors hold 2 d): a round of st_solve_csr becomes
 *   x      = v_prev * s_prev                      (k_csr_prep, unchanged)
 *   y[r]   = row r of A times x                   (k_csrp_apply, A's plan)
 *   tot_r  = row r of B times y                   (k_csrp_final, B's plan)
 *   s_next = tot_r / x[r];  v_cur[r] = v_prev[r] * (s_prev[r] / m)
 * and launch 0 is y = the row sums of A (st_csr_rowsum), s_0 = B y.  Both row
 * products sum in st_solve_csr's order (section 3c), so a row's result
 * depends only on its own entries and the gathered vector.  Three launches
 * per round, all gated on the state as st_csr_mfree_round's two; stop test,
 * m, lambda, counts, both semantics, batches, tracing, timing as
 * st_solve_csr.  With the identity as one factor every bit is st_solve_csr's
 * on the other.  No float atomics, no workgroup waits on another.
 *
 * With st_csr_transpose_ex this gives HITS (authorities: A^T A, hubs: A A^T),
 * the spectral norm sqrt(lambda_max(A^T A)), SALSA, two-step chains P^2 and
 * bipartite projections B B^T.
 *
 * Empty rows: A may have them (ST_CSR_EMPTY_ROWS_OK; such a row gives y[r] =
 * exactly 0).  Every row of M needs a positive entry.  Checked before any
 * round, in this order: both handles alive, same n, same dtype, same device,
 * then launch 0 on the device - every s_0[r] finite and > 0, else "row r of
 * B·A has no positive entry" with the lowest r (a row of M with a positive
 * entry stays positive for every positive x, so no round divides by zero).
 * An empty row of B is such a row.
 *
 * Not offered: rectangular factors (pad to square with empty rows and
 * columns), more than two factors, terms on a product, batched or
 * multi-column products, mixed dtypes. */
int64_t st_solve_csr_product(void* wq, void* csr_b, void* csr_a,
                             void* d_eigen_vec, void* eigen_vec_host,
                             void* eigen_val, unsigned int* iter_cnt,
                             const st_options* opt, st_stats* stats);
/* y = A x in the solve's row order: a reproducible SpMV on its own.  d_x and
 * d_y device [n] in the handle's dtype, distinct; an empty row gives exactly
 * 0.  Asynchronous on `stream`. */
int st_csr_apply(void* csr, const void* d_x, void* d_y, void* stream);
/* Bytes of the scratch st_csr_product_rowsum / st_csr_product_round take
 * (256-byte aligned): x [n] at offset 0, y [n] at st_csr_product_scratch_bytes
 * / 2; 0 for a bad n.  No GPU needed. */
uint64_t st_csr_product_scratch_bytes(uint32_t n);
/* "factors=2 launches_per_round=3 launches_k0=2 prep_grid=2048 x_offset=0
 * y_offset=align256(8n) empty_rows=A check_grid=8192" (check_grid: the
 * workgroup cap of the s_0 check).  What tools/bench_csr_product.py
 * measures with it is in DESIGN.md, "Product operators".  No GPU needed. */
const char* st_csr_product_shape_desc(void);
/* The host-pointer twin with two triples (B's, then A's; n and dtype are
 * shared): validates ON THE HOST - dtype, opt's flags, `flags`
 * (ST_CSR_EMPTY_ROWS_OK: empty rows of A), B's triple, A's triple (messages
 * of max_eigen_value_csr_ex behind "csr product: factor B: " / "factor A: "),
 * then row by row that B has an entry b > 0 whose column is a row of A
 * holding a value > 0 (the device's message; the two predicates can differ
 * only where a product or sum under- or overflows) - copies in, solves,
 * copies out.  Returns h2d + loop ms or negative. */
int64_t max_eigen_value_csr_product_ex(void* wq, int dtype, uint32_t n,
                                       uint64_t b_nnz, const int64_t* b_row_ptr,
                                       const int32_t* b_col_idx,
                                       const void* b_vals, uint64_t a_nnz,
                                       const int64_t* a_row_ptr,
                                       const int32_t* a_col_idx,
                                       const void* a_vals, unsigned int flags,
                                       void* eigen_val, void* eigen_vec,
                                       unsigned int* iter_cnt,
                                       const st_options* opt, st_stats* stats);
/* The Gram operators of ONE host matrix: side ST_GRAM_ATA = A^T A (its
 * eigenvalue is the square of A's spectral norm), ST_GRAM_AAT = A A^T.
 * Validates on the host (nnz < 2^32, side, dtype, flags, the triple, then the
 * product on a host transposition), copies A in, transposes on the device
 * (st_csr_transpose_ex), solves, copies out.  stats->transpose_us is the
 * transposition. */
#define ST_GRAM_ATA 0
#define ST_GRAM_AAT 1
int64_t max_eigen_value_csr_gram_ex(void* wq, int dtype, uint32_t n,
                                    uint64_t nnz, const int64_t* row_ptr,
                                    const int32_t* col_idx, const void* vals,
                                    int side, unsigned int flags,
                                    void* eigen_val, void* eigen_vec,
                                    unsigned int* iter_cnt,
                                    const st_options* opt, st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3h. sparse (CSR) solve on a pattern-only matrix with row / column scales */
/* ---------------------------------------------------------------------- */

/* The operator M = diag(r) P diag(c) of an UNWEIGHTED graph: P[i][j] = the
 * number of entries of row i with column j (row_ptr / col_idx as in 3c;
 * duplicates count, as they add up there), r and c optional dense DEVICE
 * vectors [n] in the handle's dtype, each finite and strictly positive; NULL
 * means all ones and costs nothing at run time (the kernels are instantiated
 * without it).  r = c = 1 is the adjacency matrix, r = 1 / outdeg the
 * row-stochastic one, c = 1 / outdeg on the transposed pattern the
 * column-stochastic P^T of PageRank, r = c = d^-1/2 the symmetric normalised
 * one.  No value array exists: a round reads nnz * 4 bytes of matrix where
 * st_solve_csr reads nnz * 8 (fp32) or nnz * 12 (fp64), and the device
 * footprint of the matrix shrinks alike.  Launch k >= 1 is
 *   x_i    = v_prev[i] * s_prev[i];  z_i = c[i] * x_i   (one rounding each;
 *            only z is stored; max, stop test and state as k_csr_prep)
 *   d_j    = w_j . x                j < K   (terms; on x, not on z)
 *   tot_i  = the sum of z[col[e]] over row i in st_solve_csr's order: the same
 *            lane classes, lane t on entries t, t + L, ..., the same tree;
 *            a step is acc = acc + z, bit for bit fma(1, z, acc)
 *   tot_i  = r[i] * tot_i           (one multiply, when r is given)
 *   tot_i  = fma(u_j[i], d_j, tot_i)   j = 0 .. K-1
 *   s_next = tot_i / (v_prev[i] * s_prev[i]);  v_cur as st_solve_csr
 * and launch 0 the same sweep on z = c (or ones): s_0 = r * (P c).  Hence,
 * bit for bit: without scales every result is st_solve_csr's (3c, 3e with
 * terms) on the same arrays with vals = 1; with scales that are powers of two
 * it is st_solve_csr's on vals[e] = r[row] * c[col] as long as nothing
 * under- or overflows.  Other scales differ from that matrix by roundings (z
 * is rounded once, the product r * c never formed).  A row's result depends
 * on its own entries, its r and z only.
 *
 * A pattern handle is a kind of its own: every call of 3c - 3g refuses it
 * ("not a CSR matrix handle"), and every call here refuses a st_csr_create
 * handle ("not a CSR pattern handle").  Not offered on a pattern handle: the
 * product operator and st_csr_apply (3g), the multi-column solve (3f), the
 * batched solve (3d); build a st_csr_create handle with vals = 1 for those.
 *
 * st_csr_pattern_create: row_ptr and col_idx DEVICE arrays validated exactly
 * as st_csr_create_ex validates them (same order, same messages; flags:
 * ST_CSR_EMPTY_ROWS_OK or 0), then the plan, then ONE device pass over the
 * scales that names the lowest offender, row_scale before col_scale:
 * "csr pattern: row_scale[17] = -0.5 is not finite and positive".  The four
 * arrays stay the caller's, read only, alive and unchanged until
 * st_csr_pattern_destroy. */
int st_csr_pattern_create(void* wq, int dtype, uint32_t n, uint64_t nnz,
                          const int64_t* d_row_ptr, const int32_t* d_col_idx,
                          const void* d_row_scale, const void* d_col_scale,
                          unsigned int flags, void** out);
int st_csr_pattern_destroy(void* pat);
/* As st_csr_get_plan / st_csr_empty_rows. */
int st_csr_pattern_get_plan(void* pat, uint32_t* order_out, uint32_t* class_first);
int st_csr_pattern_empty_rows(void* pat, uint32_t* count, uint32_t* lowest);
/* T(P) into the caller's DEVICE arrays d_t_row_ptr [n + 1] and d_t_col_idx
 * [nnz] (they must not overlap the source's or each other): st_csr_transpose's
 * stable sort by column with a final gather of source rows only; both arrays
 * are byte for byte st_csr_transpose_ex's on the same pattern with any values.
 * The result is a pattern handle over them with r and c SWAPPED ((D_r P
 * D_c)^T = D_c P^T D_r; the scale vectors are shared with the source handle).
 * Same refusals: a column without an entry unless flags has
 * ST_CSR_EMPTY_ROWS_OK, nnz >= 2^32, overlap. */
int st_csr_pattern_transpose(void* wq, void* pat, int64_t* d_t_row_ptr,
                             int32_t* d_t_col_idx, unsigned int flags, void** out);
/* The terms of M + sum_j u_j w_j^T on a pattern handle: st_csr_terms_create's
 * contract (1 <= K <= ST_CSR_TERMS_MAX; the vectors in one pass, then launch
 * 0, then "row r of A + Σ u wᵀ has no positive entry").  The object is bound
 * to this pattern handle - every call of 3e refuses it, and every call here
 * one of another handle - and is destroyed with st_csr_terms_destroy. */
int st_csr_pattern_terms_create(void* wq, void* pat, uint32_t K,
                                const void* const* d_u, const void* const* d_w,
                                void** out);
/* The solve: st_solve_csr's conventions, flags, tracing and timing, through
 * the same loop; `terms` a st_csr_pattern_terms_create object of `pat` or
 * NULL.  An empty-rows handle without terms is refused, the lowest row named.
 * Returns loop ms or negative. */
int64_t st_solve_csr_pattern(void* wq, void* pat, void* terms, void* d_eigen_vec,
                             void* eigen_vec_host, void* eigen_val,
                             unsigned int* iter_cnt, const st_options* opt,
                             st_stats* stats);
/* Bytes of the scratch of st_csr_pattern_rowsum / st_csr_pattern_round:
 * st_csr_terms_scratch_bytes' layout (dots [K] | partial [K][2048] | a vector
 * [n]) with z where x stands; K = 0 is allowed (256 bytes, then z).  0 for a
 * bad n or K.  No GPU needed. */
uint64_t st_csr_pattern_scratch_bytes(uint32_t n, uint32_t K);
/* The launch shape of the pattern kernels and what the gfx950 compile gives
 * them: "... vgpr_f32=.. vgpr_f64=.. waves_f32=.. waves_f64=.." (the row
 * kernels of a round without terms and without a row scale; DESIGN.md,
 * "Pattern-only CSR", has every instantiation next to the values kernels';
 * tools/bench_csr_pattern.py records it).  No GPU needed. */
const char* st_csr_pattern_shape_desc(void);
/* The host-pointer twin: validates ON THE HOST, before the queue is even
 * looked at, with the device path's predicates and messages - dtype, opt's
 * flags, `flags` (ST_CSR_EMPTY_ROWS_OK), n, row_ptr, the columns, the scales
 * (row_scale before col_scale, the lowest index), K in [0,
 * ST_CSR_TERMS_MAX], the term vectors, the rows of the operator, and without
 * terms the empty rows - then copies in, solves, copies out.  row_scale /
 * col_scale may be NULL; K = 0 takes NULL u / w.  Returns h2d + loop ms or
 * negative. */
int64_t max_eigen_value_csr_pattern_ex(void* wq, int dtype, uint32_t n, uint64_t nnz,
                                       const int64_t* row_ptr, const int32_t* col_idx,
                                       const void* row_scale, const void* col_scale,
                                       uint32_t K, const void* const* u,
                                       const void* const* w, unsigned int flags,
                                       void* eigen_val, void* eigen_vec,
                                       unsigned int* iter_cnt, const st_options* opt,
                                       st_stats* stats);

/* ---------------------------------------------------------------------- */
/* 3i. dense LEFT Perron vector (u A = lambda u), no transposed copy       */
/* ---------------------------------------------------------------------- */

/* The matrix-free solve of section 3 turned by 90 degrees: s_k[c] =
 * (sum_r A_0[r][c] x[r]) / x[c], x = v_{k-2} * s_{k-1}, on the row-major
 * matrix where it lies.  What it returns is the Perron pair of A^T: lambda
 * and the LEFT vector u of A (the stationary distribution of a row-stochastic
 * A, up to its scale).  d_mat: device pointer, dim x dim row-major, READ ONLY
 * - never written and never copied on the device; the only workspace is the
 * vectors and ceil(dim / RB) * dim elements of partial sums (RB:
 * st_left_shape).  d_eigen_vec / eigen_vec_host / eigen_val / iter_cnt as
 * st_solve_device_*.  opt: eps, max_itr, semantics and batch as there;
 * ST_FLAG_MATRIX_FREE is accepted and implied, ST_FLAG_TIME_KERNELS and
 * ST_FLAG_TRACE_SUMS work (st_last_round_times, st_last_round_sums: the
 * COLUMN sums every round evaluated); ST_FLAG_ROUND_LOOP,
 * ST_FLAG_WRITE_EVERY_ROUND and ST_FLAG_BATCH_ROUNDS are errors ("not
 * supported"), as are a NULL matrix and dim == 0 - checked before anything is
 * enqueued, never a fallback.  v and the whole st_state of every round are
 * bit for bit what st_solve_device_* with ST_FLAG_MATRIX_FREE computes from
 * the same sums; the sums themselves follow the column order below, so
 * lambda, v and the counts agree with the solve of a transposed copy to
 * rounding.  Returns loop ms or negative. */
int64_t st_solve_device_left_f32(void* wq, const float* d_mat, unsigned int dim,
                                 float* d_eigen_vec, float* eigen_vec_host,
                                 float* eigen_val, unsigned int* iter_cnt,
                                 const st_options* opt, st_stats* stats);
int64_t st_solve_device_left_f64(void* wq, const double* d_mat, unsigned int dim,
                                 double* d_eigen_vec, double* eigen_vec_host,
                                 double* eigen_val, unsigned int* iter_cnt,
                                 const st_options* opt, st_stats* stats);
/* The host-pointer twin (dtype: 0 = float32, 1 = float64): checks opt's
 * flags and semantics, the matrix, dim, the outputs and the queue, in that
 * order, then copies the dim * dim elements of `mat` in as they are, solves,
 * copies out.  Returns h2d + loop ms or negative. */
int64_t max_eigen_value_left_ex(void* wq, int dtype, const void* mat,
                                void* eigen_val, void* eigen_vec,
                                unsigned int dim, unsigned int* iter_cnt,
                                const st_options* opt, st_stats* stats);
/* The summation order of a column, which is a function of (dtype, n) alone:
 * the rows are cut into blocks of *rows_per_block consecutive rows (the last
 * one shorter); within a block one accumulator starts from 0 and takes the
 * rows in ascending order, one fused multiply-add each (launch 0: the same
 * fma with 1); *combine says how the block values are added: 0 = serially in
 * ascending block order starting from block 0's value, 1 = a balanced tree
 * (this build: always 0).  Neither the grid, the strip a column falls in, the
 * vector width, the rows in flight nor the kind of load enters.  Either
 * pointer may be NULL.  Returns 0, or negative for a dtype other than 0 / 1
 * or n outside [1, 2^31).  No GPU needed. */
int st_left_shape(int dtype, unsigned int n, uint32_t* rows_per_block,
                  uint32_t* combine);
/* ELEMENTS of the step-level scratch of st_colsum_* / st_mfree_left_round_*:
 * x (n, rounded up to 64) then the partials, ceil(n / rows_per_block) * n.
 * 0 with an error message for a bad dtype or n.  No GPU needed. */
uint64_t st_left_scratch(int dtype, unsigned int n);
/* The launch shape the kernels were built with ("block=256 bytes_per_load=16
 * rows_in_flight=8 rows_per_block=32,64,128,256 rows_from=1,2048,4096,16384
 * combine=serial finish_block=64 prep_grid=2048 nt_from_mib=512": a workgroup
 * owns rows_per_block rows by a strip of block * (16 / sizeof(element))
 * columns - block columns when n * sizeof(element) is no multiple of 16 -, a
 * lane 16 bytes of each row with 8 rows' loads issued before the first fma;
 * rows_per_block by the n it starts from; non-temporal loads from 512 MiB);
 * tools record it next to their numbers (tools/bench_left.py).  No GPU
 * needed. */
const char* st_left_shape_desc(void);

/* ---------------------------------------------------------------------- */
/* 3j. dense Perron PAIR: the right and the left vector from one pass over */
/*     the matrix per round                                                */
/* ---------------------------------------------------------------------- */

/* side index of every [2] argument below */
#define ST_PAIR_RIGHT 0 /* A v = lambda v: what st_solve_device_* returns      */
#define ST_PAIR_LEFT 1  /* u A = lambda u: what st_solve_device_left_* returns */

/* Two independent iterations on one dense matrix - the matrix-free right
 * iteration s_R = (A x_R) / x_R of section 3 and the left iteration s_L =
 * (x_L^T A) / x_L of section 3i - each with its own state, vectors and stop
 * round; they share only the loads of the matrix, which every round reads
 * once.  d_mat: device pointer, dim x dim row-major, READ ONLY - never written
 * and never copied on the device; the workspace is the vectors and
 * st_pair_scratch elements.  d_eigen_vecs (device) / eigen_vecs_host: [2][dim],
 * either may be NULL but not both; eigen_vals [2], iter_cnts [2], converged
 * [2] (may be NULL) by side, with st_solve_csr_multi's conventions:
 * stats->rounds is the larger count, stats->converged is 1 only if both sides
 * converged, stats->fused_launches is the rounds enqueued.  opt: eps, max_itr,
 * semantics and batch (rounds per look at the count of finished sides, 0 = 8);
 * reaching max_itr ends each side on its own.  ST_FLAG_MATRIX_FREE is accepted
 * and implied; ST_FLAG_TIME_KERNELS, ST_FLAG_TRACE_SUMS, ST_FLAG_ROUND_LOOP,
 * ST_FLAG_WRITE_EVERY_ROUND and ST_FLAG_BATCH_ROUNDS are errors ("not
 * supported"), as are a NULL matrix and dim == 0 - checked before anything is
 * enqueued, never a fallback.
 *   The left side's sums follow st_left_shape's order: lambda, vector, count
 * and state of side 1 are bit for bit those of st_solve_device_left_* on the
 * same matrix.  The right side's sums follow st_pair_shape's order below, not
 * k_mfree's: its v and state are bit for bit what st_mfree_round_* computes
 * from the same sums, and lambda, v and the count agree with
 * st_solve_device_* (ST_FLAG_MATRIX_FREE) to rounding.  Whether one pair solve
 * is faster than the two solves it replaces is a measured property of the
 * build and the size: README.md and DESIGN.md carry the numbers
 * (tools/bench_pair.py).  Returns loop ms or negative. */
int64_t st_solve_device_pair_f32(void* wq, const float* d_mat, unsigned int dim,
                                 float* d_eigen_vecs, float* eigen_vecs_host,
                                 float* eigen_vals, unsigned int* iter_cnts,
                                 unsigned int* converged, const st_options* opt,
                                 st_stats* stats);
int64_t st_solve_device_pair_f64(void* wq, const double* d_mat, unsigned int dim,
                                 double* d_eigen_vecs, double* eigen_vecs_host,
                                 double* eigen_vals, unsigned int* iter_cnts,
                                 unsigned int* converged, const st_options* opt,
                                 st_stats* stats);
/* The host-pointer twin (dtype: 0 = float32, 1 = float64): checks opt's
 * flags and semantics, the matrix, dim, the outputs and the queue, in that
 * order, then copies the dim * dim elements of `mat` in as they are (one copy,
 * no transposed copy), solves, copies out.  eigen_vecs: host [2][dim].
 * Returns h2d + loop ms or negative. */
int64_t max_eigen_value_pair_ex(void* wq, int dtype, const void* mat,
                                void* eigen_vals, void* eigen_vecs,
                                unsigned int dim, unsigned int* iter_cnts,
                                unsigned int* converged, const st_options* opt,
                                st_stats* stats);
/* The summation orders, functions of (dtype, n) alone.  A COLUMN's sum (left
 * side) is st_left_shape's: blocks of *rows_per_block rows, *combine_left as
 * its combine.  A ROW's sum (right side): the row is cut into strips of
 * *strip_cols columns (1024 for float32, 512 for float64, the last one
 * shorter); in a strip, lane l of 256 takes the 16 / sizeof(element) adjacent
 * columns from strip * strip_cols + l * (16 / sizeof(element)) in ascending
 * order, one fused multiply-add each from 0 (launch 0: the same fma with 1;
 * columns past n left out); the 64 lanes of each of the four waves go through
 * the balanced tree of every other kernel here (pairs, quads, rows of 16,
 * (R3 + R2) + (R1 + R0)), the four wave sums are added serially in wave
 * order, and *combine_right says how the strip values are added: 0 = serially
 * in ascending strip order starting from strip 0's value (this build: always
 * 0).  Neither the grid, rows_per_block, the rows in flight nor the kind of
 * load enters a row's order.  For nonnegative data a row's sum lies within
 * 16 / sizeof(element) + 6 + 3 + (strips - 1) + 1 ulps of the exact one.  Any
 * pointer may be NULL.  Returns 0, or negative for a dtype other than 0 / 1
 * or n outside [1, 2^31).  No GPU needed. */
int st_pair_shape(int dtype, unsigned int n, uint32_t* rows_per_block,
                  uint32_t* strip_cols, uint32_t* combine_left,
                  uint32_t* combine_right);
/* ELEMENTS of the step-level scratch of st_pair_sum_* / st_mfree_pair_round_*:
 * [x_R | x_L | column partials | row partials] = 2 * (n rounded up to 64) +
 * (ceil(n / rows_per_block) * n rounded up to 64) + ceil(n / strip_cols) * n.
 * 0 with an error message for a bad dtype or n.  No GPU needed. */
uint64_t st_pair_scratch(int dtype, unsigned int n);
/* The launch shape the kernels were built with ("block=256 bytes_per_load=16
 * rows_in_flight=8 strip_cols=1024,512 rows_per_block=32,64,128,256
 * rows_from=1,2048,4096,16384 combine_left=serial combine_right=serial
 * lds_rows=256 finish_block=64 prep_grid=2048 nt_from_mib=512
 * launches_per_round=5": a workgroup owns rows_per_block rows by one strip, a
 * lane 16 bytes of each row - loaded as one vector, or element by element
 * when n * sizeof(element) is no multiple of 16 or a pointer is not 16-byte
 * aligned - with 8 rows' loads issued before the first fma; strip_cols by
 * dtype (f32, f64)); tools record it next to their numbers
 * (tools/bench_pair.py).  No GPU needed. */
const char* st_pair_shape_desc(void);

/* ---------------------------------------------------------------------- */
/* 4. step-level kernels (asynchronous on `stream`, a hipStream_t or NULL) */
/* ---------------------------------------------------------------------- */

/* Device state of one solve (64 bytes, zero = fresh). */
typedef struct st_state
{
  uint32_t done;   /* 1 once the stop test passed or max_itr was reached  */
  uint32_t round;  /* row-sum evaluations that did not stop               */
  uint32_t iters;  /* reference iter_count, valid once done               */
  uint32_t stop;   /* stop flag of the last evaluated round               */
  double lambda;   /* s[0] of the last evaluated round                    */
  double max;      /* max row sum of the last evaluated round             */
  uint32_t end;    /* st_round_*: 1 + the round that stopped, 0 = running */
  /* scratch of the flat round's stats launch (st_round_flat_*); zero
   * between launches, as st_state_reset leaves it */
  uint32_t arrivals; /* workgroups done                                   */
  uint64_t max_bits; /* running max (bit pattern of a value >= 0)         */
  uint32_t fail;     /* some pair |s_i - s_{i+1}| >= eps (or NaN)          */
  uint32_t pad0;
  uint64_t pad[1];
} st_state;

/* zero a state (hipMemsetAsync) */
int st_state_reset(st_state* d_state, void* stream);

/* inputs for rows [row0, row0+nrows) of an ncols-wide matrix:
 *   hilbert  A[r][c] = 1/(r+c+1) in the element type (utils.cpp:137-154)
 *   random   U(0,1] from splitmix64(seed, r*ncols+c) (replaces the
 *            non-reproducible utils.cpp:125-134)
 *   identity (utils.cpp:5-27), fill (constant value) */
int st_generate_hilbert_f32(float* d_mat, unsigned int nrows,
                            unsigned int ncols, unsigned int row0,
                            void* stream);
int st_generate_hilbert_f64(double* d_mat, unsigned int nrows,
                            unsigned int ncols, unsigned int row0,
                            void* stream);
int st_generate_random_f32(float* d_mat, unsigned int nrows,
                           unsigned int ncols, unsigned int row0,
                           uint64_t seed, void* stream);
int st_generate_random_f64(double* d_mat, unsigned int nrows,
                           unsigned int ncols, unsigned int row0,
                           uint64_t seed, void* stream);
int st_generate_identity_f32(float* d_mat, unsigned int nrows,
                             unsigned int ncols, unsigned int row0,
                             void* stream);
int st_generate_identity_f64(double* d_mat, unsigned int nrows,
                             unsigned int ncols, unsigned int row0,
                             void* stream);
int st_fill_f32(float* d_x, uint64_t count, float value, void* stream);
int st_fill_f64(double* d_x, uint64_t count, double value, void* stream);

/* s[r] = sum_c A[r][c] for the nrows local rows (similarity_transform.cpp
 * :77-152, deterministic tree order, no atomics). */
int st_rowsum_f32(const float* d_mat, float* d_s, unsigned int nrows,
                  unsigned int ncols, void* stream);
int st_rowsum_f64(const double* d_mat, double* d_s, unsigned int nrows,
                  unsigned int ncols, void* stream);
/* The same row sums in the flat form, for blocks where st_round_flat_pays
 * (what the solve loops run as their initial pass there): one short
 * workgroup per (rows, column piece) writes partial sums into d_part
 * (st_round_flat_scratch(nrows, ncols) elements), a second launch sums each
 * row's pieces in a fixed order.  Deterministic and independent of the row
 * partition among blocks of one cache class, like st_round_flat's sums. */
int st_rowsum_flat_f32(const float* d_mat, float* d_s, float* d_part,
                       unsigned int nrows, unsigned int ncols, void* stream);
int st_rowsum_flat_f64(const double* d_mat, double* d_s, double* d_part,
                       unsigned int nrows, unsigned int ncols, void* stream);

/* Fused round body: for the local rows r in [0,nrows) (global row0 + r),
 *   A[r][c] = A[r][c] * ((1/s_cur[row0+r]) * s_cur[c])     (ST_SEM_SYCL)
 *   A[r][c] = ((1/s_cur[row0+r]) * A[r][c]) * s_cur[c]     (ST_SEM_MAINPY)
 * in place (similarity_transform.cpp:286-330 / main.py:13-16), and
 * s_next[r] = sum_c of the stored A[r][c] (the next round's row sums,
 * similarity_transform.cpp:40).  s_next may be NULL (transform only).
 * d_state may be NULL; otherwise the launch is a no-op once done != 0. */
int st_scale_rowsum_f32(float* d_mat, const float* d_s_cur, float* d_s_next,
                        unsigned int nrows, unsigned int ncols,
                        unsigned int row0, unsigned int semantics,
                        const st_state* d_state, void* stream);
int st_scale_rowsum_f64(double* d_mat, const double* d_s_cur,
                        double* d_s_next, unsigned int nrows,
                        unsigned int ncols, unsigned int row0,
                        unsigned int semantics, const st_state* d_state,
                        void* stream);

/* One whole round k in ONE launch (what the solve loop runs): from the full
 * row-sum vector s_cur = s_k (length ncols), for the local rows
 * r in [0,nrows) (global row0 + r):
 *   m_k = max(0, max s_k), v[row0+r] *= s_k[row0+r]/m_k, stop_k = all
 *   |s_k[i]-s_k[i+1]| < eps (cyclic for ST_SEM_SYCL), lambda = s_k[0],
 *   A <- D_k^-1 A D_k in place and s_next[r] = row sums of the stored A.
 * d_v is the FULL eigenvector accumulator (only the local rows are
 * written).  k is the round index (0-based); d_state->end = k+1 once the
 * round stops or k+1 == max_itr, and launches for later rounds are no-ops.
 * d_state must be zeroed (st_state_reset) before round 0. */
int st_round_f32(float* d_mat, const float* d_s_cur, float* d_s_next,
                 float* d_v, unsigned int nrows, unsigned int ncols,
                 unsigned int row0, float eps, unsigned int k,
                 unsigned int max_itr, unsigned int semantics,
                 st_state* d_state, void* stream);
int st_round_f64(double* d_mat, const double* d_s_cur, double* d_s_next,
                 double* d_v, unsigned int nrows, unsigned int ncols,
                 unsigned int row0, double eps, unsigned int k,
                 unsigned int max_itr, unsigned int semantics,
                 st_state* d_state, void* stream);

/* The same round for large blocks as two launches (k_flat, k_parts in
 * st_device.h): one short workgroup per (2 rows, 256 x 16-byte column
 * piece) for the in-place transform (the HBM serves many short workgroups
 * sweeping a compact address window faster than one long stream per CU),
 * whose first row group also derives m_k / stop_k / lambda / state from the
 * full s_k; then the pieces' partial sums into s_next in a fixed order and
 * the eigenvector update.
 * Results as st_round_* except the row sums' summation order (deterministic
 * and independent of the row partition among blocks of one cache class:
 * pieces are 8 KB of a row for fp64 blocks below 2 GiB, else 4 KB).
 * d_part: scratch of
 * st_round_flat_scratch(nrows, ncols) elements.  st_round_flat_pays tells
 * whether this form is the faster one for a block (dtype 0 = f32, 1 = f64);
 * the library's own solve loops use it for such blocks. */
int st_round_flat_f32(float* d_mat, const float* d_s_cur, float* d_s_next,
                      float* d_part, float* d_v, unsigned int nrows,
                      unsigned int ncols, unsigned int row0, float eps,
                      unsigned int k, unsigned int max_itr,
                      unsigned int semantics, st_state* d_state, void* stream);
int st_round_flat_f64(double* d_mat, const double* d_s_cur, double* d_s_next,
                      double* d_part, double* d_v, unsigned int nrows,
                      unsigned int ncols, unsigned int row0, double eps,
                      unsigned int k, unsigned int max_itr,
                      unsigned int semantics, st_state* d_state, void* stream);
uint64_t st_round_flat_scratch(unsigned int nrows, unsigned int ncols);
int st_round_flat_pays(unsigned int nrows, unsigned int ncols, int dtype);
/* The launch policy, as one map: what the solve loops launch for an
 * nrows x ncols block of `dtype` (0 fp32, 1 fp64; vector path, ncols a
 * multiple of 16 / sizeof element) in `form`, with `npend` pending rounds for
 * the deferred forms - read from the same shape functions and tables the
 * launchers use (st_kernels.hip), so tests/golden/launch_policy.json pins
 * every launch shape and cache policy.  Returns 0 or negative. */
#define ST_FORM_ROUND 0       /* a round that stores A (bench step; the
                                 solve's round below 144 MiB)                 */
#define ST_FORM_DEFER_READ 1  /* deferred writes: a read-only round          */
#define ST_FORM_DEFER_STORE 2 /* deferred writes: the storing round          */
#define ST_FORM_MFREE 3       /* the matrix-free round                        */
#define ST_FORM_ROWSUM 4      /* K0, the initial row-sum pass                 */
#define ST_KERNEL_ROUND 0     /* k_round: grid-stride row groups              */
#define ST_KERNEL_FLAT 1      /* k_flat + k_parts, storing every round        */
#define ST_KERNEL_FLAT_DEFERRED 2 /* k_flat<NP> + k_parts                     */
#define ST_KERNEL_MFREE 3     /* k_mfree                                      */
#define ST_KERNEL_FUSED 4     /* k_fused: grid-stride row groups, sums only    */
#define ST_KERNEL_FLAT_SUM 5  /* k_flat_sum + k_parts                         */
typedef struct st_launch_policy
{
  int kernel;               /* ST_KERNEL_*                                    */
  int rows;                 /* rows per workgroup (flat) or per row group     */
  unsigned int tile;        /* flat: row groups per piece tile, 0 = row-major */
  unsigned int cap;         /* workgroups per CU (dynamic LDS), 0 = uncapped  */
  unsigned int grid;        /* grid-stride kernels: workgroup count cap       */
  unsigned int piece_bytes; /* flat: bytes of a row per workgroup piece       */
  int load_nt;              /* matrix loads non-temporal                      */
  int store_nt;             /* matrix stores non-temporal, -1 = no stores     */
  int alt;                  /* odd rounds walk the block in reverse           */
} st_launch_policy;
int st_launch_policy_query(int dtype, unsigned int nrows, unsigned int ncols,
                           int form, unsigned int npend, st_launch_policy* out);

/* Round k of the flat round with deferred writes (what the solve loops run
 * for blocks where st_round_flat_pays): the matrix in d_mat is the last
 * STORED one, A_j; d_pend_s / d_pend_inv list the npend = k - j pending
 * rounds' gathered row sums s_j .. s_{k-1} and their reciprocals (oldest
 * first), which are re-applied in registers before round k's own update;
 * A_{k+1} is stored when `store`.  Every value (s_{k+1}, v, the state) is
 * bit-identical to st_round_flat on a matrix stored every round.  d_inv_cur
 * = 1 / d_s_cur; d_inv_next receives 1 / s_{k+1} for the block's rows (pass
 * the rank's slot, like d_s_next).  flush = 1 (with store = 1) only stores
 * A_{k+1} - no row sums, no v update - to leave the matrix as storing every
 * round would after the last round k.  npend < m = st_defer_rounds(nrows,
 * ncols, dtype), the rounds per store, and a round with npend = m - 1 (the
 * group's last) must store: other calls return -1.  d_pend_s / d_pend_inv
 * are HOST arrays of device pointers. */
int st_round_flat_deferred_f32(float* d_mat, const float* d_s_cur,
                               const float* d_inv_cur, float* d_s_next,
                               float* d_inv_next, float* d_part, float* d_v,
                               unsigned int nrows, unsigned int ncols,
                               unsigned int row0, float eps, unsigned int k,
                               unsigned int max_itr, unsigned int semantics,
                               const float* const* d_pend_s,
                               const float* const* d_pend_inv,
                               unsigned int npend, int store, int flush,
                               st_state* d_state, void* stream);
int st_round_flat_deferred_f64(double* d_mat, const double* d_s_cur,
                               const double* d_inv_cur, double* d_s_next,
                               double* d_inv_next, double* d_part,
                               double* d_v, unsigned int nrows,
                               unsigned int ncols, unsigned int row0,
                               double eps, unsigned int k,
                               unsigned int max_itr, unsigned int semantics,
                               const double* const* d_pend_s,
                               const double* const* d_pend_inv,
                               unsigned int npend, int store, int flush,
                               st_state* d_state, void* stream);
/* d_inv[i] = 1 / d_s[i], i < n (the reciprocals of s_0) */
int st_recip_f32(const float* d_s, float* d_inv, unsigned int n, void* stream);
int st_recip_f64(const double* d_s, double* d_inv, unsigned int n,
                 void* stream);
/* rounds per store of the deferred flat round on a block (dtype 0 = f32,
 * 1 = f64): 6 on every block (the arguments are kept for future shapes) */
unsigned int st_defer_rounds(unsigned int nrows, unsigned int ncols,
                             int dtype);

/* Round k split in two launches for a sharded solve that overlaps the
 * all-gather of s_k with compute (eigen_value_amd/sharded.py, overlap).
 * [col0, col1) are the columns whose s_k values this rank computed itself
 * (normally [row0, row0 + nrows)); d_part holds nrows partial row sums.
 *   span = 1 (local; d_s_cur needs only the own slot): for those columns
 *     A[r][c] <- A[r][c] * ((1/s_k[row0+r]) * s_k[c]), d_part[r] = their
 *     sum.  No m / stop / v / state work.
 *   span = 2 (remote; d_s_cur = the full gathered s_k): exactly st_round's
 *     m_k, stop_k, v update, lambda and state, plus the other columns, and
 *     d_s_next[r] = d_part[r] + (their row sum).
 * A_{k+1}, v, m and stop are bit-identical to st_round; s_{k+1} sums the
 * two column sets separately (bit-identical to st_round when the local
 * range is all columns).  Both launches are no-ops once a previous round
 * stopped. */
int st_round_split_f32(float* d_mat, const float* d_s_cur, float* d_s_next,
                       float* d_part, float* d_v, unsigned int nrows,
                       unsigned int ncols, unsigned int row0,
                       unsigned int col0, unsigned int col1, float eps,
                       unsigned int k, unsigned int max_itr,
                       unsigned int semantics, int span, st_state* d_state,
                       void* stream);
int st_round_split_f64(double* d_mat, const double* d_s_cur,
                       double* d_s_next, double* d_part, double* d_v,
                       unsigned int nrows, unsigned int ncols,
                       unsigned int row0, unsigned int col0,
                       unsigned int col1, double eps, unsigned int k,
                       unsigned int max_itr, unsigned int semantics, int span,
                       st_state* d_state, void* stream);

/* The same two halves in the flat form (st_round_flat), for blocks where
 * st_round_flat_pays: span 1 runs k_flat over the 4 KB column pieces that
 * hold [col0, col1), span 2 over all pieces with the other columns (plus
 * the m / stop / lambda / state work of k_flat's first row group), then
 * sums remote-then-local partials into d_s_next and updates v.  d_part:
 * scratch of st_round_split_flat_scratch(nrows, ncols, col0, col1)
 * elements, shared by the two halves of a round.  A_{k+1}, v, m and stop
 * are bit-identical to st_round_flat; s_{k+1} differs from it only in the
 * summation order. */
int st_round_split_flat_f32(float* d_mat, const float* d_s_cur,
                            float* d_s_next, float* d_part, float* d_v,
                            unsigned int nrows, unsigned int ncols,
                            unsigned int row0, unsigned int col0,
                            unsigned int col1, float eps, unsigned int k,
                            unsigned int max_itr, unsigned int semantics,
                            int span, st_state* d_state, void* stream);
int st_round_split_flat_f64(double* d_mat, const double* d_s_cur,
                            double* d_s_next, double* d_part, double* d_v,
                            unsigned int nrows, unsigned int ncols,
                            unsigned int row0, unsigned int col0,
                            unsigned int col1, double eps, unsigned int k,
                            unsigned int max_itr, unsigned int semantics,
                            int span, st_state* d_state, void* stream);
uint64_t st_round_split_flat_scratch(unsigned int nrows, unsigned int ncols,
                                     unsigned int col0, unsigned int col1);

/* Matrix-free round.  The transformed matrix of
 * round k is X^-1 A_0 X with x ∝ the product of all previous row-sum
 * vectors, so its row sums are (A_0 x) ⊘ x and A_0 never has to be
 * rewritten: N^2*b bytes per round instead of 2*N^2*b.  Launch k >= 1
 * (launch 0 is st_rowsum on A_0, giving s_0; v_prev = 1 for launch 1):
 *   from the FULL s_prev = s_{k-1}: m, stop, lambda of round k-1 (recorded
 *   in d_state, end = k when round k-1 stops or k == max_itr);
 *   d_v_cur[0..ncols) = d_v_prev * (s_prev / m)   (v_{k-1}, full vector);
 *   d_s_next[r] = (Σ_c A_0[r][c] x[c]) / x[row0+r], x = v_prev ∘ s_prev,
 *   for the local rows (s_k).
 * d_mat0 is read only.  v_prev/v_cur and s_prev/s_next are ping-pong
 * buffers.  Launches after the stopping one are no-ops. */
int st_mfree_round_f32(const float* d_mat0, const float* d_s_prev,
                       float* d_s_next, const float* d_v_prev, float* d_v_cur,
                       unsigned int nrows, unsigned int ncols,
                       unsigned int row0, float eps, unsigned int k,
                       unsigned int max_itr, unsigned int semantics,
                       st_state* d_state, void* stream);
int st_mfree_round_f64(const double* d_mat0, const double* d_s_prev,
                       double* d_s_next, const double* d_v_prev,
                       double* d_v_cur, unsigned int nrows, unsigned int ncols,
                       unsigned int row0, double eps, unsigned int k,
                       unsigned int max_itr, unsigned int semantics,
                       st_state* d_state, void* stream);
/* The same matrix-free launch k in the flat form (the solve loops' choice
 * for blocks where st_round_flat_pays): one short workgroup per (rows, 4 or
 * 8 KB column piece) writes partial dot products into d_part
 * (st_round_flat_scratch(nrows, ncols) elements), a second launch sums them
 * per row and writes v_{k-1}.  Results equal st_mfree_round_* up to the
 * association of the row sums (pieces summed apart; deterministic and
 * independent of the row partition). */
int st_mfree_round_flat_f32(const float* d_mat0, const float* d_s_prev,
                            float* d_s_next, const float* d_v_prev,
                            float* d_v_cur, float* d_part, unsigned int nrows,
                            unsigned int ncols, unsigned int row0, float eps,
                            unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_state,
                            void* stream);
int st_mfree_round_flat_f64(const double* d_mat0, const double* d_s_prev,
                            double* d_s_next, const double* d_v_prev,
                            double* d_v_cur, double* d_part, unsigned int nrows,
                            unsigned int ncols, unsigned int row0, double eps,
                            unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_state,
                            void* stream);

/* The matrix-free scheme on a matrix stored in 16 bits (storage =
 * ST_STORE_F16 / ST_STORE_BF16; what st_solve_device_half runs).  d_mat /
 * d_mat0: nrows x ncols row-major 16-bit elements, read only, any ncols >= 1;
 * all vectors fp32.
 *   st_rowsum_half       d_s[r] = Σ_c A[r][c] (launch 0: s_0)
 *   st_mfree_round_half  launch k >= 1, the contract of st_mfree_round_f32
 *     (row0 + nrows <= ncols).  d_v_cur and the whole st_state are bit for
 *     bit what st_mfree_round_f32 writes for the widened matrix and the same
 *     arguments; d_s_next sums each row in this kernel's own fixed order: a
 *     lane takes 8 consecutive columns per 16-byte load (lane t the columns
 *     8 (t + 256 j) ..+7, j = 0, 1, ...), one fp32 fused multiply-add per
 *     element in column order, then the 64 lanes' tree and the 4 waves'
 *     partials in wave order.  16-byte loads when ncols % 8 == 0 and d_mat0,
 *     d_s_prev and d_v_prev are 16-byte aligned; otherwise the same lanes
 *     load element-wide (same bits).  Deterministic, no atomics.
 * st_narrow_f32: d_out[i] = d_in[i] rounded to nearest even in `storage`
 * (device pointers, count elements): makes a 16-bit matrix from an fp32 one
 * (e.g. the st_generate_*_f32 inputs). */
int st_rowsum_half(int storage, const void* d_mat, float* d_s,
                   unsigned int nrows, unsigned int ncols, void* stream);
int st_mfree_round_half(int storage, const void* d_mat0, const float* d_s_prev,
                        float* d_s_next, const float* d_v_prev, float* d_v_cur,
                        unsigned int nrows, unsigned int ncols,
                        unsigned int row0, float eps, unsigned int k,
                        unsigned int max_itr, unsigned int semantics,
                        st_state* d_state, void* stream);
int st_narrow_f32(int storage, const float* d_in, void* d_out, uint64_t count,
                  void* stream);
/* The launch shape the 16-bit kernels were built with ("rows=8 xvec=0
 * unroll=2 unroll_mid=1 grid=512 nt_mib=512": rows per group where k_mfree
 * takes 4, x formed in the sweep, 16-byte chunks in flight per lane and row -
 * and in the cached 2-row shape -, the workgroup cap, non-temporal loads from
 * 512 MiB of N^2 * 2 bytes); tools record it next to their numbers.  On
 * MI355X (tools/bench_half.py, profiles/half_mfree.json, one interleaved
 * run): 0.0919 / 0.3365 ms per fp16 round at 16384^2 / 32768^2, 5844 / 6382
 * GB/s, against 0.161 / 0.627 ms for st_mfree_round_f32 on the widened
 * matrix.  No GPU needed. */
const char* st_half_shape_desc(void);

/* The dense left-vector scheme, step by step (section 3i; what
 * st_solve_device_left_* runs).  d_mat / d_mat0: n x n row-major, read only;
 * all vectors device [n]; d_scratch: st_left_scratch(dtype, n) elements,
 * 256-byte aligned, distinct from the four vectors.
 *   st_colsum_*           d_s[c] = sum_r A[r][c] in st_left_shape's order
 *     (launch 0: s_0); only the partials' part of d_scratch is used
 *   st_mfree_left_round_* launch k >= 1, the contract of st_mfree_round_* in
 *     three launches: k_csr_prep writes x = v_prev * s_prev to the start of
 *     d_scratch and folds max and the stop test of s_prev through d_state,
 *     its last workgroup publishing round k-1; k_left_sweep writes the column
 *     products of every row block behind x; k_left_finish adds them and
 *     writes s_next[c] = t / x[c] and v_cur[c] = v_prev[c] * (s_prev[c] / m).
 *     d_v_cur and every field of st_state are bit for bit what
 *     st_mfree_round_* writes for the transposed matrix and the same
 *     arguments.  All three are no-ops once d_state->end says an earlier
 *     round stopped.
 * 16-byte loads when n * sizeof(element) is a multiple of 16 and d_mat and
 * d_scratch are 16-byte aligned; otherwise element-wide (same bits).
 * Nothing outside the n * n elements of the matrix is read. */
int st_colsum_f32(const float* d_mat, float* d_s, float* d_scratch, unsigned int n,
                  void* stream);
int st_colsum_f64(const double* d_mat, double* d_s, double* d_scratch,
                  unsigned int n, void* stream);
int st_mfree_left_round_f32(const float* d_mat0, const float* d_s_prev,
                            float* d_s_next, const float* d_v_prev, float* d_v_cur,
                            float* d_scratch, unsigned int n, float eps,
                            unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_state,
                            void* stream);
int st_mfree_left_round_f64(const double* d_mat0, const double* d_s_prev,
                            double* d_s_next, const double* d_v_prev,
                            double* d_v_cur, double* d_scratch, unsigned int n,
                            double eps, unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_state,
                            void* stream);

/* The dense pair scheme, step by step (section 3j; what
 * st_solve_device_pair_* runs).  d_mat / d_mat0: n x n row-major, read only;
 * all vectors device [n]; d_scratch: st_pair_scratch(dtype, n) elements,
 * 256-byte aligned, distinct from the vectors.
 *   st_pair_sum_*         d_s_right[r] = sum_c A[r][c] and d_s_left[c] =
 *     sum_r A[r][c] from ONE pass over the matrix, in st_pair_shape's orders
 *     (launch 0: both s_0); only the partials' parts of d_scratch are used
 *   st_mfree_pair_round_* launch k >= 1 of both sides, five launches:
 *     k_csr_prep once per side (x_R / x_L to the start of d_scratch, max and
 *     the stop test of that side's s_prev through its state, d_states[0] the
 *     right side's, d_states[1] the left one's); k_pair_sweep reads the matrix
 *     once and writes the column products of every row block and the row
 *     products of every strip; k_left_finish once per side adds them and writes
 *     s_next = t / x and v_cur = v_prev * (s_prev / m).  The left side's
 *     s_next, v_cur and state are bit for bit st_mfree_left_round_*'s; the
 *     right side's v_cur and state are bit for bit st_mfree_round_*'s for the
 *     same arguments.  A side whose state says an earlier round stopped gets
 *     no write anywhere (its s_next, v_cur and partials stay as they are) and,
 *     once both have, the matrix is not read.
 * 16-byte loads when n * sizeof(element) is a multiple of 16 and d_mat and
 * d_scratch are 16-byte aligned; otherwise element-wide (same bits).
 * Nothing outside the n * n elements of the matrix is read. */
int st_pair_sum_f32(const float* d_mat, float* d_s_right, float* d_s_left,
                    float* d_scratch, unsigned int n, void* stream);
int st_pair_sum_f64(const double* d_mat, double* d_s_right, double* d_s_left,
                    double* d_scratch, unsigned int n, void* stream);
int st_mfree_pair_round_f32(const float* d_mat0, const float* d_s_prev_right,
                            float* d_s_next_right, const float* d_v_prev_right,
                            float* d_v_cur_right, const float* d_s_prev_left,
                            float* d_s_next_left, const float* d_v_prev_left,
                            float* d_v_cur_left, float* d_scratch, unsigned int n,
                            float eps, unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_states /* [2] */,
                            void* stream);
int st_mfree_pair_round_f64(const double* d_mat0, const double* d_s_prev_right,
                            double* d_s_next_right, const double* d_v_prev_right,
                            double* d_v_cur_right, const double* d_s_prev_left,
                            double* d_s_next_left, const double* d_v_prev_left,
                            double* d_v_cur_left, double* d_scratch, unsigned int n,
                            double eps, unsigned int k, unsigned int max_itr,
                            unsigned int semantics, st_state* d_states /* [2] */,
                            void* stream);

/* The sparse (CSR) scheme, step by step (what st_solve_csr runs); `csr` is a
 * st_csr_create handle, all vectors device [n] in the handle's dtype.
 *   st_csr_rowsum       d_s[r] = the sum of row r's entries (launch 0: s_0)
 *   st_csr_mfree_round  launch k >= 1, the contract of st_mfree_round_f32 /
 *     _f64 in two launches: k_csr_prep writes x = v_prev * s_prev to d_x
 *     (scratch of n elements, distinct from the four vectors) and folds max
 *     and the stop test of s_prev through d_state's scratch words (left
 *     zero), the last workgroup publishing round k-1; k_csr_spmv writes
 *     s_next[r] = (sum of a * x[col]) / x[r] and v_cur[r] = v_prev[r] *
 *     (s_prev[r] / m).  d_v_cur and every field of st_state are bit for bit
 *     what st_mfree_round_* writes for the densified matrix and the same
 *     arguments.  Both launches are no-ops once d_state->end says an earlier
 *     round stopped.  eps is a double for both dtypes (rounded to float for
 *     an fp32 handle). */
int st_csr_rowsum(void* csr, void* d_s, void* stream);
int st_csr_mfree_round(void* csr, const void* d_s_prev, void* d_s_next,
                       const void* d_v_prev, void* d_v_cur, void* d_x,
                       double eps, unsigned int k, unsigned int max_itr,
                       unsigned int semantics, st_state* d_state, void* stream);
/* The same two steps on A + sum_j u_j w_j^T (section 3e; what
 * st_solve_csr_terms runs): `terms` a st_csr_terms_create object of `csr`,
 * d_scratch st_csr_terms_scratch_bytes(n, K) bytes, 256-byte aligned.  After
 * either call dots[K] (w_j . 1 after the row sum, w_j . x after a round), in
 * the handle's dtype, stands at the start of d_scratch, and x behind the
 * partials.  st_csr_rowsum works on an empty-rows handle (such a row sums to
 * 0); st_csr_mfree_round refuses one. */
int st_csr_terms_rowsum(void* csr, void* terms, void* d_s, void* d_scratch,
                        void* stream);
int st_csr_terms_round(void* csr, void* terms, const void* d_s_prev,
                       void* d_s_next, const void* d_v_prev, void* d_v_cur,
                       void* d_scratch, double eps, unsigned int k,
                       unsigned int max_itr, unsigned int semantics,
                       st_state* d_state, void* stream);
/* The two steps on the product B A (section 3g; what st_solve_csr_product
 * runs): d_scratch st_csr_product_scratch_bytes(n) bytes, 256-byte aligned.
 * After the row sum y (the row sums of A) stands in the scratch's second
 * half; after a round x in its first half and y = A x in its second.  s_0 is
 * not checked here: st_solve_csr_product does that. */
int st_csr_product_rowsum(void* csr_b, void* csr_a, void* d_s, void* d_scratch,
                          void* stream);
int st_csr_product_round(void* csr_b, void* csr_a, const void* d_s_prev,
                         void* d_s_next, const void* d_v_prev, void* d_v_cur,
                         void* d_scratch, double eps, unsigned int k,
                         unsigned int max_itr, unsigned int semantics,
                         st_state* d_state, void* stream);
/* The two steps on the pattern operator diag(r) P diag(c) (section 3h; what
 * st_solve_csr_pattern runs): `pat` a st_csr_pattern_create handle, `terms` a
 * st_csr_pattern_terms_create object of it or NULL, d_scratch
 * st_csr_pattern_scratch_bytes(n, K) bytes (K = 0 without terms), 256-byte
 * aligned.  After a round z = c * x stands behind the partials (x itself
 * where c is NULL) and, with terms, dots[K] at the start.  The row sum works
 * on an empty-rows handle; the round without terms refuses one. */
int st_csr_pattern_rowsum(void* pat, void* terms, void* d_s, void* d_scratch,
                          void* stream);
int st_csr_pattern_round(void* pat, void* terms, const void* d_s_prev,
                         void* d_s_next, const void* d_v_prev, void* d_v_cur,
                         void* d_scratch, double eps, unsigned int k,
                         unsigned int max_itr, unsigned int semantics,
                         st_state* d_state, void* stream);
/* The same for the C operators of a st_csr_multi_create object (section 3f;
 * what st_solve_csr_multi runs).  All vectors are PACKED device arrays
 * [n][CP], aligned to a row of CP * b bytes; d_scratch
 * st_csr_multi_scratch_bytes(n, C, K) bytes, 256-byte aligned; d_states device
 * [C] (zero = fresh), d_finished one device word.  Column c of s_next, v_cur,
 * x and dots[c][.] and d_states[c] are bit for bit st_csr_terms_rowsum's /
 * st_csr_terms_round's on that column's terms alone.  A column whose state
 * has `end` set and below k gets no write at all, nor does a padding column
 * (C <= c < CP); the publisher of a round that sets a column's `end` adds 1
 * to *d_finished. */
int st_csr_multi_rowsum(void* csr, void* multi, void* d_s, void* d_scratch,
                        void* stream);
int st_csr_multi_round(void* csr, void* multi, const void* d_s_prev,
                       void* d_s_next, const void* d_v_prev, void* d_v_cur,
                       void* d_scratch, double eps, unsigned int k,
                       unsigned int max_itr, unsigned int semantics,
                       st_state* d_states, uint32_t* d_finished, void* stream);

/* The batched sparse scheme, step by step (what st_solve_csr_batched runs);
 * `h` is a st_csr_batch_create handle, all vectors device [N] stacked,
 * d_states device [batch] (zero = fresh), d_finished one device word.
 *   st_csr_batch_rowsum       K0 over the stacked rows
 *   st_csr_batch_mfree_round  launch k >= 1 for the whole batch in two
 *     launches.  k_csrb_prep: every workgroup works for exactly one matrix
 *     (one per 256 of its rows, at most 2048), writes x = v_prev * s_prev for
 *     its share and folds max and the stop test of the matrix's OWN s_prev
 *     through d_states[b]; the last row's cyclic pair wraps to the matrix's
 *     first row; the participant that publishes a round that sets `end` adds
 *     1 to *d_finished.  k_csrb_spmv: st_csr_mfree_round's row products over
 *     the batch's plan, gate and m from the row's own matrix's state, x
 *     indexed from the matrix's first row.  Each matrix's slices of s_next,
 *     v_cur and its state are bit for bit st_csr_mfree_round's on that
 *     matrix alone; a matrix whose end is set and below k gets no writes. */
int st_csr_batch_rowsum(void* h, void* d_s, void* stream);
int st_csr_batch_mfree_round(void* h, const void* d_s_prev, void* d_s_next,
                             const void* d_v_prev, void* d_v_cur, void* d_x,
                             double eps, unsigned int k, unsigned int max_itr,
                             unsigned int semantics, st_state* d_states,
                             uint32_t* d_finished, void* stream);

/* Round epilogue on the full row-sum vector s[0..n): m = max(0, max s)
 * (find_max, similarity_transform.cpp:154-227), v[i] *= s[i]/m
 * (compute_eigen_vector, :229-265), stop = all |s[i]-s[i+1]| < eps over
 * the cyclic (ST_SEM_SYCL, :332-460) or open (ST_SEM_MAINPY) pairs,
 * lambda = s[0]; then done/round/iters bookkeeping against max_itr.
 * No-op once done != 0.  d_v may be NULL (no eigenvector update). */
int st_epilogue_f32(const float* d_s, float* d_v, unsigned int n, float eps,
                    unsigned int max_itr, unsigned int semantics,
                    st_state* d_state, void* stream);
int st_epilogue_f64(const double* d_s, double* d_v, unsigned int n,
                    double eps, unsigned int max_itr, unsigned int semantics,
                    st_state* d_state, void* stream);

/* Library / device facts.  st_version names the library, the target, the
 * A/B probe switches its kernels were built with ("defaults" in every
 * library build; st_probe_switches returns that part alone) and the RCCL
 * its calls are bound to (st_rccl_version). */
const char* st_version(void);
const char* st_probe_switches(void);
int st_device_count(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
/* C++ entry mirroring include/similarity_transform.hpp:46-53
 * (int64_t similarity_transform(sycl::queue&, const float* mat, float*
 * eigen_val, float* eigen_vec, uint dim, uint wg_size, uint* iter_count)).
 * The queue becomes the opaque context; wg_size is accepted and ignored
 * (tiles are chosen by the kernels). */
inline int64_t
similarity_transform(void* q, const float* mat, float* const eigen_val,
                     float* const eigen_vec, const unsigned int dim,
                     const unsigned int /*wg_size*/,
                     unsigned int* const iter_count)
{
  return max_eigen_value_ex(q, 0, mat, eigen_val, eigen_vec, dim, iter_count,
                            nullptr, nullptr);
}
inline int64_t
similarity_transform(void* q, const double* mat, double* const eigen_val,
                     double* const eigen_vec, const unsigned int dim,
                     const unsigned int /*wg_size*/,
                     unsigned int* const iter_count)
{
  return max_eigen_value_ex(q, 1, mat, eigen_val, eigen_vec, dim, iter_count,
                            nullptr, nullptr);
}
#endif

#endif /* EIGEN_VALUE_AMD_SIMILARITY_TRANSFORM_H */
