"""ctypes binding of ``libsimilarity_transform.so`` (include/similarity_transform.h).

The library is built in-tree by ``make`` / ``__graft_entry__.build()`` into
``eigen_value_amd/lib/``.  There is no fallback: if the shared object is
missing, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
DEFAULT_LIB = os.path.join(PKG_DIR, "lib", "libsimilarity_transform.so")
# the tuning build: the same kernels plus the launch-table setters of
# include/st_tuning.h (tools and the knob tests only)
TUNING_LIB = os.path.join(PKG_DIR, "lib", "libsimilarity_transform_tuning.so")
HEADER = os.path.join(REPO_DIR, "include", "similarity_transform.h")
TUNING_HEADER = os.path.join(REPO_DIR, "include", "st_tuning.h")

ST_SEM_SYCL = 0
ST_SEM_MAINPY = 1
ST_FLAG_TIME_KERNELS = 1
ST_FLAG_MATRIX_FREE = 2
ST_FLAG_ROUND_LOOP = 4
ST_FLAG_WRITE_EVERY_ROUND = 8
ST_FLAG_TRACE_SUMS = 16
ST_FLAG_BATCH_ROUNDS = 32
ST_MAX_ITR = 1000

DTYPE_F32 = 0
DTYPE_F64 = 1
# storage codes of the half-precision entry points (*_half, st_narrow_f32)
ST_STORE_F16 = 2
ST_STORE_BF16 = 3


class EigenValueError(RuntimeError):
    """A call into libsimilarity_transform.so reported an error."""


class st_options(ctypes.Structure):
    _fields_ = [("eps", ctypes.c_double),
                ("max_itr", ctypes.c_uint32),
                ("semantics", ctypes.c_uint32),
                ("batch", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class st_stats(ctypes.Structure):
    _fields_ = [("h2d_ms", ctypes.c_double),
                ("loop_ms", ctypes.c_double),
                ("d2h_ms", ctypes.c_double),
                ("fused_ms_total", ctypes.c_double),
                ("rowsum_ms", ctypes.c_double),
                ("fused_launches", ctypes.c_uint32),
                ("rounds", ctypes.c_uint32),
                ("converged", ctypes.c_uint32),
                ("transpose_us", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class st_launch_policy(ctypes.Structure):
    """include/similarity_transform.h st_launch_policy."""
    _fields_ = [("kernel", ctypes.c_int), ("rows", ctypes.c_int), ("tile", ctypes.c_uint),
                ("cap", ctypes.c_uint), ("grid", ctypes.c_uint), ("piece_bytes", ctypes.c_uint),
                ("load_nt", ctypes.c_int), ("store_nt", ctypes.c_int), ("alt", ctypes.c_int)]


ST_FORM_ROUND, ST_FORM_DEFER_READ, ST_FORM_DEFER_STORE, ST_FORM_MFREE = 0, 1, 2, 3
ST_FORM_ROWSUM = 4
KERNEL_NAMES = {0: "k_round", 1: "k_flat", 2: "k_flat<NP>", 3: "k_mfree", 4: "k_fused",
                5: "k_flat_sum"}


def launch_policy(dtype: str, nrows: int, ncols: int, form: int, npend: int = 0) -> dict:
    """What the solve loops launch for an nrows x ncols block
    (st_launch_policy_query): kernel, rows per workgroup / group, piece
    tile, workgroups-per-CU cap, grid cap, piece bytes, cache policy."""
    L = load()
    out = st_launch_policy()
    check(L.st_launch_policy_query(1 if dtype == "f64" else 0, nrows, ncols, form, npend,
                                   ctypes.byref(out)), "st_launch_policy_query")
    d = {f: getattr(out, f) for f, _ in st_launch_policy._fields_}
    d["kernel"] = KERNEL_NAMES[d["kernel"]]
    return d


class st_state(ctypes.Structure):
    _fields_ = [("done", ctypes.c_uint32),
                ("round", ctypes.c_uint32),
                ("iters", ctypes.c_uint32),
                ("stop", ctypes.c_uint32),
                ("lambda_", ctypes.c_double),
                ("max", ctypes.c_double),
                ("end", ctypes.c_uint32),
                ("arrivals", ctypes.c_uint32),
                ("max_bits", ctypes.c_uint64),
                ("fail", ctypes.c_uint32),
                ("pad0", ctypes.c_uint32),
                ("pad", ctypes.c_uint64 * 1)]


assert ctypes.sizeof(st_state) == 64
assert ctypes.sizeof(st_options) == 24
assert ctypes.sizeof(st_stats) == 56

_lib: Optional[ctypes.CDLL] = None
_by_path: dict = {}   # every library loaded, by real path (one CDLL each)


def lib_path() -> str:
    return os.environ.get("EIGEN_VALUE_LIB") or DEFAULT_LIB


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """Load (once) and declare the C-ABI.  Raises if the .so is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or lib_path()
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"libsimilarity_transform.so not found at {p!r}: run `make` or "
            "`python -c 'import __graft_entry__ as g; g.build()'` first "
            "(there is no CPU fallback)")
    key = os.path.realpath(p)
    L = _by_path.get(key)
    if L is None:
        L = ctypes.CDLL(p)
        _declare(L)
        if hasattr(L, "st_set_defer_caps"):     # the tuning build
            declare_tuning(L)
        _by_path[key] = L
    if path is None:
        _lib = L
    return L


def load_tuning() -> ctypes.CDLL:
    """The tuning build (libsimilarity_transform_tuning.so), declared with
    the main ABI and the setters of include/st_tuning.h.  A separate library
    with its own launch tables: a knob set here moves only the launches made
    through it (run a knob study with EIGEN_VALUE_LIB pointing at it, so
    that the package's default library is this one)."""
    L = load(TUNING_LIB)
    declare_tuning(L)
    return L


def declare_tuning(L: ctypes.CDLL) -> None:
    """argtypes of the st_tuning.h setters (raises AttributeError on the
    product library, which exports none)."""
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    L.st_set_flat_grid_limit.argtypes = [u32]
    L.st_set_flat_grid_limit.restype = u32
    L.st_set_defer_caps.argtypes = [i32, i32, u32, u32]
    L.st_set_defer_caps.restype = i32
    L.st_set_defer_ntload.argtypes = [u32, u32]
    L.st_set_defer_ntload.restype = i32
    L.st_defer_ntload_class.argtypes = [u32, u32, i32]
    L.st_defer_ntload_class.restype = i32
    L.st_set_every_cache.argtypes = [u32, u32]
    L.st_set_every_cache.restype = i32
    L.st_every_cache_class.argtypes = [u32, u32, i32]
    L.st_every_cache_class.restype = i32
    L.st_set_every_tile.argtypes = [u32, u32]
    L.st_set_every_tile.restype = i32
    L.st_set_every_caps.argtypes = [u32, u32]
    L.st_set_every_caps.restype = i32
    L.st_set_defer_cache.argtypes = [i32, u32, u32]
    L.st_set_defer_cache.restype = i32
    L.st_set_mfree_shape.argtypes = [u32]
    L.st_set_mfree_shape.restype = i32
    L.st_set_k0_reverse.argtypes = [i32]
    L.st_set_k0_reverse.restype = i32


def _declare(L: ctypes.CDLL) -> None:
    P, u32, u64, i32, i64 = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64,
                             ctypes.c_int, ctypes.c_int64)
    f32, f64 = ctypes.c_float, ctypes.c_double
    L.make_queue.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    L.make_queue.restype = None
    L.destroy_queue.argtypes = [P]
    L.destroy_queue.restype = None
    L.eigen_last_error.argtypes = []
    L.eigen_last_error.restype = ctypes.c_char_p
    L.st_version.restype = ctypes.c_char_p
    L.st_probe_switches.restype = ctypes.c_char_p
    L.st_device_count.restype = i32
    L.max_eigen_value.argtypes = [P, P, P, P, u32, P]
    L.max_eigen_value.restype = i64
    L.max_eigen_value_f64.argtypes = [P, P, P, P, u32, P]
    L.max_eigen_value_f64.restype = i64
    L.max_eigen_value_ex.argtypes = [P, i32, P, P, P, u32, P, P, P]
    L.max_eigen_value_ex.restype = i64
    L.max_eigen_value_batched_ex.argtypes = [P, i32, P, P, P, u32, u32, P, P, P]
    L.max_eigen_value_batched_ex.restype = i64
    L.st_solve_batched_max_dim.argtypes = [i32]
    L.st_solve_batched_max_dim.restype = u32
    L.st_solve_batched_rounds_max_dim.argtypes = [i32]
    L.st_solve_batched_rounds_max_dim.restype = u32
    L.max_eigen_value_vbatched_ex.argtypes = [P, i32, P, P, u32, P, P, P, P, P]
    L.max_eigen_value_vbatched_ex.restype = i64
    L.st_vbatched_plan.argtypes = [i32, P, u32, P, P]
    L.st_vbatched_plan.restype = i32
    L.st_last_round_times.argtypes = [P, P, u32]
    L.st_last_round_times.restype = i32
    L.st_last_round_sums.argtypes = [P, P, u32]
    L.st_last_round_sums.restype = i32
    L.st_set_stream.argtypes = [P, P]
    L.st_set_stream.restype = i32
    L.st_use_own_stream.argtypes = [P]
    L.st_use_own_stream.restype = i32
    for sfx, T in (("f32", f32), ("f64", f64)):
        fm = getattr(L, f"st_solve_multi_{sfx}")
        fm.argtypes = [P, u32, i32, P, i32, u64, P, P, P, P, P]
        fm.restype = i64
        fn = getattr(L, f"st_solve_device_{sfx}")
        fn.argtypes = [P, P, u32, P, P, P, P, P, P]
        fn.restype = i64
        fb = getattr(L, f"st_solve_batched_{sfx}")
        fb.argtypes = [P, P, u32, u32, P, P, P, P, P, P, P]
        fb.restype = i64
        fv = getattr(L, f"st_solve_vbatched_{sfx}")
        fv.argtypes = [P, P, P, u32, P, P, P, P, P, P, P]
        fv.restype = i64
        getattr(L, f"st_generate_hilbert_{sfx}").argtypes = [P, u32, u32, u32, P]
        getattr(L, f"st_generate_random_{sfx}").argtypes = [P, u32, u32, u32, u64, P]
        getattr(L, f"st_generate_identity_{sfx}").argtypes = [P, u32, u32, u32, P]
        getattr(L, f"st_fill_{sfx}").argtypes = [P, u64, T, P]
        getattr(L, f"st_rowsum_{sfx}").argtypes = [P, P, u32, u32, P]
        getattr(L, f"st_rowsum_flat_{sfx}").argtypes = [P, P, P, u32, u32, P]
        getattr(L, f"st_scale_rowsum_{sfx}").argtypes = [P, P, P, u32, u32, u32, u32, P, P]
        getattr(L, f"st_epilogue_{sfx}").argtypes = [P, P, u32, T, u32, u32, P, P]
        getattr(L, f"st_round_{sfx}").argtypes = [P, P, P, P, u32, u32, u32, T, u32, u32,
                                                  u32, P, P]
        getattr(L, f"st_mfree_round_flat_{sfx}").argtypes = [P, P, P, P, P, P, u32, u32, u32,
                                                              T, u32, u32, u32, P, P]
        getattr(L, f"st_mfree_round_flat_{sfx}").restype = i32
        getattr(L, f"st_mfree_round_{sfx}").argtypes = [P, P, P, P, P, u32, u32, u32, T, u32,
                                                        u32, u32, P, P]
        getattr(L, f"st_round_split_{sfx}").argtypes = [P, P, P, P, P, u32, u32, u32, u32,
                                                        u32, T, u32, u32, u32, i32, P, P]
        getattr(L, f"st_round_split_flat_{sfx}").argtypes = [P, P, P, P, P, u32, u32, u32,
                                                             u32, u32, T, u32, u32, u32,
                                                             i32, P, P]
        getattr(L, f"st_round_flat_{sfx}").argtypes = [P, P, P, P, P, u32, u32, u32, T, u32,
                                                       u32, u32, P, P]
        getattr(L, f"st_round_flat_deferred_{sfx}").argtypes = [
            P, P, P, P, P, P, P, u32, u32, u32, T, u32, u32, u32, P, P, u32, i32, i32, P, P]
        getattr(L, f"st_recip_{sfx}").argtypes = [P, P, u32, P]
        for name in ("generate_hilbert", "generate_random", "generate_identity",
                     "fill", "rowsum", "rowsum_flat", "scale_rowsum", "epilogue", "round", "mfree_round",
                     "round_split", "round_split_flat", "round_flat", "round_flat_deferred",
                     "recip"):
            getattr(L, f"st_{name}_{sfx}").restype = i32
    L.st_round_flat_scratch.argtypes = [u32, u32]
    L.st_round_flat_scratch.restype = u64
    L.st_round_split_flat_scratch.argtypes = [u32, u32, u32, u32]
    L.st_round_split_flat_scratch.restype = u64
    L.st_round_flat_pays.argtypes = [u32, u32, i32]
    L.st_round_flat_pays.restype = i32
    L.st_defer_rounds.argtypes = [u32, u32, i32]
    L.st_defer_rounds.restype = u32
    L.st_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.st_comm_unique_id.restype = i32
    L.st_comm_unique_id_addr.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.st_comm_unique_id_addr.restype = i32
    L.st_comm_init.argtypes = [ctypes.POINTER(ctypes.c_void_p), i32, i32, ctypes.c_char_p, i32]
    L.st_comm_init.restype = i32
    L.st_comm_id_release.argtypes = [ctypes.c_char_p]
    L.st_comm_id_release.restype = i32
    L.st_comm_destroy.argtypes = [P]
    L.st_comm_destroy.restype = i32
    L.st_set_comm_timeout.argtypes = [ctypes.c_double]
    L.st_set_comm_timeout.restype = ctypes.c_double
    L.st_comm_info.argtypes = [P, P, P, P]
    L.st_comm_info.restype = i32
    L.st_get_comm_timeout.argtypes = []
    L.st_get_comm_timeout.restype = ctypes.c_double
    L.st_rccl_version.argtypes = [P, ctypes.c_char_p, i32]
    L.st_rccl_version.restype = i32
    for sfx in ("f32", "f64"):
        getattr(L, f"st_allgather_{sfx}").argtypes = [P, P, P, u64, P]
        getattr(L, f"st_allgather_{sfx}").restype = i32
    L.st_launch_policy_query.argtypes = [i32, u32, u32, i32, u32, P]
    L.st_launch_policy_query.restype = i32
    L.st_state_reset.argtypes = [P, P]
    L.st_state_reset.restype = i32
    # half-precision storage (fp16 / bf16 matrix, fp32 vectors)
    L.st_rowsum_half.argtypes = [i32, P, P, u32, u32, P]
    L.st_rowsum_half.restype = i32
    L.st_mfree_round_half.argtypes = [i32, P, P, P, P, P, u32, u32, u32, f32, u32, u32, u32,
                                      P, P]
    L.st_mfree_round_half.restype = i32
    L.st_narrow_f32.argtypes = [i32, P, P, u64, P]
    L.st_narrow_f32.restype = i32
    L.st_solve_device_half.argtypes = [P, i32, P, u32, P, P, P, P, P, P]
    L.st_solve_device_half.restype = i64
    L.max_eigen_value_half_ex.argtypes = [P, i32, P, P, P, u32, P, P, P]
    L.max_eigen_value_half_ex.restype = i64
    L.st_half_shape_desc.argtypes = []
    L.st_half_shape_desc.restype = ctypes.c_char_p
    # dense left vector (the matrix read where it lies, swept by columns)
    for sfx, T in (("f32", f32), ("f64", f64)):
        getattr(L, f"st_solve_device_left_{sfx}").argtypes = [P, P, u32, P, P, P, P, P, P]
        getattr(L, f"st_solve_device_left_{sfx}").restype = i64
        getattr(L, f"st_colsum_{sfx}").argtypes = [P, P, P, u32, P]
        getattr(L, f"st_colsum_{sfx}").restype = i32
        getattr(L, f"st_mfree_left_round_{sfx}").argtypes = [P, P, P, P, P, P, u32, T, u32,
                                                             u32, u32, P, P]
        getattr(L, f"st_mfree_left_round_{sfx}").restype = i32
    L.max_eigen_value_left_ex.argtypes = [P, i32, P, P, P, u32, P, P, P]
    L.max_eigen_value_left_ex.restype = i64
    L.st_left_shape.argtypes = [i32, u32, P, P]
    L.st_left_shape.restype = i32
    L.st_left_scratch.argtypes = [i32, u32]
    L.st_left_scratch.restype = u64
    L.st_left_shape_desc.argtypes = []
    L.st_left_shape_desc.restype = ctypes.c_char_p
    # dense Perron pair (both vectors from one pass over the matrix per round)
    for sfx, T in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        getattr(L, f"st_solve_device_pair_{sfx}").argtypes = [P, P, u32, P, P, P, P, P, P, P]
        getattr(L, f"st_solve_device_pair_{sfx}").restype = i64
        getattr(L, f"st_pair_sum_{sfx}").argtypes = [P, P, P, P, u32, P]
        getattr(L, f"st_pair_sum_{sfx}").restype = i32
        getattr(L, f"st_mfree_pair_round_{sfx}").argtypes = [P] * 10 + [u32, T, u32, u32, u32,
                                                                      P, P]
        getattr(L, f"st_mfree_pair_round_{sfx}").restype = i32
    L.max_eigen_value_pair_ex.argtypes = [P, i32, P, P, P, u32, P, P, P, P]
    L.max_eigen_value_pair_ex.restype = i64
    L.st_pair_shape.argtypes = [i32, u32, P, P, P, P]
    L.st_pair_shape.restype = i32
    L.st_pair_scratch.argtypes = [i32, u32]
    L.st_pair_scratch.restype = u64
    L.st_pair_shape_desc.argtypes = []
    L.st_pair_shape_desc.restype = ctypes.c_char_p
    # sparse (CSR) solve
    L.st_csr_class_limits.argtypes = [i32, P, P, i32]
    L.st_csr_class_limits.restype = i32
    L.st_csr_plan.argtypes = [P, u32, P, P]
    L.st_csr_plan.restype = i32
    L.st_csr_shape_desc.argtypes = []
    L.st_csr_shape_desc.restype = ctypes.c_char_p
    L.st_csr_create.argtypes = [P, i32, u32, u64, P, P, P, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_create.restype = i32
    L.st_csr_destroy.argtypes = [P]
    L.st_csr_destroy.restype = i32
    L.st_csr_get_plan.argtypes = [P, P, P]
    L.st_csr_get_plan.restype = i32
    L.st_solve_csr.argtypes = [P, P, P, P, P, P, P, P]
    L.st_solve_csr.restype = i64
    L.max_eigen_value_csr_ex.argtypes = [P, i32, u32, u64, P, P, P, P, P, P, P, P]
    L.max_eigen_value_csr_ex.restype = i64
    L.st_csr_transpose_host.argtypes = [i32, u32, u64, P, P, P, P, P, P]
    L.st_csr_transpose_host.restype = i32
    L.st_csr_transpose.argtypes = [P, P, P, P, P, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_transpose.restype = i32
    L.st_csr_transpose_scratch_bytes.argtypes = [u32, u64]
    L.st_csr_transpose_scratch_bytes.restype = u64
    L.st_csr_transpose_shape_desc.argtypes = []
    L.st_csr_transpose_shape_desc.restype = ctypes.c_char_p
    L.max_eigen_value_csr_left_ex.argtypes = [P, i32, u32, u64, P, P, P, P, P, P, P, P]
    L.max_eigen_value_csr_left_ex.restype = i64
    L.st_csr_rowsum.argtypes = [P, P, P]
    L.st_csr_rowsum.restype = i32
    L.st_csr_mfree_round.argtypes = [P, P, P, P, P, P, f64, u32, u32, u32, P, P]
    L.st_csr_mfree_round.restype = i32
    # low-rank terms and empty rows
    L.st_csr_create_ex.argtypes = [P, i32, u32, u64, P, P, P, u32,
                                   ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_create_ex.restype = i32
    L.st_csr_empty_rows.argtypes = [P, P, P]
    L.st_csr_empty_rows.restype = i32
    L.st_csr_transpose_ex.argtypes = [P, P, P, P, P, u32, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_transpose_ex.restype = i32
    L.st_csr_transpose_host_ex.argtypes = [i32, u32, u64, P, P, P, P, P, P, u32]
    L.st_csr_transpose_host_ex.restype = i32
    L.st_csr_terms_create.argtypes = [P, P, u32, P, P, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_terms_create.restype = i32
    L.st_csr_terms_destroy.argtypes = [P]
    L.st_csr_terms_destroy.restype = i32
    L.st_csr_terms_scratch_bytes.argtypes = [u32, u32]
    L.st_csr_terms_scratch_bytes.restype = u64
    L.st_csr_terms_shape_desc.argtypes = []
    L.st_csr_terms_shape_desc.restype = ctypes.c_char_p
    L.st_solve_csr_terms.argtypes = [P, P, P, P, P, P, P, P, P]
    L.st_solve_csr_terms.restype = i64
    L.max_eigen_value_csr_terms_ex.argtypes = [P, i32, u32, u64, P, P, P, u32, P, P, u32,
                                               P, P, P, P, P]
    L.max_eigen_value_csr_terms_ex.restype = i64
    L.st_csr_terms_rowsum.argtypes = [P, P, P, P, P]
    L.st_csr_terms_rowsum.restype = i32
    L.st_csr_terms_round.argtypes = [P, P, P, P, P, P, P, f64, u32, u32, u32, P, P]
    L.st_csr_terms_round.restype = i32
    # pattern-only matrices with row / column scales
    L.st_csr_pattern_create.argtypes = [P, i32, u32, u64, P, P, P, P, u32,
                                        ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_pattern_create.restype = i32
    L.st_csr_pattern_destroy.argtypes = [P]
    L.st_csr_pattern_destroy.restype = i32
    L.st_csr_pattern_get_plan.argtypes = [P, P, P]
    L.st_csr_pattern_get_plan.restype = i32
    L.st_csr_pattern_empty_rows.argtypes = [P, P, P]
    L.st_csr_pattern_empty_rows.restype = i32
    L.st_csr_pattern_transpose.argtypes = [P, P, P, P, u32, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_pattern_transpose.restype = i32
    L.st_csr_pattern_terms_create.argtypes = [P, P, u32, P, P,
                                              ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_pattern_terms_create.restype = i32
    L.st_solve_csr_pattern.argtypes = [P, P, P, P, P, P, P, P, P]
    L.st_solve_csr_pattern.restype = i64
    L.st_csr_pattern_scratch_bytes.argtypes = [u32, u32]
    L.st_csr_pattern_scratch_bytes.restype = u64
    L.st_csr_pattern_shape_desc.argtypes = []
    L.st_csr_pattern_shape_desc.restype = ctypes.c_char_p
    L.st_csr_pattern_rowsum.argtypes = [P, P, P, P, P]
    L.st_csr_pattern_rowsum.restype = i32
    L.st_csr_pattern_round.argtypes = [P, P, P, P, P, P, P, f64, u32, u32, u32, P, P]
    L.st_csr_pattern_round.restype = i32
    L.max_eigen_value_csr_pattern_ex.argtypes = [P, i32, u32, u64, P, P, P, P, u32, P, P,
                                                 u32, P, P, P, P, P]
    L.max_eigen_value_csr_pattern_ex.restype = i64
    L.st_csr_multi_create.argtypes = [P, P, u32, u32, P, P, ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_multi_create.restype = i32
    L.st_csr_multi_destroy.argtypes = [P]
    L.st_csr_multi_destroy.restype = i32
    L.st_csr_multi_scratch_bytes.argtypes = [u32, u32, u32]
    L.st_csr_multi_scratch_bytes.restype = u64
    L.st_csr_multi_shape_desc.argtypes = []
    L.st_csr_multi_shape_desc.restype = ctypes.c_char_p
    L.st_solve_csr_multi.argtypes = [P, P, P, P, P, P, P, P, P, P]
    L.st_solve_csr_multi.restype = i64
    L.max_eigen_value_csr_multi_ex.argtypes = [P, i32, u32, u64, P, P, P, u32, u32, P, P, u32,
                                               P, P, P, P, P, P]
    L.max_eigen_value_csr_multi_ex.restype = i64
    L.st_csr_multi_rowsum.argtypes = [P, P, P, P, P]
    L.st_csr_multi_rowsum.restype = i32
    L.st_csr_multi_round.argtypes = [P, P, P, P, P, P, P, f64, u32, u32, u32, P, P, P]
    L.st_csr_multi_round.restype = i32
    # the product operator B A (section 3g)
    L.st_solve_csr_product.argtypes = [P, P, P, P, P, P, P, P, P]
    L.st_solve_csr_product.restype = i64
    L.st_csr_apply.argtypes = [P, P, P, P]
    L.st_csr_apply.restype = i32
    L.st_csr_product_scratch_bytes.argtypes = [u32]
    L.st_csr_product_scratch_bytes.restype = u64
    L.st_csr_product_shape_desc.argtypes = []
    L.st_csr_product_shape_desc.restype = ctypes.c_char_p
    L.st_csr_product_rowsum.argtypes = [P, P, P, P, P]
    L.st_csr_product_rowsum.restype = i32
    L.st_csr_product_round.argtypes = [P, P, P, P, P, P, P, f64, u32, u32, u32, P, P]
    L.st_csr_product_round.restype = i32
    L.max_eigen_value_csr_product_ex.argtypes = [P, i32, u32, u64, P, P, P, u64, P, P, P, u32,
                                                 P, P, P, P, P]
    L.max_eigen_value_csr_product_ex.restype = i64
    L.max_eigen_value_csr_gram_ex.argtypes = [P, i32, u32, u64, P, P, P, i32, u32,
                                              P, P, P, P, P]
    L.max_eigen_value_csr_gram_ex.restype = i64
    L.st_csr_batch_create.argtypes = [P, i32, u32, P, u64, P, P, P,
                                      ctypes.POINTER(ctypes.c_void_p)]
    L.st_csr_batch_create.restype = i32
    L.st_csr_batch_destroy.argtypes = [P]
    L.st_csr_batch_destroy.restype = i32
    L.st_csr_batch_get_plan.argtypes = [P, P, P]
    L.st_csr_batch_get_plan.restype = i32
    L.st_csr_batch_shape_desc.argtypes = []
    L.st_csr_batch_shape_desc.restype = ctypes.c_char_p
    L.st_solve_csr_batched.argtypes = [P, P, P, P, P, P, P, P, P]
    L.st_solve_csr_batched.restype = i64
    L.max_eigen_value_csr_batched_ex.argtypes = [P, i32, u32, P, u64, P, P, P, P, P, P, P, P, P]
    L.max_eigen_value_csr_batched_ex.restype = i64
    L.st_csr_batch_rowsum.argtypes = [P, P, P]
    L.st_csr_batch_rowsum.restype = i32
    L.st_csr_batch_mfree_round.argtypes = [P, P, P, P, P, P, f64, u32, u32, u32, P, P, P]
    L.st_csr_batch_mfree_round.restype = i32


def batch_rounds_flag(round_loop, n: int, dtype_code: int) -> int:
    """The ``round_loop`` keyword of the batched solves as option flags:
    ``None`` / ``False`` 0 (the one-launch kernel), ``True``
    ST_FLAG_BATCH_ROUNDS, ``"auto"`` the flag only where n is beyond the
    one-launch kernel (st_solve_batched_max_dim).  Anything else is a
    ValueError, raised before any library call."""
    if round_loop is None or round_loop is False:
        return 0
    if round_loop is True:
        return ST_FLAG_BATCH_ROUNDS
    if isinstance(round_loop, str) and round_loop == "auto":
        return ST_FLAG_BATCH_ROUNDS if n > load().st_solve_batched_max_dim(dtype_code) else 0
    raise ValueError(f'round_loop must be None, True or "auto", got {round_loop!r}')


ST_VBATCH_CLASSES = 7


def vbatched_plan(dims, dtype_code: int, L: Optional[ctypes.CDLL] = None):
    """The size-class plan of a variable-size batch (st_vbatched_plan; no GPU):
    ``(order, class_first, used)`` - the matrix indices sorted by class (input
    order kept within a class) as a uint32 array[B], where each of the
    ST_VBATCH_CLASSES classes starts in it (uint32 array[8]) and the number
    of non-empty classes.  Raises EigenValueError for a dim of 0 or above
    st_solve_batched_max_dim (the message names index and dim)."""
    import numpy as np
    L = L or load()
    dims = np.ascontiguousarray(dims, dtype=np.uint32)
    order = np.zeros(len(dims), dtype=np.uint32)
    first = np.zeros(ST_VBATCH_CLASSES + 1, dtype=np.uint32)
    used = check(L.st_vbatched_plan(dtype_code, dims.ctypes.data, len(dims), order.ctypes.data,
                                    first.ctypes.data), "st_vbatched_plan", L)
    return order, first, used


ST_CSR_CLASSES = 4
ST_CSR_TERMS_MAX = 4
ST_CSR_EMPTY_ROWS_OK = 1


def csr_class_limits(dtype_code: int = DTYPE_F32, L: Optional[ctypes.CDLL] = None):
    """The row-class table of the CSR kernels (st_csr_class_limits; no GPU):
    ``(nnz_max, lanes)``, two uint32 arrays[ST_CSR_CLASSES] - a row of nnz
    entries belongs to the first class with nnz <= nnz_max and is shared by
    that class's lanes."""
    import numpy as np
    L = L or load()
    nnz_max = np.zeros(ST_CSR_CLASSES, dtype=np.uint32)
    lanes = np.zeros(ST_CSR_CLASSES, dtype=np.uint32)
    got = check(L.st_csr_class_limits(dtype_code, nnz_max.ctypes.data, lanes.ctypes.data,
                                      ST_CSR_CLASSES), "st_csr_class_limits", L)
    assert got == ST_CSR_CLASSES
    return nnz_max, lanes


def csr_plan(row_ptr, L: Optional[ctypes.CDLL] = None):
    """The plan of a host ``row_ptr`` (st_csr_plan; no GPU): ``(order,
    class_first, used)`` - the row indices sorted by class (row order kept
    within a class) as a uint32 array[n], the class starts (uint32
    array[ST_CSR_CLASSES + 1]) and the number of non-empty classes.  Raises
    EigenValueError naming the row for an empty row or a decreasing row_ptr."""
    import numpy as np
    L = L or load()
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    order = np.zeros(max(n, 0), dtype=np.uint32)
    first = np.zeros(ST_CSR_CLASSES + 1, dtype=np.uint32)
    used = check(L.st_csr_plan(row_ptr.ctypes.data, max(n, 0), order.ctypes.data,
                               first.ctypes.data), "st_csr_plan", L)
    return order, first, used


def csr_transpose_host(indptr, indices, data, L: Optional[ctypes.CDLL] = None,
                       allow_empty: bool = False):
    """T(A) of a host CSR matrix (st_csr_transpose_host; no GPU): ``(t_indptr
    int64 [n + 1], t_indices int32 [nnz], t_data [nnz])`` - the entries sorted
    by column, entries of one column in storage order; numpy's ``p =
    argsort(indices, kind="stable")``, ``rows[p]``, ``data[p]``.  ``data`` is
    float32 or float64.  Raises EigenValueError for whatever the CSR solve
    refuses, and naming the lowest column without an entry.  ``allow_empty``
    (st_csr_transpose_host_ex, ST_CSR_EMPTY_ROWS_OK): empty rows and empty
    columns are legal."""
    import numpy as np
    L = L or load()
    data = np.ascontiguousarray(data)
    if data.dtype not in (np.float32, np.float64):
        raise TypeError(f"data must be float32 or float64, got {data.dtype}")
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if len(indices) != len(data):
        raise ValueError("indices and data differ in length")
    n = len(indptr) - 1
    t_ptr = np.zeros(max(n, 0) + 1, dtype=np.int64)
    t_idx = np.zeros(len(data), dtype=np.int32)
    t_val = np.zeros(len(data), dtype=data.dtype)
    args = (DTYPE_F64 if data.dtype == np.float64 else DTYPE_F32, max(n, 0), len(data),
            indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, t_ptr.ctypes.data,
            t_idx.ctypes.data, t_val.ctypes.data)
    if allow_empty:
        check(L.st_csr_transpose_host_ex(*args, ST_CSR_EMPTY_ROWS_OK),
              "st_csr_transpose_host_ex", L)
    else:
        check(L.st_csr_transpose_host(*args), "st_csr_transpose_host", L)
    return t_ptr, t_idx, t_val


def csr_terms_shape(L: Optional[ctypes.CDLL] = None) -> dict:
    """st_csr_terms_shape_desc as a dict (integers where they are)."""
    L = L or load()
    out = {}
    for item in L.st_csr_terms_shape_desc().decode().split():
        k, v = item.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


CSR_PATTERN_SYMBOLS = (
    "st_csr_pattern_create", "st_csr_pattern_destroy", "st_csr_pattern_get_plan",
    "st_csr_pattern_empty_rows", "st_csr_pattern_transpose", "st_csr_pattern_terms_create",
    "st_solve_csr_pattern", "st_csr_pattern_scratch_bytes", "st_csr_pattern_shape_desc",
    "st_csr_pattern_rowsum", "st_csr_pattern_round", "max_eigen_value_csr_pattern_ex")


def csr_pattern_shape(L: Optional[ctypes.CDLL] = None) -> dict:
    """st_csr_pattern_shape_desc as a dict (integers where they are)."""
    L = L or load()
    out = {}
    for item in L.st_csr_pattern_shape_desc().decode().split():
        k, v = item.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


def check_terms_arg(u, w, n: int):
    """What every Python front checks of a terms argument before any library
    call: ``u`` and ``w`` are [K, n] arrays or sequences of K vectors of n
    elements, 1 <= K <= ST_CSR_TERMS_MAX, equally many of each.  Returns K."""
    try:
        ku, kw = len(u), len(w)
    except TypeError:
        raise TypeError("terms: u and w must be [K, n] arrays or sequences of K vectors")
    if ku != kw:
        raise ValueError(f"terms: {ku} vectors u but {kw} vectors w")
    if not 1 <= ku <= ST_CSR_TERMS_MAX:
        raise ValueError(f"terms: K must be in [1, {ST_CSR_TERMS_MAX}], got {ku}")
    for name, vs in (("u", u), ("w", w)):
        for j, x in enumerate(vs):
            shape = tuple(getattr(x, "shape", (len(x),)))
            if shape != (n,):
                raise ValueError(f"terms: {name}_{j} has shape {shape}, ({n},) required")
    return ku


ST_GRAM_ATA = 0
ST_GRAM_AAT = 1
CSR_PRODUCT_SYMBOLS = (
    "st_solve_csr_product", "st_csr_apply", "st_csr_product_rowsum", "st_csr_product_round",
    "st_csr_product_scratch_bytes", "st_csr_product_shape_desc",
    "max_eigen_value_csr_product_ex", "max_eigen_value_csr_gram_ex")


def csr_product_shape(L: Optional[ctypes.CDLL] = None) -> dict:
    """st_csr_product_shape_desc as a dict (integers where they are)."""
    L = L or load()
    out = {}
    for item in L.st_csr_product_shape_desc().decode().split():
        k, v = item.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


def gram_side(side) -> int:
    """The ``side`` keyword of the Gram fronts as the C-ABI's code: ``"ata"``
    (AᵀA) -> ST_GRAM_ATA, ``"aat"`` (AAᵀ) -> ST_GRAM_AAT.  Anything else is a
    ValueError, raised before any library call."""
    if isinstance(side, str) and side in ("ata", "aat"):
        return ST_GRAM_ATA if side == "ata" else ST_GRAM_AAT
    raise ValueError(f'side must be "ata" or "aat", got {side!r}')


ST_CSR_MULTI_MAX = 8


def csr_multi_cp(C: int) -> int:
    """The packed width of C columns: the smallest of 2, 4, 8 that is >= C."""
    return 2 if C <= 2 else 4 if C <= 4 else 8


def csr_multi_shape(L: Optional[ctypes.CDLL] = None) -> dict:
    """st_csr_multi_shape_desc as a dict (integers where they are, tuples of
    integers for the comma-separated tables)."""
    L = L or load()
    out = {}
    for item in L.st_csr_multi_shape_desc().decode().split():
        k, v = item.split("=")
        if "," in v:
            out[k] = tuple(int(x) for x in v.split(","))
        else:
            out[k] = int(v) if v.isdigit() else v
    return out


def check_multi_terms_arg(u, w, n: int):
    """What every Python front checks of a multi terms argument before any
    library call: ``u`` and ``w`` are [C, K, n] arrays (or [C, n], K = 1, or
    sequences of C entries ``check_terms_arg`` accepts), 1 <= C <=
    ST_CSR_MULTI_MAX, the same K for every column.  Returns (C, K, u, w) with
    u, w as lists of C lists of K vectors."""
    try:
        cu, cw = len(u), len(w)
    except TypeError:
        raise TypeError("multi terms: u and w must be [C, K, n] arrays or sequences of C "
                        "term sets")
    if cu != cw:
        raise ValueError(f"multi terms: {cu} columns u but {cw} columns w")
    if not 1 <= cu <= ST_CSR_MULTI_MAX:
        raise ValueError(f"multi terms: C must be in [1, {ST_CSR_MULTI_MAX}], got {cu}")

    def rows(x):
        return [x] if len(getattr(x, "shape", ())) == 1 else list(x)

    uu, ww = [rows(x) for x in u], [rows(x) for x in w]
    K = None
    for c in range(cu):
        try:
            k = check_terms_arg(uu[c], ww[c], n)
        except (TypeError, ValueError) as e:
            raise type(e)(f"column {c}: {e}") from None
        if K is not None and k != K:
            raise ValueError(f"multi terms: column {c} has {k} terms, column 0 has {K}: every "
                             "column takes the same K (pad with u = 0)")
        K = k
    return cu, K, uu, ww


def csr_transpose_shape(L: Optional[ctypes.CDLL] = None) -> dict:
    """st_csr_transpose_shape_desc as a dict (integers where they are)."""
    L = L or load()
    out = {}
    for item in L.st_csr_transpose_shape_desc().decode().split():
        k, v = item.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


def left_shape(dtype_code: int, n: int, L: Optional[ctypes.CDLL] = None) -> dict:
    """st_left_shape and st_left_shape_desc for one (dtype, n), no GPU: rows
    (RB of the order contract), combine (0 serial, 1 tree), block, w (columns
    per lane when the row stride allows 16-byte loads) and strip = block * w;
    rows_table / rows_from (the table's values and the n each holds from),
    rows_in_flight, nt_from_mib and nt (whether this n's sweeps load
    non-temporally: n * n elements reach nt_from_mib MiB, as left::grid
    decides it)."""
    L = L or load()
    rows, comb = ctypes.c_uint32(), ctypes.c_uint32()
    check(L.st_left_shape(dtype_code, n, ctypes.byref(rows), ctypes.byref(comb)),
          "st_left_shape", L)
    desc = dict(kv.split("=") for kv in L.st_left_shape_desc().decode().split())
    block = int(desc["block"])
    elem = 8 if dtype_code == DTYPE_F64 else 4
    w = int(desc["bytes_per_load"]) // elem
    nt_from_mib = int(desc["nt_from_mib"])
    return {"rows": rows.value, "combine": comb.value, "block": block, "w": w,
            "strip": block * w,
            "rows_table": [int(v) for v in desc["rows_per_block"].split(",")],
            "rows_from": [int(v) for v in desc["rows_from"].split(",")],
            "rows_in_flight": int(desc["rows_in_flight"]),
            "nt_from_mib": nt_from_mib,
            "nt": n * n >= (nt_from_mib << 20) // elem}


def pair_shape(dtype_code: int, n: int, L: Optional[ctypes.CDLL] = None) -> dict:
    """st_pair_shape and st_pair_shape_desc for one (dtype, n), no GPU: rows
    (RB, st_left_shape's), strip (S: the columns of a workgroup, part of a
    row's order), combine_left / combine_right (0 serial), block, w (columns
    per lane = 16 bytes of elements, whatever the kind of load), nstrips,
    rows_in_flight, lds_rows, nt_from_mib and nt."""
    L = L or load()
    rows, strip, cl, cr = (ctypes.c_uint32() for _ in range(4))
    check(L.st_pair_shape(dtype_code, n, ctypes.byref(rows), ctypes.byref(strip),
                          ctypes.byref(cl), ctypes.byref(cr)), "st_pair_shape", L)
    desc = dict(kv.split("=") for kv in L.st_pair_shape_desc().decode().split())
    elem = 8 if dtype_code == DTYPE_F64 else 4
    nt_from_mib = int(desc["nt_from_mib"])
    return {"rows": rows.value, "strip": strip.value, "combine_left": cl.value,
            "combine_right": cr.value, "block": int(desc["block"]),
            "w": int(desc["bytes_per_load"]) // elem,
            "nstrips": -(-n // strip.value),
            "rows_in_flight": int(desc["rows_in_flight"]),
            "lds_rows": int(desc["lds_rows"]),
            "nt_from_mib": nt_from_mib,
            "nt": n * n >= (nt_from_mib << 20) // elem}


def round_sums(L: ctypes.CDLL, q, n: int, dtype):
    """st_last_round_sums of queue ``q`` as a (rounds, n) array of ``dtype``."""
    import numpy as np
    r = check(L.st_last_round_sums(q, None, 0), "st_last_round_sums", L)
    out = np.zeros((r, n), dtype=dtype)
    if r and n:
        check(L.st_last_round_sums(q, out.ctypes.data, r), "st_last_round_sums", L)
    return out


def rccl_info(L: Optional[ctypes.CDLL] = None) -> dict:
    """The RCCL the library's calls are bound to in THIS process
    (st_rccl_version): {"rccl_version": "X.Y.Z", "rccl_version_code": int,
    "rccl_path": file holding the bound ncclAllGather}.  Inside a torch
    process that is torch's bundled librccl; for a C caller the /opt/rocm one."""
    L = L or load()
    code = ctypes.c_int(0)
    path = ctypes.create_string_buffer(4096)
    L.st_rccl_version(ctypes.byref(code), path, len(path))
    v = code.value
    return {"rccl_version": f"{v // 10000}.{v // 100 % 100}.{v % 100}",
            "rccl_version_code": v, "rccl_path": path.value.decode(errors="replace")}


def last_error(L: Optional[ctypes.CDLL] = None) -> str:
    """The thread-local message of the library that made the failing call
    (``L``; the default library when None)."""
    msg = (L or load()).eigen_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str, L: Optional[ctypes.CDLL] = None) -> int:
    """Raise EigenValueError for a negative return of a call into ``L``."""
    if rc < 0:
        raise EigenValueError(f"{what} failed: {last_error(L) or 'unknown error'}")
    return rc


def declared_symbols(header: str = HEADER) -> list[str]:
    """Function names declared inside the extern "C" block of the header."""
    import re
    text = open(header).read()
    body = text.split('extern "C" {', 1)[1].split('} /* extern "C" */', 1)[0]
    body = body.split("#ifdef __cplusplus", 1)[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", body)
    skip = {"sizeof"}
    return sorted({n for n in names if n not in skip and not n.isupper()})
