#!/usr/bin/env python3
"""Per-round kernel time of the CSR round on a product operator, and HITS.

One run, interleaved legs, on the matrices of tools/bench_csr.py: uniform
ones with 8 and 32 random columns per row and the banded one (32 per row
within 2048 of the diagonal) at --n rows, and 32 per row at --small-n rows,
where the launches and not the bytes decide.  The first entry of every row is
moved to the diagonal, so that no column is empty and B = A^T has no empty
row (with 8 random columns per row about n e^-8 columns would be).  Every
pass runs, in this order,

    a         solve_csr on A            (k_csr_prep + k_csr_spmv)
    at        solve_csr on A^T          (the same, on the device transposition)
    product   solve_csr_product(A^T, A) (k_csr_prep + k_csrp_apply on A +
                                         k_csrp_final on A^T)

each for --rounds fixed rounds (eps = 0) with ST_FLAG_TIME_KERNELS: all
launches of a round between the events.  A leg's figure is the median over
all its timed rounds of all passes (each solve's first round is left out).

The yardstick is the SUM a + at of the same run.  The byte model: a single
round moves nnz (b + 4) + 8 (n + 1) + 4 n + 8 n b bytes (tools/bench_csr.py;
the x gathers are not counted) - of the 8 n b, 3 n b are the vector pass (s,
v, x) and 5 n b the row pass's last step (x[r], s_prev, v_prev, s_next,
v_cur).  The product round has one vector pass, writes y (n b) in the apply
and has one last step: (nnz_A + nnz_B)(b + 4) + 2 (8 (n + 1) + 4 n) + 9 n b -
the sum minus one vector pass and one v update.  `model_ms` = (a + at) *
bytes_product / (bytes_a + bytes_at), `gap_ms` = measured - model.

Where torch.sparse.mm forms A^T A on this build (tried for the small case and
the 8-per-row case only: about n d^2 entries), the time to form it, its nnz
and solve_csr's ms per round on it are recorded; otherwise the reason.

The HITS leg: the 32-per-row graph with 1 % of the rows emptied (nodes without
out-links; the graph tools/bench_csr_terms.py uses for pagerank), `hits` end
to end - transposition, validation, the solve for --rounds rounds at eps = 0,
the hub product - wall-clock with a device synchronisation at each end;
`hits_loop_ms` is the solve's share (stats["loop_ms"]).

Prints one JSON document (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from bench_csr import banded, bytes_per_round, uniform  # noqa: E402
from bench_csr_terms import with_dangling  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402


def product_bytes(n, nnz_b, nnz_a, b):
    return (nnz_a + nnz_b) * (b + 4) + 2 * (8 * (n + 1) + 4 * n) + 9 * n * b


def med(ms):
    return {"ms_per_round": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms)}


def with_diagonal(crow, col, n, d):
    """The first entry of every row moved to the diagonal: no empty column."""
    col = col.clone()
    col[::d] = torch.arange(n, device=col.device, dtype=torch.int32)
    return col


def form_gram(A, At, solver, rounds):
    """A^T A by torch.sparse.mm, and solve_csr's round on it."""
    n = A.n
    out = {}
    try:
        sa = torch.sparse_csr_tensor(A.crow, A.col.long(), A.values, size=(n, n))
        st = torch.sparse_csr_tensor(At.crow, At.col.long(), At.values, size=(n, n))
        torch.cuda.synchronize(A.device)
        t0 = time.perf_counter()
        g = torch.sparse.mm(st, sa)
        torch.cuda.synchronize(A.device)
        out["form_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        if g.layout != torch.sparse_csr:
            g = g.to_sparse_csr()
        out["nnz"] = int(g.values().numel())
        m = dev.CsrMatrix(g.crow_indices(), g.col_indices(), g.values().contiguous(), n,
                          solver=solver)
        _, _, _, s = solver.solve_csr(m, eps=0.0, max_itr=rounds, time_kernels=True)
        out["solve_csr"] = med([float(x) for x in solver.last_round_times()][1:])
        m.close()
        del g, sa, st
    except Exception as e:              # the comparison leg only; recorded, not hidden
        out["formed"] = f"could not be formed: {e}"[:240]
    return out


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--n", type=int, default=1 << 22)
    p.add_argument("--small-n", type=int, default=16384)
    p.add_argument("--dtypes", default="f32,f64")
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default="")
    a = p.parse_args()
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    L = _lib.load()
    solver = dev.DeviceSolver(device)
    doc = {"tool": "tools/bench_csr_product.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_csr_shape_desc().decode(),
           "product_lib": L.st_csr_product_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "note": "per-round kernel time, eps = 0, median over the timed rounds of all passes "
                   "without each solve's first; B = A^T; model_ms = (a + at) * bytes_product / "
                   "(bytes_a + bytes_at), bytes_product = (nnz_A + nnz_B)(b + 4) + 2 (8 (n + 1) "
                   "+ 4 n) + 9 n b",
           "cases": {}}
    cases = [("uniform_d8", "uniform", a.n, 8, True), ("uniform_d32", "uniform", a.n, 32, False),
             ("banded_d32", "banded", a.n, 32, False), ("small_d32", "uniform", a.small_n, 32, True)]
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        b = 8 if dt_name == "f64" else 4
        for name, kind, n, d, try_gram in cases:
            g = torch.Generator(device=device).manual_seed(a.seed)
            crow, col, val = (banded if kind == "banded" else uniform)(n, d, dtype, g, device)
            col = with_diagonal(crow, col, n, d)
            nnz = int(val.numel())
            A = dev.CsrMatrix(crow, col, val, n, solver=solver)
            At = A.transpose(solver)
            legs = {"a": [], "at": [], "product": []}
            for _ in range(a.passes):
                for leg in ("a", "at", "product"):
                    if leg == "product":
                        _, _, _, st = solver.solve_csr_product(At, A, eps=0.0, max_itr=a.rounds,
                                                               time_kernels=True)
                    else:
                        _, _, _, st = solver.solve_csr(A if leg == "a" else At, eps=0.0,
                                                       max_itr=a.rounds, time_kernels=True)
                    assert st["rounds"] == a.rounds and st["converged"] == 0
                    legs[leg] += [float(x) for x in solver.last_round_times()][1:]
            one = bytes_per_round(n, nnz, b)
            pb = product_bytes(n, nnz, nnz, b)
            out = {"n": n, "nnz": nnz, "bytes_single": one, "bytes_product": pb,
                   "a": med(legs["a"]), "at": med(legs["at"]), "product": med(legs["product"])}
            both = out["a"]["ms_per_round"] + out["at"]["ms_per_round"]
            e = out["product"]
            e["gbps"] = round(pb / e["ms_per_round"] / 1e6, 1)
            e["sum_a_at_ms"] = round(both, 5)
            e["ratio_measured"] = round(e["ms_per_round"] / both, 4)
            e["ratio_model"] = round(pb / (2 * one), 4)
            e["model_ms"] = round(both * pb / (2 * one), 5)
            e["gap_ms"] = round(e["ms_per_round"] - both * pb / (2 * one), 5)
            if try_gram:
                out["torch_gram"] = form_gram(A, At, solver, a.rounds)
            else:
                out["torch_gram"] = {"formed": "not tried: about n d^2 = "
                                               f"{n * d * d} entries"}
            At.close()
            A.close()
            if name == "uniform_d32":
                # HITS end to end on the graph pagerank is measured on
                lc, lcol, lval = with_dangling(crow, col, val, n, d, g, device)
                links = dev.CsrMatrix(lc, lcol, lval, n, solver=solver, allow_empty_rows=True)
                hs = {"empty_rows": links.empty_rows, "links": int(lval.numel())}
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                auth, hubs, sigma, it, st = solver.hits(links, eps=0.0, max_itr=a.rounds)
                torch.cuda.synchronize(device)
                hs["hits_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                hs["hits_loop_ms"] = round(float(st["loop_ms"]), 3)
                hs["rounds"] = int(st["rounds"])
                hs["sigma"] = float(sigma)
                out["hits"] = hs
                links.close()
                del lc, lcol, lval, auth, hubs
            doc["cases"][f"{dt_name}_{name}"] = out
            del crow, col, val
            torch.cuda.empty_cache()
    solver.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
