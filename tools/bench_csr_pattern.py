#!/usr/bin/env python3
"""Per-round kernel time of the pattern-only CSR round against the values round.

One run, interleaved legs, on the matrices of tools/bench_csr.py with their
values set to 1: uniform with 8 and 32 random columns per row and the banded
one (32 per row within 2048 of the diagonal) at --n rows, and 32 per row at
--small-n rows, where the launches and not the bytes decide.  Every pass runs,
in this order,

    pattern     csr_pattern_round without scales (k_csr_prep +
                k_csr_pattern_spmv): nnz * 4 bytes of matrix
    pattern_c   the same with a column scale (k_csr_pattern_prep reads c)
    values_a    csr_mfree_round on the ones-valued CsrMatrix of the same
                structure (k_csr_prep + k_csr_spmv): nnz * (b + 4) bytes
    values_b    values_a again: the difference of the two medians is the
                run's own spread, to be read next to every ratio

each --rounds step-level rounds between a pair of events per round, on vectors
that do not stop (eps = 0).  A leg's figure is the median over all its timed
rounds of all passes (each pass's first round is left out).

The model column divides the pattern round's bytes, nnz * 4 + plan + vectors
(8 (n + 1) + 4 n + 8 n b, plus n b for c), by the values round's (tools/
bench_csr.py: nnz (b + 4) + 8 (n + 1) + 4 n + 8 n b; the x gathers are counted
in neither).

The PageRank leg: `pagerank` end to end (out-degrees, transposition, scales,
validation, the solve for --rounds rounds at eps = 0) on a CsrPattern of the
case's structure with 1 % of the rows emptied, against `pagerank` on the
ones-valued CsrMatrix of the same graph; wall-clock with a device
synchronisation at each end, the second of two calls of each.

Prints one JSON document (and writes it to --out, profiles/csr_pattern.json by
default).
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

LEGS = ("pattern", "pattern_c", "values_a", "values_b")


def pattern_bytes(n, nnz, b, with_c):
    return nnz * 4 + 8 * (n + 1) + 4 * n + 8 * n * b + (n * b if with_c else 0)


def med(ms, nbytes):
    m = statistics.median(ms)
    return {"ms_per_round": round(m, 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms), "bytes": nbytes,
            "gbps": round(nbytes / m / 1e6, 1)}


def timed_rounds(step, n, dtype, device, rounds):
    """`rounds` launches k = 1 .. rounds of one leg on ping-pong vectors, one
    event pair each; ms per round."""
    s = [torch.rand(n, dtype=dtype, device=device) + 0.5 for _ in range(2)]
    v = [torch.ones(n, dtype=dtype, device=device) for _ in range(2)]
    state = dev.new_state(device)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(rounds)]
    for k in range(1, rounds + 1):
        a, b = ev[k - 1]
        a.record()
        step(s[(k - 1) & 1], s[k & 1], v[(k - 1) & 1], v[k & 1], state, k)
        b.record()
    torch.cuda.synchronize(device)
    assert dev.read_state(state)["done"] == 0        # no round stopped: none was a no-op
    return [a.elapsed_time(b) for a, b in ev]


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--n", type=int, default=1 << 22)
    p.add_argument("--small-n", type=int, default=16384)
    p.add_argument("--dtypes", default="f32,f64")
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--alpha", type=float, default=0.85)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles",
                                                 "csr_pattern.json"))
    a = p.parse_args()
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    L = _lib.load()
    solver = dev.DeviceSolver(device)
    doc = {"tool": "tools/bench_csr_pattern.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_csr_shape_desc().decode(),
           "pattern_lib": L.st_csr_pattern_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed, "alpha": a.alpha,
           "note": "per-round kernel time of step-level rounds, eps = 0, median over the timed "
                   "rounds of all passes without each pass's first; ratio = leg / values_a; "
                   "spread = values_b / values_a; ratio_model = (nnz 4 + 8 (n + 1) + 4 n + "
                   "8 n b [+ n b]) / (nnz (b + 4) + 8 (n + 1) + 4 n + 8 n b)",
           "cases": {}}
    cases = [("uniform_d8", "uniform", a.n, 8), ("uniform_d32", "uniform", a.n, 32),
             ("banded_d32", "banded", a.n, 32), ("small_d32", "uniform", a.small_n, 32)]
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        b = 8 if dt_name == "f64" else 4
        for name, kind, n, d in cases:
            g = torch.Generator(device=device).manual_seed(a.seed)
            crow, col, val = (banded if kind == "banded" else uniform)(n, d, dtype, g, device)
            val.fill_(1.0)
            nnz = int(col.numel())
            m = dev.CsrMatrix(crow, col, val, n, solver=solver)
            pat = dev.CsrPattern(crow, col, n, dtype=dtype, solver=solver)
            cs = 0.5 + torch.rand(n, dtype=dtype, device=device, generator=g)
            pat_c = dev.CsrPattern(crow, col, n, col_scale=cs, solver=solver)
            x = torch.empty(n, dtype=dtype, device=device)
            scratch = dev.csr_pattern_scratch(pat)
            kw = dict(eps=0.0, max_itr=10 ** 6)

            def values_step(sp, sn, vp, vc, state, k):
                dev.csr_mfree_round(m, sp, sn, vp, vc, x, state, k=k, **kw)

            def step_of(handle):
                def step(sp, sn, vp, vc, state, k):
                    dev.csr_pattern_round(handle, None, sp, sn, vp, vc, scratch, state, k=k, **kw)
                return step

            steps = {"pattern": step_of(pat), "pattern_c": step_of(pat_c),
                     "values_a": values_step, "values_b": values_step}
            legs = {leg: [] for leg in LEGS}
            for _ in range(a.passes):
                for leg in LEGS:
                    legs[leg] += timed_rounds(steps[leg], n, dtype, device, a.rounds)[1:]
            base = bytes_per_round(n, nnz, b)
            out = {"n": n, "nnz": nnz}
            for leg in LEGS:
                nb = base if leg.startswith("values") else pattern_bytes(n, nnz, b,
                                                                         leg == "pattern_c")
                out[leg] = med(legs[leg], nb)
            va = out["values_a"]["ms_per_round"]
            out["spread"] = round(out["values_b"]["ms_per_round"] / va, 4)
            for leg in ("pattern", "pattern_c"):
                out[leg]["ratio_measured"] = round(out[leg]["ms_per_round"] / va, 4)
                out[leg]["ratio_model"] = round(out[leg]["bytes"] / base, 4)
            pat.close()
            pat_c.close()
            m.close()

            # PageRank end to end, both routes, the second call of each
            lc, lcol, lval = with_dangling(crow, col, val, n, d, g, device)
            del crow, col, val, x, scratch, cs
            pr = {"nnz": int(lcol.numel())}
            links_p = dev.CsrPattern(lc, lcol, n, dtype=dtype, solver=solver,
                                     allow_empty_rows=True)
            links_m = dev.CsrMatrix(lc, lcol, lval, n, solver=solver, allow_empty_rows=True)
            pr["empty_rows"] = links_p.empty_rows
            for key, links in (("pattern", links_p), ("values", links_m)):
                for _ in range(2):
                    torch.cuda.synchronize(device)
                    torch.cuda.reset_peak_memory_stats(device)
                    before = torch.cuda.memory_allocated(device)
                    t0 = time.perf_counter()
                    pi, lam, it, st = solver.pagerank(links, a.alpha, eps=0.0, max_itr=a.rounds)
                    torch.cuda.synchronize(device)
                    ms = (time.perf_counter() - t0) * 1e3
                pr[f"{key}_ms"] = round(ms, 3)
                pr[f"{key}_loop_ms"] = round(float(st["loop_ms"]), 3)
                pr[f"{key}_peak_torch_bytes"] = int(torch.cuda.max_memory_allocated(device)
                                                    - before)
                pr[f"{key}_pi"] = pi
            pr["max_abs_diff"] = float((pr.pop("pattern_pi") - pr.pop("values_pi")).abs().max())
            pr["total_ratio"] = round(pr["pattern_ms"] / pr["values_ms"], 4)
            pr["loop_ratio"] = round(pr["pattern_loop_ms"] / pr["values_loop_ms"], 4)
            pr["rounds"] = a.rounds
            out["pagerank"] = pr
            links_p.close()
            links_m.close()
            doc["cases"][f"{dt_name}_{name}"] = out
            del lc, lcol, lval, pi
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
