#!/usr/bin/env python3
"""Per-round kernel time of the sparse (CSR) matrix-free round.

One run, interleaved legs.  Matrices are generated on the device from a
seeded torch generator: `uniform` ones with d = 8, 32 and 128 entries per row
(random columns, duplicates allowed, values in (0, 1]) at an n where the
arrays exceed the 256 MiB memory-side cache, and one `skewed` matrix whose row
lengths are log-normal with a few rows beyond the workgroup class's limit, so
that every row class is populated; `banded_d32` is uniform_d32 with every
column within 2048 of the diagonal, the case where neighbouring rows' gathers
share cache lines.  Every pass runs, in this order,

    csr       solve_csr for --rounds fixed rounds (eps = 0) with
              ST_FLAG_TIME_KERNELS: both launches of a round between the events
    torch_mv  torch.mv on the same arrays as a torch.sparse_csr tensor (the
              vendor's SpMV, one round's dominant work), one event pair per call

and, for the `dense` case (an n where both run), the dense matrix_free=True
round on the densified matrix instead of torch_mv.  A leg's figure is the
median over all its timed rounds of all passes (each solve's first round is
left out).  GB/s counts nnz * (b + 4) + 8 (n + 1) bytes of matrix, 4 n of the
plan and 8 n b of vector traffic (x written and read once, s, v read twice,
s_next and v_cur written); the x gathers are not counted.

Prints one JSON document (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

PEAK_GBPS = 8000.0      # MI355X HBM3E


def uniform(n, d, dtype, g, device):
    crow = torch.arange(n + 1, dtype=torch.int64, device=device) * d
    col = torch.randint(0, n, (n * d,), device=device, generator=g, dtype=torch.int32)
    val = 1.0 - torch.rand(n * d, device=device, generator=g, dtype=dtype)
    return crow, col, val


def banded(n, d, dtype, g, device, half_width=2048):
    """uniform's shape with every column within half_width of the diagonal
    (mod n): the gathers of neighbouring rows share cache lines."""
    crow, col, val = uniform(n, d, dtype, g, device)
    rows = torch.arange(n, device=device, dtype=torch.int64).repeat_interleave(d)
    col = ((rows + col.long() % (2 * half_width + 1) - half_width) % n).to(torch.int32)
    return crow, col, val


def skewed(n, dtype, g, device, limits):
    """Log-normal row lengths (median 12), and 64 rows at 1.5 x the last limit."""
    lens = torch.exp(2.5 + 1.5 * torch.randn(n, device=device, generator=g))
    lens = lens.clamp(1, 1.5 * limits[-2]).to(torch.int64)
    lens[:: max(1, n // 64)] = int(1.5 * limits[-2])
    crow = torch.zeros(n + 1, dtype=torch.int64, device=device)
    crow[1:] = torch.cumsum(lens, 0)
    nnz = int(crow[-1])
    col = torch.randint(0, n, (nnz,), device=device, generator=g, dtype=torch.int32)
    val = 1.0 - torch.rand(nnz, device=device, generator=g, dtype=dtype)
    return crow, col, val


def bytes_per_round(n, nnz, b):
    return nnz * (b + 4) + 8 * (n + 1) + 4 * n + 8 * n * b


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_per_round": round(med, 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms),
            "gbps": round(nbytes / med / 1e6, 1),
            "frac_of_8TBs": round(nbytes / med / 1e6 / PEAK_GBPS, 4)}


def time_mv(sp, x, rounds):
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.mv(sp, x)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--n", type=int, default=1 << 22, help="rows of the uniform matrices")
    p.add_argument("--degrees", default="8,32,128")
    p.add_argument("--skew-n", type=int, default=1 << 21)
    p.add_argument("--dense-n", type=int, default=16384)
    p.add_argument("--dense-d", type=int, default=32)
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
    nnz_max, lanes = _lib.csr_class_limits()
    doc = {"tool": "tools/bench_csr.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_csr_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "note": "per-round kernel time, eps = 0, median over the timed rounds of all "
                   "passes without each solve's first; gbps on nnz (b + 4) + 8 (n + 1) + 4 n "
                   "+ 8 n b bytes for the csr leg and the torch_mv leg alike",
           "cases": {}}
    cases = [(f"uniform_d{d}", "uniform", a.n, int(d)) for d in a.degrees.split(",")]
    cases += [("banded_d32", "banded", a.n, 32), ("skewed", "skewed", a.skew_n, 0),
              ("dense", "uniform", a.dense_n, a.dense_d)]
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        b = 8 if dt_name == "f64" else 4
        for name, kind, n, d in cases:
            g = torch.Generator(device=device).manual_seed(a.seed)
            if kind == "skewed":
                crow, col, val = skewed(n, dtype, g, device, [int(x) for x in nnz_max])
            else:
                crow, col, val = (banded if kind == "banded" else uniform)(n, d, dtype, g, device)
            nnz = int(val.numel())
            m = dev.CsrMatrix(crow, col, val, n, solver=solver)
            _, first = m.plan()
            other, other_name = None, "torch_mv"
            if name == "dense":
                other_name = "dense_mfree"
                other = torch.zeros((n, n), dtype=dtype, device=device)
                rows = torch.repeat_interleave(torch.arange(n, device=device), torch.diff(crow))
                other.index_put_((rows, col.long()), val, accumulate=True)
            else:
                try:
                    other = torch.sparse_csr_tensor(crow.to(torch.int32), col, val, size=(n, n))
                    torch.mv(other, torch.ones(n, dtype=dtype, device=device))
                    torch.cuda.synchronize(device)
                except Exception as e:      # the comparison leg only; recorded, not hidden
                    other, other_name = None, f"torch_mv unavailable: {e}"[:200]
            legs = {"csr": [], "other": []}
            x = torch.rand(n, dtype=dtype, device=device) + 0.5
            for _ in range(a.passes):
                _, _, _, st = solver.solve_csr(m, eps=0.0, max_itr=a.rounds, time_kernels=True)
                assert st["rounds"] == a.rounds and st["converged"] == 0
                legs["csr"] += list(solver.last_round_times())[1:]
                if name == "dense":
                    solver.solve(other, eps=0.0, max_itr=a.rounds, time_kernels=True,
                                 matrix_free=True)
                    legs["other"] += list(solver.last_round_times())[1:]
                elif other is not None:
                    legs["other"] += time_mv(other, x, a.rounds)[1:]
            nbytes = bytes_per_round(n, nnz, b)
            out = {"n": n, "nnz": nnz, "bytes_per_round": nbytes,
                   "rows_per_class": {str(int(l)): int(first[i + 1] - first[i])
                                      for i, l in enumerate(lanes)},
                   "csr": summary([float(t) for t in legs["csr"]], nbytes)}
            if legs["other"]:
                key = "dense_mfree" if name == "dense" else "torch_mv"
                out[key] = summary([float(t) for t in legs["other"]],
                                   n * n * b if name == "dense" else nbytes)
                out["csr_over_" + key] = round(out["csr"]["ms_per_round"]
                                               / out[key]["ms_per_round"], 3)
            else:
                out["other"] = other_name
            doc["cases"][f"{dt_name}_{name}"] = out
            m.close()
            del m, other, crow, col, val, x
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
