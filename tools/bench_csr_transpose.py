#!/usr/bin/env python3
"""Time of the device transposition of a CSR matrix (CsrMatrix.transpose).

One run, interleaved legs, on the matrices of tools/bench_csr.py (uniform d =
8 / 32 / 128, banded_d32, skewed; fp32 and fp64) with ONE change: the first
entry of every row is moved to a column of its own - a random permutation of
the rows, the diagonal for `banded` - because a random matrix of this size has
columns without any entry, which the transposition refuses.  Every pass runs,
in this order,

    transpose  CsrMatrix.transpose() of a matrix whose handle was built
               beforehand: the output tensors, the scratch, every launch and
               the plan of the result, wall clock around the synchronous call
    to_csc     torch's own conversion of the same arrays
               (sparse_csr_tensor(...).to_sparse_csc()), wall clock with a
               device synchronisation on both sides
    round      solve_csr for --rounds fixed rounds (eps = 0) with
               ST_FLAG_TIME_KERNELS, as tools/bench_csr.py times a round

A leg's figure is the median over all passes; the first pass of every leg is
left out (allocator warm-up).  `rounds_per_transpose` is the transposition in
units of one solve_csr round of the same matrix.  GB/s is the transposition
on the byte MODEL passes * nnz * 16 + nnz * (2 b + 12) - an estimate of the
traffic of an ideal radix sort with a 4-byte key and a 4-byte payload, not a
count of what these kernels move: they read the keys twice per pass, look the
source row up by bisection, and the column histogram is not in the model.

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

from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from bench_csr import banded, skewed, uniform  # noqa: E402


def passes_of(n: int, digit_bits: int) -> int:
    return -(-(n - 1).bit_length() // digit_bits)


def model_bytes(n: int, nnz: int, b: int, digit_bits: int) -> int:
    return passes_of(n, digit_bits) * nnz * 16 + nnz * (2 * b + 12)


def no_empty_column(kind, crow, col, n, g, device):
    first = crow[:-1]
    if kind == "banded":
        own = torch.arange(n, device=device, dtype=torch.int32)
    else:
        own = torch.randperm(n, device=device, generator=g).to(torch.int32)
    col[first] = own
    return col


def wall(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3, out


def med(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "timed": len(ms)}


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--n", type=int, default=1 << 22, help="rows of the uniform matrices")
    p.add_argument("--degrees", default="8,32,128")
    p.add_argument("--skew-n", type=int, default=1 << 21)
    p.add_argument("--dtypes", default="f32,f64")
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--passes", type=int, default=4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert a.passes >= 2, "the first pass of every leg is left out"
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    L = _lib.load()
    solver = dev.DeviceSolver(device)
    nnz_max, _ = _lib.csr_class_limits()
    shape = _lib.csr_transpose_shape()
    bits = shape["digit_bits"]
    doc = {"tool": "tools/bench_csr_transpose.py",
           "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(),
           "lib": L.st_csr_transpose_shape_desc().decode(),
           "csr_lib": L.st_csr_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "note": "median over the passes without the first; transpose and to_csc are wall "
                   "clock around the whole call, round is the per-round kernel time of "
                   "solve_csr (eps = 0); gbps on the MODEL passes * nnz * 16 + nnz * (2 b + "
                   "12) bytes, an estimate and not a count",
           "cases": {}}
    cases = [(f"uniform_d{d}", "uniform", a.n, int(d)) for d in a.degrees.split(",") if d]
    cases += [("banded_d32", "banded", a.n, 32), ("skewed", "skewed", a.skew_n, 0)]
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        b = 8 if dt_name == "f64" else 4
        for name, kind, n, d in cases:
            g = torch.Generator(device=device).manual_seed(a.seed)
            if kind == "skewed":
                crow, col, val = skewed(n, dtype, g, device, [int(x) for x in nnz_max])
            else:
                crow, col, val = (banded if kind == "banded" else uniform)(n, d, dtype, g, device)
            col = no_empty_column(kind, crow, col, n, g, device)
            nnz = int(val.numel())
            m = dev.CsrMatrix(crow, col, val, n, solver=solver)
            legs = {"transpose": [], "to_csc": [], "round": []}
            csc_note = None
            for _ in range(a.passes):
                ms, t = wall(lambda: m.transpose(solver), device)
                legs["transpose"].append(ms)
                t.close()
                del t
                if csc_note is None:
                    try:
                        sp = torch.sparse_csr_tensor(crow, col, val, size=(n, n))
                        ms, out = wall(sp.to_sparse_csc, device)
                        legs["to_csc"].append(ms)
                        del sp, out
                    except Exception as e:      # the comparison leg only; recorded, not hidden
                        csc_note = f"to_sparse_csc unavailable: {e}"[:200]
                _, _, _, st = solver.solve_csr(m, eps=0.0, max_itr=a.rounds, time_kernels=True)
                assert st["rounds"] == a.rounds and st["converged"] == 0
                legs["round"].append(statistics.median(
                    float(x) for x in list(solver.last_round_times())[1:]))
            nbytes = model_bytes(n, nnz, b, bits)
            tr = med(legs["transpose"][1:])
            rd = med(legs["round"][1:])
            out = {"n": n, "nnz": nnz, "digit_passes": passes_of(n, bits),
                   "model_bytes": nbytes,
                   "scratch_bytes": int(L.st_csr_transpose_scratch_bytes(n, nnz)),
                   "transpose": dict(tr, gbps_on_model=round(nbytes / tr["ms"] / 1e6, 1)),
                   "round": rd,
                   "rounds_per_transpose": round(tr["ms"] / rd["ms"], 2)}
            if len(legs["to_csc"]) > 1 and csc_note is None:
                out["to_csc"] = med(legs["to_csc"][1:])
                out["transpose_over_to_csc"] = round(tr["ms"] / out["to_csc"]["ms"], 3)
            else:
                out["to_csc"] = csc_note or "not timed"
            doc["cases"][f"{dt_name}_{name}"] = out
            print(f"{dt_name}_{name}: transpose {tr['ms']} ms, round {rd['ms']} ms",
                  file=sys.stderr, flush=True)
            m.close()
            del m, crow, col, val
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
