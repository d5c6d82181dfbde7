#!/usr/bin/env python3
"""Per-round kernel time of the dense left-vector round against k_mfree.

One run, interleaved legs, on seeded random matrices generated on the device
(8192^2, 16384^2 and 32768^2, fp32 and fp64).  Every pass runs, in this order,

    left          st_mfree_left_round for --rounds launches (eps = 0: never
                  stops), one event pair around the three launches of each
    mfree_a / _b  st_mfree_round on the SAME matrix (the same N^2 b bytes, the
                  yardstick), twice, so that the run shows its own spread
    left_rb<R>    the left round with R rows per block through the tuning
                  build's st_set_left_rows (only when the loaded library is the
                  tuning build: run with EIGEN_VALUE_LIB pointing at it)
    solve_left    solve(A, left=True, eps = 0, max_itr = rounds) end to end:
                  wall ms, per-round kernel ms, torch's peak allocation
    transpose     A.T.contiguous() + solve(., matrix_free=True) end to end with
                  the same options: wall ms (the copy included), peak allocation

A leg's figure is the median over all its timed rounds of all passes (each
sequence's first round is left out).  The byte model of the left round is
N^2 b + 2 (N / RB) N b (the partials written and read once) plus 8 N b of
vectors (x written and read, s and v read twice, s_next and v_cur written);
k_mfree's is N^2 b + 5 N b.  Reported per case: measured left / mfree, the
model's ratio, and measured minus model in microseconds.

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

import torch  # noqa: E402

from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

PEAK_GBPS = 8000.0      # MI355X HBM3E


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_per_round": round(med, 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms),
            "gbps": round(nbytes / med / 1e6, 1),
            "frac_of_8TBs": round(nbytes / med / 1e6 / PEAK_GBPS, 4)}


def timed_rounds(launch, rounds):
    """ms of launches k = 1 .. rounds, the first left out."""
    ms = []
    for k in range(1, rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(k)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[1:]


def left_bytes(n, b, rb):
    return n * n * b + 2 * (-(-n // rb)) * n * b + 8 * n * b


def mfree_bytes(n, b):
    return n * n * b + 5 * n * b


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--sizes", default="8192,16384,32768")
    p.add_argument("--dtypes", default="f32,f64")
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--rb", default="64,128,256", help="rows per block of the A/B legs")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default="")
    a = p.parse_args()
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    L = _lib.load()
    set_rows = getattr(L, "st_set_left_rows", None) if hasattr(L, "st_set_left_rows") else None
    if set_rows is not None:
        set_rows.argtypes = [_lib.ctypes.c_uint32]
        set_rows.restype = _lib.ctypes.c_int
    solver = dev.DeviceSolver(device)
    doc = {"tool": "tools/bench_left.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_left_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "rb_ab": "st_set_left_rows" if set_rows is not None else
                    "skipped: the loaded library is not the tuning build",
           "note": "per-round kernel time, eps = 0, median over the timed rounds of all "
                   "passes without each sequence's first; left bytes N^2 b + 2 (N/RB) N b + "
                   "8 N b, mfree bytes N^2 b + 5 N b",
           "cases": {}}
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        code = _lib.DTYPE_F64 if dt_name == "f64" else _lib.DTYPE_F32
        b = 8 if dt_name == "f64" else 4
        for n in (int(x) for x in a.sizes.split(",")):
            A = dev.generate("random", n, dtype, seed=a.seed, device=device)
            s = dev.colsum(A)
            v = torch.ones(n, dtype=dtype, device=device)
            s_next, v_cur = torch.empty_like(s), torch.empty_like(v)
            rb0 = _lib.left_shape(code, n)["rows"]
            rbs = [int(x) for x in a.rb.split(",")] if set_rows is not None else []
            legs = {k: [] for k in ["left", "mfree_a", "mfree_b"] + [f"left_rb{r}" for r in rbs]}
            solves = {"solve_left": [], "transpose": []}

            def left_leg(rows):
                if set_rows is not None:
                    _lib.check(set_rows(rows), "st_set_left_rows")
                scratch = dev.left_scratch(n, dtype, device)
                state = dev.new_state(device)
                out = timed_rounds(lambda k: dev.mfree_left_round(
                    A, s, s_next, v, v_cur, scratch, state, eps=0.0, k=k, max_itr=1 << 30),
                    a.rounds)
                if set_rows is not None:
                    set_rows(0)
                return out

            def mfree_leg():
                state = dev.new_state(device)
                return timed_rounds(lambda k: dev.mfree_round(
                    A, s, s_next, v, v_cur, state, eps=0.0, k=k, max_itr=1 << 30), a.rounds)

            def solve_leg(transpose):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                if transpose:
                    At = A.T.contiguous()
                    _, _, _, st = solver.solve(At, matrix_free=True, eps=0.0, max_itr=a.rounds,
                                               time_kernels=True)
                else:
                    _, _, _, st = solver.solve(A, left=True, eps=0.0, max_itr=a.rounds,
                                               time_kernels=True)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                per_round = [float(t) for t in solver.last_round_times()][1:]
                return {"wall_ms": wall, "kernel_ms_per_round": statistics.median(per_round),
                        "peak_extra_mib": (torch.cuda.max_memory_allocated() - base) / 2**20}

            for _ in range(a.passes):
                legs["left"] += left_leg(0)
                legs["mfree_a"] += mfree_leg()
                legs["mfree_b"] += mfree_leg()
                for r in rbs:
                    legs[f"left_rb{r}"] += left_leg(r)
                solves["solve_left"].append(solve_leg(False))
                solves["transpose"].append(solve_leg(True))

            case = {"n": n, "dtype": dt_name, "matrix_mib": n * n * b / 2**20, "rows_per_block": rb0}
            case["left"] = summary(legs["left"], left_bytes(n, b, rb0))
            for k in ("mfree_a", "mfree_b"):
                case[k] = summary(legs[k], mfree_bytes(n, b))
            for r in rbs:
                case[f"left_rb{r}"] = summary(legs[f"left_rb{r}"], left_bytes(n, b, r))
            mf = min(case["mfree_a"]["ms_per_round"], case["mfree_b"]["ms_per_round"])
            ratio = left_bytes(n, b, rb0) / mfree_bytes(n, b)
            case["mfree_spread"] = round(abs(case["mfree_a"]["ms_per_round"]
                                             - case["mfree_b"]["ms_per_round"]) / mf, 4)
            case["left_over_mfree"] = round(case["left"]["ms_per_round"] / mf, 4)
            case["model_ratio"] = round(ratio, 4)
            case["measured_minus_model_us"] = round(
                (case["left"]["ms_per_round"] - mf * ratio) * 1e3, 2)
            for k, runs in solves.items():
                case[k] = {f: round(float(statistics.median(r[f] for r in runs)), 4)
                           for f in runs[0]}
            doc["cases"][f"{n}_{dt_name}"] = case
            del A, s, v, s_next, v_cur
            torch.cuda.empty_cache()
    solver.close()
    text = json.dumps(doc, indent=1, default=float)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
