#!/usr/bin/env python3
"""Per-round kernel time of the dense pair round against the two rounds it
replaces (k_mfree + the left round) on the same matrix.

One run, interleaved legs, on seeded random matrices generated on the device
(8192^2, 16384^2 and 32768^2, fp32 and fp64).  Every pass runs, in this order,

    pair              st_mfree_pair_round for --rounds launches (eps = 0: never
                      stops), one event pair around the five launches of each
    mfree_a, left_a   st_mfree_round and st_mfree_left_round on the SAME matrix:
    mfree_b, left_b   the yardstick is their SUM, taken twice so that the run
                      shows its own spread
    solve_pair        solve_pair(A, eps = 0, max_itr = rounds) end to end, wall ms
    two_solves        solve(A, matrix_free=True) then solve(A, left=True) with the
                      same options, wall ms

A leg's figure is the median over all its timed rounds of all passes (each
sequence's first round is left out).  Byte models, b bytes per element:

    pair    N^2 b (1 + 2 / RB + 2 / S) for the matrix and both sets of partials
            (written and read once), + (N / RB) N b for x_R read once per tile,
            + 16 N b of vectors (per side: s, v read and x written by the prep;
            x, s, v read and s_next, v_cur written by the finish)
    mfree   N^2 b + 5 N b           (tools/bench_left.py's)
    left    N^2 b + 2 (N / RB) N b + 8 N b

Reported per case: measured pair / yardstick (the smaller of the two), the
model's ratio, measured minus model in microseconds, the spread of the two
yardstick legs, and `pair_faster`: true only when the pair round's median is
below the smaller yardstick by more than the difference of the two.

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


def pair_bytes(n, b, rb, strip):
    nrb, ns = -(-n // rb), -(-n // strip)
    return n * n * b + 2 * nrb * n * b + 2 * ns * n * b + nrb * n * b + 16 * n * b


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--sizes", default="8192,16384,32768")
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
    doc = {"tool": "tools/bench_pair.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_pair_shape_desc().decode(),
           "lib_left": L.st_left_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "note": "per-round kernel time, eps = 0, median over the timed rounds of all "
                   "passes without each sequence's first; yardstick = mfree + left on the same "
                   "matrix in the same run, twice; pair bytes N^2 b (1 + 2/RB + 2/S) + (N/RB) N b "
                   "+ 16 N b, mfree bytes N^2 b + 5 N b, left bytes N^2 b + 2 (N/RB) N b + 8 N b",
           "cases": {}}
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        code = _lib.DTYPE_F64 if dt_name == "f64" else _lib.DTYPE_F32
        b = 8 if dt_name == "f64" else 4
        for n in (int(x) for x in a.sizes.split(",")):
            A = dev.generate("random", n, dtype, seed=a.seed, device=device)
            s_r, s_l = dev.pair_sum(A)
            v = torch.ones(n, dtype=dtype, device=device)
            nxt = [torch.empty_like(v) for _ in range(4)]     # s_next, v_cur per side
            sh = _lib.pair_shape(code, n)
            rb, strip = sh["rows"], sh["strip"]
            legs = {k: [] for k in ("pair", "mfree_a", "left_a", "mfree_b", "left_b")}
            solves = {"solve_pair": [], "two_solves": []}

            def pair_leg():
                scratch = dev.pair_scratch(n, dtype, device)
                states = torch.zeros(128, dtype=torch.uint8, device=device)
                return timed_rounds(lambda k: dev.mfree_pair_round(
                    A, (s_r, nxt[0], v, nxt[1]), (s_l, nxt[2], v, nxt[3]), scratch, states,
                    eps=0.0, k=k, max_itr=1 << 30), a.rounds)

            def left_leg():
                scratch = dev.left_scratch(n, dtype, device)
                state = dev.new_state(device)
                return timed_rounds(lambda k: dev.mfree_left_round(
                    A, s_l, nxt[2], v, nxt[3], scratch, state, eps=0.0, k=k, max_itr=1 << 30),
                    a.rounds)

            def mfree_leg():
                state = dev.new_state(device)
                return timed_rounds(lambda k: dev.mfree_round(
                    A, s_r, nxt[0], v, nxt[1], state, eps=0.0, k=k, max_itr=1 << 30), a.rounds)

            def solve_leg(pair):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if pair:
                    solver.solve_pair(A, eps=0.0, max_itr=a.rounds)
                else:
                    solver.solve(A, matrix_free=True, eps=0.0, max_itr=a.rounds)
                    solver.solve(A, left=True, eps=0.0, max_itr=a.rounds)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            solve_leg(True), solve_leg(False)                 # workspaces and code objects
            for _ in range(a.passes):
                legs["pair"] += pair_leg()
                legs["mfree_a"] += mfree_leg()
                legs["left_a"] += left_leg()
                legs["mfree_b"] += mfree_leg()
                legs["left_b"] += left_leg()
                solves["solve_pair"].append(solve_leg(True))
                solves["two_solves"].append(solve_leg(False))

            case = {"n": n, "dtype": dt_name, "matrix_mib": n * n * b / 2**20,
                    "rows_per_block": rb, "strip_cols": strip, "nt": sh["nt"]}
            case["pair"] = summary(legs["pair"], pair_bytes(n, b, rb, strip))
            for k in ("mfree_a", "mfree_b"):
                case[k] = summary(legs[k], mfree_bytes(n, b))
            for k in ("left_a", "left_b"):
                case[k] = summary(legs[k], left_bytes(n, b, rb))
            ya = case["mfree_a"]["ms_per_round"] + case["left_a"]["ms_per_round"]
            yb = case["mfree_b"]["ms_per_round"] + case["left_b"]["ms_per_round"]
            yard = min(ya, yb)
            pm = case["pair"]["ms_per_round"]
            ratio = pair_bytes(n, b, rb, strip) / (mfree_bytes(n, b) + left_bytes(n, b, rb))
            case["yardstick_a_ms"] = round(ya, 5)
            case["yardstick_b_ms"] = round(yb, 5)
            case["yardstick_spread"] = round(abs(ya - yb) / yard, 4)
            case["pair_over_yardstick"] = round(pm / yard, 4)
            case["model_ratio"] = round(ratio, 4)
            case["measured_minus_model_us"] = round((pm - yard * ratio) * 1e3, 2)
            case["pair_faster"] = bool(pm < yard and (yard - pm) > abs(ya - yb))
            for k, runs in solves.items():
                case[k + "_wall_ms"] = round(float(statistics.median(runs)), 4)
            case["solve_pair_over_two_solves"] = round(
                case["solve_pair_wall_ms"] / case["two_solves_wall_ms"], 4)
            doc["cases"][f"{n}_{dt_name}"] = case
            del A, s_r, s_l, v, nxt
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
