#!/usr/bin/env python3
"""The batched solve (DeviceSolver.solve_batched, one launch, a workgroup per
matrix) against the same matrices through sequential DeviceSolver.solve calls
(the single-matrix path, one launch and one round trip each).

Shapes: B in {1, 64, 1024, 4096} at 128^2 fp64 and 256^2 fp32, and 16^2 fp64
at B = 4096; seeded random matrices generated on the device.  Per shape, warm,
best of 10:

  batched_ms     host clock around solve_batched (results on the host)
  event_ms       device events around the same call (memset + kernel + the
                 call's own stream sync and state read-back)
  sequential_ms  host clock around the B solve() calls
  matrices_per_s B / batched_ms;  speedup = sequential_ms / batched_ms
  gbytes_per_s   2 B n^2 b bytes (every matrix read once, written once)
                 over event_ms

Each shape group runs in a child process under its own time limit; the first
child that fails ends the run.  Run by hand on the GPU box:

    python3 tools/bench_batched.py [--json profiles/batched_solve.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

GROUPS = {"f64_128": ("f64", 128, (1, 64, 1024, 4096)),
          "f32_256": ("f32", 256, (1, 64, 1024, 4096)),
          "f64_16": ("f64", 16, (4096,))}
GROUP_TIMEOUT_S = 240
SEED = 11


def run_group(name, reps):
    import torch
    from eigen_value_amd import device as dev
    sfx, n, batches = GROUPS[name]
    dt = torch.float64 if sfx == "f64" else torch.float32
    torch.cuda.set_device(0)
    solver = dev.DeviceSolver("cuda:0")
    rows = []
    for B in batches:
        base = dev.generate("random", n, dt, nrows=B * n, seed=SEED, device="cuda:0").view(B, n, n)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        best_b = best_e = best_s = float("inf")
        for rep in range(reps + 1):                     # rep 0 warms both paths
            a = base.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            lam, v, it, st = solver.solve_batched(a, inplace=True)
            ev[1].record()
            torch.cuda.synchronize()
            tb = time.perf_counter() - t0
            te = ev[0].elapsed_time(ev[1]) * 1e-3
            a = base.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lam_s = [solver.solve(a[b], inplace=True)[0] for b in range(B)]
            ts = time.perf_counter() - t0
            if rep:
                best_b, best_e, best_s = min(best_b, tb), min(best_e, te), min(best_s, ts)
        same = bool(torch.equal(lam, torch.tensor(lam_s, dtype=dt)))
        nbytes = 2 * B * n * n * (8 if sfx == "f64" else 4)
        rows.append({"dtype": sfx, "n": n, "batch": B, "rounds_max": st["rounds"],
                     "converged": st["converged"], "lambda_equal_to_sequential": same,
                     "batched_ms": round(best_b * 1e3, 4), "event_ms": round(best_e * 1e3, 4),
                     "sequential_ms": round(best_s * 1e3, 4),
                     "matrices_per_s": round(B / best_b, 1),
                     "sequential_matrices_per_s": round(B / best_s, 1),
                     "speedup": round(best_s / best_b, 2),
                     "gbytes_per_s": round(nbytes / best_e * 1e-9, 2)})
        print(json.dumps(rows[-1]), flush=True)
    solver.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(HERE, "profiles", "batched_solve.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--group", choices=sorted(GROUPS), default=None,
                    help="run one shape group in this process (the driver's children)")
    a = ap.parse_args()
    if a.group:
        print("ROWS " + json.dumps(run_group(a.group, a.reps)), flush=True)
        return 0
    rows = []
    for name in GROUPS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", name,
                                  "--reps", str(a.reps)], capture_output=True, text=True,
                                 timeout=GROUP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {GROUP_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 1
        got = [ln[5:] for ln in out.stdout.splitlines() if ln.startswith("ROWS ")]
        if out.returncode != 0 or not got:
            print(f"{name}: exit {out.returncode}; stopping\n{out.stderr[-2000:]}", file=sys.stderr)
            return 1
        rows += json.loads(got[0])
        for r in rows[-len(GROUPS[name][2]):]:
            print(r, flush=True)
    import eigen_value_amd
    doc = {"tool": "tools/bench_batched.py", "version": eigen_value_amd.__version__,
           "reps": a.reps, "seed": SEED,
           "note": "best of reps after one warm-up; sequential = DeviceSolver.solve per matrix",
           "rows": rows}
    json.dump(doc, open(a.json, "w"), indent=1)
    print("wrote", a.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
