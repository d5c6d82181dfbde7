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

The round-loop leg (--rounds): solve_batched(round_loop=True), one launch per
round for the whole batch (k_round_batched), for matrices beyond one
workgroup's registers.  Shapes: 256^2, 512^2, 1024^2, 2048^2 fp64 and 512^2
fp32 at B in {1, 16, 64, 256}, against the same sequential solve() calls, host
to host, warm, best of 10; gbytes_per_s is 2 B n^2 b rounds_max bytes over
event_ms.  It ends with the comparator: the per-round kernel time of
64 x 512^2 fp64 next to one k_round round of a single 4096^2 fp64 matrix (the
same 128 MiB), both as (t(72 rounds) - t(8 rounds)) / 64 of eps = 0 solves
enqueued in one go, device events around the call.

Each shape group runs in a child process under its own time limit; the first
child that fails ends the run.  Run by hand on the GPU box:

    python3 tools/bench_batched.py [--json profiles/batched_solve.json]
    python3 tools/bench_batched.py --rounds [--json profiles/batched_rounds.json]
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
ROUND_GROUPS = {"r_f64_256": ("f64", 256, (1, 16, 64, 256)),
                "r_f64_512": ("f64", 512, (1, 16, 64, 256)),
                "r_f64_1024": ("f64", 1024, (1, 16, 64, 256)),
                "r_f64_2048": ("f64", 2048, (1, 16, 64, 256)),
                "r_f32_512": ("f32", 512, (1, 16, 64, 256)),
                "r_comparator": ("f64", 512, (64,))}
GROUP_TIMEOUT_S = 240
SEED = 11


def per_round_ms(call, reps, k_lo=8, k_hi=72):
    """Kernel time of one round: eps = 0 solves of k_lo and k_hi rounds, every
    round enqueued before the first host check, device events around the
    call; (best t(k_hi) - best t(k_lo)) / (k_hi - k_lo)."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = {}
    for k in (k_lo, k_hi):
        best[k] = float("inf")
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            ev[0].record()
            call(k)
            ev[1].record()
            torch.cuda.synchronize()
            if rep:
                best[k] = min(best[k], ev[0].elapsed_time(ev[1]))
    return (best[k_hi] - best[k_lo]) / (k_hi - k_lo)


def run_comparator(reps):
    """64 x 512^2 fp64 per batched round against one k_round round of a single
    4096^2 fp64 matrix: the same 128 MiB.  (The matrices keep being
    transformed from call to call; eps = 0 never stops and the transform keeps
    them finite.)"""
    import torch
    from eigen_value_amd import device as dev
    torch.cuda.set_device(0)
    solver = dev.DeviceSolver("cuda:0")
    dt = torch.float64
    mats = dev.generate("random", 512, dt, nrows=64 * 512, seed=SEED, device="cuda:0").view(64, 512, 512)
    one = dev.generate("random", 4096, dt, seed=SEED, device="cuda:0")
    b_ms = per_round_ms(lambda k: solver.solve_batched(mats, inplace=True, round_loop=True, eps=0.0,
                                                       max_itr=k, batch=k), reps)
    s_ms = per_round_ms(lambda k: solver.solve(one, inplace=True, eps=0.0, max_itr=k, batch=k), reps)
    solver.close()
    row = {"comparator": "64 x 512^2 f64 batched round vs one k_round round of 4096^2 f64",
           "bytes_per_round": 2 * 4096 * 4096 * 8,
           "batched_round_ms": round(b_ms, 5), "single_4096_round_ms": round(s_ms, 5),
           "ratio_batched_over_single": round(b_ms / s_ms, 3),
           "batched_gbytes_per_s": round(2 * 4096 * 4096 * 8 / b_ms * 1e-6, 1),
           "single_gbytes_per_s": round(2 * 4096 * 4096 * 8 / s_ms * 1e-6, 1)}
    print(json.dumps(row), flush=True)
    return [row]


def run_group(name, reps):
    import torch
    from eigen_value_amd import device as dev
    if name == "r_comparator":
        return run_comparator(reps)
    rounds_leg = name in ROUND_GROUPS
    sfx, n, batches = (ROUND_GROUPS if rounds_leg else GROUPS)[name]
    kw = {"round_loop": True} if rounds_leg else {}
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
            lam, v, it, st = solver.solve_batched(a, inplace=True, **kw)
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
        nbytes = 2 * B * n * n * (8 if sfx == "f64" else 4) * (st["rounds"] if rounds_leg else 1)
        rows.append({"dtype": sfx, "n": n, "batch": B, "rounds_max": st["rounds"],
                     **({"round_launches": st["fused_launches"]} if rounds_leg else {}),
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
    ap.add_argument("--group", choices=sorted(GROUPS) + sorted(ROUND_GROUPS), default=None,
                    help="run one shape group in this process (the driver's children)")
    ap.add_argument("--rounds", action="store_true",
                    help="the round-loop leg (round_loop=True); writes profiles/batched_rounds.json")
    ap.add_argument("--only", default=None, help="comma-separated groups of the chosen leg")
    a = ap.parse_args()
    if a.rounds and a.json == ap.get_default("json"):
        a.json = os.path.join(HERE, "profiles", "batched_rounds.json")
    if a.group:
        print("ROWS " + json.dumps(run_group(a.group, a.reps)), flush=True)
        return 0
    rows = []
    groups = ROUND_GROUPS if a.rounds else GROUPS
    if a.only:
        groups = {g: groups[g] for g in a.only.split(",")}
    for name in groups:
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
        for r in rows[-len(groups[name][2]):]:
            print(r, flush=True)
    import eigen_value_amd
    from eigen_value_amd import _lib
    doc = {"tool": "tools/bench_batched.py" + (" --rounds" if a.rounds else ""),
           "version": eigen_value_amd.__version__,
           "probe_switches": _lib.load().st_probe_switches().decode(),
           "reps": a.reps, "seed": SEED,
           "note": "best of reps after one warm-up; sequential = DeviceSolver.solve per matrix",
           "rows": rows}
    json.dump(doc, open(a.json, "w"), indent=1)
    print("wrote", a.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
