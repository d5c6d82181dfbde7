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

The variable-size leg (--vbatched): solve_vbatched, matrices of different n in
one call (one launch per workgroup-shape class), host to host, warm, best of
10.  fp64 with dims drawn uniformly from 8..128 (fixed seed) at B in {64, 1024,
4096} and fp32 with dims from 8..256 at B = 1024, against

  grouped_ms     the same matrices grouped by n on the host, one solve_batched
                 per distinct n, the gather (stack) and scatter (matrices, v, λ,
                 counts back to input order) copies included
  sequential_ms  one solve() per matrix

and one control: every dim 128, fp64, B = 4096 through solve_vbatched against
solve_batched on the stacked array, both measured in the same process
(vbatched_over_uniform is the price of the descriptor upload and the
indirection; the *_event_ms columns are device events around the same calls).

Each shape group runs in a child process under its own time limit; the first
child that fails ends the run.  Run by hand on the GPU box:

    python3 tools/bench_batched.py [--json profiles/batched_solve.json]
    python3 tools/bench_batched.py --rounds [--json profiles/batched_rounds.json]
    python3 tools/bench_batched.py --vbatched [--json profiles/vbatched_solve.json]
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
# name: (dtype, lowest dim, highest dim, batches); lo == hi: the control
VB_GROUPS = {"v_f64": ("f64", 8, 128, (64, 1024, 4096)),
             "v_f32": ("f32", 8, 256, (1024,)),
             "v_control": ("f64", 128, 128, (4096,))}
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


def best_of(reps, restore, call):
    """(best host-clock s, best device-event s, last result) of call() over
    `reps` timed runs after one warm-up; restore() runs untimed before each."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best_h = best_e = float("inf")
    out = None
    for rep in range(reps + 1):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        out = call()
        ev[1].record()
        torch.cuda.synchronize()
        th = time.perf_counter() - t0
        if rep:
            best_h, best_e = min(best_h, th), min(best_e, ev[0].elapsed_time(ev[1]) * 1e-3)
    return best_h, best_e, out


def run_vbatched(name, reps):
    import numpy as np
    import torch
    from eigen_value_amd import device as dev
    sfx, lo, hi, batches = VB_GROUPS[name]
    dt = torch.float64 if sfx == "f64" else torch.float32
    esz = 8 if sfx == "f64" else 4
    torch.cuda.set_device(0)
    solver = dev.DeviceSolver("cuda:0")
    rows = []
    for B in batches:
        dims = [int(x) for x in np.random.RandomState(SEED).randint(lo, hi + 1, size=B)]
        # one workspace, each matrix at a 16-byte aligned offset; `base` keeps A_0
        per16 = 16 // esz
        offs, total = [], 0
        for n in dims:
            offs.append(total)
            total += -(-n * n // per16) * per16
        base = torch.zeros(total, dtype=dt, device="cuda:0")
        for i, (o, n) in enumerate(zip(offs, dims)):
            dev.generate("random", n, dt, seed=SEED + i, out=base[o:o + n * n].view(n, n))
        flat = base.clone()
        work = [flat[o:o + n * n].view(n, n) for o, n in zip(offs, dims)]

        def restore():
            flat.copy_(base)

        tv, tve, (lam_v, vs_v, it_v, st_v) = best_of(
            reps, restore, lambda: solver.solve_vbatched(work, inplace=True))
        row = {"dtype": sfx, "batch": B, "dim_lo": lo, "dim_hi": hi, "distinct_dims": len(set(dims)),
               "class_launches": st_v["fused_launches"], "rounds_max": st_v["rounds"],
               "converged": st_v["converged"], "vbatched_ms": round(tv * 1e3, 4),
               "vbatched_event_ms": round(tve * 1e3, 4), "matrices_per_s": round(B / tv, 1)}
        if lo == hi:                                    # the control: the uniform batched solve
            stacked = flat[:B * lo * lo].view(B, lo, lo)
            tu, tue, (lam_u, v_u, it_u, st_u) = best_of(
                reps, restore, lambda: solver.solve_batched(stacked, inplace=True))
            # the C call alone (pointer and dim arrays built once, outside the
            # clock): what is left of the ratio is the Python front's per-tensor work
            import ctypes
            from eigen_value_amd import _lib
            ptrs = (ctypes.c_void_p * B)(*[w.data_ptr() for w in work])
            dims_a = np.array(dims, np.uint32)
            v = torch.empty(sum(dims), dtype=dt, device="cuda:0")
            lam, it = np.zeros(B, np.float64), np.zeros(B, np.uint32)
            stats = _lib.st_stats()
            tc, tce, rc = best_of(reps, restore, lambda: solver.L.st_solve_vbatched_f64(
                solver.q, ptrs, dims_a.ctypes.data, B, v.data_ptr(), None, lam.ctypes.data,
                it.ctypes.data, None, None, ctypes.byref(stats)))
            _lib.check(rc, "st_solve_vbatched_f64")
            row.update({"vbatched_c_call_ms": round(tc * 1e3, 4),
                        "vbatched_c_call_event_ms": round(tce * 1e3, 4),
                        "c_call_over_uniform": round(tc / tu, 3)})
            row.update({"uniform_ms": round(tu * 1e3, 4), "uniform_event_ms": round(tue * 1e3, 4),
                        "vbatched_over_uniform": round(tv / tu, 3),
                        "vbatched_over_uniform_event": round(tve / tue, 3),
                        "equal_to_uniform": bool(torch.equal(lam_v, lam_u) and torch.equal(it_v, it_u)
                                                 and torch.equal(torch.stack(vs_v), v_u))})
        else:
            by_n = {}
            for i, n in enumerate(dims):
                by_n.setdefault(n, []).append(i)
            voff = np.concatenate([[0], np.cumsum(dims)])

            def grouped():
                lam = torch.empty(B, dtype=dt)
                it = torch.empty(B, dtype=torch.int64)
                v = torch.empty(int(voff[-1]), dtype=dt, device="cuda:0")
                for n, idx in by_n.items():
                    a = torch.stack([work[i] for i in idx])             # gather
                    l, vv, k, _ = solver.solve_batched(a, inplace=True)
                    lam[idx], it[idx] = l, k
                    for j, i in enumerate(idx):                         # scatter
                        work[i].copy_(a[j])
                        v[int(voff[i]):int(voff[i + 1])].copy_(vv[j])
                return lam, it, v

            tg, _, (lam_g, it_g, v_g) = best_of(reps, restore, grouped)
            ts, _, lam_s = best_of(reps, restore,
                                   lambda: [solver.solve(w, inplace=True)[0] for w in work])
            row.update({"grouped_ms": round(tg * 1e3, 4), "sequential_ms": round(ts * 1e3, 4),
                        "speedup_vs_grouped": round(tg / tv, 2),
                        "speedup_vs_sequential": round(ts / tv, 2),
                        "equal_to_grouped": bool(torch.equal(lam_v, lam_g) and torch.equal(it_v, it_g)
                                                 and torch.equal(torch.cat(vs_v), v_g))})
        rows.append(row)
        print(json.dumps(row), flush=True)
    solver.close()
    return rows


def run_group(name, reps):
    import torch
    from eigen_value_amd import device as dev
    if name == "r_comparator":
        return run_comparator(reps)
    if name in VB_GROUPS:
        return run_vbatched(name, reps)
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
    ap.add_argument("--group", choices=sorted(GROUPS) + sorted(ROUND_GROUPS) + sorted(VB_GROUPS),
                    default=None,
                    help="run one shape group in this process (the driver's children)")
    ap.add_argument("--rounds", action="store_true",
                    help="the round-loop leg (round_loop=True); writes profiles/batched_rounds.json")
    ap.add_argument("--vbatched", action="store_true",
                    help="the variable-size leg (solve_vbatched); writes profiles/vbatched_solve.json")
    ap.add_argument("--only", default=None, help="comma-separated groups of the chosen leg")
    a = ap.parse_args()
    if a.rounds and a.json == ap.get_default("json"):
        a.json = os.path.join(HERE, "profiles", "batched_rounds.json")
    if a.vbatched and a.json == ap.get_default("json"):
        a.json = os.path.join(HERE, "profiles", "vbatched_solve.json")
    if a.group:
        print("ROWS " + json.dumps(run_group(a.group, a.reps)), flush=True)
        return 0
    rows = []
    groups = VB_GROUPS if a.vbatched else ROUND_GROUPS if a.rounds else GROUPS
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
        for r in rows[-len(groups[name][-1]):]:
            print(r, flush=True)
    import eigen_value_amd
    from eigen_value_amd import _lib
    doc = {"tool": "tools/bench_batched.py" + (" --vbatched" if a.vbatched else
                                               " --rounds" if a.rounds else ""),
           "version": eigen_value_amd.__version__,
           "probe_switches": _lib.load().st_probe_switches().decode(),
           "reps": a.reps, "seed": SEED,
           "note": ("best of reps after one warm-up, one run; grouped = one solve_batched per "
                    "distinct n with gather / scatter copies; sequential = DeviceSolver.solve per "
                    "matrix" if a.vbatched else
                    "best of reps after one warm-up; sequential = DeviceSolver.solve per matrix"),
           "rows": rows}
    json.dump(doc, open(a.json, "w"), indent=1)
    print("wrote", a.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
