#!/usr/bin/env python3
"""The rounding error of every row-sum kernel against an exact sum, in ulps,
per stage - the table behind tests/test_gpu_rowsum_exact.py, which asserts
bounds on the same figures but records nothing.

For every step-level kernel (tests/rowsum_kernels.py), dtype, semantics and
shape (tests/exact_sums.py SHAPES) and stage (total; for the flat forms also
a piece's partial sum and the sum over a row's partials): the stage's
`levels`, then max|e|, rms and signed mean of e = (s - exact) / ulp(exact)
over the rows, and the oracle's figures on the same stored matrix; pooled per
(kernel, dtype, semantics).  For circulant row blocks (every exact row sum
equal): the spread max e - min e of the kernel and of the oracle, and EPS =
1e-3f in ulps of the sum.  For the fp32 circulant solves: counts, rounds and
lambda's error through the drop-in and the device solver.  Test
infrastructure: the oracle is a checker here.

    python3 tools/rowsum_error.py --json profiles/rowsum_exact_error.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))


def rnd(d):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in d.items()}


def fig(st):
    return [round(st[k], 3) for k in ("max", "rms", "mean")]


def dump(out, f):
    """JSON with one table row per line."""
    def rows(x):
        return "[\n" + ",\n".join(json.dumps(r) for r in x) + "\n]"
    parts = []
    for k, v in out.items():
        if isinstance(v, dict) and "rows" in v:
            head = {a: b for a, b in v.items() if a != "rows"}
            body = json.dumps(head)[:-1] + ', "rows": ' + rows(v["rows"]) + "}"
        elif isinstance(v, list):
            body = rows(v)
        else:
            body = json.dumps(v)
        parts.append(json.dumps(k) + ": " + body)
    f.write("{\n" + ",\n".join(parts) + "\n}\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--json", default=None)
    p.add_argument("--no-solves", action="store_true", help="skip the whole-solve section")
    p.add_argument("--commit", default=None,
                   help="the commit the tree was built from (default: git rev-parse HEAD)")
    a = p.parse_args()
    import numpy as np
    import torch
    import eigen_value_amd as ev
    from eigen_value_amd import _lib
    from eigen_value_amd import device as dev
    from oracle import oracle as orc
    import exact_sums as xs
    import rowsum_kernels as rk
    torch.cuda.set_device(0)
    t0 = time.time()
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", HERE, "rev-parse", "--short", "HEAD"],
                                          capture_output=True, text=True).stdout.strip() or None
    except OSError:
        pass
    out = {"tool": "tools/rowsum_error.py", "st_version": _lib.load().st_version().decode(),
           "commit": commit, "unit": "ulps of the matrix dtype at the exact sum",
           "bound": "levels + 1 (tests/exact_sums.py)", "seed": xs.SEED,
           "piece_cols": {"f32": xs.piece_cols(np.float32), "f64": xs.piece_cols(np.float64)},
           "random": {"columns": ["kernel", "dtype", "semantics", "nrows", "ncols",
                                  "total", "oracle", "piece", "parts"],
                      "stage": ["levels", "max|e|", "rms", "mean"], "rows": []},
           "pooled": [],
           "circulant": {"columns": ["kernel", "dtype", "semantics", "ncols", "seed", "S",
                                     "eps_ulps", "spread_gpu", "spread_oracle", "max|e|_gpu"],
                         "blocks": "256 rows from row0 = 0, 1000, ncols - 128", "rows": []},
           "solves": []}
    dts = ((np.float32, "f32"), (np.float64, "f64"))

    # 1 / 2: random inputs, per stage, and pooled over the shapes
    inputs = {}
    for variant, sem in rk.cases():
        for dt, key in dts:
            pool = {"total": [], "oracle": []}
            for nrows, ncols in xs.SHAPES:
                if not rk.fits(variant, nrows, ncols):
                    continue
                if (key, nrows, ncols) not in inputs:
                    inputs[key, nrows, ncols] = orc.generate_c("random", ncols, xs.SEED, dt,
                                                               nrows=nrows)
                row0 = rk.block_row0(nrows, ncols) if rk.VARIANTS[variant][2] else 0
                m = rk.measure(orc, variant, inputs[key, nrows, ncols], sem, row0)
                row = [variant, key, sem, nrows, ncols]
                for stage in ("total", "oracle", "piece", "parts"):
                    row.append([m[stage]["levels"], *fig(rk.stats(m[stage]["e"]))]
                               if stage in m else None)
                out["random"]["rows"].append(row)
                pool["total"].append(m["total"]["e"])
                pool["oracle"].append(m["oracle"]["e"])
            g, o = (np.concatenate(pool[k]) for k in ("total", "oracle"))
            rec = {"kernel": variant, "dtype": key, "semantics": sem, "rows": int(g.size),
                   "gpu": rnd(rk.stats(g)), "oracle": rnd(rk.stats(o))}
            out["pooled"].append(rec)
            print(json.dumps(rec), flush=True)

    # 3: equal-sum inputs
    row0s = lambda ncols: (0, 1000, ncols - 128)          # the last runs over into row 0
    worst = {}
    for variant, sem in rk.cases():
        for dt, key in dts:
            for ncols in (4099, 6144, 8200):
                for seed in (1, 2):
                    S = xs.circulant_sum(ncols, dt, seed, orc)
                    sg, so, emax = [], [], 0.0
                    for row0 in row0s(ncols):
                        blk = xs.circulant(ncols, dt, seed, rows=(row0, 256), orc=orc)
                        r = rk.run(orc, variant, blk, sem, 0, unit=True)
                        eg = xs.err_ulps_of(r["s"], np.full(256, S), dt)
                        eo = xs.err_ulps_of(orc.rowsum(blk), np.full(256, S), dt)
                        sg.append(round(float(eg.max() - eg.min()), 3))
                        so.append(round(float(eo.max() - eo.min()), 3))
                        emax = max(emax, float(np.abs(eg).max()))
                    eps = (round(float(xs.EPS_F32) / float(xs.ulp_of(np.float64(S), dt)), 3)
                           if dt == np.float32 else None)
                    out["circulant"]["rows"].append(
                        [variant, key, sem, ncols, seed, S, eps, sg, so, round(emax, 3)])
                    worst[variant, key] = max(worst.get((variant, key), (0.0, 0.0)),
                                              *zip(sg, so))
    for (k, d), (g, o) in sorted(worst.items()):
        print(f"circulant {k} {d}: widest spread gpu {g} (oracle {o} on that block)", flush=True)

    # 4: whole solves of the fp32 circulants
    if not a.no_solves:
        forms = {"deferred": {}, "every": dict(write_every_round=True),
                 "mfree": dict(matrix_free=True)}
        solver = dev.DeviceSolver("cuda:0")
        with ev.EigenValue() as eig:
            for n, seed in xs.CIRC_CASES:
                mat = xs.circulant(n, np.float32, seed, orc=orc)
                S = xs.circulant_sum(n, np.float32, seed, orc)
                t = torch.from_numpy(mat).to("cuda:0")
                for sem in (rk.SYCL, rk.MAINPY):
                    ref = orc.similarity_transform(mat, sem)
                    for form in (forms if n in (6144, 7000) else ("deferred",)):
                        lam, _, _, it, st = eig.similarity_transform_ex(mat, semantics=sem,
                                                                        **forms[form])
                        lam2, _, it2, st2 = solver.solve(t, semantics=sem, **forms[form])
                        rec = {"n": n, "seed": seed, "semantics": sem, "form": form, "S": S,
                               "oracle": [ref.iter_count, ref.rounds_evaluated],
                               "dropin": [it, st["rounds"]], "device": [it2, st2["rounds"]],
                               "lambda_err": [round(float(xs.err_ulps_of(
                                   np.float32(x), np.float64(S), np.float32)), 3)
                                   for x in (lam, lam2)]}
                        out["solves"].append(rec)
                        print(json.dumps(rec), flush=True)
                del t
        solver.close()
    out["seconds"] = round(time.time() - t0, 1)
    if a.json:
        with open(a.json, "w") as f:
            dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
