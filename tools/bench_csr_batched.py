#!/usr/bin/env python3
"""Host-to-host time of the batched sparse (stacked CSR) solve against the
same matrices solved one after the other.

One process, interleaved legs, wall clock around calls that return after the
stream completed, best of --reps (default 10) with the first pass of each
shape left out as warm-up.  Matrices are generated on the device from a seeded
torch generator, make_csr's shape: d random columns per row (duplicates
allowed), values in (0, 1].  Legs of a shape, run in this order inside every
pass:

    batched     solve_csr_batched on a CsrBatch built beforehand
    sequential  solve_csr on each of the B CsrMatrix handles built beforehand,
                same solver (same stream), same options
    vbatched    fp32 shapes with every n <= 256 only: solve_vbatched on the
                densified matrices

Creation is timed apart, once per pass: one CsrBatch(...) against B
CsrMatrix(...) calls.  The iteration counts of both legs are compared (they
must be equal: the batched solve is bit-identical).  Shapes: B = 64, 1024, 4096
of n = 1024 with 16 per row; B = 1024 of n = 256 with 16 per row (the vbatched
comparison); B = 1024 with n drawn from 64 .. 4096 and 8 .. 32 per row; and the
control B = 1, n = 4194304, 8 per row.

Prints one JSON document (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402


def make_batch(dims, degs, dtype, g, device):
    """Stacked arrays of len(dims) matrices: matrix b has dims[b] rows of
    degs[b] entries each.  (mat_first numpy, crow, col, val)."""
    dims_t = torch.as_tensor(dims, dtype=torch.int64, device=device)
    degs_t = torch.as_tensor(degs, dtype=torch.int64, device=device)
    n_of_row = torch.repeat_interleave(dims_t, dims_t)
    d_of_row = torch.repeat_interleave(degs_t, dims_t)
    crow = torch.zeros(n_of_row.numel() + 1, dtype=torch.int64, device=device)
    crow[1:] = torch.cumsum(d_of_row, 0)
    nnz = int(crow[-1])
    n_of_entry = torch.repeat_interleave(n_of_row, d_of_row)
    col = (torch.randint(0, 2**31 - 1, (nnz,), device=device, generator=g, dtype=torch.int64)
           % n_of_entry).to(torch.int32)
    val = 1.0 - torch.rand(nnz, device=device, generator=g, dtype=dtype)
    mat_first = np.concatenate([[0], np.cumsum(dims)]).astype(np.uint32)
    return mat_first, crow, col, val


def single_arrays(mat_first, crow, col, val):
    """Per matrix (crow rebased to 0, col, val, n): int64 / int32 / dtype
    tensors, so that CsrMatrix converts nothing.  Made outside the timed
    region: the create leg times st_csr_create and its Python wrapper only."""
    ptr = crow.cpu().numpy()
    out = []
    for b in range(len(mat_first) - 1):
        lo, hi = int(mat_first[b]), int(mat_first[b + 1])
        e0, e1 = int(ptr[lo]), int(ptr[hi])
        out.append(((crow[lo:hi + 1] - e0).contiguous(), col[e0:e1], val[e0:e1], hi - lo))
    return out


def singles_of(arrays, solver):
    return [dev.CsrMatrix(c, i, v, n, solver=solver) for c, i, v, n in arrays]


def densified(mat_first, crow, col, val):
    out = []
    ptr = crow.cpu().numpy()
    for b in range(len(mat_first) - 1):
        lo, hi = int(mat_first[b]), int(mat_first[b + 1])
        e0, e1 = int(ptr[lo]), int(ptr[hi])
        n = hi - lo
        a = torch.zeros((n, n), dtype=val.dtype, device=val.device)
        rows = torch.repeat_interleave(torch.arange(n, device=val.device),
                                       torch.diff(crow[lo:hi + 1]))
        a.index_put_((rows, col[e0:e1].long()), val[e0:e1], accumulate=True)
        out.append(a)
    return out


def wall(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3, r


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--shapes", default="b64,b1024,b4096,small,mixed,control")
    p.add_argument("--dtype", default="f32")
    p.add_argument("--max-itr", type=int, default=1000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default="")
    a = p.parse_args()
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    dtype = torch.float64 if a.dtype == "f64" else torch.float32
    L = _lib.load()
    solver = dev.DeviceSolver(device)
    rng = np.random.default_rng(a.seed)
    shapes = {
        "b64": ([1024] * 64, [16] * 64),
        "b1024": ([1024] * 1024, [16] * 1024),
        "b4096": ([1024] * 4096, [16] * 4096),
        "small": ([256] * 1024, [16] * 1024),
        "mixed": (rng.integers(64, 4097, size=1024).tolist(),
                  rng.integers(8, 33, size=1024).tolist()),
        "control": ([1 << 22], [8]),
    }
    doc = {"tool": "tools/bench_csr_batched.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "csr_shape": L.st_csr_shape_desc().decode(),
           "batch_shape": L.st_csr_batch_shape_desc().decode(), "dtype": a.dtype,
           "reps": a.reps, "seed": a.seed, "max_itr": a.max_itr,
           "note": "host-to-host wall ms, best of reps after one warm-up pass, legs "
                   "interleaved in one process; creation timed apart",
           "cases": {}}
    for name in a.shapes.split(","):
        dims, degs = shapes[name]
        B = len(dims)
        g = torch.Generator(device=device).manual_seed(a.seed)
        mat_first, crow, col, val = make_batch(dims, degs, dtype, g, device)
        with_vb = dtype == torch.float32 and max(dims) <= 256
        dense = densified(mat_first, crow, col, val) if with_vb else None
        arrays = single_arrays(mat_first, crow, col, val)
        t = {"batched": [], "sequential": [], "vbatched": [], "create_batched": [],
             "create_sequential": []}
        its_b = its_s = None
        rounds = launches = 0
        for rep in range(a.reps + 1):
            ms_cb, bt = wall(lambda: dev.CsrBatch(crow, col, val, mat_first, solver=solver),
                             device)
            ms_cs, ones = wall(lambda: singles_of(arrays, solver), device)
            ms_b, rb = wall(lambda: solver.solve_csr_batched(bt, max_itr=a.max_itr), device)
            ms_s, rs = wall(lambda: [solver.solve_csr(m, max_itr=a.max_itr) for m in ones],
                            device)
            if with_vb:
                ms_v, _ = wall(lambda: solver.solve_vbatched(dense, max_itr=a.max_itr), device)
            its_b = [int(x) for x in rb[2]]
            its_s = [int(r[2]) for r in rs]
            rounds, launches = rb[4]["rounds"], rb[4]["fused_launches"]
            assert its_b == its_s, "batched and sequential iteration counts differ"
            assert all(float(rb[0][i]) == float(rs[i][0]) for i in range(B))
            bt.close()
            for m in ones:
                m.close()
            if rep == 0:
                continue
            t["batched"].append(ms_b)
            t["sequential"].append(ms_s)
            t["create_batched"].append(ms_cb)
            t["create_sequential"].append(ms_cs)
            if with_vb:
                t["vbatched"].append(ms_v)
        out = {"batch": B, "n_min": int(min(dims)), "n_max": int(max(dims)),
               "rows": int(mat_first[-1]), "nnz": int(val.numel()),
               "per_row_min": int(min(degs)), "per_row_max": int(max(degs)),
               "iterations_min": min(its_b), "iterations_max": max(its_b),
               "rounds": rounds, "rounds_enqueued": launches}
        for k, v in t.items():
            if v:
                out[k + "_ms"] = round(min(v), 4)
                out[k + "_ms_median"] = round(float(np.median(v)), 4)
        out["sequential_over_batched"] = round(out["sequential_ms"] / out["batched_ms"], 2)
        out["create_sequential_over_batched"] = round(out["create_sequential_ms"]
                                                      / out["create_batched_ms"], 2)
        if with_vb:
            out["vbatched_over_batched"] = round(out["vbatched_ms"] / out["batched_ms"], 2)
        doc["cases"][name] = out
        print(name, json.dumps(out), flush=True)
        del crow, col, val, dense, arrays
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
