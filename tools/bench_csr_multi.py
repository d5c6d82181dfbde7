#!/usr/bin/env python3
"""Per-round time of the multi-column CSR round against C single rounds, and
personalised PageRank end to end.

One run, interleaved legs, on the matrices of tools/bench_csr.py: uniform
ones with 8 and 32 random columns per row and the banded one (32 per row
within 2048 of the diagonal) at --n rows, and 32 per row at --small-n rows,
where the launches and not the bytes decide.  K = 1.  Every pass runs, for C =
1, 2, 4, 8 in this order,

    multi     --rounds calls of csr_multi_round (k_csrm_prep + k_csrm_dots +
              k_csrm_spmv: one pass over the matrix for the C columns)
    seq       --rounds times C calls of csr_terms_round, one per column (the
              kernels the library always had): the yardstick, in the same run

each round between two events on the stream, eps = 0 (no column ever stops),
the vectors ping-ponging as in a solve from K0's row sums.  A leg's figure is
the median over all its timed rounds of all passes (each leg's first round of
a pass is left out).

Next to each ratio multi / seq stands what the byte model predicts:
    multi  nnz (b + 4) + 8 (n + 1) + 4 n + CP (8 n b + 2 K n b)
    seq    C (nnz (b + 4) + 8 (n + 1) + 4 n + 8 n b + 2 K n b + 2 K G b)
(the x gathers are not counted in either: they are what the packing changes).

The PageRank leg: the case's graph with 1 % of the rows emptied (dangling
nodes); `pagerank_multi` with 8 seeded teleports end to end against 8
`pagerank` calls, both for --rounds rounds at eps = 0, wall-clock with a device
synchronisation at each end.

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

from bench_csr import banded, bytes_per_round, uniform  # noqa: E402
from bench_csr_terms import terms_bytes, with_dangling  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

COLUMNS = (1, 2, 4, 8)
K = 1


def multi_bytes(n, nnz, b, cp):
    return nnz * (b + 4) + 8 * (n + 1) + 4 * n + cp * (8 * n * b + 2 * K * n * b)


def med(ms):
    return {"ms_per_round": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms)}


def timed(fn, rounds, stream):
    """ms of each of `rounds` calls fn(j), events around each."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(rounds)]
    for j, (a, b) in enumerate(ev):
        a.record(stream)
        fn(j)
        b.record(stream)
    torch.cuda.synchronize()
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
    p.add_argument("--out", default="")
    a = p.parse_args()
    device = torch.device(a.device)
    torch.cuda.set_device(device)
    stream = torch.cuda.current_stream(device)
    L = _lib.load()
    solver = dev.DeviceSolver(device)
    doc = {"tool": "tools/bench_csr_multi.py", "device": torch.cuda.get_device_name(device),
           "library": L.st_version().decode(), "lib": L.st_csr_shape_desc().decode(),
           "multi_lib": L.st_csr_multi_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed, "alpha": a.alpha, "K": K,
           "note": "per-round time between stream events, eps = 0, median over the timed "
                   "rounds of all passes without each leg's first; multi = one csr_multi_round, "
                   "seq = C csr_terms_round calls; ratio = multi / seq; bytes_multi = nnz (b + 4) "
                   "+ 8 (n + 1) + 4 n + CP (8 n b + 2 K n b), bytes_seq = C x the single round's",
           "cases": {}}
    cases = [("uniform_d8", "uniform", a.n, 8), ("uniform_d32", "uniform", a.n, 32),
             ("banded_d32", "banded", a.n, 32), ("small_d32", "uniform", a.small_n, 32)]
    for dt_name in a.dtypes.split(","):
        dtype = torch.float64 if dt_name == "f64" else torch.float32
        b = 8 if dt_name == "f64" else 4
        for name, kind, n, d in cases:
            g = torch.Generator(device=device).manual_seed(a.seed)
            crow, col, val = (banded if kind == "banded" else uniform)(n, d, dtype, g, device)
            nnz = int(val.numel())
            m = dev.CsrMatrix(crow, col, val, n, solver=solver)
            uw = 0.5 / n * (1.0 + torch.rand((2, 8, n), device=device, generator=g, dtype=dtype))
            singles = [dev.CsrTerms(m, [uw[0, c]], [uw[1, c]], solver=solver) for c in range(8)]
            s_scr = singles[0].scratch()
            sbuf = [torch.empty(n, dtype=dtype, device=device) for _ in range(2)]
            vbuf = [torch.ones(n, dtype=dtype, device=device) for _ in range(2)]
            single_bytes = bytes_per_round(n, nnz, b) + terms_bytes(n, K, b)
            out = {"n": n, "nnz": nnz, "bytes_single_round": single_bytes}
            for C in COLUMNS:
                mt = dev.CsrMultiTerms(m, uw[0, :C], uw[1, :C], solver=solver)
                m_scr = mt.scratch()
                ms_buf = [mt.packed(), mt.packed()]
                mv_buf = [mt.packed(), mt.packed()]
                legs = {"multi": [], "seq": []}
                for _ in range(a.passes):
                    states, fin = mt.new_states()
                    dev.csr_multi_rowsum(m, mt, m_scr, out=ms_buf[0])
                    mv_buf[0].fill_(1.0)

                    def multi(j):
                        dev.csr_multi_round(m, mt, ms_buf[j & 1], ms_buf[(j + 1) & 1],
                                            mv_buf[j & 1], mv_buf[(j + 1) & 1], m_scr, states, fin,
                                            eps=0.0, k=j + 1, max_itr=1000)

                    legs["multi"] += timed(multi, a.rounds, stream)[1:]
                    assert int(fin.item()) == 0
                    sstates = [dev.new_state(device) for _ in range(C)]
                    dev.csr_terms_rowsum(m, singles[0], s_scr, out=sbuf[0])
                    vbuf[0].fill_(1.0)

                    def seq(j):
                        # every column from the same vectors: the traffic of C rounds; the
                        # last call's outputs carry the iteration on
                        for c in range(C):
                            dev.csr_terms_round(m, singles[c], sbuf[j & 1], sbuf[(j + 1) & 1],
                                                vbuf[j & 1], vbuf[(j + 1) & 1], s_scr, sstates[c],
                                                eps=0.0, k=j + 1, max_itr=1000)

                    legs["seq"] += timed(seq, a.rounds, stream)[1:]
                e = {"CP": mt.CP, "multi": med(legs["multi"]), "seq": med(legs["seq"])}
                e["bytes_multi"] = multi_bytes(n, nnz, b, mt.CP)
                e["bytes_seq"] = C * single_bytes
                e["multi"]["gbps"] = round(e["bytes_multi"] / e["multi"]["ms_per_round"] / 1e6, 1)
                e["seq"]["gbps"] = round(e["bytes_seq"] / e["seq"]["ms_per_round"] / 1e6, 1)
                e["ratio_measured"] = round(e["multi"]["ms_per_round"]
                                            / e["seq"]["ms_per_round"], 4)
                e["ratio_model"] = round(e["bytes_multi"] / e["bytes_seq"], 4)
                out[f"C{C}"] = e
                mt.close()
                del mt, m_scr, ms_buf, mv_buf
                torch.cuda.empty_cache()
            for t in singles:
                t.close()
            m.close()
            del sbuf, vbuf, s_scr

            # personalised PageRank end to end: 8 teleports against 8 pagerank calls
            lc, lcol, lval = with_dangling(crow, col, val, n, d, g, device)
            del crow, col, val
            links = dev.CsrMatrix(lc, lcol, lval, n, solver=solver, allow_empty_rows=True)
            T = 0.5 + torch.rand((8, n), device=device, generator=g, dtype=dtype)
            pr = {"empty_rows": links.empty_rows, "nnz": int(lval.numel()), "teleports": 8}
            for leg in ("multi", "calls", "multi", "calls"):      # the second pair is kept
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                if leg == "multi":
                    Pi, _, _, st = solver.pagerank_multi(links, a.alpha, teleports=T, eps=0.0,
                                                         max_itr=a.rounds)
                    loop = float(st["loop_ms"])
                else:
                    rows, loop = [], 0.0
                    for c in range(8):
                        pi, _, _, st = solver.pagerank(links, a.alpha, teleport=T[c], eps=0.0,
                                                       max_itr=a.rounds)
                        rows.append(pi)
                        loop += float(st["loop_ms"])
                torch.cuda.synchronize(device)
                pr[f"{leg}_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                pr[f"{leg}_loop_ms"] = round(loop, 3)
            pr["same_bits"] = bool(torch.equal(Pi, torch.stack(rows)))
            pr["multi_over_calls"] = round(pr["multi_ms"] / pr["calls_ms"], 4)
            pr["loop_multi_over_calls"] = round(pr["multi_loop_ms"] / pr["calls_loop_ms"], 4)
            out["pagerank"] = pr
            links.close()
            doc["cases"][f"{dt_name}_{name}"] = out
            del lc, lcol, lval, uw, T, Pi, rows
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
