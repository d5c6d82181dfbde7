#!/usr/bin/env python3
"""Per-round kernel time of the half-precision matrix-free round against the
fp32 matrix-free round of the same (widened) matrix.

One run, interleaved legs, per size n (default 8192, 16384, 32768):
a random matrix is generated in fp32 on the device (st_generate_random_f32)
and narrowed with st_narrow_f32 to fp16 and to bf16; every pass then runs, in
this order,

    fp16   solve_half(fp16 matrix)
    fp32a  solve(widened fp16 matrix, matrix_free=True)
    bf16   solve_half(bf16 matrix)
    fp32b  solve(the same widened matrix, matrix_free=True) - the fp32 leg a
           second time, so that its own run-to-run spread is on record

each for --rounds fixed rounds (eps = 0) with ST_FLAG_TIME_KERNELS; a leg's
figure is the median over all its timed rounds of all passes (each solve's
first round, which meets a cold cache, is left out).  Reported per leg: ms
per round, GB/s on N^2 * 2 bytes (for the fp32 legs too, so the columns
compare) and on the bytes the leg really reads, and the fraction of 8 TB/s.
Note that an 8192^2 half matrix is 128 MiB and sits inside the 256 MiB
memory-side cache: its rate is not an HBM rate.

--ab NAME=LIB[,NAME=LIB...] adds the A/B of launch shapes: probe builds of the
library (`make probe PROBE="-DST_HALF_ROWS=4 -DST_HALF_XVEC=1"`) timed on the
fp16 leg in the same process, interleaved with the product library pass by
pass ("lib" in the output names each one's st_half_shape_desc).

Prints one JSON document (and writes it to --out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from eigen_value_amd import _lib  # noqa: E402

PEAK_GBPS = 8000.0      # MI355X HBM3E


class Runner:
    """One library (product or probe build) and a queue of its own."""

    def __init__(self, L, dev):
        self.L, self.dev = L, dev
        self.q = ctypes.c_void_p()
        with torch.cuda.device(dev):
            L.make_queue(ctypes.byref(self.q))
        if not self.q.value:
            raise RuntimeError("make_queue failed: " + _lib.last_error(L))

    def _times(self):
        n = _lib.check(self.L.st_last_round_times(self.q, None, 0), "round_times", self.L)
        buf = (ctypes.c_float * max(1, n))()
        _lib.check(self.L.st_last_round_times(self.q, buf, n), "round_times", self.L)
        return list(buf)[:n]

    def run(self, mat, rounds):
        """`rounds` fixed rounds on `mat` (half: the half solve; float32: the
        matrix-free solve); the timed rounds' ms."""
        n = mat.shape[0]
        v = torch.empty(n, dtype=torch.float32, device=mat.device)
        ev, it = ctypes.c_float(), ctypes.c_uint32()
        opt = _lib.st_options(0.0, rounds, _lib.ST_SEM_SYCL, 0,
                              _lib.ST_FLAG_TIME_KERNELS | _lib.ST_FLAG_MATRIX_FREE)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, torch.cuda.current_stream(mat.device).cuda_stream),
                   "st_set_stream", self.L)
        if mat.dtype == torch.float32:
            rc = self.L.st_solve_device_f32(self.q, mat.data_ptr(), n, v.data_ptr(), None,
                                            ctypes.byref(ev), ctypes.byref(it), ctypes.byref(opt),
                                            ctypes.byref(stats))
        else:
            code = _lib.ST_STORE_F16 if mat.dtype == torch.float16 else _lib.ST_STORE_BF16
            rc = self.L.st_solve_device_half(self.q, code, mat.data_ptr(), n, v.data_ptr(), None,
                                             ctypes.byref(ev), ctypes.byref(it),
                                             ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "solve", self.L)
        assert stats.rounds == rounds and stats.converged == 0, (stats.rounds, stats.converged)
        return self._times(), float(ev.value)

    def close(self):
        self.L.destroy_queue(self.q)


def summary(ms, n, elem):
    med = statistics.median(ms)
    return {"ms_per_round": round(med, 5), "ms_min": round(min(ms), 5),
            "ms_max": round(max(ms), 5), "timed_rounds": len(ms),
            "gbps_on_2_bytes": round(n * n * 2 / med / 1e6, 1),
            "frac_of_8TBs_on_2_bytes": round(n * n * 2 / med / 1e6 / PEAK_GBPS, 4),
            "gbps_read": round(n * n * elem / med / 1e6, 1),
            "frac_of_8TBs_read": round(n * n * elem / med / 1e6 / PEAK_GBPS, 4)}


def narrow(L, src, dt):
    out = torch.empty(src.shape, dtype=dt, device=src.device)
    code = _lib.ST_STORE_F16 if dt == torch.float16 else _lib.ST_STORE_BF16
    _lib.check(L.st_narrow_f32(code, src.data_ptr(), out.data_ptr(), src.numel(),
                               torch.cuda.current_stream(src.device).cuda_stream),
               "st_narrow_f32", L)
    return out


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--sizes", default="8192,16384,32768")
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--ab", default="", help="NAME=LIB[,NAME=LIB...]: probe builds for the A/B")
    p.add_argument("--ab-only", action="store_true", help="skip the bf16 and fp32 legs")
    p.add_argument("--out", default="")
    a = p.parse_args()
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    L = _lib.load()
    main_run = Runner(L, dev)
    variants = {}
    for spec in filter(None, a.ab.split(",")):
        name, path = spec.split("=", 1)
        variants[name] = Runner(_lib.load(os.path.abspath(path)), dev)
    doc = {"tool": "tools/bench_half.py", "device": torch.cuda.get_device_name(dev),
           "library": L.st_version().decode(), "lib": L.st_half_shape_desc().decode(),
           "rounds": a.rounds, "passes": a.passes, "seed": a.seed,
           "input": "st_generate_random_f32 narrowed with st_narrow_f32",
           "note": "per-round kernel time (ST_FLAG_TIME_KERNELS), eps = 0, median over the "
                   "timed rounds of all passes without each solve's first; 8192^2 half is "
                   "128 MiB, inside the 256 MiB memory-side cache",
           "sizes": {}, "ab": {}}
    if variants:
        doc["ab_libs"] = {k: r.L.st_half_shape_desc().decode() for k, r in variants.items()}
    for n in [int(x) for x in a.sizes.split(",")]:
        src = torch.empty((n, n), dtype=torch.float32, device=dev)
        _lib.check(L.st_generate_random_f32(src.data_ptr(), n, n, 0, a.seed,
                                            torch.cuda.current_stream(dev).cuda_stream),
                   "generate", L)
        h16 = narrow(L, src, torch.float16)
        hb = None if a.ab_only else narrow(L, src, torch.bfloat16)
        del src
        w = None if a.ab_only else h16.float()
        legs = {"fp16": [], "fp32a": [], "bf16": [], "fp32b": []}
        ab = {k: [] for k in ("lib", *variants)}
        lam = {}
        for _ in range(a.passes):
            if not a.ab_only:
                for leg, m in (("fp16", h16), ("fp32a", w), ("bf16", hb), ("fp32b", w)):
                    ms, lam[leg] = main_run.run(m, a.rounds)
                    legs[leg] += ms[1:]
            if variants:
                for name, r in (("lib", main_run), *variants.items()):
                    ms, lam["ab_" + name] = r.run(h16, a.rounds)
                    ab[name] += ms[1:]
        out = {}
        if not a.ab_only:
            out = {leg: summary(ms, n, 4 if leg.startswith("fp32") else 2)
                   for leg, ms in legs.items()}
            f32 = [out["fp32a"]["ms_per_round"], out["fp32b"]["ms_per_round"]]
            spread = abs(f32[0] - f32[1])
            out["fp32_spread_ms"] = round(spread, 5)
            for leg in ("fp16", "bf16"):
                gain = min(f32) - out[leg]["ms_per_round"]
                out[leg]["speedup_vs_fp32"] = round(statistics.mean(f32) / out[leg]["ms_per_round"], 3)
                out[leg]["faster_than_fp32_by_ms"] = round(gain, 5)
                out[leg]["beats_fp32_beyond_spread"] = bool(gain > spread)
            out["lambda"] = {k: v for k, v in lam.items() if not k.startswith("ab_")}
            doc["sizes"][str(n)] = out
        if variants:
            doc["ab"][str(n)] = {k: summary(ms, n, 2) for k, ms in ab.items()}
            # a launch shape changes no result (a row's sum does not depend on
            # the rows grouped with it, a stored x is the product's own bits)
            assert len({lam["ab_" + k] for k in ab}) == 1, lam
        del h16, hb, w
        torch.cuda.empty_cache()
    main_run.close()
    for r in variants.values():
        r.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
