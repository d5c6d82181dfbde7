#!/usr/bin/env python3
"""Benchmark of the similarity-transform round (BASELINE.json `metric`).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--n N0]
                    [--kind hilbert|random] [--dtype f64|f32] [--strong] [--one-gpu]
                    [--dump-outputs DIR]
                    [--full [--no-cpu] [--no-north-star] [--no-headline]]

A plain run does what the headline figure needs and no more: it generates
the matrix, runs W warm-up rounds, times K rounds and prints the line
(`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, the
workload's `config`, and at N = 1 the `roofline` of the same timed rounds).
`--dump-outputs DIR` also writes what the last timed round left (λ, the
eigenvector, the row sums, the matrix or a fixed seeded sample of it) as
DIR/<name>.npy; the inputs come from fixed seeds, so two builds run with
the same arguments can be compared file by file.  Every other leg listed
under "Extra objects" below runs only with `--full`.

One *step* = one round of the hot path on the HBM-resident matrix: the
single fused launch (max / eigenvector update / stop test of s_k, then
A_{k+1} = D^-1 A_k D in place and its row sums) that moves 2*N^2*b bytes
(read A_k, write A_{k+1}), plus, for N > 1 GPUs, the all-gather of the
row-sum vector.  The stop tolerance is set to 0 inside the timed region so
that every one of the K rounds does the full work (after convergence the
reference would stop; a fixed round count is how SURVEY.md §8d prices
ms/iteration).

Launch: `--gpus N` with N > 1 runs one process per GPU.  Under
torch.distributed.run (WORLD_SIZE set) this process is one rank; without it
this process starts the N ranks itself (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_ADDR=127.0.0.1 / a free MASTER_PORT in their environment) and exits
with their status, never touching a GPU itself.

Workload (config.workload): BASELINE.json configs[1], 8192x8192 Hilbert
fp64 on one GPU.  For N GPUs the row-block sharded path runs with per-GPU
bytes held constant (weak scaling): n = 8192*sqrt(N) rounded to a multiple
of 64*N, rows split in contiguous blocks, one RCCL all-gather per round.
`--strong` keeps n fixed instead.  `value` = algorithmic bytes of all ranks
/ max-over-ranks time (GB/s); `ms_per_step` = ms/iteration.

Extra objects on the JSON line (`--full` only, but for the N = 1 roofline):
  roofline         the round's kernels (HIP events on the launch stream)
  round_distribution  (N = 1) per-round HIP-event times of a second pass of
                   the same schedule (first / median / max, first and last
                   5) and the GPU's clock levels around both passes
  solve            the reference-semantics solve to convergence (rounds, λ)
  matrix_free      the read-only form of the iteration,
                   priced against its own N^2*b bytes
  configs3_strong  (N > 1) BASELINE configs[3]: 65536^2 random fp64,
                   rows_per_gpu = 65536/N, one all-gather per round, checked
                   against the oracle's solve and the P = 1 count
  configs3_p1      (N = 1) the same matrix on one GPU: the strong-scaling
                   anchor (also `configs3_p1_ms_per_iteration`), and
                   `rank_blocks`: rank 0's block at P = 2, 4, 8 timed alone
                   (no all-gather) - the compute side of the curve
  weak_rank_blocks (N = 1) rank 0's block of the N = 2, 4, 8 headline
                   timed alone (no all-gather)
  north_star       (N = 1) 32768^2 random fp64, both forms
  configs4_f32     (N = 1) 32768^2 random fp32: every-round roofline, the
                   deferred-write rounds, the fp32-vs-fp64 tolerance study
  deferred_writes  (N = 1) the solve loop's form (A stored every m-th
                   round, bit-identical), timed with HIP events over whole
                   store cycles, priced against (m+1)/m*N^2*b
  reference_headline  the reference's own published whole-solve table
  cpu_baseline     the oracle's 3-pass schedule on every host core
`--one-gpu` (all ranks on cuda:0, a plumbing rehearsal) marks the line
"representative": false and drops every roofline fraction.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MALL_BYTES = 256 << 20  # memory-side (Infinity) cache
# fp64 Hilbert 8192, reference semantics (cyclic, EPS=1e-3): 17 rounds,
# λ = 2.5999921826283514 (CPU oracle; README.md:76 publishes 17 rounds)
HILBERT8192_F64 = (17, 2.5999921826283514)
BIG = 2 ** 31           # max_itr of the timed rounds (never reached)


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--n", type=int, default=8192, help="matrix size at N=1 GPU")
    p.add_argument("--kind", default="hilbert", choices=["hilbert", "random"])
    p.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    p.add_argument("--full", action="store_true",
                   help="beside the headline, run every other leg: the reference-semantics "
                        "solve, the per-round distribution, the matrix-free form, the rank "
                        "blocks, the full-size legs, the published fp32 comparison, the CPU "
                        "baseline and (N > 1) the overlapped exchange and configs[3]; "
                        "the --no-* options below trim a --full run")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed round left "
                        "(DIR/<name>.npy: eigen_val, eigen_vec, row_sums, the matrix or a "
                        "fixed seeded sample of it)")
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--no-north-star", action="store_true",
                   help="skip the full-size legs (north_star, configs3, configs4_f32, "
                        "deferred_writes, the CPU's 32768^2 sample)")
    p.add_argument("--no-configs3", action="store_true",
                   help="skip the 65536^2 configs[3] leg")
    p.add_argument("--no-headline", action="store_true",
                   help="skip the fp32 whole-solve comparison with the published numbers")
    p.add_argument("--cpu-seconds", type=float, default=15.0,
                   help="CPU baseline sample length (rounds are calibrated to it)")
    p.add_argument("--strong", action="store_true",
                   help="keep n fixed for every N (strong scaling)")
    p.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                   help="torch.distributed backend for N > 1 (nccl = RCCL over xGMI)")
    p.add_argument("--overlap", action="store_true",
                   help="N > 1: time the overlapped exchange (split round, all-gather on a "
                        "second stream) as the headline instead of an extra leg")
    p.add_argument("--no-overlap-leg", action="store_true",
                   help="N > 1: skip the extra overlapped-exchange leg")
    p.add_argument("--stall-timeout", type=float, default=300.0,
                   help="N > 1: seconds without progress after which a rank gives up "
                        "(and the self-spawning parent ends the run) naming its last leg")
    p.add_argument("--stall-rank", type=int, default=None, help=argparse.SUPPRESS)  # test hook
    p.add_argument("--stall-in", default="barrier", choices=["barrier", "rendezvous"],
                   help=argparse.SUPPRESS)  # test hook: where the other ranks wait
    p.add_argument("--comm-timeout", type=float, default=None,
                   help="seconds each rank waits for its peers when the library's RCCL "
                        "communicator is made (st_set_comm_timeout; default "
                        "ST_COMM_TIMEOUT_S or 120)")
    p.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # child mode
    p.add_argument("--leg-args", default="{}", help=argparse.SUPPRESS)
    p.add_argument("--one-gpu", action="store_true",
                   help="rehearsal: every rank on cuda:0 (use with --backend gloo); the "
                        "line is marked non-representative")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------
# launch
# ---------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


HEARTBEAT_ENV = "ST_BENCH_HEARTBEAT"   # directory of per-rank progress files
STALL_EXIT = 124                       # exit status of a run ended for no progress


def _last_legs(hb_dir: str, n: int) -> dict:
    """rank -> the last progress line it reported (heartbeat files)."""
    out = {}
    for r in range(n):
        try:
            with open(os.path.join(hb_dir, f"rank{r}")) as f:
                out[r] = json.load(f)["leg"]
        except (OSError, ValueError, KeyError):
            out[r] = "(nothing reported)"
    return out


def spawn_ranks(n: int, argv, stall_timeout: float) -> int:
    """Start the N ranks of `bench.py argv` as child processes (this parent
    never initialises a GPU) and return the worst exit status.  A rank that
    fails ends the others (by their own PIDs).  No-progress deadline: every
    rank writes its progress lines to a heartbeat file; if no rank has
    exited and none has reported for `stall_timeout` + 30 s (each rank's
    own watchdog gives up after `stall_timeout`), the ranks are ended and
    the parent exits with STALL_EXIT.  Either way, a failed run prints the
    leg each rank last reported."""
    import tempfile
    port = _free_port()
    hb_dir = tempfile.mkdtemp(prefix="st_bench_hb_")
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env[HEARTBEAT_ENV] = hb_dir
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv],
                                      env=env))
    rcs = [None] * n
    t_start = time.time()
    stalled = False

    def end_all():
        for i, pr in enumerate(procs):
            if rcs[i] is None:
                pr.terminate()
        for i, pr in enumerate(procs):
            if rcs[i] is None:
                try:
                    rcs[i] = pr.wait(timeout=30)
                except subprocess.TimeoutExpired:
                    pr.kill()
                    rcs[i] = pr.wait()

    while any(rc is None for rc in rcs):
        for i, pr in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = pr.poll()
        if any(rc not in (None, 0) for rc in rcs):
            end_all()
            break
        last = t_start
        for r in range(n):
            try:
                last = max(last, os.path.getmtime(os.path.join(hb_dir, f"rank{r}")))
            except OSError:
                pass
        if all(rc is None for rc in rcs) and time.time() - last > stall_timeout + 30:
            stalled = True
            end_all()
            break
        time.sleep(0.2)
    bad = [rc for rc in rcs if rc != 0]
    if stalled or bad:
        legs = _last_legs(hb_dir, n)
        why = (f"no rank reported progress for {stall_timeout + 30:.0f} s" if stalled
               else f"exit statuses {rcs}")
        print(f"bench.py: {n}-rank run failed ({why}); last reported per rank:", file=sys.stderr)
        for r in range(n):
            print(f"bench.py:   rank {r} (exit {rcs[r]}): {legs[r]}", file=sys.stderr)
        sys.stderr.flush()
    import shutil
    shutil.rmtree(hb_dir, ignore_errors=True)
    if stalled:
        return STALL_EXIT
    return (bad[0] if bad[0] > 0 else 1) if bad else 0


_T0 = time.perf_counter()


_BEAT = {"t": time.monotonic(), "leg": "start"}


def progress(msg: str) -> None:
    """One line on stderr per finished leg (rank 0 only): long multi-rank
    runs show they are alive, and a log shows where a failed run stopped.
    Every rank also records it as its heartbeat (the watchdog below, and the
    self-spawning parent's heartbeat file)."""
    _BEAT["t"], _BEAT["leg"] = time.monotonic(), msg
    hb = os.environ.get(HEARTBEAT_ENV)
    if hb:
        path = os.path.join(hb, f"rank{os.environ.get('RANK', '0')}")
        try:
            with open(path + ".tmp", "w") as f:
                json.dump({"leg": msg, "t": time.time()}, f)
            os.replace(path + ".tmp", path)
        except OSError:
            pass
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench {time.perf_counter() - _T0:7.1f} s] {msg}", file=sys.stderr, flush=True)


def start_watchdog(timeout: float) -> None:
    """N > 1: a rank that reports no progress for `timeout` seconds (a peer
    that never arrives at a collective, an RCCL or topology stall) prints
    where it stopped and exits with STALL_EXIT, so the launcher
    (torch.distributed.run, or spawn_ranks) ends the other ranks and the
    run fails with the leg named instead of burning the step limit."""
    import threading

    def watch():
        while True:
            time.sleep(1.0)
            idle = time.monotonic() - _BEAT["t"]
            if idle > timeout:
                print(f"bench.py: rank {os.environ.get('RANK', '0')}: no progress for "
                      f"{idle:.0f} s after '{_BEAT['leg']}' (--stall-timeout {timeout:.0f}); "
                      "giving up", file=sys.stderr, flush=True)
                os._exit(STALL_EXIT)

    threading.Thread(target=watch, name="bench-watchdog", daemon=True).start()


def scaled_n(n1: int, world: int) -> int:
    if world == 1:
        return n1
    q = 64 * world
    return int(round(n1 * math.sqrt(world) / q)) * q


# ---------------------------------------------------------------------------
# committed evidence read by the line
# ---------------------------------------------------------------------------
def true_lambda(n, dtype, seed):
    """Committed CPU Perron root (tests/golden/large_pins.json) or None."""
    path = os.path.join(HERE, "tests", "golden", "large_pins.json")
    try:
        for c in json.load(open(path))["cases"]:
            if (c["n"], c["dtype"], c["seed"]) == (n, dtype, seed):
                return c["lambda"]
    except (OSError, ValueError, KeyError):
        pass
    return None


def oracle_pin(name):
    """The oracle's solve of a full-size seeded input
    (tests/golden/large_oracle.json, make_large_oracle.py) or None."""
    try:
        return json.load(open(os.path.join(HERE, "tests", "golden",
                                           "large_oracle.json")))["cases"][name]
    except (OSError, ValueError, KeyError):
        return None


def load_traffic(workload: str, kernel: str = "k_round"):
    """Per-launch HBM bytes of a hot kernel from the committed rocprofv3 PMC
    passes of this workload (profiles/*_pmc.json, tools/pmc_traffic.py;
    FETCH_SIZE and WRITE_SIZE from separate passes, FETCH_SIZE doubled per
    the gfx950 correction).  The latest round's file wins."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(HERE, "profiles", "*_pmc.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload") != workload:
            continue
        for e in d.get("entries", []):
            if e.get("kernel") == kernel:
                best = (e["hbm_bytes_per_launch"], os.path.relpath(f, HERE))
    return best


def cw_bound(torch, a0, v, lam):
    """Bound on |λ - λ_true| / λ from the Collatz–Wielandt bracket of a
    positive matrix: λ_true lies in [min, max] of (A0 v)_i / v_i."""
    q = torch.mv(a0, v.to(a0.dtype)) / v.to(a0.dtype)
    lo, hi = q.min().item(), q.max().item()
    return max(abs(lam - lo), abs(lam - hi)) / abs(lam)


def cgroup_cpu_quota():
    """CPUs' worth of time the cgroup grants this process (cpu.max on v2,
    cpu.cfs_quota_us / cpu.cfs_period_us on v1), or None if unlimited."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else int(q) / int(per)
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def host_info() -> dict:
    """The host the CPU baseline runs on.  `threads` = every CPU this
    process may actually use: the affinity mask, bounded by the cgroup's
    CPU quota and by OMP_NUM_THREADS when the environment sets it (the GPU
    box's lease exposes all 256 CPUs in the mask but grants a 16-CPU share:
    256 OpenMP threads there ran 55x slower than 16)."""
    model = None
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    aff = len(os.sched_getaffinity(0))
    quota = cgroup_cpu_quota()
    omp = os.environ.get("OMP_NUM_THREADS")
    threads = aff
    if quota is not None:
        threads = min(threads, max(1, int(math.ceil(quota))))
    if omp and omp.isdigit() and int(omp) > 0:
        threads = min(threads, int(omp))
    return {"cpu_model": model, "nproc": os.cpu_count(), "affinity_cpus": aff,
            "cgroup_cpu_quota": quota, "omp_num_threads": omp, "threads": threads}


def gpu_clocks(torch, index: int = 0):
    """The GPU's current shader / memory / fabric clock levels, read from the
    amdgpu driver's sysfs files of this device's PCI function (the starred
    line of pp_dpm_sclk / pp_dpm_mclk / pp_dpm_fclk); None where unreadable."""
    try:
        pr = torch.cuda.get_device_properties(index)
        pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
    except Exception:   # noqa: BLE001 - no PCI identity: no reading
        return None
    out = {"pci": pci}
    for key in ("sclk", "mclk", "fclk"):
        try:
            lines = open(f"/sys/bus/pci/devices/{pci}/pp_dpm_{key}").read().splitlines()
            cur = [ln for ln in lines if ln.rstrip().endswith("*")]
            out[key] = cur[0].split(":", 1)[-1].replace("*", "").strip() if cur else None
        except OSError:
            out[key] = None
    return out


def round_distribution(sh, kind, steps, warmup, torch):
    """Per-round HIP-event times of a second pass of the bench's exact
    schedule (fresh A_0, W warm-up rounds, K rounds), one event between
    rounds: whether the first timed rounds run slower than the rest (a ramp
    inside a short K) shows here.  A separate pass, so that the events
    between rounds stay out of the timed region whose K rounds give
    `value`."""
    sh.load(kind)
    cool_down(torch)
    clk0 = gpu_clocks(torch, torch.cuda.current_device())
    sh.start()
    for _ in range(warmup):
        sh.round(0.0, BIG)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for k in range(steps):
        sh.round(0.0, BIG)
        ev[k + 1].record()
    torch.cuda.synchronize()
    clk1 = gpu_clocks(torch, torch.cuda.current_device())
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(steps)]
    srt = sorted(ms)
    return {"first": round(ms[0], 5), "median": round(srt[len(srt) // 2], 5),
            "max": round(srt[-1], 5), "min": round(srt[0], 5),
            "mean": round(sum(ms) / len(ms), 5), "first5": [round(x, 5) for x in ms[:5]],
            "last5": [round(x, 5) for x in ms[-5:]],
            "clocks_before": clk0, "clocks_after": clk1,
            "timing": ("a second pass of the same schedule (fresh A_0, W warm-up rounds, "
                       "K rounds) with a HIP event between rounds; not the timed region")}


# ---------------------------------------------------------------------------
# timing
# ---------------------------------------------------------------------------
def _max_over_ranks(torch, dist, world, *vals):
    if world == 1:
        return vals
    t = torch.tensor(vals, dtype=torch.float64,
                     device="cuda" if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return tuple(float(x) for x in t)


CLOCKS = {}   # GPU clock levels around the headline's timed region (rank 0, N = 1)


def timed_rounds(sh, steps, warmup, torch, dist, world, clocks_key=None, after=None,
                 launch_pass=True):
    """Warmup + K timed rounds; returns (elapsed_s_max, kernel_ms_avg).
    `after(sh)` runs right behind the timed region, on the state its last
    round left (--dump-outputs); launch_pass=False leaves out the N > 1
    per-launch pass below (kernel_ms_avg is then None).

    The kernel's average launch duration comes from HIP events recorded on
    the launch stream (torch's current stream, which the C-ABI launches on).
    At N = 1 the timed region holds nothing but the round launches, so two
    events bracket it (per-launch events would add ~7 us of event work to
    every 175 us round).  With N > 1 the all-gathers sit between launches:
    the timed region runs without events, and a separate pass after it
    brackets each launch with its own pair for the kernel average."""
    cool_down(torch)
    # the clock levels are read before the warm-up rounds, not at t0, so the
    # amdgpu sysfs read (an SMU query) stays out of the timed region
    if clocks_key:
        CLOCKS[clocks_key + "_before"] = gpu_clocks(torch, torch.cuda.current_device())
    sh.start()
    sh.rounds(warmup, 0.0, BIG)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if world == 1:
        ev[0][0].record()
    # the K rounds through pre-resolved launches (sh.rounds: round()'s
    # kernels, arguments and all-gather, without its per-call Python work)
    sh.rounds(steps, 0.0, BIG)
    if world == 1:
        ev[0][1].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if clocks_key:
        CLOCKS[clocks_key + "_after"] = gpu_clocks(torch, torch.cuda.current_device())
    if after is not None:
        after(sh)
    if world == 1:
        return el, ev[0][0].elapsed_time(ev[0][1]) / steps
    if not launch_pass:
        return _max_over_ranks(torch, dist, world, el) + (None,)
    n_ev = min(steps, 50)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(n_ev)]
    for k in range(n_ev):
        sh.round(0.0, BIG, events=ev[k])
    torch.cuda.synchronize()
    fused = sum(a.elapsed_time(b) for a, b in ev) / n_ev
    return _max_over_ranks(torch, dist, world, el, fused)


def timed_deferred(sh, cycles, warm_cycles, torch, dist, world):
    """The deferred-write loop over whole store cycles: rounds k0 .. k0 +
    cycles*m - 1 with k0 a multiple of m, i.e. starting on the first round
    after a store (no pending scaling) and ending on a storing round, no
    flush inside.  Returns (elapsed_s_max, event_ms_per_round, m) — HIP
    events bracket the cycles on the launch stream."""
    cool_down(torch)
    sh.deferred_start()
    m = sh._defer_m
    for _ in range(warm_cycles * m):
        sh.deferred_round(0.0, BIG)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(cycles * m):
        sh.deferred_round(0.0, BIG)
    e1.record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    ev_ms = e0.elapsed_time(e1) / (cycles * m)
    el, ev_ms = _max_over_ranks(torch, dist, world, el, ev_ms)
    return el, ev_ms, m


def deferred_bitwise(sh, kind, seed, torch):
    """2m rounds from A_0 with deferred writes and with a store every round:
    λ, v and the final matrix bit for bit (P = 1)."""
    m = sh._defer_m
    sh.load(kind, seed=seed)
    sh.deferred_start()
    for _ in range(2 * m):
        sh.deferred_round(0.0, BIG)
    st_d = sh.ops.read_state(sh.state)
    a_d, v_d = sh.mat.clone(), sh.v.clone()
    sh.load(kind, seed=seed)
    sh.start()
    for _ in range(2 * m):
        sh.round(0.0, BIG)
    st_e = sh.ops.read_state(sh.state)
    same = (st_d["eigen_val"] == st_e["eigen_val"] and torch.equal(v_d, sh.v)
            and torch.equal(a_d, sh.mat))
    del a_d, v_d
    return bool(same)


def profile_cycle_ms(workload: str):
    """The committed rocprof kernel time per round of the deferred-write
    loop for `workload`, from a kernel trace of this bench's own deferred
    leg (profiles/*_defer_bench_*.json, tools/defer_profile.py --bench-leg:
    k_flat + k_parts of the timed cycles, median pass of 3, each from a
    fresh A_0 - the procedure the leg times with HIP events).  The latest
    round's file wins; (ms per round, path, the trace's own slowdown of the
    leg's HIP-event time or None) or None."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(HERE, "profiles", "*_defer_bench_*.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        for blk in d.get("blocks", []):
            if blk.get("workload") == workload:
                best = (blk["rocprof_ms_per_round"], os.path.relpath(f, HERE),
                        blk.get("trace_slowdown"))
    return best


def add_rocprof(out: dict, workload: str, ev_ms: float, by: float) -> None:
    """The rocprof figure of the same procedure beside a deferred leg's
    HIP-event one (profile_cycle_ms), and its roofline fraction."""
    prof = profile_cycle_ms(workload)
    if prof is not None:
        out["rocprof_ms_per_round"] = prof[0]
        out["rocprof_frac"] = round(rate(by, prof[0]) / HBM_PEAK_GBS, 4)
        out["rocprof_source"] = prof[1]
        out["events_vs_rocprof"] = round(ev_ms / prof[0], 4)
        if prof[2]:
            # kernel tracing slows short rounds itself (a completion signal
            # and timestamps per dispatch): the same leg untraced on the
            # profiling box, so the two untraced figures compare directly
            out["rocprof_trace_slowdown"] = prof[2]
            out["events_vs_rocprof_untraced"] = round(ev_ms * prof[2] / prof[0], 4)


# ---------------------------------------------------------------------------
# legs
# ---------------------------------------------------------------------------
def rate(bytes_, ms):
    return bytes_ / (ms * 1e-3) / 1e9


COOL_S = float(os.environ.get("BENCH_COOL_S", "0"))


def cool_down(torch):
    """Idle before a leg's timed region (BENCH_COOL_S seconds): each leg
    of a long bench starts from a comparable thermal state instead of
    inheriting the clock the previous leg's streaming left behind."""
    if COOL_S > 0:
        torch.cuda.synchronize()
        time.sleep(COOL_S)


DUMP_MATRIX_ELEMS = 1 << 22   # elements of the matrix written by --dump-outputs (<= 32 MiB)
DUMP_SEED = 20240229          # the sample's positions: the same for every run


def dump_outputs(path, sh, np_, torch, rank):
    """--dump-outputs DIR: what the last timed round left on the device, i.e.
    what a caller of the round path holds after it - λ (eigen_val), the
    eigenvector (eigen_vec), the row sums s_{k+1} of the transformed block
    (row_sums) and the block itself (matrix; blocks of more than
    DUMP_MATRIX_ELEMS elements as the values at a fixed seeded set of sorted
    flat positions) - as DIR/<name>.npy in the bench's own precision.  The
    inputs are generated from fixed seeds, so two builds run with the same
    arguments are comparable file by file.  Every rank takes part (the
    eigenvector is gathered); rank 0 writes, its own block for N > 1."""
    p = sh.part
    torch.cuda.synchronize()
    v = sh.eigen_vector()
    flat = sh.mat.reshape(-1)
    if flat.numel() > DUMP_MATRIX_ELEMS:
        pos = np_.sort(np_.random.default_rng(DUMP_SEED).integers(
            0, flat.numel(), size=DUMP_MATRIX_ELEMS, dtype=np_.int64))
        flat = flat[torch.from_numpy(pos).to(flat.device)]
    npdt = np_.float64 if sh.dtype == torch.float64 else np_.float32
    arrays = {"eigen_val": np_.array([sh.ops.read_state(sh.state)["eigen_val"]], dtype=npdt),
              "eigen_vec": v.cpu().numpy().astype(npdt, copy=False),
              "row_sums": sh.s[sh.cur][:p.n].cpu().numpy().astype(npdt, copy=False),
              "matrix": flat.cpu().numpy().astype(npdt, copy=False)}
    if rank == 0:
        os.makedirs(path, exist_ok=True)
        for name, arr in arrays.items():
            np_.save(os.path.join(path, name + ".npy"), arr)


def configs3_leg(sharded, torch, dist, world, rank, steps, warmup, representative):
    """BASELINE configs[3]: 65536^2 random fp64 row-block sharded over the
    world (P = 1: the whole 32 GiB on one GPU), one all-gather per round:
    the reference-semantics solve checked against the oracle's solve of the
    same matrix (tests/golden/large_oracle.json: iteration count = the P = 1
    count, λ) and the true Perron root, then K timed every-round steps and
    whole store cycles of the solve loop's deferred-write form."""
    n = 65536
    sh = sharded.ShardedSimilarityTransform(n, torch.float64)
    p = sh.part
    sh.load("random", seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lam, v, it, rounds = sh.solve(eps=1e-3, max_itr=1000, batch=1)
    torch.cuda.synchronize()
    solve_ms = (time.perf_counter() - t0) * 1e3
    progress(f"configs[3] 65536^2 over {world}: solve {it} iterations ({solve_ms:.1f} ms)")
    pin, perron = oracle_pin("random65536_f64"), true_lambda(n, "f64", 0)
    check = {}
    if pin is not None:
        check.update(oracle_iter_count=pin["iter_count"],
                     iter_count_equal=it == pin["iter_count"],
                     eigen_val_rel_err_vs_oracle=abs(lam - pin["eigen_val"]) / pin["eigen_val"])
    if perron is not None:
        check["eigen_val_rel_err_vs_true"] = abs(lam - perron) / perron
    sh.load("random", seed=0)
    el, fused = timed_rounds(sh, steps, warmup, torch, dist, world)
    by_total, by_local = 2.0 * n * n * 8, 2.0 * p.nrows * n * 8
    leg = {"workload": "random65536_f64", "n": n, "rows_per_gpu": p.chunk, "n_gpus": world,
           "ms_per_iteration": round(el / steps * 1e3, 4), "steps": steps,
           "value": round(by_total * steps / el / 1e9, 2), "unit": "GB/s",
           "bytes_per_round": by_total,
           "kernel_ms_avg": round(fused, 4), "achieved": round(rate(by_local, fused), 1),
           "solve": {"iter_count": it, "rounds_evaluated": rounds, "eigen_val": lam,
                     "ms": round(solve_ms, 2), "check": check}}
    if representative:
        leg["frac"] = round(rate(by_local, fused) / HBM_PEAK_GBS, 4)
    if sh.deferred_writes:
        el_d, ev_d, m = timed_deferred(sh, 4, 1, torch, dist, world)
        by_d = (m + 1.0) / m * n * n * 8
        leg["deferred_writes"] = {"stores_every": m,
                                  "ms_per_iteration": round(el_d / (4 * m) * 1e3, 4),
                                  "event_ms_per_round": round(ev_d, 4),
                                  "value": round(rate(by_d, el_d / (4 * m) * 1e3), 2),
                                  "bytes_per_round": by_d}
    if sh.rccl is not None:
        leg["rccl_ranks"] = sh.rccl.info()["nranks"]
    if world > 1:
        from eigen_value_amd import _lib
        leg["rccl_version"] = _lib.rccl_info()["rccl_version"]
    sh.close()
    del sh, v
    torch.cuda.empty_cache()
    return leg


def rank_block_legs(sharded, torch, cases, kind, steps, warmup, representative):
    """Per-rank work of a P-way row-block partition on this one GPU, for
    each (P, n) in `cases`: rank 0's block (ceil(n/P) rows x n columns)
    through the same round launches a rank runs - every-round steps and
    whole store cycles of the deferred-write solve - WITHOUT the all-gather
    (the other ranks' row sums stay 1.0): the compute side of a scaling
    curve, not a multi-GPU measurement."""
    out = {}
    for P, n in cases:
        sh = sharded.ShardedSimilarityTransform(n, torch.float64, rank_block=(P, 0))
        p = sh.part
        sh.load(kind, seed=0)
        el, fused = timed_rounds(sh, steps, warmup, torch, None, 1)
        by = 2.0 * p.nrows * n * 8
        r = {"rows": p.nrows, "cols": n, "block_gib": round(p.nrows * n * 8 / 2 ** 30, 2),
             "ms_per_iteration": round(el / steps * 1e3, 4), "kernel_ms_avg": round(fused, 4),
             "achieved": round(rate(by, fused), 1)}
        if representative:
            r["frac"] = round(rate(by, fused) / HBM_PEAK_GBS, 4)
        if sh.deferred_writes:
            # ~60 ms of whole store cycles, three passes, the median, each
            # pass from a fresh A_0 (a block timed alone holds the other
            # ranks' row sums at 1.0, so its off-block columns shrink every
            # round and the memory-side cache streams the decayed values
            # faster or slower: round 4's passes without the reload read
            # 0.1015 / 0.1039 / 0.1040 ms on the P = 4 block; round 3 timed 4
            # cycles once, 7 % above the A/B tool's figure)
            cycles = max(3, int(round(60.0 / max(el / steps * 1e3, 1e-3) / 6)))

            def one_pass():
                sh.load(kind, seed=0)
                return timed_deferred(sh, cycles, 1, torch, None, 1)
            runs = sorted((one_pass() for _ in range(3)), key=lambda x: x[1])
            _, ev_d, m = runs[1]
            by_d = (m + 1.0) / m * p.nrows * n * 8
            r["deferred_writes"] = {"stores_every": m, "cycles": cycles,
                                    "ms_per_iteration": round(ev_d, 4),
                                    "ms_per_iteration_passes": [round(x[1], 4) for x in runs],
                                    "achieved": round(rate(by_d, ev_d), 1)}
            if representative:
                r["deferred_writes"]["frac"] = round(rate(by_d, ev_d) / HBM_PEAK_GBS, 4)
                add_rocprof(r["deferred_writes"], f"{kind}{n}_p{P}_f64", ev_d, by_d)
        out[f"P{P}"] = r
        sh.close()
        del sh
        torch.cuda.empty_cache()
    return out


def deferred_leg(sharded, dev, torch, kind, n, dt, seed, every_ms):
    """The solve loop's deferred writes at P = 1 (ShardedSimilarityTransform
    runs the same st_round_flat_deferred launches as DeviceSolver): HIP
    events over whole store cycles, the bitwise check against storing every
    round, and the committed rocprof cycle sum beside it."""
    sh = sharded.ShardedSimilarityTransform(n, dt)
    if not sh.deferred_writes:
        return None
    cycles = max(3, int(round(60.0 / max(every_ms, 1e-3) / 6)))  # ~40-60 ms of rounds
    # three passes over the same number of whole cycles, the median by HIP
    # events (the rounds with pending scalings are issue-bound and follow the
    # clock, which drifts by a few per cent over a bench run); every pass
    # from a fresh A_0 with 2 warm-up cycles, so that each times the same
    # data (on memory-side-cache-assisted blocks the streaming rate depends
    # on the values, profiles/r03_data_dependence.log: round 4 ran passes 2
    # and 3 on from pass 1's matrix, and its rocprof source - another
    # process, other data - read 5 % slower).  The committed
    # rocprof source is a kernel trace of THIS leg (tools/defer_profile.py
    # --bench-leg), summarised the same way: median pass, timed cycles only

    def one_pass():
        sh.load(kind, seed=seed)
        return timed_deferred(sh, cycles, 2, torch, None, 1)
    runs = sorted((one_pass() for _ in range(3)), key=lambda r: r[1])
    el, ev_ms, m = runs[1]
    same = deferred_bitwise(sh, kind, seed, torch)
    bpe = 8 if dt == torch.float64 else 4
    by = (m + 1.0) / m * n * n * bpe
    workload = f"{kind}{n}_{'f64' if bpe == 8 else 'f32'}"
    out = {"stores_every": m, "cycles": cycles, "passes": 3, "ms_per_iteration": round(ev_ms, 4),
           "ms_per_iteration_passes": [round(r[1], 4) for r in runs],
           "ms_per_iteration_host_clock": round(el / (cycles * m) * 1e3, 4),
           "ms_per_iteration_write_every_round": round(every_ms, 4),
           "speedup": round(every_ms / ev_ms, 3), "bytes_per_round": by,
           "achieved": round(rate(by, ev_ms), 1),
           "frac": round(rate(by, ev_ms) / HBM_PEAK_GBS, 4),
           "bitwise_equal_to_write_every_round": same,
           "timing": "HIP events around whole store cycles (first round after a store "
                     "... the storing round), no flush inside; median of 3 passes, each "
                     "from a fresh A_0 after 2 warm-up cycles"}
    add_rocprof(out, workload, ev_ms, by)
    sh.close()
    del sh
    torch.cuda.empty_cache()
    return out


def configs4_leg(sharded, dev, torch, np_, dist):
    """BASELINE configs[4]: 32768^2 random fp32 on one GPU — the every-round
    step (roofline on 2*N^2*4 bytes), the solve loop's deferred rounds, and
    the fp32-vs-fp64 tolerance study on the same input: λ and v after 8
    rounds against the fp64 iteration and the oracle's fp32 solve, and the
    stop test at the reference's EPS = 1e-3f (never passes at this size)."""
    n = 32768
    sh = sharded.ShardedSimilarityTransform(n, torch.float32)
    sh.load("random", seed=0)
    el, fused = timed_rounds(sh, 50, 3, torch, dist, 1)
    by = 2.0 * n * n * 4
    flat = dev.flat_round_pays(n, n, torch.float32)
    tr = load_traffic("random32768_f32", "k_flat" if flat else "k_round")
    out = {"workload": "random32768_f32",
           "kernel": "flat round: k_flat + k_parts (round time)" if flat else "k_round",
           "ms_per_iteration": round(el / 50 * 1e3, 4),
           "roofline": {"bound": "hbm", "achieved": round(rate(by, fused), 1),
                        "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(rate(by, fused) / HBM_PEAK_GBS, 4),
                        "traffic": None if tr is None else tr[0],
                        "traffic_source": None if tr is None else tr[1],
                        "fused_ms_avg": round(fused, 5), "bytes_per_launch": by}}
    # tolerance study: 8 rounds (eps = 0) in fp32 and fp64 on the same input
    sh.load("random", seed=0)
    lam32, v32, it32, _ = sh.solve(eps=0.0, max_itr=8, batch=8)
    v32 = v32.double()
    sh.close()
    del sh
    torch.cuda.empty_cache()
    sh64 = sharded.ShardedSimilarityTransform(n, torch.float64)
    sh64.load("random", seed=0)
    lam64, v64, it64, _ = sh64.solve(eps=0.0, max_itr=8, batch=8)
    sh64.close()
    del sh64
    torch.cuda.empty_cache()
    tol = {"rounds": 8, "eigen_val_f32": lam32, "eigen_val_f64": lam64,
           "eigen_val_rel_diff": abs(lam32 - lam64) / lam64,
           "eigen_vec_max_abs_diff": (v32 - v64).abs().max().item()}
    pin = oracle_pin("random32768_f32_8rounds")
    if pin is not None:   # the oracle's fp32 solve, EPS = 1e-3f, max_itr = 8
        tol["eigen_val_rel_err_vs_oracle_f32"] = abs(lam32 - pin["eigen_val"]) / pin["eigen_val"]
    perron = true_lambda(n, "f32", 0)
    if perron is not None:
        tol["eigen_val_rel_err_vs_true"] = abs(lam32 - perron) / perron
    # the reference's fp32 stop test at this size: run the library's solve
    # loop at EPS = 1e-3f to MAX_ITR
    solver = dev.DeviceSolver(torch.device("cuda", torch.cuda.current_device()))
    a = dev.generate("random", n, torch.float32, seed=0,
                     device=torch.device("cuda", torch.cuda.current_device()))
    lam_r, _, it_r, st_r = solver.solve(a, inplace=True, batch=64)
    solver.close()
    del a
    torch.cuda.empty_cache()
    tol["reference_eps"] = {"eps": 1e-3, "iter_count": it_r, "converged": bool(st_r["converged"]),
                            "loop_ms": round(st_r["loop_ms"], 1), "eigen_val": float(lam_r)}
    tol["study"] = "profiles/r01_fp32_study.json (per-round λ / max adjacent |Δs| tables)"
    out["tolerance_study"] = tol
    out["_every_ms"] = el / 50 * 1e3
    return out


def cpu_leg(args, np_, workload, n, bytes_round_total, ms_per_step):
    """The oracle's 3-pass schedule (oracle/st_oracle.c: row sums, stats,
    transform per round; OpenMP over rows) on every CPU of this process's
    affinity mask: a bounded sample of the bench workload, configs[0]'s
    128^2 Hilbert on one core, and (full runs) the random 32768^2 fp64
    sample BASELINE.md §3 plans."""
    from oracle import oracle as orc
    info = host_info()
    threads = info["threads"]
    b = 8 if args.dtype == "f64" else 4
    npdt = np_.float64 if args.dtype == "f64" else np_.float32
    mat = orc.generate_c(args.kind, n, 0, npdt)
    # an untimed warm-up of >= 1 s first: the first calls of a process ran up
    # to 100x slower for about a second (OpenMP team start-up, first touch
    # of the working copies, the host's clock ramp)
    t_w = time.perf_counter()
    while True:
        orc.similarity_transform(mat, orc.SEM_SYCL, eps=0.0, max_itr=3, nthreads=threads)
        if time.perf_counter() - t_w >= 1.0:
            break
    cal = orc.similarity_transform(mat, orc.SEM_SYCL, eps=0.0, max_itr=3, nthreads=threads)
    est = max(cal.loop_ms / 3, 1e-3)
    # three samples of ~cpu_seconds/3 each: `value` is the median, the
    # spread is stated beside it (round 1 saw 1.77x between boxes)
    rounds_cpu = int(min(5000, max(3, args.cpu_seconds * 1e3 / 3 / est)))
    samples = []
    for _ in range(3):
        r = orc.similarity_transform(mat, orc.SEM_SYCL, eps=0.0, max_itr=rounds_cpu,
                                     nthreads=threads)
        samples.append(r.loop_ms / rounds_cpu)
    # every round = row-sum pass + stats + transform pass: the CPU moves
    # 3*N^2*b per round (read, read, write); `value` uses the GPU line's
    # 2*N^2*b accounting so the two are comparable
    per_round_ms = sorted(samples)[1]
    solve_cpu = orc.similarity_transform(mat, orc.SEM_SYCL, nthreads=threads)
    del mat
    out = {"value": round(rate(bytes_round_total, per_round_ms), 3), "unit": "GB/s",
           "ms_per_iteration": round(per_round_ms, 3), "cores": threads, "kind": "port",
           "sample": f"{workload}: 3 samples of {rounds_cpu} rounds (eps=0, "
                     f"{sum(samples) * rounds_cpu / 1e3:.1f} s in all) of the reference's 3-pass "
                     "schedule (oracle/st_oracle.c, gcc -O3, OpenMP over rows, "
                     f"{threads} threads); value = the median sample",
           "samples": {"ms_per_iteration": [round(x, 3) for x in samples],
                       "median": round(per_round_ms, 3), "min": round(min(samples), 3),
                       "max": round(max(samples), 3),
                       "spread": round(max(samples) / min(samples), 3)},
           "traffic_rate_3pass": round(rate(1.5 * bytes_round_total, per_round_ms), 3),
           "solve_ms": round(solve_cpu.loop_ms, 2), "solve_iter_count": solve_cpu.iter_count,
           **info}
    out["_per_round_ms"] = per_round_ms
    if not args.no_north_star:
        n2 = 32768
        m2 = orc.generate_c("random", n2, 0, np_.float64)
        orc.similarity_transform(m2, orc.SEM_SYCL, eps=0.0, max_itr=1, nthreads=threads)
        s2 = []
        for _ in range(3):
            rr = orc.similarity_transform(m2, orc.SEM_SYCL, eps=0.0, max_itr=3, nthreads=threads)
            s2.append(rr.loop_ms / 3)
        del m2
        ms2 = sorted(s2)[1]
        out["random32768_f64"] = {"rounds": 3, "ms_per_iteration": round(ms2, 2),
                                  "value": round(rate(2.0 * n2 * n2 * 8, ms2), 2),
                                  "traffic_rate_3pass": round(rate(3.0 * n2 * n2 * 8, ms2), 2),
                                  "threads": threads,
                                  "samples": {"ms_per_iteration": [round(x, 2) for x in s2],
                                              "median": round(ms2, 2), "min": round(min(s2), 2),
                                              "max": round(max(s2), 2),
                                              "spread": round(max(s2) / min(s2), 3)}}
    # configs[0]: 128x128 Hilbert on the CPU path:
    # the C restatement on one core (fp64 / fp32, the SYCL loop), a numpy
    # restatement of main.py's loop, eigenvalues against eigvalsh
    h64 = orc.hilbert(128)
    true128 = float(np_.max(np_.linalg.eigvalsh(h64)))
    c64 = orc.similarity_transform(h64, orc.SEM_SYCL, nthreads=1)
    c32 = orc.similarity_transform(orc.hilbert(128, np_.float32), orc.SEM_SYCL, nthreads=1)
    t0 = time.perf_counter()
    a, v, itr = h64.copy(), np_.ones(128), 0
    for itr in range(1000):          # main.py:30-47, elementwise (no O(N^3) matmul)
        s_ = a.sum(axis=1)
        v = v * (s_ / s_.max())
        if np_.all(np_.abs(np_.diff(s_)) < 1e-3):
            break
        a = (a / s_[:, None]) * s_[None, :]
    np_ms = (time.perf_counter() - t0) * 1e3
    out["config1_hilbert128"] = {
        "c_1core_f64": {"ms": round(c64.loop_ms, 4), "iter_count": c64.iter_count,
                        "rel_err_vs_eigvalsh": abs(c64.eigen_val - true128) / true128},
        "c_1core_f32": {"ms": round(c32.loop_ms, 4), "iter_count": c32.iter_count},
        "numpy_mainpy_semantics": {"ms": round(np_ms, 3), "iter_count": itr + 1,
                                   "eigen_val": float(s_[0])}}
    return out


def north_star_leg(sharded, dev, torch):
    """32768^2 random fp64 on one GPU: the
    reference-semantics solve (checked against the oracle's solve and the
    Perron root) and 50 every-round steps (the matrix-free form: north_star_mf_leg)."""
    ns = sharded.ShardedSimilarityTransform(32768, torch.float64)
    ns.load("random", seed=0)
    lam_ns, _, it_ns, _ = ns.solve(eps=1e-3, max_itr=1000, batch=1)
    ns.load("random", seed=0)
    el_ns, fused_ns = timed_rounds(ns, 50, 3, torch, None, 1)
    by = 2.0 * 32768 * 32768 * 8
    ach = rate(by, fused_ns)
    flat_ns = dev.flat_round_pays(32768, 32768, torch.float64)
    tr = load_traffic("random32768_f64", "k_flat" if flat_ns else "k_round")
    out = {"workload": "random32768_f64",
           "kernel": "flat round: k_flat + k_parts (round time)" if flat_ns else "k_round",
           "ms_per_iteration": round(el_ns / 50 * 1e3, 4),
           "fused_ms_avg": round(fused_ns, 4), "achieved": round(ach, 1),
           "frac": round(ach / HBM_PEAK_GBS, 4), "target_frac": 0.70,
           "traffic": None if tr is None else tr[0],
           "solve_iter_count": it_ns, "eigen_val": lam_ns}
    pin = true_lambda(32768, "f64", 0)
    if pin is not None:  # CPU Perron root of the same matrix (tests/golden)
        out["eigen_val_rel_err_vs_true"] = abs(lam_ns - pin) / pin
    opin = oracle_pin("random32768_f64")
    if opin is not None:  # the oracle's solve of the same matrix
        out["check"] = {
            "iter_count_equal_oracle": it_ns == opin["iter_count"],
            "eigen_val_rel_err_vs_oracle": abs(lam_ns - opin["eigen_val"]) / opin["eigen_val"]}
    ns.close()
    del ns
    torch.cuda.empty_cache()
    return {"north_star": out, "every_ms": el_ns / 50 * 1e3}


def north_star_mf_leg(sharded, torch, lam_ns):
    """The matrix-free form on the north star's 32768^2 input (N^2*b per
    round), λ against the transform's."""
    mf = sharded.ShardedSimilarityTransform(32768, torch.float64, matrix_free=True)
    mf.load("random", seed=0)
    lam_mf, _, it_mf, _ = mf.solve(eps=1e-3, max_itr=1000, batch=1)
    el_mf, k_mf = timed_rounds(mf, 50, 3, torch, None, 1)
    by_mf = 1.0 * 32768 * 32768 * 8
    tr_mf = load_traffic("random32768_f64", "k_mfree")
    out = {
        "traffic": None if tr_mf is None else tr_mf[0],
        "ms_per_iteration": round(el_mf / 50 * 1e3, 4), "kernel_ms_avg": round(k_mf, 4),
        "achieved": round(rate(by_mf, k_mf), 1),
        "frac": round(rate(by_mf, k_mf) / HBM_PEAK_GBS, 4),
        "bytes_per_round": by_mf, "solve_iter_count": it_mf,
        "eigen_val_rel_diff_vs_transform": abs(lam_mf - lam_ns) / lam_ns}
    mf.close()
    del mf
    torch.cuda.empty_cache()
    return {"matrix_free": out}


def run_leg(name, a):
    """One full-size N = 1 leg; `a` = the parent's shape arguments."""
    import numpy as np
    import torch

    from eigen_value_amd import device as dev
    from eigen_value_amd import sharded
    if name == "north_star":
        return north_star_leg(sharded, dev, torch)
    if name == "north_star_mf":
        return north_star_mf_leg(sharded, torch, a["lam_ns"])
    if name == "configs4":
        c4 = configs4_leg(sharded, dev, torch, np, None)
        return {"configs4_f32": c4, "every_ms": c4.pop("_every_ms")}
    if name == "deferred":
        dt = torch.float64 if a["dtype"] == "f64" else torch.float32
        name_, kind, nn, ddt, key = (
            ("configs[1] " + f"{a['kind']}{a['n']}_{a['dtype']}", a["kind"], a["n"], dt,
             f"{a['kind']}{a['n']}_{a['dtype']}"),
            ("north_star random32768_f64", "random", 32768, torch.float64, "random32768_f64"),
            ("configs[4] random32768_f32", "random", 32768, torch.float32, "random32768_f32"),
        )[a["which"]]
        leg = deferred_leg(sharded, dev, torch, kind, nn, ddt, 0, a["every_ms"][key])
        return {"deferred_writes": {} if leg is None else {name_: leg}}
    if name == "configs3":
        return {"configs3_p1": configs3_leg(sharded, torch, None, 1, 0,
                                            max(5, min(a["steps"], 20)), min(a["warmup"], 3),
                                            a["representative"])}
    if name == "weak_rank_blocks":
        wb = rank_block_legs(sharded, torch, [(P, scaled_n(a["n"], P)) for P in (2, 4, 8)],
                             a["kind"], a["steps"], a["warmup"], a["representative"])
        wb["note"] = ("rank 0's block of the weak-scaled headline (n = "
                      f"{a['n']}*sqrt(N)) on one GPU, no all-gather; ~512 MiB blocks, "
                      "memory-side-cache assisted like the N = 1 line")
        return {"weak_rank_blocks": wb}
    if name == "rank_blocks":
        rb = rank_block_legs(sharded, torch, [(P, 65536) for P in (2, 4, 8)], "random",
                             max(5, min(a["steps"], 20)), min(a["warmup"], 3),
                             a["representative"])
        rb["note"] = ("one rank's row block on one GPU, no all-gather (the other ranks' row "
                      "sums held at 1.0): per-GPU compute of configs[3] at P = 2, 4, 8")
        return {"rank_blocks": rb}
    raise ValueError(f"unknown leg {name}")


LEG_TAG = "@@LEG "


LEG_FAILURES = []


def child_leg(name, a):
    """Run leg `name` in a fresh child process (`bench.py --leg`) and return
    its result, or None if the child failed or timed out.  A failed leg is
    NOT re-run here (this process holds the GPU and the headline's
    allocations, the condition the child process exists to avoid, and a
    leg that faulted or hung must not be repeated): the failure goes into
    the line's `leg_failures` and the leg's keys are left out."""
    import torch
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--leg-args", json.dumps(a)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        for ln in reversed(r.stdout.splitlines()):
            if ln.startswith(LEG_TAG):
                progress(f"leg {name} done")
                return json.loads(ln[len(LEG_TAG):])
        err = f"child exited {r.returncode}: {r.stderr[-400:]}"
    except Exception as e:  # noqa: BLE001 - reported in the line
        err = repr(e)[:400]
    LEG_FAILURES.append({"leg": name, "error": err})
    print(f"bench.py: leg {name} failed: {err}", file=sys.stderr, flush=True)
    return None


def leg_main(args):
    """--leg NAME: one full-size leg in this (child) process; prints its
    result as one tagged JSON line."""
    a = json.loads(args.leg_args)
    import torch
    torch.cuda.set_device(a["device"])
    from eigen_value_amd import _lib
    _lib.load()
    print(LEG_TAG + json.dumps(run_leg(args.leg, a)), flush=True)


def strip_fracs(obj):
    """Drop every roofline fraction (one-GPU rehearsals share one card)."""
    if isinstance(obj, dict):
        return {k: strip_fracs(v) for k, v in obj.items() if k not in ("frac", "target_frac")}
    if isinstance(obj, list):
        return [strip_fracs(v) for v in obj]
    return obj


def stall_test(args, dist):
    """--stall-rank R (tests/test_bench.py, CPU, gloo): rank R stops
    reporting progress and never reaches the point the others wait at - so
    the watchdog, the spawning parent's deadline and the communicator
    rendezvous can be tested without a GPU.  --stall-in barrier: the others
    wait in a barrier (a rank stuck in a collective); --stall-in rendezvous:
    they take the library communicator as a sharded solve does
    (make_comm_agreed over RcclComm: the id hand-over, then st_comm_init's
    pre-RCCL rendezvous), which names rank R within --comm-timeout."""
    dist.init_process_group("gloo")
    progress("stall test: process group up")
    if dist.get_rank() == args.stall_rank:
        progress("stall test: this rank sleeps")
        time.sleep(10 ** 6)
    if args.stall_in == "rendezvous":
        from eigen_value_amd import _lib, sharded
        _lib.load().st_set_comm_timeout(args.comm_timeout)
        try:
            comm, _ = sharded.make_comm_agreed(
                None, lambda: sharded.RcclComm(None, device_index=0, timeout=args.comm_timeout))
            if comm is not None:
                comm.close()
        except sharded.PeerMissingError as e:
            print(f"bench.py: rank {dist.get_rank()}: {e}", file=sys.stderr, flush=True)
            raise SystemExit(3) from None   # no RCCL state exists: a normal exit
        return
    dist.barrier()


# ---------------------------------------------------------------------------
def main():
    args = parse()
    if args.leg:
        return leg_main(args)
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and world_env is None:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:], args.stall_timeout))
    if args.gpus > 1 and os.environ.get("ST_BENCH_WATCHDOG", "1") != "0":
        start_watchdog(args.stall_timeout)
    progress("rank started")

    import numpy as np
    import torch
    import torch.distributed as dist

    if args.stall_rank is not None:
        return stall_test(args, dist)
    progress("torch imported")

    from eigen_value_amd import sharded
    from eigen_value_amd import _lib
    from eigen_value_amd import device as dev

    world = int(world_env or "1")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    representative = not args.one_gpu
    dev_index = 0 if args.one_gpu else local
    torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group("gloo")
        progress(f"process group up ({args.backend}, world {world})")
    L = _lib.load()   # fail loudly before anything else if the HIP library is missing
    if args.comm_timeout:
        L.st_set_comm_timeout(args.comm_timeout)
    # a plain run times the headline only; --full adds every other leg
    full = args.full
    big_legs = full and not args.no_north_star
    dump = None
    if args.dump_outputs:
        def dump(s):
            dump_outputs(args.dump_outputs, s, np, torch, rank)

    dt = torch.float64 if args.dtype == "f64" else torch.float32
    b = 8 if args.dtype == "f64" else 4
    n = args.n if args.strong else scaled_n(args.n, world)
    workload = f"{args.kind}{n}_{args.dtype}"
    sh = sharded.ShardedSimilarityTransform(n, dt, overlap=args.overlap)
    p = sh.part
    if world > 1:
        progress(f"{workload}: row blocks allocated, exchange "
                 + ("library RCCL communicator" if sh.rccl is not None else "torch.distributed"))

    # ---- reference-semantics solve to convergence (EPS = 1e-3) ----------
    solve = None
    if full:
        sh.load(args.kind)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # batch=1: the host checks the stop flag after every round, as the
        # reference does (similarity_transform.cpp:45-50); no gated launches
        lam, v, iters, rounds = sh.solve(eps=1e-3, max_itr=1000, batch=1)
        torch.cuda.synchronize()
        solve_ms = (time.perf_counter() - t0) * 1e3
        progress(f"{workload}: solve {iters} iterations ({solve_ms:.1f} ms), world {world}")
        solve = {"eps": 1e-3, "iter_count": iters, "rounds_evaluated": rounds,
                 "eigen_val": lam, "ms": round(solve_ms, 3)}
        if args.kind == "hilbert" and n == 8192 and args.dtype == "f64":
            solve["check"] = {"iter_count_expected": HILBERT8192_F64[0],
                              "eigen_val_rel_err_vs_oracle":
                                  abs(lam - HILBERT8192_F64[1]) / HILBERT8192_F64[1]}
    if full and world == 1:
        # accuracy against the TRUE eigenvalue: Collatz–Wielandt bracket of the
        # positive input, min (A0 v)_i / v_i <= λ_true <= max (A0 v)_i / v_i
        # (torch.mv as the checker); and the same solve at eps = 1e-6
        a0 = sh.load(args.kind)
        solve["rel_err_bound_vs_true"] = cw_bound(torch, a0, v, lam)
        lam6, v6, it6, _ = sh.solve(eps=1e-6, max_itr=1000, batch=1)
        a0 = sh.load(args.kind)
        solve["eps_1e-6"] = {"iter_count": it6, "eigen_val": lam6,
                             "rel_err_bound_vs_true": cw_bound(torch, a0, v6, lam6)}
        del a0

    # ---- timed rounds ----------------------------------------------------
    # (with N > 1 a --full run may time its headline again below, after the
    # schedule selection: the outputs are then written behind that pass)
    selects = full and world > 1 and not args.overlap and not args.no_overlap_leg
    sh.load(args.kind, mat=None)
    el, fused_ms = timed_rounds(sh, args.steps, args.warmup, torch, dist, world,
                                clocks_key="headline" if full else None,
                                after=None if selects else dump, launch_pass=full)
    bytes_round_total = 2.0 * n * n * b
    bytes_round_local = 2.0 * p.nrows * n * b
    value = bytes_round_total * args.steps / el / 1e9
    achieved = None if fused_ms is None else rate(bytes_round_local, fused_ms)
    progress(f"{workload}: {args.steps} timed rounds, {el / args.steps * 1e3:.4f} ms per round")
    # ---- N > 1: the same rounds with the exchange overlapped --------------
    # (split launch: local columns while the all-gather runs on a second
    # stream, sharded.py overlap=True).  Both schedules compute the same
    # round (A, v, m and the stop decisions bitwise; s to rounding where a
    # piece straddles the local columns).  A selection pass times both; the
    # line's `value` is then a FRESH pass of the faster one, and the other
    # is reported beside it (`exchange_other_schedule`; --overlap forces the
    # overlapped one).  Rounds 1-3 timed the plain schedule only; round 4
    # took the faster selection timing as the value (biased up)
    overlap_leg = None
    schedule = "overlapped" if args.overlap else "plain"
    if selects:
        ov = sharded.ShardedSimilarityTransform(n, dt, overlap=True)
        ov.load(args.kind)
        lam_ov, _, it_ov, _ = ov.solve(eps=1e-3, max_itr=1000, batch=1)
        ov.load(args.kind)
        el_ov, k_ov = timed_rounds(ov, args.steps, args.warmup, torch, dist, world)
        progress(f"overlapped-exchange selection pass: {el_ov / args.steps * 1e3:.5f} ms per "
                 f"round (plain {el / args.steps * 1e3:.5f})")
        # the two timings above only SELECT the schedule; the headline is a
        # fresh timed pass of the chosen one (taking the faster of two noisy
        # runs as the value would bias it upward)
        chosen_ov = el_ov < el and it_ov == iters
        sel = {"plain_ms_per_iteration": round(el / args.steps * 1e3, 5),
               "overlapped_ms_per_iteration": round(el_ov / args.steps * 1e3, 5),
               "chosen": "overlapped" if chosen_ov else "plain"}
        if chosen_ov:
            overlap_leg = {"schedule": "plain (all-gather after the round)",
                           "ms_per_iteration": sel["plain_ms_per_iteration"],
                           "value": round(value, 2), "round_ms_avg": round(fused_ms, 5),
                           "solve_iter_count": iters}
            tgt, schedule = ov, "overlapped"
        else:
            overlap_leg = {"schedule": "overlapped (split round, all-gather on a second stream)",
                           "ms_per_iteration": sel["overlapped_ms_per_iteration"],
                           "value": round(bytes_round_total * args.steps / el_ov / 1e9, 2),
                           "round_ms_avg": round(k_ov, 5), "solve_iter_count": it_ov,
                           "eigen_val_rel_diff": abs(lam_ov - lam) / abs(lam)}
            tgt = sh
        tgt.load(args.kind)
        el, fused_ms = timed_rounds(tgt, args.steps, args.warmup, torch, dist, world, after=dump)
        value = bytes_round_total * args.steps / el / 1e9
        achieved = rate(bytes_round_local, fused_ms)
        overlap_leg["selection_pass"] = sel
        overlap_leg["timing"] = ("the other schedule's selection-pass timing; the headline "
                                 "is a fresh pass of the chosen schedule")
        ov.close()
        del ov, tgt
        progress(f"headline pass ({schedule}): {el / args.steps * 1e3:.5f} ms per round")

    # ---- the per-round distribution of the same schedule (a second pass) ----
    dist_rounds = None
    if full and world == 1:
        dist_rounds = round_distribution(sh, args.kind, args.steps, args.warmup, torch)
        dist_rounds["headline_clocks"] = dict(CLOCKS)
        dist_rounds["headline_events_ms_per_round"] = round(fused_ms, 5)
        dist_rounds["headline_host_ms_per_round"] = round(el / args.steps * 1e3, 5)
        progress(f"per-round distribution: first {dist_rounds['first']} median "
                 f"{dist_rounds['median']} max {dist_rounds['max']} ms")

    use_overlap = schedule == "overlapped"
    flat_pays = dev.flat_round_pays(p.nrows, n, dt)
    flat = (not use_overlap) and flat_pays
    traffic = load_traffic(workload, "k_flat" if flat else "k_round")
    # (a plain N > 1 run has no per-launch pass, so no kernel time to price)
    roofline = None if achieved is None else {
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": None if traffic is None else traffic[0],
                "kernel": (("flat split: k_flat local + k_flat remote + k_parts" if flat_pays
                            else "k_round_split local + remote") + " (overlapped exchange)"
                           if use_overlap
                           else "flat round: k_flat + k_parts" if flat
                           else "k_round (fused stats + scale + row-sum)"),
                "fused_ms_avg": round(fused_ms, 5),
                "bytes_per_launch": bytes_round_local,
                "timing": ("HIP events bracketing the K timed rounds on the launch stream"
                           + ("; a round is k_flat + k_parts: compare with the sum of their "
                              "rocprof averages (profiles/*_kernel_stats.csv)" if flat else "")
                           if world == 1 else
                           "HIP events around every launch of a 50-round pass after the timed region"),
                "traffic_source": None if traffic is None else traffic[1]}
    if roofline is not None and bytes_round_local / 2 <= 2 * MALL_BYTES:
        roofline["note"] = ("matrix partly resident in the 256 MB memory-side cache: an "
                            "effective rate, not an HBM-roofline claim (see north_star)")
    exchange = None
    if world > 1:
        exchange = {"backend": dist.get_backend(),
                    "collective": ("library RCCL communicator (st_allgather)" if sh.rccl
                                   else "torch.distributed all_gather")}
        exchange["rccl_ranks"] = sh.rccl.info()["nranks"] if sh.rccl is not None else None
    # which RCCL the library's calls bind in this process (torch's bundled one
    # under torch: it is loaded first and has the same soname) - the one that
    # produces an N > 1 line's exchange
    rccl = _lib.rccl_info()
    if exchange is not None:
        exchange.update(rccl_version=rccl["rccl_version"], rccl_path=rccl["rccl_path"])
        if dist.get_backend() == "nccl":
            exchange["torch_nccl_version"] = ".".join(map(str, torch.cuda.nccl.version()))

    # ---- the matrix-free form on the same workload (N^2*b per round) -----
    matrix_free = None
    if full:
        mf = sharded.ShardedSimilarityTransform(n, dt, matrix_free=True)
        mf.load(args.kind)
        lam_mf, _, it_mf, _ = mf.solve(eps=1e-3, max_itr=1000, batch=1)
        el_mf, k_mf = timed_rounds(mf, args.steps, args.warmup, torch, dist, world)
        by_mf_local = 1.0 * p.nrows * n * b
        tr_mf = load_traffic(workload, "k_mfree")
        matrix_free = {"ms_per_iteration": round(el_mf / args.steps * 1e3, 5),
                       "traffic": None if tr_mf is None else tr_mf[0],
                       "value": round(1.0 * n * n * b * args.steps / el_mf / 1e9, 2),
                       "kernel_ms_avg": round(k_mf, 5),
                       "achieved": round(rate(by_mf_local, k_mf), 1),
                       "frac": round(rate(by_mf_local, k_mf) / HBM_PEAK_GBS, 4),
                       "bytes_per_round": 1.0 * n * n * b, "solve_iter_count": it_mf,
                       "eigen_val": lam_mf}
        mf.close()
        del mf
        progress("matrix-free leg done")

    # ---- N = 1: the weak-scaled headline's per-GPU blocks at N = 2, 4, 8 --
    # (rank 0's block of n = 8192*sqrt(N), timed alone: the compute side of
    # the driver's 1 -> 8 weak-scaling curve; the all-gather is not in it)
    # (a child process too, so that a profile of this process holds the
    # headline's launches only)
    weak_blocks = None
    if full and world == 1 and not args.strong and args.dtype == "f64":
        wb = child_leg("weak_rank_blocks", {
            "device": dev_index, "steps": args.steps, "warmup": args.warmup,
            "kind": args.kind, "n": args.n, "dtype": args.dtype,
            "representative": representative})
        weak_blocks = None if wb is None else wb["weak_rank_blocks"]

    out = {"metric": "ms/iteration + achieved HBM GB/s (% roofline), N×N Hilbert fp64",
           "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(el / args.steps * 1e3, 5),
           "higher_is_better": True, "scaling": "strong" if args.strong else "weak",
           "vs_baseline": None,
           "dtype": args.dtype, "data": f"synthetic ({args.kind}, generated in HBM)",
           "config": {"workload": workload, "n": n, "rows_per_gpu": p.chunk,
                      "bytes_per_round": bytes_round_total, "parallelism": f"rowblock{world}",
                      "baseline_config": ("configs[1]: 8192x8192 Hilbert fp64, 1xMI355X"
                                          if (world == 1 and n == 8192) else
                                          f"row-block sharding over {world} GPU(s), "
                                          + ("strong" if args.strong else "weak") + "-scaled")},
           "full": full, "rccl": rccl}
    for key, leg in (("roofline", roofline), ("solve", solve), ("matrix_free", matrix_free)):
        if leg is not None:
            out[key] = leg
    if use_overlap:
        out["config"]["exchange"] = "overlapped (split round, all-gather on a second stream)"
    if world > 1:
        out["config"]["exchange_schedule"] = schedule
    if exchange is not None:
        out["exchange"] = exchange
        out["rccl_ranks"] = exchange["rccl_ranks"]
    if overlap_leg is not None:
        out["exchange_other_schedule"] = overlap_leg
    if dist_rounds is not None:
        out["round_distribution"] = dist_rounds
    if weak_blocks is not None:
        out["weak_rank_blocks"] = weak_blocks
    sh.close()
    del sh
    torch.cuda.empty_cache()

    # ---- N = 1: the full-size legs, each in a fresh child process --------
    # (a block allocated after other multi-GiB blocks in the same process
    # streams 1-2.5 % slower - tools/alloc_probe.py --pre,
    # profiles/r02_alloc_probe_pre.log - so every full-size leg gets a
    # process of its own, the way the driver's fresh N = 1 run gets its
    # headline block; a child that fails is reported in `leg_failures`, not
    # re-run here)
    if world == 1 and big_legs:
        sh_args = {"device": dev_index, "steps": args.steps, "warmup": args.warmup,
                   "kind": args.kind, "n": n, "dtype": args.dtype,
                   "representative": representative}
        ns = child_leg("north_star", sh_args)
        every_ms = {workload: el / args.steps * 1e3}
        if ns is not None:
            out["north_star"] = ns["north_star"]
            every_ms["random32768_f64"] = ns["every_ms"]
            mf = child_leg("north_star_mf",
                           dict(sh_args, lam_ns=ns["north_star"]["eigen_val"]))
            if mf is not None:
                out["north_star"]["matrix_free"] = mf["matrix_free"]
        c4 = child_leg("configs4", sh_args)
        if c4 is not None:
            out["configs4_f32"] = c4["configs4_f32"]
            every_ms["random32768_f32"] = c4["every_ms"]
        deferred = {}
        for i, key in enumerate((workload, "random32768_f64", "random32768_f32")):
            if key not in every_ms:      # its every-round leg failed: no reference time
                continue
            d = child_leg("deferred", dict(sh_args, which=i, every_ms=every_ms))
            if d is not None:
                deferred.update(d["deferred_writes"])
        out["deferred_writes"] = deferred
        if "configs[4] random32768_f32" in deferred and "configs4_f32" in out:
            out["configs4_f32"]["deferred_writes"] = deferred["configs[4] random32768_f32"]
        if not args.no_configs3:
            c3 = child_leg("configs3", sh_args)
            if c3 is not None:
                c3 = c3["configs3_p1"]
                rb = child_leg("rank_blocks", sh_args)
                if rb is not None:
                    c3["rank_blocks"] = rb["rank_blocks"]
                out["configs3_p1"] = c3
                out["configs3_p1_ms_per_iteration"] = c3["ms_per_iteration"]

    # ---- N > 1: configs[3] strong-scaled over the world ------------------
    if full and world > 1 and not args.no_configs3:
        out["configs3_strong"] = configs3_leg(sharded, torch, dist, world, rank,
                                              max(5, min(args.steps, 20)),
                                              min(args.warmup, 3), representative)
        progress(f"configs3_strong done: {out['configs3_strong']['ms_per_iteration']} ms per round")

    # ---- the reference's own headline, apples to apples ----------------
    # README.md:66-158 of the reference publishes whole solves of the fp32
    # 8192x8192 Hilbert matrix through its C++ entry (host matrix in, H2D
    # inside the timed region); the fastest published device is a Xeon
    # Platinum 8358 at 126 ms (17 rounds).  Same call shape here: the
    # drop-in max_eigen_value on a host fp32 Hilbert matrix.
    if full and world == 1 and rank == 0 and not args.no_headline:
        from eigen_value_amd.similarity_transform import EigenValue
        idx = np.arange(8192, dtype=np.int64)
        h32 = np.float32(1.0) / (idx[:, None] + idx[None, :] + 1).astype(np.float32)  # utils.cpp:150
        with EigenValue() as e:
            e.similarity_transform(h32)                      # warm the context
            runs = [e.similarity_transform_ex(h32) for _ in range(3)]
        lam32, _, ts32, it32, st32 = min(runs, key=lambda r: r[4]["h2d_ms"] + r[4]["loop_ms"])
        out["reference_headline"] = {
            "workload": "hilbert8192_f32 whole solve via max_eigen_value (host matrix)",
            "ms": round(st32["h2d_ms"] + st32["loop_ms"], 3), "h2d_ms": round(st32["h2d_ms"], 3),
            "loop_ms": round(st32["loop_ms"], 3), "iter_count": it32,
            "published_ms": {"Xeon Platinum 8358": 126, "i9-10920X": 510, "Xeon Gold 6128": 339,
                             "Xeon E5-2686 v4": 3759, "Iris Xe MAX": 2509, "UHD P630": 8259},
            "speedup_vs_fastest_published": round(126.0 / (st32["h2d_ms"] + st32["loop_ms"]), 1)}
        # configs[0]'s size (128x128 Hilbert) on the GPU through the same
        # drop-in call: the whole solve is ONE workgroup launch
        # (k_solve_small); the per-round launch loop beside it
        c0 = {}
        with EigenValue() as e:
            for name, ndt in (("f32", np.float32), ("f64", np.float64)):
                h = (ndt(1.0) / (np.arange(128)[:, None] + np.arange(128)[None, :] + 1)
                     .astype(ndt))
                e.similarity_transform(h)                    # warm
                one = min((e.similarity_transform_ex(h) for _ in range(5)),
                          key=lambda r: r[4]["loop_ms"])
                loop = min((e.similarity_transform_ex(h, round_loop=True) for _ in range(5)),
                           key=lambda r: r[4]["loop_ms"])
                c0[name] = {"iter_count": one[3], "eigen_val": float(one[0]),
                            "loop_ms_single_launch": round(one[4]["loop_ms"], 4),
                            "loop_ms_round_launches": round(loop[4]["loop_ms"], 4)}
        out["reference_headline"]["config0_hilbert128_gpu"] = c0

    # ---- CPU baseline (rank 0, N = 1) ------------------------------------
    if full and world == 1 and rank == 0 and not args.no_cpu:
        cb = cpu_leg(args, np, workload, n, bytes_round_total, out["ms_per_step"])
        per_round_ms = cb.pop("_per_round_ms")
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu"] = round(per_round_ms / out["ms_per_step"], 1)

    if LEG_FAILURES:
        out["leg_failures"] = LEG_FAILURES
    if not representative:
        out = strip_fracs(out)
        out["representative"] = False
        out["note"] = ("--one-gpu rehearsal: every rank shares cuda:0; plumbing only, not "
                       "scaling data")
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
        if sharded.INIT_THREAD_LEFT_BEHIND:
            # a library communicator's init thread is still blocked (RCCL's
            # abort did not release it): end without the runtimes' teardown
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)


if __name__ == "__main__":
    main()
