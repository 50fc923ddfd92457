#!/usr/bin/env python3
"""CG that stops: what the device-side convergence test costs and what it saves (docs/RESULTS.md,
"A stopping test on the device"). The protocol of scripts/cg_batch.py.

One process, one GPU, m rows, form="sr" with nrhs = 1 and 8, each as the greedy one-stream
schedule compiled to a hipGraph of `--unroll` iterations, in three variants:

  tol0      tol = 0: the kernels without a test, the yardstick
  disarmed  tol > 0 after set_armed(False): the stopping kernels on their full path
  frozen    tol > 0 after a solve has converged: two launches that return at once

The variants alternate `--reps` times; each measurement is `--iters` iterations after `--warmup`,
wall clock around a device synchronize.

Then the comparison the option exists for, nrhs = 1: the wall clock of a whole solve() to `--tol`
from a reset (without the host-side true residual) with check_every = 1, 8, 32, each with a
hipGraph of check_every iterations, against the same number of tol = 0 iterations with a host
read of rr() after every one. `--solves` repetitions each; the median and the extremes.
Prints one JSON document (and writes it to `--out`).
"""
import argparse
import json
import statistics
import time

import numpy as np

import tenzing_amd as tz
from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.models.cg import solve
from tenzing_amd.search import greedy_schedule

NRHS = (1, 8)
VARIANTS = ("tol0", "disarmed", "frozen")
CHECK_EVERY = (1, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=150_000)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solves", type=int, default=21)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert tz.hip_device_count() > 0, "needs a GPU"

    plat = tz.Platform(2)  # as scripts/cg_forms.py: greedy keeps the two ops on one of the two streams
    cg, sched = {}, {}
    for k in NRHS:
        for tol in (0.0, a.tol):
            cg[k, tol > 0], g = build_cg(CgConfig(m=a.m, form="sr", nrhs=k, tol=tol), None, 0)
            sched[k, tol > 0] = greedy_schedule(g, plat)
            assert tz.verify(sched[k, tol > 0], tz.resolve_graph(g, sched[k, tol > 0]), 2) == []

    def ops(seq):
        return [(o.name, o.stream) for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]

    rt = tz.HipRuntime(device=0, n_streams=2, mode=tz.ExecMode.Graph, graph_unroll=a.unroll)
    out = {"m": a.m, "nnz": cg[1, False].args.nnz_actual, "tol": a.tol, "unroll": a.unroll, "warmup": a.warmup,
           "iters": a.iters, "reps": a.reps, "schedules": {f"{k}/{'tol' if t else 'tol0'}": ops(s)
                                                           for (k, t), s in sched.items()},
           "us_per_iter": {f"{k}/{v}": [] for k in NRHS for v in VARIANTS}, "iterations_to_tol": {}}

    def stage(k, variant):
        """the variant's workload, prepared and in the state the variant times"""
        c = cg[k, variant != "tol0"]
        rt.prepare(sched[k, variant != "tol0"])
        c.reset()
        if variant == "disarmed":
            c.set_armed(False)
        if variant == "frozen":
            sol = solve(c, rt, a.max_iters, residual=False)
            assert all(sol.converged), sol
            out["iterations_to_tol"][str(k)] = sol.iterations
        return c

    for _ in range(a.reps):
        for k in NRHS:
            for variant in VARIANTS:
                c = stage(k, variant)
                rt.precompile(a.warmup)
                rt.run(a.warmup)
                rt.precompile(a.iters)
                rt.device_sync()
                t0 = time.perf_counter()
                rt.run(a.iters)
                rt.device_sync()
                out["us_per_iter"][f"{k}/{variant}"].append(round((time.perf_counter() - t0) / a.iters * 1e6, 3))
                if variant == "frozen":  # still where the solve left it
                    assert [c.iterations(j) for j in range(k)] == out["iterations_to_tol"][str(k)]
                out.setdefault("finite_after_timing", {})[f"{k}/{variant}"] = bool(
                    all(np.isfinite(c.x(j)).all() for j in range(k)))
    med = {key: statistics.median(v) for key, v in out["us_per_iter"].items()}
    out["median_us_per_iter"] = med
    out["spread_us"] = {key: round(max(v) - min(v), 3) for key, v in out["us_per_iter"].items()}
    out["minus_tol0_us"] = {f"{k}/{v}": round(med[f"{k}/{v}"] - med[f"{k}/tol0"], 3)
                            for k in NRHS for v in VARIANTS[1:]}

    # a whole solve against iterating with a host read of rr() after every iteration
    def summary(ts):
        return {"median_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
                "max_us": round(max(ts) * 1e6, 1)}

    c = cg[1, True]
    out["solve"] = {"solves": a.solves}
    kstar = None
    for every in CHECK_EVERY:
        rt.set_graph_unroll(every)
        rt.prepare(sched[1, True])
        ts = []
        for _ in range(a.solves):
            c.reset()
            t0 = time.perf_counter()
            sol = solve(c, rt, a.max_iters, check_every=every, residual=False)
            ts.append(time.perf_counter() - t0)
            assert sol.converged == [True]
            assert kstar in (None, sol.iterations[0])  # the count does not depend on check_every
            kstar = sol.iterations[0]
        out["solve"][f"check_every_{every}"] = dict(summary(ts), launched=sol.launched)
    out["solve"]["iterations"] = kstar
    out["solve"]["residual"] = c.residual()
    c0 = cg[1, False]
    thresh = c.threshold()
    rt.set_graph_unroll(1)
    rt.prepare(sched[1, False])
    ts = []
    for _ in range(a.solves):
        c0.reset()
        t0 = time.perf_counter()
        n = 0
        while n < a.max_iters and c0.rr() > thresh:  # rr() synchronizes and downloads
            rt.run(1)
            n += 1
        ts.append(time.perf_counter() - t0)
    out["solve"]["host_rr_every_iteration"] = dict(summary(ts), launched=n)
    del rt
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
