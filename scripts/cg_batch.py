#!/usr/bin/env python3
"""Batched CG: what 2, 4 and 8 right-hand sides per two-launch iteration cost (docs/RESULTS.md,
"Batched right-hand sides"). The protocol of scripts/cg_forms.py.

One process, one GPU, m rows, form="sr" with nrhs = 1, 2, 4, 8, each as the greedy one-stream
schedule compiled to a hipGraph of `--unroll` iterations. nrhs = 1 is the single solve's code and
kernels: the yardstick. The four schedules alternate `--reps` times; each measurement is `--iters`
iterations after `--warmup`, wall clock around a device synchronize. Also per nrhs: residual(col)
of every column after 25 iterations from a reset. Prints one JSON document (and writes it to
`--out`).
"""
import argparse
import json
import time

import numpy as np

import tenzing_amd as tz
from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import greedy_schedule

NRHS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=150_000)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert tz.hip_device_count() > 0, "needs a GPU"

    plat = tz.Platform(2)  # as scripts/cg_forms.py: greedy keeps the two ops on one of the two streams
    cg, sched = {}, {}
    for k in NRHS:
        cg[k], g = build_cg(CgConfig(m=a.m, form="sr", nrhs=k), None, 0)
        sched[k] = greedy_schedule(g, plat)
        assert tz.verify(sched[k], tz.resolve_graph(g, sched[k]), 2) == []

    def ops(seq):
        return [(o.name, o.stream) for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]

    rt = tz.HipRuntime(device=0, n_streams=2, mode=tz.ExecMode.Graph, graph_unroll=a.unroll)
    out = {"m": a.m, "nnz": cg[1].args.nnz_actual, "unroll": a.unroll, "warmup": a.warmup, "iters": a.iters,
           "reps": a.reps, "schedules": {str(k): ops(s) for k, s in sched.items()},
           "us_per_iter": {str(k): [] for k in NRHS}}
    for _ in range(a.reps):
        for k in NRHS:
            rt.prepare(sched[k])
            cg[k].reset()
            rt.precompile(a.warmup)
            rt.run(a.warmup)
            rt.precompile(a.iters)
            rt.device_sync()
            t0 = time.perf_counter()
            rt.run(a.iters)
            rt.device_sync()
            out["us_per_iter"][str(k)].append(round((time.perf_counter() - t0) / a.iters * 1e6, 3))
            out.setdefault("finite_after_timing", {})[str(k)] = bool(
                all(np.isfinite(cg[k].x(j)).all() for j in range(k)))
    out["spread_us"] = {k: round(max(v) - min(v), 3) for k, v in out["us_per_iter"].items()}
    out["us_per_iter_per_rhs"] = {k: [round(t / int(k), 3) for t in v] for k, v in out["us_per_iter"].items()}
    out["spread_us_per_rhs"] = {k: round(max(v) - min(v), 3) for k, v in out["us_per_iter_per_rhs"].items()}
    out["residual_after_25"] = {}
    for k in NRHS:
        rt.prepare(sched[k])
        cg[k].reset()
        rt.run(25)
        rt.device_sync()
        out["residual_after_25"][str(k)] = [cg[k].residual(j) for j in range(k)]
    del rt
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
