#!/usr/bin/env python3
"""The three conjugate-gradient forms side by side (docs/RESULTS.md, "Extension: CG").

One process, one GPU, m rows, every schedule compiled to a hipGraph of `--unroll` iterations:
  A  plain form, greedy, one stream (8 launches)
  B  fused form, greedy, one stream (4 launches)
  D  single-reduction form, greedy, one stream (2 launches)
  E  best of an MCTS over form="all" on 2 streams, seeded with A, B and D
The schedules alternate `--reps` times; each measurement is `--iters` iterations after
`--warmup`, wall clock around a device synchronize. Also per form: residual() and check() after
25 iterations from a reset. Prints one JSON document (and writes it to `--out`).
"""
import argparse
import json
import time

import numpy as np

import tenzing_amd as tz
from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import greedy_schedule, search


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=150_000)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mcts-iters", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert tz.hip_device_count() > 0, "needs a GPU"

    c, g = build_cg(CgConfig(m=a.m, form="all"), None, 0)
    plat = tz.Platform(2)
    sched = {k: greedy_schedule(g, plat, {"cg_form": "cg_" + f})
             for k, f in (("A", "plain"), ("B", "fused"), ("D", "sr"))}
    ctrl = tz.SelfCtrl()
    t0 = time.perf_counter()
    res = search(g, streams=2, iters=a.mcts_iters, mode="graph", graph_unroll=a.unroll, ctrl=ctrl, device=0,
                 seeds=list(sched.values()))
    search_s = time.perf_counter() - t0
    sched["E"] = res.sims[res.best()].seq
    assert tz.verify(sched["E"], tz.resolve_graph(g, sched["E"]), 2) == []

    def ops(seq):
        return [(o.name, o.stream) for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]

    rt = tz.HipRuntime(device=0, n_streams=2, mode=tz.ExecMode.Graph, graph_unroll=a.unroll)
    out = {"m": a.m, "nnz": c.args.nnz_actual, "unroll": a.unroll, "warmup": a.warmup, "iters": a.iters,
           "mcts": {"iters": a.mcts_iters, "candidates": len(res.sims), "failed": res.failed,
                    "wall_s": round(search_s, 1)},
           "schedules": {k: ops(s) for k, s in sched.items()}, "us_per_iter": {k: [] for k in sched}}
    for _ in range(a.reps):
        for k, seq in sched.items():
            rt.prepare(seq)
            c.reset()
            rt.precompile(a.warmup)
            rt.run(a.warmup)
            rt.precompile(a.iters)
            rt.device_sync()
            t0 = time.perf_counter()
            rt.run(a.iters)
            rt.device_sync()
            out["us_per_iter"][k].append(round((time.perf_counter() - t0) / a.iters * 1e6, 3))
            out.setdefault("finite_after_timing", {})[k] = bool(np.isfinite(c.x()).all())
    out["spread_us"] = {k: round(max(v) - min(v), 3) for k, v in out["us_per_iter"].items()}
    out["after_25"] = {}
    for k, seq in sched.items():
        rt.prepare(seq)
        c.reset()
        rt.run(25)
        rt.device_sync()
        out["after_25"][k] = {"residual": c.residual(), "check": c.check(25), "rr": c.rr()}
    del rt
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
