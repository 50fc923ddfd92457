#!/usr/bin/env python3
"""Jacobi-preconditioned CG: what the preconditioned pair costs per iteration and what it saves
(docs/RESULTS.md, "A Jacobi preconditioner in the same two launches"). The protocol of
scripts/cg_tol.py: one process, one GPU, m rows, form="sr", the greedy one-stream schedule
compiled to a hipGraph of `--unroll` iterations; variants alternate `--reps` times, each
measurement is `--iters` iterations after `--warmup`, wall clock around a device synchronize;
medians and spreads are reported.

Sections (`--section`, default all):

  cost       precond none and jacobi, each with tol = 0 and with tol > 0 disarmed (the stopping
             kernels on their full path), nrhs = 1
  unchanged  precond none only, nrhs = 1 and 8, tol = 0: the path this option must not touch. It
             uses nothing the option added, so the same file measures a checkout from before it;
             run both in one session, alternating, and compare with the spread of either
  solve      time to solution at diag_scale = `--diag-scale`, tol = `--tol`: solve() from a reset
             (check_every 8, without the host-side true residual), both forms, iterations and ms

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="all", choices=["all", "cost", "unchanged", "solve"])
    ap.add_argument("--m", type=int, default=150_000)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--diag-scale", type=int, default=2)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=11)
    ap.add_argument("--max-iters", type=int, default=20_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert tz.hip_device_count() > 0, "needs a GPU"
    sections = ("cost", "unchanged", "solve") if a.section == "all" else (a.section,)
    plat = tz.Platform(2)  # as scripts/cg_forms.py: greedy keeps the two ops on one of the two streams
    rt = tz.HipRuntime(device=0, n_streams=2, mode=tz.ExecMode.Graph, graph_unroll=a.unroll)
    out = {"m": a.m, "unroll": a.unroll, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}

    def build(**kw):
        c, g = build_cg(CgConfig(m=a.m, form="sr", **kw), None, 0)
        seq = greedy_schedule(g, plat)
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []
        return c, seq

    def time_variants(variants):
        """variants: name -> (workload, schedule, disarm). Alternating; us per iteration"""
        us = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, (c, seq, disarm) in variants.items():
                rt.prepare(seq)
                c.reset()
                if disarm:
                    c.set_armed(False)
                rt.precompile(a.warmup)
                rt.run(a.warmup)
                rt.precompile(a.iters)
                rt.device_sync()
                t0 = time.perf_counter()
                rt.run(a.iters)
                rt.device_sync()
                us[name].append(round((time.perf_counter() - t0) / a.iters * 1e6, 3))
                assert all(np.isfinite(c.x(j)).all() for j in range(c.args.nrhs)), name
        return {"us_per_iter": us, "median_us_per_iter": {k: statistics.median(v) for k, v in us.items()},
                "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()}}

    if "cost" in sections:
        variants = {}
        for pre in ("none", "jacobi"):
            for tol in (0.0, a.tol):
                c, seq = build(precond=pre, tol=tol)
                variants[f"{pre}/{'disarmed' if tol else 'tol0'}"] = (c, seq, tol > 0)
        out["nnz"] = variants["none/tol0"][0].args.nnz_actual
        out["cost"] = time_variants(variants)
        med = out["cost"]["median_us_per_iter"]
        out["cost"]["jacobi_minus_none_us"] = {v: round(med[f"jacobi/{v}"] - med[f"none/{v}"], 3)
                                               for v in ("tol0", "disarmed")}
        del variants

    if "unchanged" in sections:
        variants = {}
        for k in (1, 8):
            c, seq = build(nrhs=k)
            variants[f"nrhs{k}"] = (c, seq, False)
        out["unchanged"] = time_variants(variants)
        del variants

    if "solve" in sections:
        out["solve"] = {"diag_scale": a.diag_scale, "tol": a.tol, "solves": a.solves, "check_every": 8,
                        "max_iters": a.max_iters}
        rt.set_graph_unroll(8)
        for pre in ("jacobi", "none"):
            c, seq = build(precond=pre, tol=a.tol, diag_scale=a.diag_scale)
            rt.prepare(seq)
            ts = []
            for _ in range(a.solves if pre == "jacobi" else max(1, a.solves // 4)):
                c.reset()
                t0 = time.perf_counter()
                sol = solve(c, rt, a.max_iters, check_every=8, residual=False)
                ts.append(time.perf_counter() - t0)
            out["solve"][pre] = {"iterations": sol.iterations[0], "converged": sol.converged[0],
                                 "launched": sol.launched, "median_ms": round(statistics.median(ts) * 1e3, 3),
                                 "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                                 "residual": c.residual()}
    del rt
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
