#!/usr/bin/env python3
"""f64 accuracy by iterative refinement around the f32 CG solve: what a refinement step costs and
what a refined solve costs against today's solve to 1e-6 (docs/RESULTS.md, "f64 accuracy by
iterative refinement"). The protocol of scripts/cg_precond.py: one process, one GPU, m rows,
form="sr", the greedy one-stream schedule compiled to a hipGraph; wall clock around a device
synchronize; medians and spreads are reported.

Sections (`--section`, default all):

  step       one refine_step() (synchronize, three launches on the null stream, synchronize) on a
             state that is not refined, precond none and jacobi: `--steps` calls each, us per call,
             beside an empty synchronize pair for scale
  solve      time to solution, solve() from a reset (check_every 8, hipGraph of 8 iterations, without
             the host-side residuals): refine_tol 1e-10 and 1e-12 with inner tol 1e-3 and 1e-5, and
             the solve to tol = `--tol` without refinement, Jacobi on diag_scale = `--diag-scale`
             and unpreconditioned on diag_scale = 0; outer steps, inner iterations, ms, residuals
  unchanged  precond none, nrhs = 1 and 8, tol = 0, no refinement: the path this option must not
             touch. It uses nothing the option added, so the same file measures a checkout from
             before it; run both in one session, alternating, and compare with the spread of either

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
    ap.add_argument("--section", default="all", choices=["all", "step", "solve", "unchanged"])
    ap.add_argument("--m", type=int, default=150_000)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--diag-scale", type=int, default=2)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--solves", type=int, default=11)
    ap.add_argument("--max-iters", type=int, default=2_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert tz.hip_device_count() > 0, "needs a GPU"
    sections = ("step", "solve", "unchanged") if a.section == "all" else (a.section,)
    plat = tz.Platform(2)  # as scripts/cg_forms.py: greedy keeps the two ops on one of the two streams
    rt = tz.HipRuntime(device=0, n_streams=2, mode=tz.ExecMode.Graph, graph_unroll=a.unroll)
    out = {"m": a.m, "unroll": a.unroll, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}

    def build(**kw):
        c, g = build_cg(CgConfig(m=a.m, form="sr", **kw), None, 0)
        seq = greedy_schedule(g, plat)
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []
        return c, seq

    def summary(us):
        return {"median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3),
                "p90_us": round(sorted(us)[int(0.9 * (len(us) - 1))], 3)}

    if "step" in sections:
        out["step"] = {"steps": a.steps}
        rt.set_graph_unroll(8)
        for pre, d in (("none", 0), ("jacobi", a.diag_scale)):
            c, seq = build(precond=pre, diag_scale=d, tol=1e-3, refine_tol=1e-14)
            rt.prepare(seq)
            us, sync = [], []
            for _ in range(a.steps):
                c.reset()  # every step on the same state, which is not refined
                rt.run(8)  # a correction to accumulate, as in a solve
                rt.device_sync()
                t0 = time.perf_counter()
                c.refine_step()
                us.append((time.perf_counter() - t0) * 1e6)
                t0 = time.perf_counter()
                rt.device_sync()
                rt.device_sync()
                sync.append((time.perf_counter() - t0) * 1e6)
            out["step"][pre] = {"refine_step": summary(us), "two_empty_synchronizes": summary(sync),
                                "refined": c.refined(), "outer_steps": c.outer_steps(),
                                "residual64": c.residual64()}

    if "solve" in sections:
        out["solve"] = {"solves": a.solves, "check_every": 8, "graph_unroll": 8, "max_iters": a.max_iters,
                        "baseline_tol": a.tol, "runs": []}
        rt.set_graph_unroll(8)
        for pre, d in (("jacobi", a.diag_scale), ("none", 0)):
            cases = [(a.tol, 0.0)] + [(t, e) for t in (1e-3, 1e-5) for e in (1e-10, 1e-12)]
            for tol, refine_tol in cases:
                c, seq = build(precond=pre, diag_scale=d, tol=tol, refine_tol=refine_tol)
                rt.prepare(seq)
                ts = []
                for _ in range(a.solves):
                    c.reset()
                    t0 = time.perf_counter()
                    sol = solve(c, rt, a.max_iters, check_every=8, residual=False)
                    ts.append(time.perf_counter() - t0)
                run = {"precond": pre, "diag_scale": d, "tol": tol, "refine_tol": refine_tol,
                       "inner_iterations": sol.iterations[0], "launched": sol.launched,
                       "outer_steps": sol.outer_steps, "refined": sol.refined, "converged": sol.converged[0],
                       "median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
                       "max_ms": round(max(ts) * 1e3, 3)}
                if refine_tol > 0:
                    run["residual64"] = c.residual64()
                else:
                    run["residual"] = c.residual()
                out["solve"]["runs"].append(run)

    if "unchanged" in sections:
        rt.set_graph_unroll(a.unroll)
        variants = {}
        for k in (1, 8):
            c, seq = build(nrhs=k)
            variants[f"nrhs{k}"] = (c, seq)
        us = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, (c, seq) in variants.items():
                rt.prepare(seq)
                c.reset()
                rt.precompile(a.warmup)
                rt.run(a.warmup)
                rt.precompile(a.iters)
                rt.device_sync()
                t0 = time.perf_counter()
                rt.run(a.iters)
                rt.device_sync()
                us[name].append(round((time.perf_counter() - t0) / a.iters * 1e6, 3))
                assert all(np.isfinite(c.x(j)).all() for j in range(c.args.nrhs)), name
        out["unchanged"] = {"us_per_iter": us, "median_us_per_iter": {k: statistics.median(v) for k, v in us.items()},
                            "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()}}
        del variants

    del rt
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
