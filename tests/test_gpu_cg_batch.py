"""Batched CG on the GPU: ``CgConfig(form="sr", nrhs=k)`` against k separate single solves.

Column j of a batch must have the bits of ``ConjugateGradient(nrhs=1, rhs_first=j, form="sr")``
run for the same iterations: x, r, p and rr(). That single solve is held to its numpy models by
test_gpu_cg_sr.py, so no tolerance appears here except the bound on the true residual that test
asserts too (1e-5 after 28 iterations)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import greedy_schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("eager", 1), ("graph", 1), ("graph", 3)]
STEPS = (1, 3, 28)  # iterations since the reset: 1, 3, then 25 more
CASES = [(50, 8, 2), (50, 8, 4), (50, 8, 8), (1037, 0, 2), (1037, 0, 4), (1037, 0, 8), (20_011, 0, 4)]


def _runtime(tz, gpu, streams, mode, unroll=1):
    return tz.HipRuntime(device=gpu, n_streams=streams,
                         mode=tz.ExecMode.Graph if mode == "graph" else tz.ExecMode.Eager,
                         graph_unroll=unroll)


def _schedule(tz, g, spmv_stream=0, update_stream=1):
    return greedy_schedule(g, tz.Platform(2), {"cg_form": "cg_sr"},
                           stream_for=lambda name: update_stream if name.endswith("_update") else spmv_stream)


def _state(c, col=0):
    return c.x(col), c.r(col), c.p(col), c.rr(col)


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a[:3], b[:3])) and \
        np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _single(tz, gpu, m, bw, j):
    """the oracle, computed once per (shape, right-hand side) and never changed: iterations ->
    (x, r, p, rr) of a single solve of right-hand side j, eager on two streams"""
    c, g = build_cg(CgConfig(m=m, bw=bw, form="sr", nrhs=1, rhs_first=j), None, gpu)
    rt = _runtime(tz, gpu, 2, "eager")
    rt.prepare(_schedule(tz, g))
    out, done = {0: _state(c)}, 0
    for k in STEPS:
        rt.run(k - done)
        rt.device_sync()
        done = k
        out[k] = _state(c)
    out["b"] = c.b()
    del rt
    return out


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("m,bw,nrhs", CASES)
def test_columns_are_single_solves_bit_for_bit(tz, gpu, m, bw, nrhs, mode, unroll):
    c, g = build_cg(CgConfig(m=m, bw=bw, form="sr", nrhs=nrhs), None, gpu)
    seq = _schedule(tz, g)
    ops = [(o.name, o.stream) for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]
    assert ops == [("cg_s_spmvdot", 0), ("cg_s_update", 1)]
    rt = _runtime(tz, gpu, 2, mode, unroll)
    rt.prepare(seq)
    assert (rt.effective_mode == tz.ExecMode.Graph) == (mode == "graph")
    for j in range(nrhs):  # the reset state: x = 0, r = p = b_j
        ref = _single(tz, gpu, m, bw, j)
        assert np.array_equal(c.b(j), ref["b"])
        assert _same(_state(c, j), ref[0]), j
    done = 0
    for k in STEPS:
        if k == 3:
            c.reset()
            done = 0
        rt.run(k - done)
        rt.device_sync()
        done = k
        for j in range(nrhs):
            assert _same(_state(c, j), _single(tz, gpu, m, bw, j)[k]), (k, j)
    for j in range(nrhs):
        x = c.x(j)
        assert np.isfinite(x).all()
        res = c.residual(j)
        print(f"cg batch residual m={m} nrhs={nrhs} {mode}/{unroll} col {j}: {res:.3e}")
        assert res < 1e-5, j
    with pytest.raises(Exception, match="out of range"):
        c.x(nrhs)
    del rt


@pytest.mark.parametrize("nrhs", [2, 8])
def test_schedules_do_not_matter_bit_for_bit(tz, gpu, nrhs):
    """eager, hipGraph and unrolled hipGraph, under every placement of the two ops on two
    streams: every column's x, r, p and rr() are bit-identical"""
    c, g = build_cg(CgConfig(m=1037, form="sr", nrhs=nrhs), None, gpu)
    states = []
    for mode, unroll in MODES:
        rt = _runtime(tz, gpu, 2, mode, unroll)
        for placement in ((0, 0), (0, 1), (1, 0), (1, 1)):
            rt.prepare(_schedule(tz, g, *placement))
            c.reset()
            rt.run(5)
            rt.device_sync()
            states.append([_state(c, j) for j in range(nrhs)])
        del rt
    for s in states[1:]:
        assert all(_same(a, b) for a, b in zip(states[0], s))
    assert not _same(states[0][0], states[0][1])  # the columns are different systems


def test_state_carries_across_runs(tz, gpu):
    nrhs = 4
    c, g = build_cg(CgConfig(m=1037, form="sr", nrhs=nrhs), None, gpu)
    start = [_state(c, j) for j in range(nrhs)]
    for j in range(nrhs):
        b = c.b(j)
        assert not start[j][0].any() and np.array_equal(start[j][1], b) and np.array_equal(start[j][2], b)
        assert c.residual(j) == 1.0  # x = 0
    rt = _runtime(tz, gpu, 2, "graph")
    rt.prepare(_schedule(tz, g))
    rt.run(5)
    rt.device_sync()
    five = [_state(c, j) for j in range(nrhs)]
    assert not any(_same(a, b) for a, b in zip(five, start))
    c.reset()
    assert all(_same(a, b) for a, b in zip([_state(c, j) for j in range(nrhs)], start))
    rt.run(2)
    rt.device_sync()
    rt.run(3)
    rt.device_sync()
    assert all(_same(a, b) for a, b in zip([_state(c, j) for j in range(nrhs)], five))


def test_zero_right_hand_sides_stay_finite(tz, gpu):
    """b = 0 in every column: every division is guarded, x stays 0, nothing is NaN"""
    c, g = build_cg(CgConfig(m=1037, form="sr", nrhs=4, rhs="zero"), None, gpu)
    rt = _runtime(tz, gpu, 2, "eager")
    rt.prepare(_schedule(tz, g))
    rt.run(30)
    rt.device_sync()
    for j in range(4):
        assert not c.b(j).any()
        x, r, p, rr = _state(c, j)
        assert not x.any() and rr == 0.0 and c.residual(j) == 0.0
        assert np.isfinite(x).all() and np.isfinite(r).all() and np.isfinite(p).all()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "tenzing_amd", *args], cwd=ROOT, capture_output=True, text=True,
                          timeout=240)


def test_cli_search_then_run(gpu, tmp_path):
    path = tmp_path / "batch.json"
    r = _cli("search", "--workload", "cg", "--cg-form", "sr", "--cg-nrhs", "4", "--cg-m", "1037", "--iters", "4",
             "--bench-iters", "3", "--target-secs", "0.001", "--mode", "graph", "--save-best", str(path))
    assert r.returncode == 0, r.stderr[-3000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])
    assert s["workload"] == "cg" and s["best_pct10_ms"] > 0
    doc = json.loads(path.read_text())
    assert doc["args"]["cg_form"] == "sr" and doc["args"]["cg_nrhs"] == 4
    r = _cli("run", str(path), "--iters", "50", "--warmup", "5")
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["correct"] and out["workload"] == "cg"
    assert out["cg_nrhs"] == 4
    assert 0 <= out["cg_max_rel_err"] < 1e-4  # the maximum over the four columns
    assert out["cg_residual"] >= 0


def test_cli_refuses_a_batched_fused_form(gpu, tmp_path):
    r = _cli("search", "--workload", "cg", "--cg-form", "fused", "--cg-nrhs", "4", "--cg-m", "1037", "--iters", "2")
    assert r.returncode != 0
    assert "needs form sr" in r.stderr
