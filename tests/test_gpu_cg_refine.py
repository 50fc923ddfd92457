"""Mixed-precision iterative refinement around the f32 single-reduction CG
(``CgConfig(form="sr", tol=t, refine_tol=e)``) on the GPU, through the workload and ``solve``.

Systems: the three shapes of the sr and pcg tests, unpreconditioned on ``diag_scale=0`` and Jacobi
on ``diag_scale=2``. Inner tol 1e-3 and 1e-5, refine_tol 1e-9 and 1e-12.

What is held to what:
  * before the first step the state is the one of the same config without refinement, bit for bit;
  * a step is x64 += f64(x) exactly, x = s = 0, r = f32(r64), p = r (Jacobi: u = f32(dinv r), p = u),
    r64 within (K_i + 2) 2^-53 (|b_i| + sum_j |a_ij| |x64_j|) of numpy's b - A x64 (the bound of an
    f64 dot product in any order), and the inner threshold tol^2 sum r^2 within (n + 2) 2^-53;
  * a solve is refined within cap = ceil(log(refine_tol) / log(tol)) + 1 refine_step() calls
    (outer_steps counts the restarts, one fewer), on the condition test_cg_refine_graph.py asserts
    on the numpy model (it needs cap - 1 on every case here), with residual64() <= refine_tol plus
    the f64 evaluation error of that check, (K + 2) 2^-53 || |b| + |A| |x64| || / ||b||;
  * the same config without refinement, run for as many inner iterations, stays above 1e-8.

Measured on an MI355X over every case of this file: the device took exactly the model's steps and
inner iterations on all 24 (shape, system, tol, refine_tol) cases in all three modes; worst
|r64 - ref| / bound 0.23; residual64 between 1.9e-16 and 4.8e-10, always below refine_tol; without
refinement the residual stays at 1.2e-7 to 2.0e-7.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cg_refine_model import (REFINE_TOLS, SHAPES, SYSTEMS, TOLS, U64, cap, check_floor, residual64,
                             residual_bound)
from tenzing_amd.models.cg import solve
from test_gpu_pcg import MODES, _build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def _state(c):
    st = [c.x(), c.r(), c.p(), c.s()]
    return st + [c.u()] if c.args.precond == "jacobi" else st


def _same(a, b):
    return len(a) == len(b) and all(_bits_equal(u, v) for u, v in zip(a, b))


def _mk(tz, gpu, m, bw, system, mode="eager", unroll=1, placement=(0, 1), **kw):
    precond, d = system
    return _build(tz, gpu, m, bw, mode, unroll, placement, precond=precond, diag_scale=d, **kw)


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_todays_bits_before_the_first_step(tz, gpu, m, bw, system, mode, unroll):
    tol = 1e-5
    c0, rt0 = _mk(tz, gpu, m, bw, system, mode, unroll, tol=tol)
    c1, rt1 = _mk(tz, gpu, m, bw, system, mode, unroll, tol=tol, refine_tol=1e-12)
    assert _same(_state(c1), _state(c0)) and c1.threshold() == c0.threshold() == c1.inner_threshold()
    assert not c1.x64().any() and not c1.r64().any() and c1.outer_steps() == 0 and not c1.refined()
    for rt in (rt0, rt1):  # to the inner stop and past it
        rt.run(96)
        rt.device_sync()
    assert c0.converged() and c1.converged() and 0 < c0.iterations() < 90
    assert c1.iterations() == c0.iterations()
    assert _same(_state(c1), _state(c0))
    assert not c1.x64().any() and c1.outer_steps() == 0 and not c1.refined()
    del rt0, rt1


def _check_step(c, tol, x64_before, steps_before):
    """one refine_step() on the current state against numpy"""
    (rp, ci, val), b = c.matrix(), c.b()
    n = c.rows()
    x_before, iters = c.x(), c.iterations()
    c.refine_step()
    x64 = c.x64()
    assert x64.dtype == np.float64
    assert _bits_equal(x64, x64_before + x_before.astype(np.float64))
    zero = np.zeros(n, dtype=np.float32)
    assert _bits_equal(c.x(), zero) and _bits_equal(c.s(), zero)
    r64 = c.r64()
    err = np.abs(r64 - residual64(rp, ci, val, b, x64))
    bound = residual_bound(rp, ci, val, b, x64)
    print(f"step m={n}: worst |r64 - ref| / bound = {(err / bound).max():.3f}, ||r64|| / ||b|| = "
          f"{np.linalg.norm(r64) / np.linalg.norm(b.astype(np.float64)):.3e}")
    assert (err <= bound).all()
    r = r64.astype(np.float32)
    assert _bits_equal(c.r(), r)
    if c.args.precond == "jacobi":
        u = c.dinv() * r
        assert _bits_equal(c.u(), u) and _bits_equal(c.p(), u)
    else:
        assert _bits_equal(c.p(), r)
    assert not c.refined() and c.outer_steps() == steps_before + 1 and not c.converged()
    assert c.iterations() == iters  # counts on over the whole solve
    rr = float(np.dot(r.astype(np.float64), r.astype(np.float64)))
    assert abs(c.inner_threshold() - tol * tol * rr) <= (n + 2) * U64 * tol * tol * rr
    rr64 = float(np.dot(r64, r64))
    assert abs(c.rr64() - rr64) <= (n + 2) * U64 * rr64 and c.rr64() > c.outer_threshold()
    return x64


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_step_algebra_through_the_workload(tz, gpu, m, bw, system, mode, unroll):
    tol = 1e-5
    c, rt = _mk(tz, gpu, m, bw, system, mode, unroll, tol=tol, refine_tol=1e-12)
    thresh0 = c.threshold()
    rt.run(3)  # not converged: the step is valid at any time
    rt.device_sync()
    assert not c.converged() and c.iterations() == 3 and c.x().any()
    x64 = _check_step(c, tol, np.zeros(m), 0)
    assert c.threshold() == thresh0  # keeps its meaning, tol^2 b.b
    rt.run(96)  # the restarted solve, to its stop
    rt.device_sync()
    assert c.converged() and c.x().any()
    x64 = _check_step(c, tol, x64, 1)
    rt.run(2)
    rt.device_sync()
    assert c.iterations() > 5 and c.x().any()
    _check_step(c, tol, x64, 2)
    del rt


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("refine_tol", REFINE_TOLS)
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_it_gets_there(tz, gpu, m, bw, system, tol, refine_tol, mode, unroll):
    c, rt = _mk(tz, gpu, m, bw, system, mode, unroll, tol=tol, refine_tol=refine_tol)
    sol = solve(c, rt, 400)
    (rp, ci, val), b = c.matrix(), c.b()
    floor = check_floor(rp, ci, val, b, c.x64())
    print(f"refined m={m} {system} tol={tol} refine_tol={refine_tol} {mode}/{unroll}: {sol.outer_steps} restarts, "
          f"{sol.iterations[0]} inner iterations ({sol.launched} launched), residual64 {sol.residual64:.3e} "
          f"(check floor {floor:.1e}), cap {cap(tol, refine_tol)}")
    assert sol.refined and c.refined()
    assert sol.outer_steps == c.outer_steps() and sol.outer_steps + 1 <= cap(tol, refine_tol)
    assert sol.residual64 == c.residual64() and sol.residual64 <= refine_tol + floor
    ref = residual64(rp, ci, val, b, c.x64())
    assert abs(sol.residual64 - np.linalg.norm(ref) / np.linalg.norm(b.astype(np.float64))) <= floor
    assert c.rr64() <= c.outer_threshold()
    del rt
    if mode != "eager":
        return
    # what refinement buys: the same config without it, run for as many inner iterations
    c0, rt0 = _mk(tz, gpu, m, bw, system, mode, unroll, tol=tol)
    c0.set_armed(False)
    rt0.run(sol.iterations[0])
    rt0.device_sync()
    assert c0.iterations() == sol.iterations[0]
    print(f"  without refinement after {sol.iterations[0]} iterations: residual {c0.residual():.3e}")
    assert c0.residual() > 1e-8
    del rt0


def test_nothing_but_the_looks_decide(tz, gpu):
    m, bw, tol, refine_tol = 1037, 0, 1e-5, 1e-12
    seen = []
    for system in SYSTEMS:
        for placement in ((0, 0), (0, 1)):
            c, rt = _mk(tz, gpu, m, bw, system, "graph", 3, placement, tol=tol, refine_tol=refine_tol)
            for every in (1, 3, 8):
                c.reset()
                sol = solve(c, rt, 400, check_every=every, residual=False)
                assert sol.refined and sol.residual64 is None
                seen.append((system, c.x64(), sol.outer_steps, sol.iterations[0]))
            del rt
    for system in SYSTEMS:
        mine = [s for s in seen if s[0] == system]
        assert len(mine) == 6
        for s in mine[1:]:
            assert _bits_equal(s[1], mine[0][1]) and s[2:] == mine[0][2:]


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("system", SYSTEMS)
def test_frozen_when_refined(tz, gpu, system, mode, unroll):
    c, rt = _mk(tz, gpu, 1037, 0, system, mode, unroll, tol=1e-3, refine_tol=1e-9)
    assert solve(c, rt, 400).refined

    def snap():
        return [c.x64(), c.r64()] + _state(c), (c.outer_steps(), c.iterations(), c.refined(), c.converged(),
                                                 c.inner_threshold(), c.rr64())

    before = snap()
    rt.run(16)
    rt.device_sync()
    c.refine_step()
    c.refine_step()
    rt.run(3)
    rt.device_sync()
    after = snap()
    assert _same(after[0], before[0]) and after[1] == before[1]
    del rt


@pytest.mark.parametrize("system", SYSTEMS)
def test_zero_right_hand_side(tz, gpu, system):
    c, rt = _mk(tz, gpu, 1037, 0, system, "graph", 1, tol=1e-5, refine_tol=1e-12, rhs="zero")
    sol = solve(c, rt, 50)
    assert sol.refined and sol.outer_steps == 0 and sol.iterations == [0] and sol.launched == 8
    assert sol.residual64 == 0.0
    for v in [c.x64(), c.r64()] + _state(c):
        assert not np.isnan(v).any() and not v.any()
    del rt


@pytest.mark.parametrize("system", SYSTEMS)
def test_reset_after_a_refined_solve(tz, gpu, system):
    c, rt = _mk(tz, gpu, 1037, 0, system, "graph", 3, tol=1e-3, refine_tol=1e-12)
    start = _state(c)
    first = solve(c, rt, 400)
    assert first.refined and first.outer_steps > 0
    x64, r64 = c.x64(), c.r64()
    c.reset()
    assert _same(_state(c), start) and not c.x64().any() and not c.r64().any()
    assert not c.refined() and c.outer_steps() == 0 and c.iterations() == 0 and not c.converged()
    assert c.inner_threshold() == c.threshold() and c.rr64() == 0.0 and c.armed()
    second = solve(c, rt, 400)
    assert second == first
    assert _bits_equal(c.x64(), x64) and _bits_equal(c.r64(), r64)
    del rt


def test_arming_and_stepping_exclude_each_other(tz, gpu):
    c, rt = _mk(tz, gpu, 50, 8, SYSTEMS[0], tol=1e-5, refine_tol=1e-12)
    c.set_armed(False)
    with pytest.raises(Exception, match="refine_step: the workload is disarmed"):
        c.refine_step()
    assert c.outer_steps() == 0 and not c.x64().any()
    c.set_armed(True)
    rt.run(2)
    rt.device_sync()
    c.refine_step()
    for armed in (False, True):
        with pytest.raises(Exception, match="set_armed: a refinement step was taken since the last reset"):
            c.set_armed(armed)
    c.reset()
    c.set_armed(False)  # a fresh state again
    del rt


def test_matrix_market_input(tz, gpu, tmp_path):
    m = 1037
    rp, ci, val = tz._tz.spd_band_matrix(m, m, 5 * m, 3)
    path = str(tmp_path / "a.mtx")
    tz._tz.write_matrix_market(m, m, rp, ci, val, path)
    c, rt = _build(tz, gpu, m, 0, "graph", 1, matrix=path, precond="jacobi", diag_scale=1, tol=1e-4,
                   refine_tol=1e-11)
    sol = solve(c, rt, 400)
    (rp, ci, val), b = c.matrix(), c.b()
    assert sol.refined and sol.outer_steps + 1 <= cap(1e-4, 1e-11)
    assert sol.residual64 <= 1e-11 + check_floor(rp, ci, val, b, c.x64())
    del rt


def test_cli_search_then_run_reports_the_refined_solve(gpu, tmp_path):
    path = tmp_path / "refine.json"

    def cli(*args):
        r = subprocess.run([sys.executable, "-m", "tenzing_amd", *args], cwd=ROOT, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    s = cli("search", "--workload", "cg", "--cg-form", "sr", "--cg-tol", "1e-5", "--cg-refine-tol", "1e-12",
            "--cg-precond", "jacobi", "--cg-diag-scale", "2", "--cg-m", "20011", "--iters", "4", "--bench-iters", "3",
            "--target-secs", "0.001", "--mode", "graph", "--save-best", str(path))
    assert s["workload"] == "cg" and s["best_pct10_ms"] > 0
    doc = json.loads(path.read_text())
    assert doc["args"]["cg_refine_tol"] == 1e-12 and doc["args"]["cg_tol"] == 1e-5
    r = cli("run", str(path), "--iters", "50", "--warmup", "5")
    assert r["correct"] and r["workload"] == "cg"
    assert r["cg_refine_tol"] == 1e-12 and r["cg_refined"] is True
    assert r["cg_outer_steps"] + 1 <= cap(1e-5, 1e-12) and 0 < r["cg_iterations"] < 100
    assert 0 <= r["cg_residual64"] <= 1.1e-12  # refine_tol and the check's own f64 error (9e-15 here)
    assert 0 <= r["cg_max_rel_err"] < 1e-4  # the fixed-k check, run before any step with the test disarmed
