"""CG that stops: ``CgConfig(form="sr", tol=...)`` and ``models.cg.solve`` on the GPU.

The oracle is the same form with ``tol=0`` (held to its numpy models by test_gpu_cg_sr.py), run
one iteration at a time: after each iteration x, r, p and rho_k = r_k . r_k, formed in numpy f64
from the downloaded r. With the threshold of ``threshold()`` the expected count is k* = min{k >=
0 : rho_k <= thresh}, and a solve must end with the bits of the ``tol=0`` state after k*
iterations, whatever the execution mode, the placement of the two ops or ``check_every``.

Condition, asserted on the reference alone before anything else (``_kstar``): no rho_k up to the
stop lies within a relative 1e-6 of the threshold. The kernel's gamma and numpy's rho differ only
by the order of the f64 sum (about n 2^-53, 2e-12 here), so outside that band both comparisons
agree. Measured on an MI355X for right-hand side 0 of the three shapes: the nearest rho_k lies
4.1e-2 to 4.8e-1 x thresh away from its threshold; for right-hand sides 0..11 the f32 host model
of test_gpu_cg_sr.py, which gives the same counts, puts it at 1.4e-2 x thresh or more.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.models.cg import solve
from tenzing_amd.search import greedy_schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(50, 8), (1037, 0), (20_011, 0)]
TOLS = [1e-3, 1e-5]
MODES = [("eager", 1), ("graph", 1), ("graph", 3)]
REF_ITERS = 32  # iterations of the reference run: every k* + 5 of this file lies below (asserted)
BAND = 1e-6


def _runtime(tz, gpu, streams, mode, unroll=1):
    return tz.HipRuntime(device=gpu, n_streams=streams,
                         mode=tz.ExecMode.Graph if mode == "graph" else tz.ExecMode.Eager,
                         graph_unroll=unroll)


def _schedule(tz, g, spmv_stream=0, update_stream=1):
    return greedy_schedule(g, tz.Platform(2), {"cg_form": "cg_sr"},
                           stream_for=lambda name: update_stream if name.endswith("_update") else spmv_stream)


def _state(c, col=0):
    return c.x(col), c.r(col), c.p(col)


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@functools.lru_cache(maxsize=None)
def _reference(tz, gpu, m, bw, j=0):
    """the oracle, computed once per (shape, right-hand side) and never changed: the tol=0 form,
    eager on two streams, one iteration at a time; k -> (x, r, p), rho_k and residual()"""
    c, g = build_cg(CgConfig(m=m, bw=bw, form="sr", rhs_first=j), None, gpu)
    rt = _runtime(tz, gpu, 2, "eager")
    rt.prepare(_schedule(tz, g))
    states, rho, res = [], [], []
    for k in range(REF_ITERS + 1):
        if k:
            rt.run(1)
            rt.device_sync()
        states.append(_state(c))
        r = states[-1][1].astype(np.float64)
        rho.append(float(np.dot(r, r)))
        res.append(c.residual())
    del rt
    return {"states": states, "rho": rho, "residual": res}


@functools.lru_cache(maxsize=None)
def _threshold(tz, m, bw, tol, j=0):
    return tz._tz.ConjugateGradient(CgConfig(m=m, bw=bw, form="sr", rhs_first=j, tol=tol).args()).threshold()


def _kstar(ref, thresh):
    """k* = min{k : rho_k <= thresh}, after the condition on the reference: no rho_k up to the stop
    within a relative 1e-6 of the threshold"""
    ks = [k for k, v in enumerate(ref["rho"]) if v <= thresh]
    assert ks and ks[0] + 5 <= REF_ITERS, "the reference run is too short for this threshold"
    k = ks[0]
    gap = min(abs(v - thresh) for v in ref["rho"][:k + 1])
    print(f"k*={k} rho_k*={ref['rho'][k]:.3e} thresh={thresh:.3e} nearest rho: {gap / thresh:.2e} x thresh away")
    assert gap > BAND * thresh, "a rho_k lies in the band around the threshold: change the seed, not the band"
    return k


def _build(tz, gpu, m, bw, tol, mode="eager", unroll=1, placement=(0, 1), **kw):
    c, g = build_cg(CgConfig(m=m, bw=bw, form="sr", tol=tol, **kw), None, gpu)
    seq = _schedule(tz, g, *placement)
    ops = [(o.name, o.stream) for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]
    assert [name for name, _ in ops] == ["cg_s_spmvdot", "cg_s_update"]
    rt = _runtime(tz, gpu, 2, mode, unroll)
    rt.prepare(seq)
    assert (rt.effective_mode == tz.ExecMode.Graph) == (mode == "graph")
    return c, g, rt


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_solve_stops_where_the_reference_crosses_and_stays_there(tz, gpu, m, bw, tol, mode, unroll):
    ref = _reference(tz, gpu, m, bw)
    thresh = _threshold(tz, m, bw, tol)
    ks = _kstar(ref, thresh)  # the condition first
    assert 0 < ks
    c, g, rt = _build(tz, gpu, m, bw, tol, mode, unroll)
    assert c.threshold() == thresh and c.armed()
    assert c.iterations() == 0 and not c.converged()
    sol = solve(c, rt, 200)
    assert sol.iterations == [ks] and sol.converged == [True]
    assert ks < sol.launched <= ks + 8
    assert c.iterations() == ks and c.converged()
    assert _same(_state(c), ref["states"][ks])
    print(f"cg tol m={m} tol={tol} {mode}/{unroll}: k*={ks} residual={sol.residual[0]:.3e} "
          f"tol=0 run at k*: {ref['residual'][ks]:.3e}")
    assert sol.residual[0] <= 8.0 * ref["residual"][ks]
    assert sol.residual[0] == c.residual()
    # frozen: further iterations, one launch pair at a time, change nothing
    for _ in range(7):
        rt.run(1)
    rt.device_sync()
    assert _same(_state(c), ref["states"][ks])
    assert c.iterations() == ks and c.converged()
    del rt


def test_every_placement_and_mode_gives_the_same_bits_and_count(tz, gpu):
    m, bw, tol = 1037, 0, 1e-5
    ref = _reference(tz, gpu, m, bw)
    ks = _kstar(ref, _threshold(tz, m, bw, tol))
    # the streams are interchangeable and a schedule names them in order of first use, so the four
    # wishes give the two schedules there are: both ops on one stream, or one op on each
    streams = set()
    for placement in ((0, 0), (0, 1), (1, 0), (1, 1)):
        seq = _schedule(tz, build_cg(CgConfig(m=m, bw=bw, form="sr", tol=tol), setup=False)[1], *placement)
        streams.add(tuple(o.stream for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)))
    assert streams == {(0, 0), (0, 1)}
    for mode, unroll in MODES:
        for placement in ((0, 0), (0, 1), (1, 0), (1, 1)):
            c, g, rt = _build(tz, gpu, m, bw, tol, mode, unroll, placement)
            sol = solve(c, rt, 200)
            assert sol.iterations == [ks] and sol.converged == [True], (mode, unroll, placement)
            assert _same(_state(c), ref["states"][ks]), (mode, unroll, placement)
            del rt


def test_check_every_only_changes_the_launches(tz, gpu):
    m, bw, tol = 20_011, 0, 1e-5
    ref = _reference(tz, gpu, m, bw)
    ks = _kstar(ref, _threshold(tz, m, bw, tol))
    c, g, rt = _build(tz, gpu, m, bw, tol, "graph", 3)
    launched = []
    for every in (1, 3, 8):
        c.reset()
        sol = solve(c, rt, 200, check_every=every)
        assert sol.iterations == [ks] and sol.converged == [True], every
        assert _same(_state(c), ref["states"][ks]), every
        assert ks < sol.launched <= ks + every
        launched.append(sol.launched)
    assert launched[0] == ks + 1  # the update after iteration k* is the one that finds rho_k* <= thresh
    assert len(set(launched)) > 1
    del rt


def test_max_iters_below_the_count(tz, gpu):
    m, bw, tol = 1037, 0, 1e-5
    ref = _reference(tz, gpu, m, bw)
    ks = _kstar(ref, _threshold(tz, m, bw, tol))
    cap = ks - 3
    assert cap > 0
    c, g, rt = _build(tz, gpu, m, bw, tol, "graph", 1)
    sol = solve(c, rt, cap)
    assert sol.converged == [False] and sol.iterations == [cap] and sol.launched == cap
    assert _same(_state(c), ref["states"][cap])
    # exactly k* launches perform k* iterations; the test that stops is the next update's
    c.reset()
    sol = solve(c, rt, ks, check_every=ks)
    assert sol.converged == [False] and sol.iterations == [ks] and sol.launched == ks
    assert _same(_state(c), ref["states"][ks])
    sol = solve(c, rt, 1)  # goes on from the current state
    assert sol.converged == [True] and sol.iterations == [ks] and sol.launched == 1
    assert _same(_state(c), ref["states"][ks])
    del rt


@pytest.mark.parametrize("nrhs", [1, 4])
def test_zero_right_hand_side_converges_at_once(tz, gpu, nrhs):
    c, g, rt = _build(tz, gpu, 1037, 0, 1e-5, rhs="zero", nrhs=nrhs)
    sol = solve(c, rt, 50)
    assert sol.iterations == [0] * nrhs and sol.converged == [True] * nrhs and sol.launched == 8
    assert sol.residual == [0.0] * nrhs
    for j in range(nrhs):
        assert c.threshold(j) == 0.0
        x, r, p = _state(c, j)
        assert not x.any() and not r.any() and not p.any()
        assert np.isfinite(x).all() and np.isfinite(r).all() and np.isfinite(p).all()
        assert c.rr(j) == 0.0
    del rt


@pytest.mark.parametrize("nrhs", [1, 4])
def test_disarmed_is_the_form_without_tol(tz, gpu, nrhs):
    m, bw, tol = 1037, 0, 1e-3
    refs = [_reference(tz, gpu, m, bw, j) for j in range(nrhs)]
    ks = [_kstar(refs[j], _threshold(tz, m, bw, tol, j)) for j in range(nrhs)]
    n = max(ks) + 5
    c, g, rt = _build(tz, gpu, m, bw, tol, "graph", 3, nrhs=nrhs)
    c.set_armed(False)
    assert not c.armed()
    rt.run(n)
    rt.device_sync()
    for j in range(nrhs):
        assert _same(_state(c, j), refs[j]["states"][n]), j
        assert not c.converged(j) and c.iterations(j) == n
        assert c.threshold(j) == _threshold(tz, m, bw, tol, j)  # the armed value
    c.reset()  # re-arms
    assert c.armed()
    sol = solve(c, rt, 200)
    assert sol.iterations == ks and sol.converged == [True] * nrhs
    for j in range(nrhs):
        assert _same(_state(c, j), refs[j]["states"][ks[j]]), j
    # set_armed(True) after a disarmed reset does the same
    c.reset()
    c.set_armed(False)
    c.set_armed(True)
    assert solve(c, rt, 200).iterations == ks
    del rt


@functools.lru_cache(maxsize=None)
def _single_solve(tz, gpu, m, bw, tol, j):
    """a single solve of right-hand side j with the same tol: (x, r, p), iterations"""
    c, g, rt = _build(tz, gpu, m, bw, tol, rhs_first=j)
    sol = solve(c, rt, 200)
    assert sol.converged == [True]
    out = _state(c), sol.iterations[0]
    del rt
    return out


# (m, tol, rhs_first). On the 1037-row system right-hand sides 0 and 1 cross 1e-3 at different
# iterations (9 and 10 in the f32 host model), so every batch that starts at 0 has columns that
# stop apart; on the 20 011-row one all eight stop together, which takes the all_done path.
BATCHES = [(1037, 1e-3, 0), (20_011, 1e-5, 0)]


@pytest.mark.parametrize("mode,unroll", [("eager", 1), ("graph", 3)])
@pytest.mark.parametrize("nrhs", [2, 4, 8])
@pytest.mark.parametrize("m,tol,first", BATCHES)
def test_batch_columns_stop_as_single_solves(tz, gpu, m, tol, first, nrhs, mode, unroll):
    refs = [_reference(tz, gpu, m, 0, first + j) for j in range(nrhs)]
    ks = [_kstar(refs[j], _threshold(tz, m, 0, tol, first + j)) for j in range(nrhs)]
    if m == 1037:
        assert len(set(ks)) > 1, ks  # on the reference first: the columns stop at different iterations
    c, g, rt = _build(tz, gpu, m, 0, tol, mode, unroll, nrhs=nrhs, rhs_first=first)
    sol = solve(c, rt, 200)
    assert sol.converged == [True] * nrhs
    assert sol.iterations == ks
    assert max(ks) < sol.launched <= max(ks) + 8
    for j in range(nrhs):
        state, iters = _single_solve(tz, gpu, m, 0, tol, first + j)
        assert iters == ks[j] and c.iterations(j) == iters, j
        assert _same(_state(c, j), state), j
        assert _same(state, refs[j]["states"][ks[j]]), j
        assert c.threshold(j) == _threshold(tz, m, 0, tol, first + j)
        assert sol.residual[j] <= 8.0 * refs[j]["residual"][ks[j]], j
    for _ in range(7):  # frozen, each column where it stopped
        rt.run(1)
    rt.device_sync()
    for j in range(nrhs):
        assert _same(_state(c, j), refs[j]["states"][ks[j]]) and c.iterations(j) == ks[j], j
    del rt


def test_accessors_refuse_a_workload_without_tol(tz, gpu):
    c, g = build_cg(CgConfig(m=50, bw=8, form="sr"), None, gpu)
    for f in (c.iterations, c.converged, c.threshold, lambda: c.set_armed(False)):
        with pytest.raises(Exception, match="tol = 0"):
            f()
    c, g = build_cg(CgConfig(m=50, bw=8, form="sr", nrhs=2, tol=1e-3), None, gpu)
    for f in (c.iterations, c.converged, c.threshold):
        with pytest.raises(Exception, match="out of range"):
            f(2)


def test_cli_search_then_run(gpu, tmp_path):
    path = tmp_path / "tol.json"

    def cli(*args):
        r = subprocess.run([sys.executable, "-m", "tenzing_amd", *args], cwd=ROOT, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    s = cli("search", "--workload", "cg", "--cg-form", "sr", "--cg-tol", "1e-5", "--cg-m", "20011", "--iters", "4",
            "--bench-iters", "3", "--target-secs", "0.001", "--mode", "graph", "--save-best", str(path))
    assert s["workload"] == "cg" and s["best_pct10_ms"] > 0
    doc = json.loads(path.read_text())
    assert doc["args"]["cg_form"] == "sr" and doc["args"]["cg_tol"] == 1e-5
    r = cli("run", str(path), "--iters", "50", "--warmup", "5")
    assert r["correct"] and r["workload"] == "cg"
    assert r["cg_converged"] is True
    assert 0 < r["cg_iterations"] < 100
    assert 0 <= r["cg_residual"] < 1e-4
    assert 0 <= r["cg_max_rel_err"] < 1e-4  # the fixed-k check, run with the test disarmed
