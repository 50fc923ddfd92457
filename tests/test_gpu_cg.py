"""The conjugate-gradient workload on the GPU against numpy references built in this file from
``spd_band_matrix`` and ``cg.b()`` (never from ``check()``): accuracy after 1 and 3 iterations
(CG corrects its own errors, so a wrong dot product is visible early and invisible by iteration
25), convergence, bit-identical results under every schedule, state across runs, the degenerate
system, Matrix Market input, a search and the CLI.

Two host runs with the kernels' guards: one in f64, one with f32 vectors and f64 dot products.
e32(k) = max|x32 - x64| / max|x64| is what f32 storage costs; the device must stay within
8 x max(e32(k), 2^-23): it sums rows and partials in another order than numpy, which changes
rounding constants, not orders of magnitude.
"""
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

SHAPES = [(50, 8), (1037, 0), (20_011, 0)]
EPS = 2.0 ** -23
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _div(a, b):
    return a / b if b != 0 else 0.0


class HostCg:
    """CG on the host with the kernels' guards; f32=True keeps the vectors (and the SpMV) in
    f32 and accumulates the dot products in f64, as the device does"""

    def __init__(self, rp, ci, val, b, f32):
        self.rp = np.asarray(rp, dtype=np.int64)
        self.ci = np.asarray(ci, dtype=np.int64)
        self.t = np.float32 if f32 else np.float64
        self.val = np.asarray(val, dtype=np.float32).astype(self.t)
        self.b = np.asarray(b, dtype=np.float32)
        self.x = np.zeros(len(self.b), dtype=self.t)
        self.r = self.b.astype(self.t)
        self.p = self.r.copy()
        self.rr = float(np.dot(self.r.astype(np.float64), self.r.astype(np.float64)))
        self.k = 0

    def matvec(self, v, t=None):
        t = t or self.t
        prod = self.val.astype(t) * v.astype(t)[self.ci]
        return np.add.reduceat(prod, self.rp[:-1]).astype(t)  # every row holds its diagonal

    def step(self):
        d = np.float64
        q = self.matvec(self.p)
        alpha = _div(self.rr, float(np.dot(self.p.astype(d), q.astype(d))))
        a = d(np.float32(alpha)) if self.t is np.float32 else alpha
        self.x = (self.x.astype(d) + a * self.p.astype(d)).astype(self.t)
        self.r = (self.r.astype(d) - a * q.astype(d)).astype(self.t)
        rr_new = float(np.dot(self.r.astype(d), self.r.astype(d)))
        beta = _div(rr_new, self.rr)
        bt = d(np.float32(beta)) if self.t is np.float32 else beta
        self.rr = rr_new
        self.p = (self.r.astype(d) + bt * self.p.astype(d)).astype(self.t)
        self.k += 1

    def residual(self, x):
        """||b - A x|| / ||b|| in f64"""
        d = np.float64
        return float(np.linalg.norm(self.b.astype(d) - self.matvec(np.asarray(x), d)) /
                     np.linalg.norm(self.b.astype(d)))


@functools.lru_cache(maxsize=None)
def _reference(tz, m, bw):
    """per shape, computed once and never changed: k -> (x64, rr64, e32, err_rr32) for k = 1, 3,
    5; the f32 run's residual after 28 iterations; and the matrix"""
    bw = bw or m
    rp, ci, val = tz._tz.spd_band_matrix(m, bw, 5 * m, 1)
    b = tz._tz.ConjugateGradient(CgConfig(m=m, bw=bw).args()).b()
    h64, h32 = HostCg(rp, ci, val, b, False), HostCg(rp, ci, val, b, True)
    at = {}
    for k in range(1, 29):
        h64.step()
        h32.step()
        if k in (1, 3, 5):
            e32 = np.abs(h32.x - h64.x).max() / np.abs(h64.x).max()
            at[k] = (h64.x.copy(), h64.rr, float(e32), abs(h32.rr - h64.rr) / h64.rr)
    return {"at": at, "res32": h64.residual(h32.x.astype(np.float64)), "host": h64}


def _ratios(ref, k, x, rr):
    x64, rr64, e32, err32 = ref["at"][k]
    e_dev = np.abs(x.astype(np.float64) - x64).max() / np.abs(x64).max()
    return e_dev / max(e32, EPS), (abs(rr - rr64) / rr64) / max(err32, EPS)


def _check_accuracy(ref, k, x, rr, what=""):
    """e_dev / max(e32, 2^-23) <= 8 for x and for rr. Measured on an MI355X over every case of
    this file the worst ratio is 1.3 (below 4)."""
    rx, rrr = _ratios(ref, k, x, rr)
    print(f"cg accuracy {what} k={k}: e_dev/max(e32,eps)={rx:.3f} rr ratio={rrr:.3f}")
    assert rx <= 8.0, (what, k, rx)
    assert rrr <= 8.0, (what, k, rrr)


def _runtime(tz, gpu, streams, mode, unroll=1):
    return tz.HipRuntime(device=gpu, n_streams=streams,
                         mode=tz.ExecMode.Graph if mode == "graph" else tz.ExecMode.Eager,
                         graph_unroll=unroll)


def _two_stream_schedule(tz, g, form):
    # the x update on a stream of its own, beside the r -> rr -> beta -> p chain
    return greedy_schedule(g, tz.Platform(2), {"cg_form": "cg_" + form},
                           stream_for=lambda name: 1 if name.endswith("_x") else 0)


def _state(c):
    return c.x(), c.r(), c.p(), c.rr()


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a[:3], b[:3])) and \
        np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64)


@pytest.mark.parametrize("mode,unroll", [("eager", 1), ("graph", 1), ("graph", 3)])
@pytest.mark.parametrize("form", ["plain", "fused"])
@pytest.mark.parametrize("m,bw", SHAPES)
def test_accuracy_and_convergence(tz, gpu, m, bw, form, mode, unroll):
    """e_dev(k) <= 8 max(e32(k), 2^-23) for k = 1 and 3, the same for rr; after 25 more
    iterations the true residual is within 8 x the host f32 run's."""
    ref = _reference(tz, m, bw)
    c, g = build_cg(CgConfig(m=m, bw=bw), None, gpu)
    seq = _two_stream_schedule(tz, g, form)
    names = [o.name for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]
    assert len(names) == (4 if form == "fused" else 8)
    rt = _runtime(tz, gpu, 2, mode, unroll)
    rt.prepare(seq)
    assert (rt.effective_mode == tz.ExecMode.Graph) == (mode == "graph")
    for k in (1, 3):
        c.reset()
        rt.run(k)
        rt.device_sync()
        _check_accuracy(ref, k, c.x(), c.rr(), f"m={m} {form} {mode}/{unroll}")
    rt.run(25)
    rt.device_sync()
    x = c.x()
    assert np.isfinite(x).all()
    res, res32 = ref["host"].residual(x), ref["res32"]
    print(f"cg residual m={m} {form} {mode}/{unroll}: dev={res:.3e} host f32={res32:.3e}")
    assert res <= 8.0 * res32
    assert res < 1e-5  # convergence is real (the numpy model gives 1.5e-7 to 1e-6)
    del rt


def test_schedules_do_not_matter_bit_for_bit(tz, gpu):
    """12 random rollouts per stream count, eager and as a hipGraph: within a form x, r, p and rr
    are bit-identical whatever the order, the streams and the mode. An update that started
    before its alpha was final, or a p overwritten while the SpMV still read it, changes bits."""
    m = 20_011
    ref = _reference(tz, m, 0)
    c, g = build_cg(CgConfig(m=m), None, gpu)
    groups = {"plain": [], "fused": []}
    for streams in (2, 3):
        plat = tz.Platform(streams)
        seqs = [tz.random_rollout(tz.State(g, plat), seed) for seed in range(12)]
        for mode in ("eager", "graph"):
            rt = _runtime(tz, gpu, streams, mode)
            for seq in seqs:
                names = {o.name for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)}
                rt.prepare(seq)
                c.reset()
                rt.run(5)
                rt.device_sync()
                groups["fused" if "cg_f_spmvdot" in names else "plain"].append(_state(c))
            del rt
    for form, states in groups.items():
        assert len(states) >= 4, (form, len(states))  # seeds 0..11 reach both forms (checked on the CPU)
        for s in states[1:]:
            assert _same(states[0], s), form
        _check_accuracy(ref, 5, states[0][0], states[0][3], form)


@pytest.mark.parametrize("form", ["plain", "fused"])
def test_state_carries_across_runs(tz, gpu, form):
    c, g = build_cg(CgConfig(m=1037, form=form), None, gpu)
    start = _state(c)
    b = c.b()
    assert not start[0].any() and np.array_equal(start[1], b) and np.array_equal(start[2], b)
    assert abs(start[3] - float(np.dot(b.astype(np.float64), b.astype(np.float64)))) <= 1e-12 * start[3]
    rt = _runtime(tz, gpu, 2, "graph")
    rt.prepare(tz.random_rollout(tz.State(g, tz.Platform(2)), 3))
    rt.run(5)
    rt.device_sync()
    five = _state(c)
    assert not _same(five, start)
    c.reset()
    assert _same(_state(c), start)
    rt.run(2)
    rt.device_sync()
    rt.run(3)
    rt.device_sync()
    assert _same(_state(c), five)


@pytest.mark.parametrize("form", ["plain", "fused"])
def test_zero_right_hand_side_stays_finite(tz, gpu, form):
    """b = 0 (CgConfig.rhs = "zero"): every division is guarded, x stays 0, nothing is NaN"""
    c, g = build_cg(CgConfig(m=1037, form=form, rhs="zero"), None, gpu)
    assert not c.b().any()
    rt = _runtime(tz, gpu, 2, "eager")
    rt.prepare(tz.random_rollout(tz.State(g, tz.Platform(2)), 1))
    rt.run(4)
    rt.device_sync()
    x, r, p, rr = _state(c)
    assert not x.any() and rr == 0.0
    assert np.isfinite(x).all() and np.isfinite(r).all() and np.isfinite(p).all()


def test_matrix_market_input(tz, gpu, tmp_path):
    a, ga = build_cg(CgConfig(m=257, bw=16), None, gpu)
    rp, ci, val = a.matrix()
    path = str(tmp_path / "spd.mtx")
    tz._tz.write_matrix_market(257, 257, list(rp), list(ci), list(val), path)
    f, gf = build_cg(CgConfig(matrix=path), None, gpu)
    assert f.rows() == 257 and np.array_equal(f.b(), a.b())
    rt = _runtime(tz, gpu, 2, "eager")
    out = []
    for c, g in ((a, ga), (f, gf)):
        rt.prepare(_two_stream_schedule(tz, g, "fused"))
        rt.run(3)
        rt.device_sync()
        out.append(_state(c))
    assert _same(out[0], out[1])
    _check_accuracy(_reference(tz, 257, 16), 3, out[1][0], out[1][3], "matrix market")
    vals = list(val)
    rows = np.repeat(np.arange(257), np.diff(np.array(rp)))
    vals[int(np.nonzero(rows != np.array(ci))[0][0])] += 0.5  # the first off-diagonal entry
    bad = str(tmp_path / "bad.mtx")
    tz._tz.write_matrix_market(257, 257, list(rp), list(ci), vals, bad)
    with pytest.raises(Exception, match="not symmetric"):
        build_cg(CgConfig(matrix=bad), None, gpu)


def test_search_finds_a_correct_schedule(tz, gpu):
    m = 20_011
    c, g = build_cg(CgConfig(m=m), None, gpu)
    rt = _runtime(tz, gpu, 2, "graph")
    ctrl = tz.SelfCtrl()
    o = tz.MctsOpts()
    o.n_iters = 10
    o.bench = tz.BenchOpts(n_iters=3, max_retries=1, target_secs=0.001)
    res = tz.mcts_explore(g, tz.Platform(2), tz.EmpiricalBenchmarker(rt, ctrl), ctrl, o)
    assert res.best() >= 0 and res.failed == 0
    best = res.sims[res.best()].seq
    assert tz.verify(best, tz.resolve_graph(g, best), 2) == []
    rt.prepare(best)
    c.reset()
    rt.run(3)
    rt.device_sync()
    _check_accuracy(_reference(tz, m, 0), 3, c.x(), c.rr(), "search best")


def test_cli_search_then_run(gpu, tmp_path):
    path = tmp_path / "f.json"

    def cli(*args):
        r = subprocess.run([sys.executable, "-m", "tenzing_amd", *args], cwd=ROOT, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    s = cli("search", "--workload", "cg", "--cg-m", "20011", "--iters", "6", "--bench-iters", "3",
            "--target-secs", "0.001", "--mode", "graph", "--save-best", str(path))
    assert s["workload"] == "cg" and s["best_pct10_ms"] > 0
    doc = json.loads(path.read_text())
    assert doc["args"]["cg_m"] == 20011 and doc["args"]["cg_check_iters"] == 25
    r = cli("run", str(path), "--iters", "50", "--warmup", "5")
    assert r["correct"] and r["workload"] == "cg" and r["cg_check_iters"] == 25
    assert 0 <= r["cg_max_rel_err"] < 1e-4 and r["ms_per_iter"] > 0
