"""Jacobi-preconditioned single-reduction CG (``CgConfig(form="sr", precond="jacobi")``) on the GPU.

Host models, built in this file from ``matrix()``, ``b()`` and ``dinv()`` (never from ``check()``):
``HostPcg`` runs the preconditioned Chronopoulos-Gear recurrence with the kernels' guards, once in
f64 and once with f32 vectors, f64 dot products and coefficients rounded to f32, as the device
does. e32(k) = max|x32 - x64| / max|x64| is what f32 storage costs this recurrence; the device must
stay within 8 x max(e32(k), 2^-23) for x at k = 1, 3, 5 (the criterion and the constant of
test_gpu_cg.py and test_gpu_cg_sr.py), and after 25 more iterations ``residual()`` within 8 x the
f32 model's. All systems but the unscaled side of the change-of-units test are posed with
``diag_scale=2``, where the preconditioner matters.

The stopping tests follow test_gpu_cg_tol.py: the oracle is the same preconditioned form with
``tol=0``, eager, one iteration at a time, rho_k = r_k . r_k formed in numpy f64 from the downloaded
r, k* = min{k : rho_k <= thresh}, after the condition that no rho_k up to the stop lies within a
relative 1e-6 of the threshold.

Measured on an MI355X over every case of this file: worst e_dev / max(e32, 2^-23) 0.91 for x (m =
20 011, k = 5), worst residual ratio 0.94 against the f32 model; the change of units is bit-exact
in eager mode and under hipGraphs; k* = 6 (tol 1e-3) and 10 (tol 1e-5) on all three shapes, the
nearest rho_k 0.41 to 0.71 x thresh away from its threshold; at m = 1037, diag_scale = 2, tol = 1e-5
the preconditioned solve takes 10 iterations while the unpreconditioned form after 40 still has
r.r = 1.3e7 x its threshold.
"""
import functools

import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.models.cg import solve
from tenzing_amd.search import greedy_schedule
from test_gpu_cg_sr import HostSrCg, _div, _Host

pytestmark = pytest.mark.gpu

SHAPES = [(50, 8), (1037, 0), (20_011, 0)]
MODES = [("eager", 1), ("graph", 1), ("graph", 3)]
TOLS = [1e-3, 1e-5]
EPS = 2.0 ** -23
BAND = 1e-6
D = 2  # diag_scale of the systems solved here
REF_ITERS = 24  # iterations of the reference run: every k* + 5 of this file lies below (asserted)


class HostPcg(_Host):
    """u = dinv o r; w = A u; gamma = r.u, delta = u.w; beta = gamma / gamma_prev; alpha = gamma /
    (delta - beta gamma / alpha_prev); p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s,
    u = dinv o r; every division guarded, from gamma_prev = alpha_prev = 0 and s = 0. In the f32 run
    u is the f32 product of two f32 values, as the device stores it."""

    def __init__(self, rp, ci, val, b, dinv, f32):
        super().__init__(rp, ci, val, b, f32)
        self.dinv = np.asarray(dinv, dtype=np.float32).astype(self.t)
        self.s = np.zeros(len(self.b), dtype=self.t)
        self.u = self.dinv * self.r
        self.gamma_prev = self.alpha_prev = 0.0

    def step(self):
        d = np.float64
        w = self.matvec(self.u)
        gamma = float(np.dot(self.r.astype(d), self.u.astype(d)))
        delta = float(np.dot(self.u.astype(d), w.astype(d)))
        beta = _div(gamma, self.gamma_prev)
        alpha = _div(gamma, delta - beta * _div(gamma, self.alpha_prev))
        bt, a = self.coef(beta), self.coef(alpha)
        self.p = self.fma(bt, self.p, self.u)
        self.s = self.fma(bt, self.s, w)
        self.x = self.fma(a, self.p, self.x)
        self.r = self.fma(-a, self.s, self.r)
        self.u = self.dinv * self.r
        self.gamma_prev, self.alpha_prev = gamma, alpha
        self.k += 1


def _cfg(m, bw, **kw):
    kw.setdefault("diag_scale", D)
    kw.setdefault("precond", "jacobi")
    return CgConfig(m=m, bw=bw, form="sr", **kw)


def _system(tz, m, bw, **kw):
    """(rowPtr, colInd, val), b, dinv of the system a config poses, from the accessors"""
    c = tz._tz.ConjugateGradient(_cfg(m, bw, **kw).args())
    return c.matrix(), c.b(), c.dinv() if c.args.precond == "jacobi" else None


@functools.lru_cache(maxsize=None)
def _host_reference(tz, m, bw):
    """per shape, once: k -> (x64, e32) for k = 1, 3, 5, and the f32 model's true residual after 30"""
    (rp, ci, val), b, dinv = _system(tz, m, bw)
    h64, h32 = HostPcg(rp, ci, val, b, dinv, False), HostPcg(rp, ci, val, b, dinv, True)
    at = {}
    for k in range(1, 31):
        h64.step()
        h32.step()
        if k in (1, 3, 5):
            at[k] = (h64.x.copy(), float(np.abs(h32.x - h64.x).max() / np.abs(h64.x).max()))
    return {"at": at, "res32": h64.residual(h32.x.astype(np.float64)), "host": h64}


def _runtime(tz, gpu, streams, mode, unroll=1):
    return tz.HipRuntime(device=gpu, n_streams=streams,
                         mode=tz.ExecMode.Graph if mode == "graph" else tz.ExecMode.Eager,
                         graph_unroll=unroll)


def _schedule(tz, g, spmv_stream=0, update_stream=1):
    return greedy_schedule(g, tz.Platform(2), {"cg_form": "cg_sr"},
                           stream_for=lambda name: update_stream if name.endswith("_update") else spmv_stream)


def _build(tz, gpu, m, bw, mode="eager", unroll=1, placement=(0, 1), **kw):
    c, g = build_cg(_cfg(m, bw, **kw), None, gpu)
    seq = _schedule(tz, g, *placement)
    ops = [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]
    assert [o.name for o in ops] == ["cg_s_spmvdot", "cg_s_update"]
    if c.args.precond == "jacobi":
        assert [o.unbound.kind for o in ops] == ["CgPcgSpmvDot3", "CgPcgUpdate"]
    rt = _runtime(tz, gpu, 2, mode, unroll)
    rt.prepare(seq)
    assert (rt.effective_mode == tz.ExecMode.Graph) == (mode == "graph")
    return c, rt


def _state(c):
    return c.x(), c.r(), c.p(), c.u()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_against_the_host_models(tz, gpu, m, bw, mode, unroll):
    ref = _host_reference(tz, m, bw)
    c, rt = _build(tz, gpu, m, bw, mode, unroll)
    for k in (1, 3, 5):
        c.reset()
        rt.run(k)
        rt.device_sync()
        x64, e32 = ref["at"][k]
        e_dev = np.abs(c.x().astype(np.float64) - x64).max() / np.abs(x64).max()
        ratio = e_dev / max(e32, EPS)
        print(f"pcg accuracy m={m} {mode}/{unroll} k={k}: e_dev={e_dev:.3e} e32={e32:.3e} "
              f"e_dev/max(e32,eps)={ratio:.3f} check(k)={c.check(k):.3e}")
        assert ratio <= 8.0, (k, ratio)
    rt.run(25)
    rt.device_sync()
    x = c.x()
    assert np.isfinite(x).all()
    res, want = c.residual(), ref["host"].residual(x)
    print(f"pcg residual m={m} {mode}/{unroll}: dev={res:.3e} numpy={want:.3e} f32 model={ref['res32']:.3e} "
          f"(x{res / ref['res32']:.3f})")
    assert abs(res - want) <= 1e-9 * want
    assert res <= 8.0 * ref["res32"]
    del rt


@pytest.mark.parametrize("m,bw", SHAPES)
def test_u_is_dinv_times_r_bit_for_bit(tz, gpu, m, bw):
    c, rt = _build(tz, gpu, m, bw, "eager")
    dinv = c.dinv()
    assert dinv.dtype == np.float32
    assert _same([c.u()], [dinv * c.b()]) and _same([c.r()], [c.b()])  # the start state
    assert not c.x().any()
    for k in range(1, 7):
        rt.run(1)
        rt.device_sync()
        r, u = c.r(), c.u()
        assert _same([u], [dinv * r]), k  # numpy's f32 product: one rounding
        assert np.isfinite(u).all() and u.any()
    c.reset()
    assert _same([c.u()], [dinv * c.b()])
    del rt


@pytest.mark.parametrize("mode,unroll", [("eager", 1), ("graph", 3)])
@pytest.mark.parametrize("m,bw", SHAPES[:2])
def test_change_of_units_is_exact(tz, gpu, m, bw, mode, unroll):
    """(S A S) y = S b against A x = b after 12 iterations: y = x / s and r' = r s bit for bit, since
    every quantity of the preconditioned recurrence scales by an exact power of two while gamma and
    delta keep their bits"""
    k = 12
    c0, rt0 = _build(tz, gpu, m, bw, mode, unroll, diag_scale=0)
    c2, rt2 = _build(tz, gpu, m, bw, mode, unroll, diag_scale=2)
    s = c2.scale()
    assert len(set(s.tolist())) > 1 and np.array_equal(c0.scale(), np.ones(m, dtype=np.float32))
    rt0.run(k)
    rt2.run(k)
    rt0.device_sync()
    rt2.device_sync()
    x, r, x2, r2 = c0.x(), c0.r(), c2.x(), c2.r()
    assert x.any() and r.any()
    # exact: a power of two times an f32 value well inside the normal range
    assert _same([x2], [x / s])
    assert _same([r2], [r * s])
    assert _same([c2.u()], [c0.u() / s])
    del rt0, rt2


@functools.lru_cache(maxsize=None)
def _reference(tz, gpu, m, bw):
    """the oracle of the stopping tests, once per shape and never changed: the preconditioned form
    with tol = 0, eager, one iteration at a time; k -> (x, r, p, u) and rho_k"""
    c, rt = _build(tz, gpu, m, bw, "eager")
    states, rho = [], []
    for k in range(REF_ITERS + 1):
        if k:
            rt.run(1)
            rt.device_sync()
        states.append(_state(c))
        r = states[-1][1].astype(np.float64)
        rho.append(float(np.dot(r, r)))
    del rt
    return {"states": states, "rho": rho}


@functools.lru_cache(maxsize=None)
def _threshold(tz, m, bw, tol, **kw):
    return tz._tz.ConjugateGradient(_cfg(m, bw, tol=tol, **kw).args()).threshold()


def _kstar(ref, thresh):
    ks = [k for k, v in enumerate(ref["rho"]) if v <= thresh]
    assert ks and ks[0] + 5 <= REF_ITERS, "the reference run is too short for this threshold"
    k = ks[0]
    gap = min(abs(v - thresh) for v in ref["rho"][:k + 1])
    print(f"k*={k} rho_k*={ref['rho'][k]:.3e} thresh={thresh:.3e} nearest rho: {gap / thresh:.2e} x thresh away")
    assert gap > BAND * thresh, "a rho_k lies in the band around the threshold: change the seed, not the band"
    return k


@pytest.mark.parametrize("mode,unroll", MODES)
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_solve_stops_where_the_reference_crosses_and_stays_there(tz, gpu, m, bw, tol, mode, unroll):
    ref = _reference(tz, gpu, m, bw)
    thresh = _threshold(tz, m, bw, tol)
    ks = _kstar(ref, thresh)  # the condition first
    assert 0 < ks
    c, rt = _build(tz, gpu, m, bw, mode, unroll, tol=tol)
    assert c.threshold() == thresh and c.armed()
    assert c.iterations() == 0 and not c.converged()
    sol = solve(c, rt, 200)
    assert sol.iterations == [ks] and sol.converged == [True]
    assert ks < sol.launched <= ks + 8
    assert _same(_state(c), ref["states"][ks])
    for _ in range(7):  # frozen: one launch pair at a time changes nothing
        rt.run(1)
    rt.device_sync()
    assert _same(_state(c), ref["states"][ks])
    assert c.iterations() == ks and c.converged()
    del rt


def test_check_every_and_placement_do_not_matter(tz, gpu):
    m, bw, tol = 1037, 0, 1e-5
    ref = _reference(tz, gpu, m, bw)
    ks = _kstar(ref, _threshold(tz, m, bw, tol))
    for mode, unroll in MODES:
        for placement in ((0, 0), (0, 1), (1, 0), (1, 1)):
            c, rt = _build(tz, gpu, m, bw, mode, unroll, placement, tol=tol)
            sol = solve(c, rt, 200)
            assert sol.iterations == [ks] and sol.converged == [True], (mode, unroll, placement)
            assert _same(_state(c), ref["states"][ks]), (mode, unroll, placement)
            del rt
    c, rt = _build(tz, gpu, m, bw, "graph", 3, tol=tol)
    launched = []
    for every in (1, 3, 8):
        c.reset()
        sol = solve(c, rt, 200, check_every=every)
        assert sol.iterations == [ks] and sol.converged == [True], every
        assert _same(_state(c), ref["states"][ks]), every
        assert ks < sol.launched <= ks + every
        launched.append(sol.launched)
    assert launched[0] == ks + 1  # the update after iteration k* finds rho_k* <= thresh
    # disarmed, the stopping kernels are the tol = 0 pair
    c.reset()
    c.set_armed(False)
    rt.run(ks + 5)
    rt.device_sync()
    assert _same(_state(c), ref["states"][ks + 5]) and c.iterations() == ks + 5 and not c.converged()
    del rt


def _host_iterations(h, thresh, cap):
    """iterations until the recurrence's own r . r <= thresh, or None after `cap`"""
    for k in range(cap + 1):
        if h.rr <= thresh:
            return k
        h.step()
    return None


def test_it_pays(tz, gpu):
    """the same problem in badly chosen units: the preconditioned solve converges where the
    unpreconditioned one, given four times the iterations, does not"""
    m, bw, tol = 1037, 0, 1e-5
    (rp, ci, val), b, dinv = _system(tz, m, bw)
    thresh = _threshold(tz, m, bw, tol)
    assert thresh == _threshold(tz, m, bw, tol, precond="none")  # the same criterion for both
    # the conditions, on host models alone
    kp = _host_iterations(HostPcg(rp, ci, val, b, dinv, False), thresh, 100)
    assert kp is not None and kp > 0
    plain = HostSrCg(rp, ci, val, b, True)
    stalled = _host_iterations(plain, thresh, 4 * kp) is None
    print(f"it pays m={m} diag_scale={D} tol={tol}: f64 host PCG {kp} iterations; f32 host sr after {4 * kp}: "
          f"rr / thresh = {plain.rr / thresh:.3e}")
    assert stalled
    # the device
    ks = _kstar(_reference(tz, gpu, m, bw), thresh)
    c, rt = _build(tz, gpu, m, bw, "graph", 1, tol=tol)
    sol = solve(c, rt, 200)
    assert sol.converged == [True] and sol.iterations == [ks]
    print(f"it pays: device PCG {ks} iterations, residual {sol.residual[0]:.3e}")
    del rt
    c, rt = _build(tz, gpu, m, bw, "graph", 1, tol=tol, precond="none")
    sol = solve(c, rt, 4 * kp)
    assert sol.converged == [False] and sol.iterations == [4 * kp] and sol.launched == 4 * kp
    print(f"it pays: device sr after {4 * kp} iterations: rr / thresh = {c.rr() / thresh:.3e}")
    del rt
