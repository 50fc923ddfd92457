"""Mixed-precision iterative refinement of the CG workload (``CgConfig(form="sr", tol=t,
refine_tol=e)``) without a GPU: which combinations are refused and why, the field in config, args
and json, the graph the search sees (the one of the same config without refinement), the command
line, and the numpy model of the refined solve on the project's own systems.

The model (cg_refine_model.HostRefine: f32 inner solves by the host models of the sr and pcg
tests, x64 and b - A x64 in f64) is the condition of test_gpu_cg_refine.py: on every system that
test solves, the model must be refined within cap = ceil(log(refine_tol) / log(tol)) + 1 steps,
and the plain f32 recurrence run for as many iterations must still have a true residual above
1e-8. Counts of the model, refine_step() calls (the last one finds the solve refined) / inner
iterations, the same for ``none`` on diag_scale 0 and ``jacobi`` on diag_scale 2 unless two are
given (none, jacobi):

    (m, bw)        tol   refine_tol  cap  steps  inner iterations   ||r64||/||b|| after each step (none)
    (50, 8)        1e-3  1e-9        4    3      23, 19             9.8e-4 6.6e-7 4.0e-10
    (50, 8)        1e-3  1e-12       5    4      31, 26             ... 3.3e-13
    (50, 8)        1e-5  1e-9        3    2      24, 21             7.2e-6 6.5e-11
    (50, 8)        1e-5  1e-12       4    3      37, 31             ... 2.1e-16
    (1037, 0)      1e-3  1e-9        4    3      30, 20             9.4e-4 9.2e-7 4.8e-10
    (1037, 0)      1e-3  1e-12       5    4      40, 27             ... 3.9e-13
    (1037, 0)      1e-5  1e-9        3    2      33, 20             6.3e-6 2.7e-11
    (1037, 0)      1e-5  1e-12       4    3      49, 30             ... 2.8e-16
    (20 011, 0)    1e-3  1e-9        4    3      41, 19             7.7e-4 5.5e-7 3.2e-10
    (20 011, 0)    1e-3  1e-12       5    4      55, 26             ... 2.4e-13
    (20 011, 0)    1e-5  1e-9        3    2      44, 20             7.0e-6 4.1e-11
    (20 011, 0)    1e-5  1e-12       4    3      68, 31             ... 2.8e-16

Every step cuts the true residual by about the inner tol, and the model always needs one step
fewer than the cap. The f64 evaluation error of the residual check itself (check_floor) is 5e-15 to
9e-15 on these systems.
"""
import functools
import json
import math

import numpy as np
import pytest

from cg_refine_model import REFINE_TOLS, SHAPES, SYSTEMS, TOLS, HostRefine, cap, check_floor
from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.models.cg import CgSolve
from tenzing_amd.search import greedy_schedule
from test_gpu_cg_sr import HostSrCg
from test_gpu_pcg import HostPcg

M, BW = 257, 16


def _cg(tz, **kw):
    kw.setdefault("m", M)
    kw.setdefault("bw", BW)
    return tz._tz.ConjugateGradient(CgConfig(**kw).args())


def _gpu_ops(tz, seq):
    return [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]


@pytest.mark.parametrize("form", ["plain", "fused", "choice", "all"])
@pytest.mark.parametrize("tol", [0.0, 1e-5])
def test_refinement_needs_the_single_reduction_form(tz, form, tol):
    with pytest.raises(Exception, match="refine_tol > 0 needs form sr: the refinement step restarts"):
        _cg(tz, form=form, tol=tol, refine_tol=1e-9)


@pytest.mark.parametrize("nrhs", [2, 4, 8])
def test_refinement_needs_one_right_hand_side(tz, nrhs):
    with pytest.raises(Exception, match="refine_tol > 0 needs nrhs 1: batched refinement is not built"):
        _cg(tz, form="sr", nrhs=nrhs, tol=1e-5, refine_tol=1e-9)
    _cg(tz, form="sr", nrhs=nrhs, tol=1e-5)


def test_refinement_needs_an_inner_tolerance(tz):
    with pytest.raises(Exception, match="refine_tol > 0 needs tol > 0: tol is the inner solve's relative tolerance"):
        _cg(tz, form="sr", refine_tol=1e-9)


@pytest.mark.parametrize("refine_tol", [1e-5, 1e-3, 1.0])
def test_refine_tol_must_be_below_tol(tz, refine_tol):
    with pytest.raises(Exception, match="refine_tol must be below tol"):
        _cg(tz, form="sr", tol=1e-5, refine_tol=refine_tol)


@pytest.mark.parametrize("refine_tol", [-1e-9, float("nan"), float("inf")])
def test_refine_tol_must_be_finite_and_not_negative(tz, refine_tol):
    with pytest.raises(Exception, match="refine_tol must be finite and not negative"):
        _cg(tz, form="sr", tol=1e-5, refine_tol=refine_tol)


def test_existing_refusals_keep_their_messages(tz):
    with pytest.raises(Exception, match="CG with tol > 0 needs form sr"):
        _cg(tz, form="fused", tol=1e-5)
    with pytest.raises(Exception, match="only the single-reduction form for one right-hand side has preconditioned"):
        _cg(tz, form="sr", nrhs=2, precond="jacobi")


def test_fields_in_args_json_and_config(tz):
    assert CgConfig().refine_tol == 0.0
    assert json.loads(tz._tz.CgArgs().json())["refine_tol"] == 0.0
    a = CgConfig(m=M, bw=BW, form="sr", tol=1e-4, refine_tol=1e-11).args()
    assert a.refine_tol == 1e-11 and a.tol == 1e-4
    assert json.loads(a.json())["refine_tol"] == 1e-11
    c = tz._tz.ConjugateGradient(a)
    assert c.args.refine_tol == 1e-11
    bb = 0.0
    for v in c.b().astype(np.float64):
        bb += float(v) * float(v)
    assert c.outer_threshold() == 1e-11 * 1e-11 * bb and c.threshold() == 1e-4 * 1e-4 * bb
    s = CgSolve([3], [True], 8, [])
    assert (s.outer_steps, s.refined, s.residual64) == (0, False, None)


def test_accessors_without_refinement_or_setup_raise(tz):
    plain = _cg(tz, form="sr", tol=1e-5)
    for name in ("x64", "r64", "outer_steps", "refined", "inner_threshold", "rr64", "outer_threshold",
                 "residual64", "refine_step"):
        with pytest.raises(Exception, match="refine_tol = 0"):
            getattr(plain, name)()
    c = _cg(tz, form="sr", tol=1e-5, refine_tol=1e-9)
    for name in ("x64", "r64", "outer_steps", "refined", "inner_threshold", "residual64", "refine_step"):
        with pytest.raises(Exception, match="not set up"):
            getattr(c, name)()


@pytest.mark.parametrize("precond,d", SYSTEMS)
def test_the_graph_is_the_one_without_refinement(tz, precond, d):
    def descr(**kw):
        c, g = build_cg(CgConfig(m=1037, form="sr", tol=1e-5, precond=precond, diag_scale=d, **kw), setup=False)
        assert not c.ready()
        ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1)))]
        return g, [(o.name, o.kind, o.cost_us, o.bytes) for o in ops]

    g, with_refine = descr(refine_tol=1e-10)
    assert with_refine == descr()[1]
    assert [d[0] for d in with_refine] == ["cg_s_spmvdot", "cg_s_update"]
    for seed in range(5):
        seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
        assert [o.name for o in _gpu_ops(tz, seq)] == ["cg_s_spmvdot", "cg_s_update"]
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []


def test_cli_parser_and_saved_args(tz):
    from tenzing_amd import cli

    a = cli._parser().parse_args(["search", "--workload", "cg"])
    assert a.cg_refine_tol == 0.0
    a = cli._parser().parse_args(["search", "--workload", "cg", "--cg-form", "sr", "--cg-tol", "1e-4",
                                  "--cg-refine-tol", "1e-11"])
    assert a.cg_refine_tol == 1e-11 and a.cg_tol == 1e-4
    assert "cg_refine_tol" in cli._WORKLOAD_KEYS
    w = cli._saved_args({k: getattr(a, k) for k in cli._WORKLOAD_KEYS})
    assert w.cg_refine_tol == 1e-11 and w.cg_tol == 1e-4 and w.cg_form == "sr"
    # through JSON, as a saved schedule keeps them
    w = cli._saved_args(json.loads(json.dumps({k: getattr(a, k) for k in cli._WORKLOAD_KEYS})))
    assert w.cg_refine_tol == 1e-11
    # a document saved before the option existed
    w = cli._saved_args({k: getattr(a, k) for k in cli._WORKLOAD_KEYS if k != "cg_refine_tol"})
    assert w.cg_refine_tol == 0.0


def test_cli_sim_search_with_refinement(tz, capsys):
    from tenzing_amd import cli

    rc = cli.main(["search", "--workload", "cg", "--sim", "--cg-form", "sr", "--cg-tol", "1e-5", "--cg-refine-tol",
                   "1e-12", "--cg-precond", "jacobi", "--cg-diag-scale", "2", "--cg-m", "1037", "--iters", "4",
                   "--bench-iters", "2", "--streams", "2"])
    assert rc == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["workload"] == "cg" and out["best_pct10_ms"] > 0 and math.isfinite(out["best_pct10_ms"])


def test_cap():
    assert [cap(t, e) for t in TOLS for e in REFINE_TOLS] == [4, 5, 3, 4]


@functools.lru_cache(maxsize=None)
def _system(tz, m, bw, precond, d):
    c = tz._tz.ConjugateGradient(CgConfig(m=m, bw=bw, form="sr", precond=precond, diag_scale=d).args())
    return c.matrix(), c.b(), c.dinv() if precond == "jacobi" else None


@pytest.mark.parametrize("precond,d", SYSTEMS)
@pytest.mark.parametrize("m,bw", SHAPES)
def test_the_model_is_refined_within_the_cap(tz, m, bw, precond, d):
    (rp, ci, val), b, dinv = _system(tz, m, bw, precond, d)
    most = 0
    for tol in TOLS:
        for refine_tol in REFINE_TOLS:
            h = HostRefine(rp, ci, val, b, dinv, tol, refine_tol).solve(cap(tol, refine_tol))
            print(f"model m={m} {precond} d={d} tol={tol} refine_tol={refine_tol}: cap {cap(tol, refine_tol)} "
                  f"steps {h.steps} inner {h.inner_iters} history {' '.join(f'{v:.1e}' for v in h.history)}")
            assert h.refined and h.steps <= cap(tol, refine_tol)
            # the check can see refine_tol at all: its own f64 evaluation error lies far below
            assert check_floor(rp, ci, val, b, h.x64) < 0.1 * refine_tol
            # each step but the last gains at least a factor 10 tol (about tol, measured)
            assert all(b1 <= 10 * tol * b0 for b0, b1 in zip(h.history[:-2], h.history[1:-1]))
            most = max(most, h.inner_iters)
    # what refinement buys: the f32 recurrence alone, given the most iterations any refined solve
    # took, is still above 1e-8
    plain = HostSrCg(rp, ci, val, b, True) if dinv is None else HostPcg(rp, ci, val, b, dinv, True)
    for _ in range(most):
        plain.step()
    res = plain.residual(plain.x.astype(np.float64))
    print(f"model m={m} {precond}: f32 recurrence after {most} iterations: residual {res:.3e}")
    assert res > 1e-8
