"""The stopping option of the single-reduction CG form (``CgConfig(form="sr", tol=...)``) without
a GPU: which combinations are refused, that the graph the search sees is the one of ``tol=0``
(same ops, names, kinds and costs), the threshold the host forms, and the command line."""
import json
import math

import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import greedy_schedule

M, BW = 257, 16


def _cg(tz, **kw):
    kw.setdefault("m", M)
    kw.setdefault("bw", BW)
    return tz._tz.ConjugateGradient(CgConfig(**kw).args())


def _gpu_ops(tz, seq):
    return [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]


@pytest.mark.parametrize("form", ["plain", "fused", "choice", "all"])
def test_tol_needs_the_single_reduction_form(tz, form):
    with pytest.raises(Exception, match="tol > 0 needs form sr"):
        _cg(tz, form=form, tol=1e-6)
    _cg(tz, form=form, tol=0.0)  # the default is accepted everywhere


@pytest.mark.parametrize("tol", [-1e-6, -1.0, float("nan"), float("inf"), -float("inf")])
def test_negative_or_non_finite_tol_raises(tz, tol):
    with pytest.raises(Exception, match="tol must be finite and not negative"):
        _cg(tz, form="sr", tol=tol)


@pytest.mark.parametrize("nrhs", [1, 2, 4, 8])
def test_same_graph_as_without_tol(tz, nrhs):
    descr = []
    for tol in (0.0, 1e-6):
        c, g = build_cg(CgConfig(m=1037, form="sr", nrhs=nrhs, tol=tol), setup=False)
        assert not c.ready()
        ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1)))]
        descr.append([(o.name, o.kind, o.cost_us, o.bytes) for o in ops])
        for seed in range(5):
            seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
            assert [o.name for o in _gpu_ops(tz, seq)] == ["cg_s_spmvdot", "cg_s_update"]
            assert [o.unbound.kind for o in _gpu_ops(tz, seq)] == ["CgSpmvDot2", "CgSrUpdate"]
            assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []
    assert descr[0] == descr[1]
    assert [d[:2] for d in descr[0]] == [("cg_s_spmvdot", "CgSpmvDot2"), ("cg_s_update", "CgSrUpdate")]


def test_fields_in_args_json_and_config(tz):
    assert CgConfig().tol == 0.0
    assert json.loads(tz._tz.CgArgs().json())["tol"] == 0.0
    a = CgConfig(m=M, bw=BW, form="sr", tol=1e-6).args()
    assert a.tol == 1e-6
    assert json.loads(a.json())["tol"] == 1e-6
    assert tz._tz.ConjugateGradient(a).args.tol == 1e-6


def test_threshold_is_tol_squared_times_b_dot_b(tz):
    """the sum of squares in f64 in index order, then one product with tol * tol"""
    tol = 1e-5
    c = _cg(tz, form="sr", nrhs=4, rhs_first=2, tol=tol)
    for j in range(4):
        bb = 0.0
        for v in c.b(j).astype(np.float64):
            bb += float(v) * float(v)
        assert c.threshold(j) == tol * tol * bb
        assert c.threshold(j) > 0
    assert _cg(tz, form="sr", rhs="zero", tol=tol).threshold() == 0.0
    with pytest.raises(Exception, match="out of range"):
        c.threshold(4)
    with pytest.raises(Exception, match="tol = 0"):
        _cg(tz, form="sr").threshold()


def test_accessors_need_setup_and_tol(tz):
    c = _cg(tz, form="sr", tol=1e-6)
    for f in (c.iterations, c.converged, lambda: c.set_armed(False)):
        with pytest.raises(Exception, match="not set up"):
            f()
    assert c.armed()


def test_solve_checks_its_arguments(tz):
    from tenzing_amd.models.cg import solve

    c = _cg(tz, form="sr")
    with pytest.raises(ValueError, match="tol > 0"):
        solve(c, None, 10)
    c = _cg(tz, form="sr", tol=1e-6)
    with pytest.raises(ValueError, match="check_every"):
        solve(c, None, 10, check_every=0)
    with pytest.raises(ValueError, match="max_iters"):
        solve(c, None, -1)


def test_cli_parser_keeps_cg_tol(tz):
    from tenzing_amd import cli

    a = cli._parser().parse_args(["search", "--workload", "cg"])
    assert a.cg_tol == 0.0 and a.cg_max_iters == 1000
    a = cli._parser().parse_args(["search", "--workload", "cg", "--cg-form", "sr", "--cg-tol", "1e-5",
                                  "--cg-max-iters", "300"])
    assert a.cg_tol == 1e-5 and a.cg_max_iters == 300
    assert "cg_tol" in cli._WORKLOAD_KEYS
    w = cli._saved_args({k: getattr(a, k) for k in cli._WORKLOAD_KEYS})
    assert w.cg_tol == 1e-5 and w.cg_max_iters == 300 and w.cg_form == "sr"
    # a document saved before the option existed
    old = {k: getattr(a, k) for k in cli._WORKLOAD_KEYS if k not in ("cg_tol", "cg_max_iters")}
    w = cli._saved_args(old)
    assert w.cg_tol == 0.0 and w.cg_max_iters == 1000
    assert not math.isnan(w.cg_tol)
