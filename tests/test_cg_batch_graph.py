"""Batched CG (``nrhs`` = 2, 4, 8 right-hand sides on the single-reduction form) without a GPU:
the graph it gives the search, which combinations are refused, the sequence of right-hand sides
(number 0 is the single solve's b, column j of a batch is number ``rhs_first + j``) and the cost
model's bytes."""
import json

import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import greedy_schedule

M, BW = 257, 16


def _cg(tz, **kw):
    kw.setdefault("m", M)
    kw.setdefault("bw", BW)
    return tz._tz.ConjugateGradient(CgConfig(**kw).args())


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _gpu_ops(tz, seq):
    return [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]


def test_builds_without_setup_and_is_two_ops(tz):
    c = tz._tz.ConjugateGradient(CgConfig(nrhs=4, form="sr", m=1037).args())
    assert not c.ready()
    g = tz._tz.Graph()
    c.add_to_graph(g)
    for seed in range(5):
        seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
        ops = _gpu_ops(tz, seq)
        assert [o.name for o in ops] == ["cg_s_spmvdot", "cg_s_update"]
        assert [o.unbound.kind for o in ops] == ["CgSpmvDot2", "CgSrUpdate"]
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []


def test_fields_in_args_json_and_config(tz):
    assert CgConfig().nrhs == 1 and CgConfig().rhs_first == 0
    a = CgConfig(m=M, bw=BW, form="sr", nrhs=4, rhs_first=3).args()
    assert a.nrhs == 4 and a.rhs_first == 3
    doc = json.loads(a.json())
    assert doc["nrhs"] == 4 and doc["rhs_first"] == 3
    d = json.loads(tz._tz.CgArgs().json())
    assert d["nrhs"] == 1 and d["rhs_first"] == 0
    assert tz._tz.ConjugateGradient(a).args.nrhs == 4


@pytest.mark.parametrize("kw,why", [
    (dict(nrhs=3, form="sr"), "1, 2, 4 or 8"),
    (dict(nrhs=0, form="sr"), "1, 2, 4 or 8"),
    (dict(nrhs=16, form="sr"), "1, 2, 4 or 8"),
    (dict(nrhs=2, form="fused"), "needs form sr"),
    (dict(nrhs=2, form="choice"), "needs form sr"),
    (dict(nrhs=2, form="all"), "needs form sr"),
    (dict(nrhs=2, form="plain"), "needs form sr"),
    (dict(nrhs=2, form="sr", rhs_first=-1), "rhs_first"),
])
def test_refused_with_the_reason(tz, kw, why):
    with pytest.raises(Exception, match=why):
        _cg(tz, **kw)


def test_right_hand_side_zero_is_todays_b(tz):
    b = _cg(tz).b()
    assert b.dtype == np.float32 and b.shape == (M,)
    assert np.array_equal(_bits(_cg(tz).b(0)), _bits(b))
    for kw in (dict(form="sr"), dict(form="sr", nrhs=2), dict(form="sr", nrhs=8), dict(form="fused")):
        c = _cg(tz, rhs_first=0, **kw)
        assert np.array_equal(_bits(c.b(0)), _bits(b)), kw
        assert np.array_equal(_bits(c.b()), _bits(b)), kw


def test_columns_are_the_sequence(tz):
    c8 = _cg(tz, form="sr", nrhs=8)
    cols = [c8.b(j) for j in range(8)]
    for j in range(8):
        one = _cg(tz, form="sr", nrhs=1, rhs_first=j)
        assert np.array_equal(_bits(cols[j]), _bits(one.b())), j
        assert cols[j].min() >= -1 and cols[j].max() < 1 and cols[j].std() > 0.3
    for i in range(8):
        for j in range(i + 1, 8):
            assert not np.array_equal(cols[i], cols[j]), (i, j)
    # a window of the sequence that starts elsewhere
    c4 = _cg(tz, form="sr", nrhs=4, rhs_first=3)
    for j in range(4):
        assert np.array_equal(_bits(c4.b(j)), _bits(cols[3 + j])), j
    # another seed, another sequence
    assert not np.array_equal(_cg(tz, form="sr", nrhs=2, seed=2).b(1), cols[1])


def test_zero_right_hand_sides(tz):
    z = _cg(tz, form="sr", nrhs=8, rhs="zero")
    for j in range(8):
        assert z.b(j).shape == (M,) and not z.b(j).any()


def test_out_of_range_column_raises(tz):
    c8 = _cg(tz, form="sr", nrhs=8)
    with pytest.raises(Exception, match="out of range"):
        c8.b(8)
    with pytest.raises(Exception, match="out of range"):
        c8.b(-1)
    with pytest.raises(Exception, match="out of range"):
        _cg(tz).b(1)


def test_sim_search_finds_a_verified_schedule(tz):
    c, g = build_cg(CgConfig(m=1037, form="sr", nrhs=4), setup=False)
    assert not c.ready()
    res = tz.search(g, streams=2, iters=10, sim=True)
    assert res.best() >= 0 and len(res.sims) > 0
    best = res.sims[res.best()].seq
    assert tz.verify(best, tz.resolve_graph(g, best), 2) == []
    assert [o.name for o in _gpu_ops(tz, best)] == ["cg_s_spmvdot", "cg_s_update"]


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_cost_model_bytes(tz, k):
    """the matrix (8 bytes per entry) once, every gather and every vector k times as wide; k = 1
    is the single form's 12 nnz + 8 n and 36 n"""
    n = 1037
    c, g = build_cg(CgConfig(m=n, form="sr", nrhs=k), setup=False)
    nnz = c.args.nnz_actual
    ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1)))]
    assert ops[0].bytes == 8.0 * nnz + 4.0 * nnz * k + 8.0 * n * k
    assert ops[1].bytes == 36.0 * n * k
    assert ops[0].cost_us == pytest.approx(4.5 + ops[0].bytes / 3.0e6, rel=1e-12)
    assert ops[1].cost_us == pytest.approx(3.5 + ops[1].bytes / 4.0e6, rel=1e-12)


def test_cli_parser_keeps_cg_nrhs(tz):
    from tenzing_amd import cli

    a = cli._parser().parse_args(["search", "--workload", "cg", "--cg-form", "sr", "--cg-nrhs", "4"])
    assert a.cg_nrhs == 4
    assert "cg_nrhs" in cli._WORKLOAD_KEYS
    w = cli._saved_args({k: getattr(a, k) for k in cli._WORKLOAD_KEYS})
    assert w.cg_nrhs == 4 and w.cg_form == "sr"
    # a document saved before the option existed
    old = {k: getattr(a, k) for k in cli._WORKLOAD_KEYS if k != "cg_nrhs"}
    assert cli._saved_args(old).cg_nrhs == 1
