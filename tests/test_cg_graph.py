"""The conjugate-gradient workload without a GPU: its SPD matrix generator, the graph it gives
the search (forms, op counts, race-free schedules, the x update free to overlap the r chain)
and the cost model's view of it."""
import numpy as np
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import choice_alternatives, greedy_schedule

SHAPES = [(50, 8), (257, 16), (1037, 1037)]


def _dense(tz, n, bw):
    rp, ci, v = tz._tz.spd_band_matrix(n, bw, 5 * n, 1)
    rp, ci, v = np.array(rp), np.array(ci), np.array(v, dtype=np.float32)
    A = np.zeros((n, n), dtype=np.float32)
    present = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(rp))
    A[rows, ci] = v
    present[rows, ci] = True
    return rp, ci, v, A, present


@pytest.mark.parametrize("n,bw", SHAPES)
def test_spd_band_matrix(tz, n, bw):
    rp, ci, v, A, present = _dense(tz, n, bw)
    assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) == len(v)
    for r in range(n):  # rows sorted, no duplicates, inside the band
        c = ci[rp[r]:rp[r + 1]]
        assert np.all(np.diff(c) > 0), r
        assert c.min() >= max(0, r - bw) and c.max() <= min(n - 1, r + bw)
    assert np.array_equal(present, present.T)
    assert np.array_equal(A.view(np.uint32), A.T.view(np.uint32))  # mirrored values bit-equal
    assert present.sum() > n  # not only the diagonal
    d = A.diagonal().astype(np.float64)
    off = np.abs(A.astype(np.float64)).sum(axis=1) - np.abs(d)
    assert np.all(d - off >= 1 - 1e-5 * d)
    # the off-diagonal pattern is random_band_matrix's, mirrored
    brp, bci, _ = tz._tz.random_band_matrix(n, bw, 5 * n, 1)
    B = np.zeros((n, n), dtype=bool)
    B[np.repeat(np.arange(n), np.diff(np.array(brp))), np.array(bci)] = True
    np.fill_diagonal(B, False)
    P = present.copy()
    np.fill_diagonal(P, False)
    assert np.array_equal(P, B | B.T)
    again = tz._tz.spd_band_matrix(n, bw, 5 * n, 1)
    assert list(again[0]) == list(rp) and list(again[1]) == list(ci)
    assert np.array_equal(np.array(again[2], dtype=np.float32).view(np.uint32), v.view(np.uint32))


def _gpu_ops(tz, seq):
    return [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]


def test_forms_and_op_counts(tz):
    _, g = build_cg(CgConfig(m=1037), setup=False)
    assert choice_alternatives(g, "cg_form") == ["cg_plain", "cg_fused"]
    for form, count in (("fused", 4), ("plain", 8)):
        _, gf = build_cg(CgConfig(m=1037, form=form), setup=False)
        assert choice_alternatives(gf, "cg_form") == []
        for seed in range(5):
            seq = tz.random_rollout(tz.State(gf, tz.Platform(2)), seed)
            assert len(_gpu_ops(tz, seq)) == count
            assert tz.verify(seq, tz.resolve_graph(gf, seq), 2) == []
    plain = [o.name for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1), {"cg_form": "cg_plain"}))]
    assert sorted(plain) == sorted(["cg_spmv", "cg_dot_pq", "cg_alpha", "cg_x", "cg_r", "cg_dot_rr",
                                    "cg_beta", "cg_p"])
    # every true dependency orders the plain form: the SpMV first, p's update last, alpha before
    # both updates, the rr chain in order
    at = {n: i for i, n in enumerate(plain)}
    assert at["cg_spmv"] == 0 and at["cg_p"] == 7
    assert at["cg_dot_pq"] < at["cg_alpha"] < min(at["cg_x"], at["cg_r"])
    assert at["cg_r"] < at["cg_dot_rr"] < at["cg_beta"]


@pytest.mark.parametrize("streams", [2, 3])
def test_rollouts_are_race_free_and_overlap_the_x_update(tz, streams):
    _, g = build_cg(CgConfig(m=1037), setup=False)
    plat = tz.Platform(streams)
    forms, split = set(), set()
    for seed in range(60):
        seq = tz.random_rollout(tz.State(g, plat), seed)
        assert tz.verify(seq, tz.resolve_graph(g, seq), streams) == []
        ops = {o.name: o.stream for o in _gpu_ops(tz, seq)}
        form = "fused" if "cg_f_spmvdot" in ops else "plain"
        assert len(ops) == (4 if form == "fused" else 8)
        forms.add(form)
        x, r = ("cg_f_x", "cg_f_r") if form == "fused" else ("cg_x", "cg_r")
        if ops[x] != ops[r]:
            split.add(form)
    assert forms == {"plain", "fused"}
    # the graph does not over-constrain: the x update may run beside the r -> rr -> beta chain
    assert split == {"plain", "fused"}


def test_one_rank_only(tz):
    a = CgConfig(m=50, bw=8).args(0, 2)
    with pytest.raises(Exception, match="one rank"):
        tz._tz.ConjugateGradient(a)
    with pytest.raises(Exception, match="form"):
        tz._tz.ConjugateGradient(CgConfig(m=50, bw=8, form="both").args())


def test_sim_search_and_prices(tz):
    c, g = build_cg(CgConfig(m=1037), setup=False)
    assert not c.ready()
    res = tz.search(g, streams=2, iters=20, sim=True)
    assert res.best() >= 0 and len(res.sims) > 0
    best = res.sims[res.best()].seq
    assert tz.verify(best, tz.resolve_graph(g, best), 2) == []
    one = tz.Platform(1)
    p = tz.SimParams()
    t_plain = tz.SimExecutor(1, p).run_once(greedy_schedule(g, one, {"cg_form": "cg_plain"}))
    t_fused = tz.SimExecutor(1, p).run_once(greedy_schedule(g, one, {"cg_form": "cg_fused"}))
    assert t_fused < t_plain
    # every op carries a cost estimate (and the streaming ones their bytes)
    for o in _gpu_ops(tz, greedy_schedule(g, one, {"cg_form": "cg_plain"})):
        assert o.unbound.cost_us > 0
    sp = _gpu_ops(tz, greedy_schedule(g, one, {"cg_form": "cg_fused"}))[0].unbound
    assert sp.kind == "CgSpmvDot" and sp.traffic()[0][0] == "hbm"


def test_matrix_and_rhs_without_a_gpu(tz, tmp_path):
    """the matrix is the generator's, b lies in [-1, 1), a non-symmetric file is rejected"""
    c, _ = build_cg(CgConfig(m=257, bw=16), setup=False)
    rp, ci, v = c.matrix()
    ref = tz._tz.spd_band_matrix(257, 16, 5 * 257, 1)
    assert list(rp) == list(ref[0]) and list(ci) == list(ref[1]) and list(v) == list(ref[2])
    b = c.b()
    assert b.dtype == np.float32 and b.shape == (257,) and b.min() >= -1 and b.max() < 1 and b.std() > 0.3
    z, _ = build_cg(CgConfig(m=257, bw=16, rhs="zero"), setup=False)
    assert not z.b().any()
    path = str(tmp_path / "a.mtx")
    tz._tz.write_matrix_market(257, 257, list(rp), list(ci), list(v), path)
    m, _ = build_cg(CgConfig(matrix=path), setup=False)
    assert m.rows() == 257 and list(m.matrix()[2]) == list(v)
    vals = list(v)
    rows = np.repeat(np.arange(257), np.diff(np.array(rp)))
    vals[int(np.nonzero(rows != np.array(ci))[0][0])] += 0.5  # the first off-diagonal entry
    bad = str(tmp_path / "bad.mtx")
    tz._tz.write_matrix_market(257, 257, list(rp), list(ci), vals, bad)
    with pytest.raises(Exception, match="not symmetric"):
        build_cg(CgConfig(matrix=bad), setup=False)
