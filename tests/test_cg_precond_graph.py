"""The Jacobi preconditioner and the change of units of the CG workload
(``CgConfig(form="sr", precond="jacobi", diag_scale=d)``) without a GPU: which combinations are
refused, the fields in config, args and json, what ``diag_scale`` does to the matrix and the
right-hand sides (exact powers of two), the graph the search sees, and the command line."""
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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dense(c):
    rp, ci, v = c.matrix()
    rows = c.rows()
    a = np.zeros((rows, rows), dtype=np.float32)
    for i in range(rows):
        for j in range(rp[i], rp[i + 1]):
            a[i, ci[j]] = v[j]
    return a, np.asarray(rp), np.asarray(ci)


@pytest.mark.parametrize("form", ["plain", "fused", "choice", "all"])
def test_jacobi_needs_the_single_reduction_form(tz, form):
    with pytest.raises(Exception, match="only the single-reduction form for one right-hand side has preconditioned"):
        _cg(tz, form=form, precond="jacobi")
    _cg(tz, form=form, precond="none")


@pytest.mark.parametrize("nrhs", [2, 4, 8])
def test_jacobi_needs_one_right_hand_side(tz, nrhs):
    with pytest.raises(Exception, match="only the single-reduction form for one right-hand side has preconditioned"):
        _cg(tz, form="sr", nrhs=nrhs, precond="jacobi")
    _cg(tz, form="sr", nrhs=nrhs)


def test_unknown_preconditioner_raises(tz):
    with pytest.raises(Exception, match="precond must be none or jacobi"):
        _cg(tz, form="sr", precond="ilu")


@pytest.mark.parametrize("d", [-1, 9])
def test_diag_scale_out_of_range_raises(tz, d):
    with pytest.raises(Exception, match="diag_scale must be 0..8"):
        _cg(tz, form="sr", diag_scale=d)


def _mtx(path, n, entries):
    lines = ["%%MatrixMarket matrix coordinate real general", f"{n} {n} {len(entries)}"]
    lines += [f"{i} {j} {v}" for i, j, v in entries]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_diagonal_must_be_there_and_positive(tz, tmp_path):
    off = [(1, 2, -1.0), (2, 1, -1.0), (2, 3, -1.0), (3, 2, -1.0)]
    good = _mtx(tmp_path / "good.mtx", 3, off + [(1, 1, 4.0), (2, 2, 8.0), (3, 3, 2.0)])
    c = tz._tz.ConjugateGradient(CgConfig(matrix=good, form="sr", precond="jacobi").args())
    assert np.array_equal(c.dinv(), np.float32([0.25, 0.125, 0.5]))
    missing = _mtx(tmp_path / "missing.mtx", 3, off + [(1, 1, 4.0), (3, 3, 2.0)])
    with pytest.raises(Exception, match="row 2 has no diagonal entry"):
        tz._tz.ConjugateGradient(CgConfig(matrix=missing, form="sr", precond="jacobi").args())
    for name, val in (("zero", 0.0), ("negative", -8.0)):
        bad = _mtx(tmp_path / f"{name}.mtx", 3, off + [(1, 1, 4.0), (2, 2, val), (3, 3, 2.0)])
        # a reader that drops explicit zeros makes the zero a missing entry: row 2 either way
        with pytest.raises(Exception, match="precond jacobi: row 2 has"):
            tz._tz.ConjugateGradient(CgConfig(matrix=bad, form="sr", precond="jacobi").args())
        # without the preconditioner nothing looks at the diagonal
        tz._tz.ConjugateGradient(CgConfig(matrix=bad, form="sr").args())
    # the generated matrix, scaled or not, passes
    _cg(tz, form="sr", precond="jacobi", diag_scale=8)


def test_fields_in_args_json_and_config(tz):
    assert CgConfig().precond == "none" and CgConfig().diag_scale == 0
    j = json.loads(tz._tz.CgArgs().json())
    assert j["precond"] == "none" and j["diag_scale"] == 0
    a = CgConfig(m=M, bw=BW, form="sr", precond="jacobi", diag_scale=3).args()
    assert a.precond == "jacobi" and a.diag_scale == 3
    j = json.loads(a.json())
    assert j["precond"] == "jacobi" and j["diag_scale"] == 3
    c = tz._tz.ConjugateGradient(a)
    assert c.args.precond == "jacobi" and c.args.diag_scale == 3


def test_accessors(tz):
    c = _cg(tz, form="sr", precond="jacobi")
    a, rp, ci = _dense(c)
    assert np.array_equal(_bits(c.dinv()), _bits(np.float32(1.0) / np.diag(a)))
    with pytest.raises(Exception, match="not set up"):
        c.u()
    plain = _cg(tz, form="sr")
    with pytest.raises(Exception, match="precond none"):
        plain.dinv()
    with pytest.raises(Exception, match="precond none"):
        plain.u()


@pytest.mark.parametrize("d", [1, 2, 8])
def test_diag_scale_is_an_exact_change_of_units(tz, d):
    c0 = _cg(tz, form="sr", nrhs=2, tol=1e-5)
    c = _cg(tz, form="sr", nrhs=2, tol=1e-5, diag_scale=d)
    s = c.scale()
    assert s.dtype == np.float32 and s.shape == (M,)
    e = np.log2(s.astype(np.float64))
    assert np.array_equal(e, np.round(e)) and e.min() >= -d and e.max() <= d
    assert len(set(e.tolist())) > 1  # it does scale
    assert np.array_equal(np.exp2(e).astype(np.float32), s)
    a0, rp0, ci0 = _dense(c0)
    a, rp, ci = _dense(c)
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0)  # the same pattern
    want = (s.astype(np.float64)[:, None] * a0.astype(np.float64) * s.astype(np.float64)[None, :])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)  # exact in f32
    assert np.array_equal(_bits(a), _bits(want.astype(np.float32)))
    assert np.array_equal(_bits(a), _bits(a.T))
    for j in range(2):
        wb = s.astype(np.float64) * c0.b(j).astype(np.float64)
        assert np.array_equal(_bits(c.b(j)), _bits(wb.astype(np.float32)))
        # the thresholds are formed from the scaled b
        bb = 0.0
        for v in c.b(j).astype(np.float64):
            bb += float(v) * float(v)
        assert c.threshold(j) == 1e-5 * 1e-5 * bb and c.threshold(j) != c0.threshold(j)
    # another seed, another scaling
    assert not np.array_equal(_cg(tz, form="sr", diag_scale=d, seed=2).scale(), s[:M])


def test_diag_scale_zero_is_todays_bits(tz, tmp_path):
    c0 = tz._tz.ConjugateGradient(CgConfig(m=M, bw=BW, form="sr").args())
    c = _cg(tz, form="sr", precond="jacobi", diag_scale=0)
    assert np.array_equal(c.scale(), np.ones(M, dtype=np.float32))
    (rp, ci, v), (rp0, ci0, v0) = c.matrix(), c0.matrix()
    assert list(rp) == list(rp0) and list(ci) == list(ci0)
    assert np.array_equal(_bits(v), _bits(v0))
    assert np.array_equal(_bits(c.b()), _bits(c0.b()))
    # a file matrix is scaled like a generated one
    off = [(1, 2, -1.0), (2, 1, -1.0), (2, 3, -1.0), (3, 2, -1.0)]
    path = _mtx(tmp_path / "a.mtx", 3, off + [(1, 1, 4.0), (2, 2, 8.0), (3, 3, 2.0)])
    f0 = tz._tz.ConjugateGradient(CgConfig(matrix=path, form="sr").args())
    f = tz._tz.ConjugateGradient(CgConfig(matrix=path, form="sr", precond="jacobi", diag_scale=4).args())
    s = f.scale().astype(np.float64)
    assert np.array_equal(_dense(f)[0], (s[:, None] * _dense(f0)[0] * s[None, :]).astype(np.float32))
    assert np.array_equal(f.b(), (s * f0.b()).astype(np.float32))
    assert np.array_equal(f.dinv(), np.float32(1.0) / np.diag(_dense(f)[0]))


@pytest.mark.parametrize("tol", [0.0, 1e-6])
def test_graph_of_the_preconditioned_form(tz, tol):
    c, g = build_cg(CgConfig(m=1037, form="sr", precond="jacobi", diag_scale=2, tol=tol), setup=False)
    assert not c.ready()
    ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1)))]
    assert [(o.name, o.kind) for o in ops] == [("cg_s_spmvdot", "CgPcgSpmvDot3"), ("cg_s_update", "CgPcgUpdate")]
    for seed in range(5):
        seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
        assert [o.name for o in _gpu_ops(tz, seq)] == ["cg_s_spmvdot", "cg_s_update"]
        assert [o.unbound.kind for o in _gpu_ops(tz, seq)] == ["CgPcgSpmvDot3", "CgPcgUpdate"]
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []


def test_same_graph_with_and_without_tol_and_more_bytes_than_unpreconditioned(tz):
    def descr(**kw):
        c, g = build_cg(CgConfig(m=1037, form="sr", **kw), setup=False)
        ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, tz.Platform(1)))]
        return c, [(o.name, o.kind, o.cost_us, o.bytes) for o in ops]

    c, d0 = descr(precond="jacobi")
    assert descr(precond="jacobi", tol=1e-6)[1] == d0
    n, nnz = 1037, c.args.nnz_actual
    assert d0[0][3] == 12.0 * nnz + 12.0 * n  # matrix and gather; r, u read and w written per row
    assert d0[1][3] == 44.0 * n  # w, dinv, r, p, s, x read; p, s, x, r, u written
    plain = descr()[1]
    assert [d[:2] for d in plain] == [("cg_s_spmvdot", "CgSpmvDot2"), ("cg_s_update", "CgSrUpdate")]
    assert d0[0][3] == plain[0][3] + 4.0 * n and d0[1][3] == plain[1][3] + 8.0 * n


def test_cli_parser_and_saved_args(tz):
    from tenzing_amd import cli

    a = cli._parser().parse_args(["search", "--workload", "cg"])
    assert a.cg_precond == "none" and a.cg_diag_scale == 0
    a = cli._parser().parse_args(["search", "--workload", "cg", "--cg-form", "sr", "--cg-precond", "jacobi",
                                  "--cg-diag-scale", "2"])
    assert a.cg_precond == "jacobi" and a.cg_diag_scale == 2
    with pytest.raises(SystemExit):
        cli._parser().parse_args(["search", "--workload", "cg", "--cg-precond", "ilu"])
    assert "cg_precond" in cli._WORKLOAD_KEYS and "cg_diag_scale" in cli._WORKLOAD_KEYS
    w = cli._saved_args({k: getattr(a, k) for k in cli._WORKLOAD_KEYS})
    assert w.cg_precond == "jacobi" and w.cg_diag_scale == 2 and w.cg_form == "sr"
    # a document saved before the options existed
    old = {k: getattr(a, k) for k in cli._WORKLOAD_KEYS if k not in ("cg_precond", "cg_diag_scale")}
    w = cli._saved_args(old)
    assert w.cg_precond == "none" and w.cg_diag_scale == 0


def test_cli_sim_search_of_the_preconditioned_form(tz, capsys):
    from tenzing_amd import cli

    rc = cli.main(["search", "--workload", "cg", "--sim", "--cg-form", "sr", "--cg-precond", "jacobi",
                   "--cg-diag-scale", "2", "--cg-m", "1037", "--iters", "4", "--bench-iters", "2", "--streams", "2"])
    assert rc == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["workload"] == "cg" and out["best_pct10_ms"] > 0 and math.isfinite(out["best_pct10_ms"])
