"""The distributed SpMV workload (csrc/workloads/spmv.cpp) against the numpy model of
tenzing_amd/utils/dist_spmv_ref.py: every rank's y, row by row, within the derived bound
(L + 2) 2^-24 sum |a| |x| of an f32 dot product and no other tolerance.

The workload's own check() compares with a reference built from the code under test, and x
never changed between runs, so a schedule whose exchange, put, wait, remote product or final add
did nothing still found the right values in the buffers. Here every comparison follows a new value
generation of x (DistSpmv.set_generation), the first of each schedule also NaNs in every buffer a
schedule must write (DistSpmv.poison); tests/test_dist_spmv_plan.py asserts that any single input
left at the previous generation moves some row by more than 4 bounds (by more than 10^4 on these
matrices).

Worst measured |err| / bound (MI355X), over all schedules, generations and ranks:

    one process, 4099 rows, forms split / accum / choice, eager and hipGraph:
        0.3041 for each of w4, w8, w16, i1, i2, i4, stream and rocsparse_adaptive, in either form
        (the rows of one entry set it: one rounding of a product against a bound of 3 u)
    2 ranks 0.3964, 3 ranks 0.3513, 8 ranks 0.3499 (4099 rows, the three bandwidths)
    4 ranks, 5 rows 0.2436; 4 ranks, the irregular 300-row file 0.3074
"""
import pytest

from tenzing_amd.utils import dist_spmv_ref as ref
from tenzing_amd.utils import spmv_ref

pytestmark = pytest.mark.gpu

M = 4099  # prime; 65 stream blocks, the last one ragged; more than one workgroup in every kernel

VARIANTS = {"yl_w4", "yl_w8", "yl_w16", "yl_i1", "yl_i2", "yl_i4", "yl_stream", "yl_rocsparse_adaptive"}


@pytest.fixture(scope="module")
def rows():
    """the one-rank model of the default band matrix of M rows, shared and never changed"""
    return ref.Rows(ref.default_band(M, 1), 0, M)


def _variants(tz, g, want):
    """one schedule per local-kernel variant, found by rollout"""
    by_variant = {}
    for seed in range(2000):
        seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
        v = [o.name for o in seq.ops() if o.name.startswith(("yl_", "a_yl_"))]
        assert len(v) == 1, v
        by_variant.setdefault(v[0], seq)
        if len(by_variant) == len(want):
            break
    assert set(by_variant) == want, sorted(by_variant)
    return by_variant


@pytest.mark.parametrize("form", ["split", "accum", "choice"])
def test_every_variant_from_poisoned_buffers_and_new_generations(tz, gpu, rows, form):
    """each of the 8 local-kernel variants (in both forms with "choice"), eager and as a hipGraph:
    generation g from NaN-filled buffers, then g + 1 on top of g's results, then three more runs"""
    from tenzing_amd.models import SpmvConfig, build_spmv

    sp, g = build_spmv(SpmvConfig(m=M, form=form), tz.SelfCtrl(), device=0)
    assert sp.local_rows() == M and sp.remote_nnz() == 0
    want = set(VARIANTS) if form != "choice" else VARIANTS | {"a_" + v for v in VARIANTS}
    by_variant = _variants(tz, g, want)
    gen = 0
    worst = {}
    for mode in (tz.ExecMode.Eager, tz.ExecMode.Graph):
        rt = tz.HipRuntime(device=0, n_streams=2, mode=mode,
                           graph_unroll=3 if mode == tz.ExecMode.Graph else 1)
        for name, seq in sorted(by_variant.items()):
            ratios = []
            gen = (gen + 1) % ref.GENERATIONS
            sp.set_generation(gen)
            sp.poison()
            rt.prepare(seq)
            assert rt.effective_mode == mode, name
            rt.run(1)
            rt.device_sync()
            ratios.append(rows.ratio(sp.y(), gen))
            gen = (gen + 1) % ref.GENERATIONS
            sp.set_generation(gen)
            rt.run(1)
            rt.device_sync()
            ratios.append(rows.ratio(sp.y(), gen))
            rt.run(3)
            rt.device_sync()
            ratios.append(rows.ratio(sp.y(), gen))
            print(f"RATIO one_process {form} {name} {mode} {max(ratios):.4f}")
            worst[name, str(mode)] = ratios
            assert sp.check() < 1e-4, (name, mode)
        del rt
    bad = {k: v for k, v in worst.items() if not max(v) <= 1.0}
    assert not bad, bad


def test_the_comparison_fails_on_stale_y_and_on_nan(tz, gpu, rows):
    """the two ways the workload's own check could be fooled, without provoking anything: y of
    generation g held against g + 1 is outside the bound on most rows and far above check()'s
    threshold; NaN-filled buffers make check() infinite"""
    from tenzing_amd.models import SpmvConfig, build_spmv

    sp, g = build_spmv(SpmvConfig(m=M, form="split"), tz.SelfCtrl(), device=0)
    rt = tz.HipRuntime(device=0, n_streams=2)
    seq = tz.random_rollout(tz.State(g, tz.Platform(2)), 0)
    sp.set_generation(1)
    sp.poison()
    assert sp.check() == float("inf")
    assert rows.ratio(sp.y(), 1) == float("inf") and rows.outside(sp.y(), 1).all()
    rt.prepare(seq)
    rt.run(1)
    rt.device_sync()
    assert rows.ratio(sp.y(), 1) <= 1.0 and sp.check() < 1e-4
    sp.set_generation(2)  # no run: y is the product of generation 1
    assert sp.generation() == 2
    nonempty = rows.lengths > 0
    outside = rows.outside(sp.y(), 2)
    assert outside[nonempty].sum() > nonempty.sum() / 2, (int(outside.sum()), int(nonempty.sum()))
    assert sp.check() > 1e-4
    sp.poison()
    assert sp.check() == float("inf")
    sp.set_generation(0)
    rt.run(1)
    rt.device_sync()
    assert rows.ratio(sp.y(), 0) <= 1.0 and sp.check() < 1e-4


# ------------------------------------------------------------------ several ranks (loopback, IPC)

def _check_ranks(res, world, what):
    worst = 0.0
    for r in res:
        assert r["size"] == world and r["transport"] == "ipc", r
        assert len(r["runs"]) > 0
        for run in r["runs"]:
            assert run["ipc"] and run["ipc_err"] == 0, run
            worst = max(worst, run["ratio1"], run["ratio2"], run["ratio3"])
    print(f"RATIO {what} world {world} {worst:.4f}")
    for r in res:
        for run in r["runs"]:
            assert run["ratio1"] <= 1.0 and run["ratio2"] <= 1.0 and run["ratio3"] <= 1.0, (r["rank"], run)
            assert max(run["err1"], run["err2"], run["err3"]) < 1e-4, (r["rank"], run)
    return res


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_match_the_model_loopback(gpu, world):
    """2, 3 and 8 ranks on one GPU over IPC puts, M rows, three bandwidths (neighbours only;
    everyone talks to everyone; a few remote columns): 4 broadcast schedules each, eager and as
    hipGraphs unrolled 3 times. Per schedule: next generation and NaNs everywhere on every rank,
    one run; next generation on top of that, one run (a transport that delivers the last run's
    data fails here); 5 more runs."""
    from test_gpu_multirank import _launch

    res = _launch("spmv_ref", world, extra_env={"TZ_TEST_M": str(M), "TZ_TEST_BWS": f"{M // world},{M},8"})
    _check_ranks(res, world, "band")
    for r in res:
        assert len(r["runs"]) == 3 * 2 * 4
        assert all(run["remote_nnz"] > 0 for run in r["runs"])
        assert any(run["library"] for run in r["runs"])


def test_five_rows_on_four_ranks_loopback(gpu):
    """m = 5 on 4 ranks: one rank with two rows, three with one; 12 of the 13 entries of the
    tridiagonal band"""
    from test_gpu_multirank import _launch

    _check_ranks(_launch("spmv_ref", 4, extra_env={"TZ_TEST_M": "5", "TZ_TEST_NNZ": "12", "TZ_TEST_BWS": "1"}),
                 4, "five_rows")


def test_irregular_file_on_four_ranks_loopback(tz, gpu, tmp_path):
    """300 x 300 with all columns below 200, empty rows and rows of 127 to 129 entries: the rank
    of rows 225..299 has an empty local block (its library variant falls back, all it computes is
    remote), sends nothing yet receives (a put without segments beside a wait with senders)"""
    from test_gpu_multirank import _launch

    c = spmv_ref.squared(spmv_ref.lengths_case(300))
    f = str(tmp_path / "lengths.mtx")
    tz._tz.write_matrix_market(300, 300, c.row_ptr, c.col_ind, c.val, f)
    res = _check_ranks(_launch("spmv_ref", 4, extra_env={"TZ_TEST_MATRIX": f, "TZ_TEST_LENGTHS_ROWS": "300"}),
                       4, "file")
    last = [r for r in res if r["rank"] == 3][0]["runs"]
    assert all(run["local_nnz"] == 0 and run["remote_nnz"] > 0 for run in last)
    assert any(run["library"] for run in last)
