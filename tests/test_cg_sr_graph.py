"""The single-reduction CG form (``form="sr"``, ``form="all"``) without a GPU: the graph it gives
the search, its two ops and their order, race-free rollouts over all three forms, and the cost
model's view of two launches against four."""
import pytest

from tenzing_amd.models import CgConfig, build_cg
from tenzing_amd.search import choice_alternatives, greedy_schedule


def _gpu_ops(tz, seq):
    return [o for o in seq.ops() if isinstance(o, tz._tz.BoundGpuOp)]


def test_forms_offered(tz):
    _, g = build_cg(CgConfig(m=1037, form="all"), setup=False)
    assert choice_alternatives(g, "cg_form") == ["cg_plain", "cg_fused", "cg_sr"]
    _, gs = build_cg(CgConfig(m=1037, form="sr"), setup=False)
    assert choice_alternatives(gs, "cg_form") == []
    # the default is untouched: exactly two alternatives
    _, gc = build_cg(CgConfig(m=1037), setup=False)
    assert choice_alternatives(gc, "cg_form") == ["cg_plain", "cg_fused"]


def test_sr_is_two_ops_in_order(tz):
    _, g = build_cg(CgConfig(m=1037, form="sr"), setup=False)
    for seed in range(5):
        seq = tz.random_rollout(tz.State(g, tz.Platform(2)), seed)
        ops = _gpu_ops(tz, seq)
        assert [o.name for o in ops] == ["cg_s_spmvdot", "cg_s_update"]
        assert [o.unbound.kind for o in ops] == ["CgSpmvDot2", "CgSrUpdate"]
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []


def test_rollouts_over_all_forms_are_race_free(tz):
    _, g = build_cg(CgConfig(m=1037, form="all"), setup=False)
    plat = tz.Platform(2)
    forms = set()
    for seed in range(60):
        seq = tz.random_rollout(tz.State(g, plat), seed)
        assert tz.verify(seq, tz.resolve_graph(g, seq), 2) == []
        names = {o.name for o in _gpu_ops(tz, seq)}
        form = "sr" if "cg_s_spmvdot" in names else "fused" if "cg_f_spmvdot" in names else "plain"
        assert len(names) == {"sr": 2, "fused": 4, "plain": 8}[form]
        forms.add(form)
    assert forms == {"plain", "fused", "sr"}


def test_sim_prices_two_launches_below_four(tz):
    _, g = build_cg(CgConfig(m=1037, form="all"), setup=False)
    one = tz.Platform(1)
    p = tz.SimParams()
    t = {f: tz.SimExecutor(1, p).run_once(greedy_schedule(g, one, {"cg_form": "cg_" + f}))
         for f in ("plain", "fused", "sr")}
    assert t["sr"] < t["fused"] < t["plain"]
    ops = [o.unbound for o in _gpu_ops(tz, greedy_schedule(g, one, {"cg_form": "cg_sr"}))]
    assert len(ops) == 2
    n, nnz = 1037, build_cg(CgConfig(m=1037, form="sr"), setup=False)[0].args.nnz_actual
    # 4.5 us + the SpMV's bytes at 3e6 B/us; 3.5 us + 36 B per row at 4e6 B/us
    assert ops[0].cost_us == pytest.approx(4.5 + (12.0 * nnz + 8.0 * n) / 3.0e6, rel=1e-12)
    assert ops[1].cost_us == pytest.approx(3.5 + 36.0 * n / 4.0e6, rel=1e-12)
    assert ops[1].traffic()[0][0] == "hbm"


def test_one_rank_only_and_form_names(tz):
    with pytest.raises(Exception, match="one rank"):
        tz._tz.ConjugateGradient(CgConfig(m=50, bw=8, form="sr").args(0, 2))
    with pytest.raises(Exception, match="form"):
        tz._tz.ConjugateGradient(CgConfig(m=50, bw=8, form="both").args())
