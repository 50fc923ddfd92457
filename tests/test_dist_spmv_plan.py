"""The distributed SpMV's host-side plan (DistSpmv.plan()) against the numpy model of
tenzing_amd/utils/dist_spmv_ref.py, which builds it from the global matrix alone; and the
condition under which the GPU tests of tests/test_gpu_dist_spmv.py mean something: between two
value generations of x, any single stale input moves the reference by far more than the bound
those tests allow. No GPU."""
import functools
import json
import os
import socket
import sys

import numpy as np
import pytest

from tenzing_amd.utils import dist_spmv_ref as ref
from tenzing_amd.utils import spmv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4099 is prime (remainder rows for every size > 1); (9, 8) and (5, 4): one rank with two rows
# and one row each for the others; (64, 8) divides exactly
SHAPES = [(4099, 1), (4099, 2), (4099, 3), (4099, 8), (9, 8), (5, 4), (64, 8)]
BWS = ["neighbours", "all", "8"]
CASES = [(m, size, bw) for m, size in SHAPES for bw in BWS] + [(300, 4, "file")]


def band_params(m, size, bw):
    """(half-width, entries): 10 per row as in the workload's default, or for the small shapes
    seven eighths of what the band holds (m = 5, half-width 1: 12 of 13)"""
    half = {"neighbours": m // size, "all": m, "8": 8}[bw]
    cap = sum(min(m - 1, r + half) - max(0, r - half) + 1 for r in range(m))
    return half, min(10 * m, cap - cap // 8)


def file_case():
    """300 x 300, every column below 200: empty rows, rows of 127 to 129 entries, and a last
    rank (rows 225..299 of 4) whose entries are all remote"""
    c = spmv_ref.squared(spmv_ref.lengths_case(300))
    return c.row_ptr, c.col_ind, c.val


@functools.lru_cache(maxsize=None)
def matrix(m, size, bw):
    import tenzing_amd as tz

    if bw == "file":
        return ref.as_csr(file_case())
    half, nnz = band_params(m, size, bw)
    return ref.as_csr(tz._tz.random_band_matrix(m, half, nnz, 11))


@functools.lru_cache(maxsize=None)
def plans(m, size, bw):
    """every rank's plan() (as built with distribute="local", no device)"""
    import tempfile

    import tenzing_amd as tz
    from tenzing_amd.models import SpmvConfig

    if bw == "file":
        rp, ci, v = file_case()
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "lengths.mtx")
            tz._tz.write_matrix_market(m, m, rp, ci, v, f)
            return [tz._tz.DistSpmv(SpmvConfig(matrix=f).args(r, size, -1)).plan() for r in range(size)]
    half, nnz = band_params(m, size, bw)
    cfg = SpmvConfig(m=m, bw=half, nnz=nnz, seed=11)
    return [tz._tz.DistSpmv(cfg.args(r, size, -1)).plan() for r in range(size)]


def assert_same_plan(got, want, what):
    assert set(got) == set(want), what
    for k in ("r0", "r1"):
        assert int(got[k]) == int(want[k]), (what, k)
    for k in ("local", "remote"):
        for name, a, b in zip(("rowPtr", "colInd", "val"), got[k], want[k]):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and np.array_equal(a, b), (what, k, name)
        assert np.asarray(got[k][2]).dtype == np.float32
    for k in ("remote_cols", "recv_count", "recv_off", "send_count", "send_off", "send_idx"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, a, b)


@pytest.mark.parametrize("m,size,bw", CASES)
def test_plan_equals_the_model(m, size, bw):
    A = matrix(m, size, bw)
    for rank, p in enumerate(plans(m, size, bw)):
        assert_same_plan(p, ref.plan_ref(A, rank, size), (m, size, bw, rank))


@pytest.mark.parametrize("m,size,bw", CASES)
def test_blocks_reassemble_the_rows_of_a(m, size, bw):
    """local (through r0) and remote (through remote_cols) hold exactly the entries of my rows
    whose column I own, and those I do not: rows, columns, values, and the order within a row"""
    rp, ci, val = matrix(m, size, bw)
    row = np.repeat(np.arange(m), np.diff(rp))
    seen = 0
    for rank, p in enumerate(plans(m, size, bw)):
        r0, r1 = int(p["r0"]), int(p["r1"])
        assert (r0, r1) == ref.row_partition(m, rank, size)
        mine = (row >= r0) & (row < r1)
        own = (ci >= r0) & (ci < r1)
        for key, keep, to_global in (("local", mine & own, lambda c: c + r0),
                                     ("remote", mine & ~own, lambda c: np.asarray(p["remote_cols"])[c])):
            brp, bci, bval = (np.asarray(a) for a in p[key])
            assert len(brp) == r1 - r0 + 1 and brp[0] == 0 and brp[-1] == len(bci) == len(bval)
            assert (np.diff(brp) >= 0).all()
            brow = np.repeat(np.arange(r0, r1), np.diff(brp))
            assert np.array_equal(brow, row[keep]), (rank, key)
            assert np.array_equal(to_global(bci.astype(np.int64)), ci[keep]), (rank, key)
            assert np.array_equal(bval, val[keep]), (rank, key)
            seen += len(bci)
    assert seen == len(ci)


@pytest.mark.parametrize("m,size,bw", CASES)
def test_remote_columns_are_sorted_and_grouped_by_owner(m, size, bw):
    for rank, p in enumerate(plans(m, size, bw)):
        rc = np.asarray(p["remote_cols"])
        cnt, off = np.asarray(p["recv_count"]), np.asarray(p["recv_off"])
        assert (np.diff(rc) > 0).all()
        assert len(cnt) == len(off) == size and cnt[rank] == 0 and cnt.sum() == len(rc)
        assert ((rc < p["r0"]) | (rc >= p["r1"])).all() and (rc >= 0).all() and (rc < m).all()
        for q in range(size):
            seg = rc[off[q]:off[q] + cnt[q]]
            assert len(seg) == cnt[q] and (ref.owner_of(seg, m, size) == q).all(), (rank, q)


@pytest.mark.parametrize("m,size,bw", CASES)
def test_every_pair_agrees_on_what_is_sent(m, size, bw):
    """what p gathers for q is what q expects from p, column for column in q's slot order: the
    IPC put stores blind on this agreement"""
    ps = plans(m, size, bw)
    talking = 0
    for p in range(size):
        sc, so, si = (np.asarray(ps[p][k]) for k in ("send_count", "send_off", "send_idx"))
        assert len(sc) == len(so) == size and sc[p] == 0 and sc.sum() == len(si)
        assert ((si >= 0) & (si < ps[p]["r1"] - ps[p]["r0"])).all()
        for q in range(size):
            sent = int(ps[p]["r0"]) + si[so[q]:so[q] + sc[q]].astype(np.int64)
            rc, cnt, off = (np.asarray(ps[q][k]) for k in ("remote_cols", "recv_count", "recv_off"))
            assert np.array_equal(sent, rc[off[p]:off[p] + cnt[p]]), (p, q)
            talking += len(sent) > 0
    if bw == "all" and size > 1 and m == 4099:
        assert talking == size * (size - 1)  # everyone talks to everyone
    if bw == "8" and size == 8 and m == 4099:
        assert talking == 2 * (size - 1)     # neighbours only


def test_file_case_premises():
    """what the GPU test of the irregular file relies on"""
    A = matrix(300, 4, "file")
    ps = plans(300, 4, "file")
    lengths = np.diff(A[0])
    assert (lengths == 0).any() and {127, 128, 129} <= set(lengths.tolist()) and A[1].max() < 200
    last = ps[3]
    assert (int(last["r0"]), int(last["r1"])) == (225, 300)
    assert len(last["local"][1]) == 0 and len(last["remote"][1]) > 0
    assert np.asarray(last["send_count"]).sum() == 0 and (np.asarray(last["recv_count"])[:3] > 0).all()
    # ranks 0 and 1 own columns that only other ranks' rows use (and rank 3 needs from them)
    for q in (0, 1):
        assert np.asarray(ps[q]["send_count"])[3] > 0


def stale_ratios(A, rank, size, g0, g1):
    """for every single stale input of rank `rank` when x went from generation g0 to g1, the
    largest move of a y_ref row in units of that row's bound at g1: {input: ratio}"""
    rp, ci, val = A
    n = len(rp) - 1
    r0, r1 = ref.row_partition(n, rank, size)
    brp, bci, bval = ref.rows_of(A, r0, r1)
    dx = ref.x_gen(np.arange(n), g1).astype(np.float64) - ref.x_gen(np.arange(n), g0).astype(np.float64)
    b = ref.bound(A, g1, r0, r1)
    own = ref.owner_of(bci, n, size)
    inputs = {f"x from rank {q}": own == q for q in range(size) if q != rank}
    inputs["local product"] = own == rank
    inputs["remote product"] = own != rank
    out = {}
    for name, mask in inputs.items():
        if not mask.any():
            continue
        moved = np.abs(spmv_ref.csr_matvec_f64(brp, bci, np.where(mask, bval, np.float32(0)), dx))
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = float(np.where(moved > 0, moved / b, 0.0).max())
    return out


@pytest.mark.parametrize("m,size,bw", CASES)
def test_a_stale_input_moves_the_reference_far_beyond_the_bound(m, size, bw):
    """a condition on the reference alone: with it, a schedule that leaves one peer's x segment,
    the local product or the remote product at the previous generation cannot stay within the
    bound on every row. Asserted so that a change of x_gen cannot void the GPU tests."""
    A = matrix(m, size, bw)
    worst = np.inf
    for rank in range(size):
        for g in range(ref.GENERATIONS):
            for name, r in stale_ratios(A, rank, size, g, (g + 1) % ref.GENERATIONS).items():
                assert r > 4.0, (m, size, bw, rank, g, name, r)
                worst = min(worst, r)
    print(f"smallest stale move / bound at {(m, size, bw)}: {worst:.3g}")


def test_generations_differ_everywhere_and_match_the_native_rule(tz):
    g = np.concatenate((np.arange(10_000), np.arange(149_000, 151_000), [2 ** 31 - 1]))
    xs = [ref.x_gen(g, k) for k in range(ref.GENERATIONS)]
    for a in range(ref.GENERATIONS):
        assert xs[a].dtype == np.float32 and (xs[a] >= -1).all() and (xs[a] < 1).all()
        for b in range(a):
            assert (xs[a] != xs[b]).all(), (a, b)
        native = np.array([tz._tz.DistSpmv.x_gen(int(i), a) for i in g[::7]], dtype=np.float32)
        assert np.array_equal(native, xs[a][::7]), a


def test_generation_hooks_without_a_device(tz):
    from tenzing_amd.models import SpmvConfig

    s = tz._tz.DistSpmv(SpmvConfig(m=64, bw=8, nnz=300).args(1, 4, -1))
    assert s.generation() == 0
    s.set_generation(3)
    assert s.generation() == 3
    for bad in (-1, 4):
        with pytest.raises(Exception, match="generation"):
            s.set_generation(bad)
    assert s.generation() == 3
    for needs_setup in (s.poison, s.y):
        with pytest.raises(Exception, match="not set up"):
            needs_setup()


# ------------------------------------------------------------------ root distribution, 3 ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _root_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tenzing_amd as tz
    import test_dist_spmv_plan as me
    from tenzing_amd.models import SpmvConfig
    from tenzing_amd.parallel import init_ctrl

    c = init_ctrl(timeout_s=60)
    res = {}
    for bw in BWS:
        half, nnz = band_params(4099, world, bw)
        got = {}
        for how in ("root", "local"):
            cfg = SpmvConfig(m=4099, bw=half, nnz=nnz, seed=11, distribute=how)
            s = tz._tz.DistSpmv(cfg.args(c.rank, c.size, -1), c)
            assert s.args.distribute == how
            got[how] = s.plan()
        me.assert_same_plan(got["root"], got["local"], (bw, rank, "root against local"))
        me.assert_same_plan(got["root"], ref.plan_ref(me.matrix(4099, world, bw), rank, world),
                            (bw, rank, "root against the model"))
        res[bw] = int(len(got["root"]["remote_cols"]))
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)


def test_root_distribution_builds_the_same_plan(tmp_path):
    """distribute="root" (rank 0 sends every rank its rows; the ranks ask the owners for the x
    entries they need) over 3 ranks of the CPU control plane: every rank's plan() is the one
    distribute="local" builds, and the model's"""
    pytest.importorskip("torch")
    import torch.multiprocessing as mp

    mp.start_processes(_root_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True,
                       start_method="spawn")
    for r in range(3):
        got = json.loads((tmp_path / f"r{r}.json").read_text())
        assert set(got) == set(BWS) and all(v > 0 for v in got.values()), got
