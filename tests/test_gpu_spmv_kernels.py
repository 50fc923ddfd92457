"""The SpMV kernel family against an independent float64 reference (tenzing_amd/utils/spmv_ref.py,
itself checked by tests/test_spmv_ref.py) on irregular matrices: ``csr_spmv`` under every lane
setting (twelve values: 0 and seven widths, CSR-stream, three ILP widths), ``csr_spmv_dot`` /
``csr_spmv_dot2`` / ``csr_spmm_dot2``, the workgroup interleave of ``box_move_spmv``, and the
grid-stride loops of ``gather_f32`` and ``vector_add_f32``.

On `exact_data` every f32 summation order is exact, so results must equal the reference: every
such assertion is ``torch.equal`` or ``==`` on float64 sums. On random-normal data the one
tolerance is `abs_bound`, the derived bound of an f32 dot product.

Conventions: outputs start as a NaN of fixed payload and a guard of 64 elements behind them must
keep it; every x entry that no matrix entry references is NaN, so a kernel that gathers x for a
masked lane and multiplies by zero poisons its row (the SpMV + dot kernels read every entry of
their vector for the dot product, so theirs has none); empty col_ind / val are 16-byte device
buffers, never null."""
import functools

import numpy as np
import pytest

from tenzing_amd.utils import spmv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SLAB = 256  # kernels.CG_MAX_PARTIALS
ILP = 1000  # kernels.SPMV_ILP
GUARD = 64
SETTINGS = [0, 1, 2, 4, 8, 16, 32, 64, -1, ILP + 1, ILP + 2, ILP + 4]
NAMES = ["tiny_1", "tiny_63", "tiny_64", "tiny_65", "tiny_257", "empty_all", "empty_runs", "lengths",
         "long_row", "cap", "narrow", "wide", "dups", "band"]
PAYLOAD32, PAYLOAD64 = 0x7FC0BEEF, 0x7FF80000DEADBEEF


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan32(*shape):
    return torch.full(shape, PAYLOAD32, dtype=torch.int32, device="cuda").view(torch.float32)


def _nan64(*shape):
    return torch.full(shape, PAYLOAD64, dtype=torch.int64, device="cuda").view(torch.float64)


def _untouched(t):
    """every element still holds the payload"""
    bits, want = (t.view(torch.int32), PAYLOAD32) if t.dtype == torch.float32 else (t.view(torch.int64), PAYLOAD64)
    return bool((bits == want).all())


@functools.lru_cache(maxsize=None)
def _zoo():
    return {c.name: c for c in sr.zoo()}


def _dev(a, dtype):
    """a host array on the device; an empty one as a 16-byte buffer"""
    t = torch.zeros(max(len(a), 16 // np.dtype(a.dtype).itemsize), dtype=dtype, device="cuda")
    t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a))
    return t


@functools.lru_cache(maxsize=None)
def _structure(name, square=False):
    """(case, row_ptr, col_ind) with the two index arrays on the device, built once"""
    case = _zoo()[name]
    if square:
        case = sr.squared(case)
    return case, _dev(case.row_ptr, torch.int32), _dev(case.col_ind, torch.int32)


def _x_dev(case, x, poison=True):
    """x on the device, NaN in every entry that no matrix entry references"""
    x = x.copy()
    if poison:
        x[~sr.referenced(case)] = np.nan
    return torch.from_numpy(x).cuda()


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _spmv(tz, case, rp, ci, v, x, y, lanes, acc):
    tz._tz.kernels.csr_spmv(case.nrows, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), x.data_ptr(), y.data_ptr(),
                            lanes, acc, _stream())
    torch.cuda.synchronize()


def test_constants(tz):
    assert tz._tz.kernels.SPMV_ILP == ILP and tz._tz.kernels.CG_MAX_PARTIALS == SLAB
    assert list(_zoo()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_csr_spmv_exact(tz, gpu, name):
    """every lane setting on every zoo case: y == A x, then y0 + A x and y0 + 2 A x by two
    accumulating launches, bit for bit; the guard keeps its payload"""
    case, rp, ci = _structure(name)
    val, x, y0 = sr.exact_data(case, seed=11)
    if name != "band":
        assert not sr.referenced(case).all()  # some x entry is NaN
    v, xd = _dev(val, torch.float32), _x_dev(case, x)
    ref = [_f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, m * x, b)) for m, b in ((1, None), (1, y0), (2, y0))]
    assert not ref[0].isnan().any() and (name == "empty_all" or ref[0].any())
    n = case.nrows
    for lanes in SETTINGS:
        y = _nan32(n + GUARD)
        _spmv(tz, case, rp, ci, v, xd, y, lanes, False)
        assert torch.equal(y[:n].double().cpu(), ref[0]), (name, lanes)
        y[:n] = torch.from_numpy(y0).cuda()
        for k in (1, 2):
            _spmv(tz, case, rp, ci, v, xd, y, lanes, True)
            assert torch.equal(y[:n].double().cpu(), ref[k]), (name, lanes, "accumulate", k)
        assert _untouched(y[n:]), (name, lanes)


@pytest.mark.parametrize("name", ["lengths", "long_row", "cap", "band"])
def test_csr_spmv_random_within_bound(tz, gpu, name):
    """random-normal values and x: every row within the derived bound of an f32 dot product"""
    case, rp, ci = _structure(name)
    val, x = sr.normal_data(case, seed=12)
    v, xd = _dev(val, torch.float32), _x_dev(case, x)
    ref = _f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x))
    bound = _f64(sr.abs_bound(case.row_ptr, case.col_ind, val, x))
    n = case.nrows
    for lanes in SETTINGS:
        y = _nan32(n + GUARD)
        _spmv(tz, case, rp, ci, v, xd, y, lanes, False)
        err = (y[:n].double().cpu() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{name} lanes {lanes}: max error / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (name, lanes, worst)  # a NaN fails it
        assert _untouched(y[n:])


def test_csr_spmv_without_rows_touches_nothing(tz, gpu):
    case, rp, ci = _structure("tiny_64")
    val, x, _ = sr.exact_data(case, seed=11)
    v, xd = _dev(val, torch.float32), _x_dev(case, x)
    y = _nan32(GUARD)
    for lanes in SETTINGS:
        for acc in (False, True):
            tz._tz.kernels.csr_spmv(0, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), xd.data_ptr(), y.data_ptr(),
                                    lanes, acc, _stream())
    torch.cuda.synchronize()
    assert _untouched(y)


def _check_partials(part, cnt, want, what):
    """the first `cnt` partials of every slab sum (float64, exact on this data) to `want`; the
    rest of the slab, and the guard behind the last, keep the payload"""
    want = np.atleast_1d(want)
    for j, wj in enumerate(want):
        slab = part[j * SLAB:(j + 1) * SLAB]
        got = slab[:cnt].cpu().numpy()
        assert not np.isnan(got).any(), (what, j)
        assert float(got.sum()) == float(wj), (what, j)
        assert _untouched(slab[cnt:]), (what, j)
    assert _untouched(part[len(want) * SLAB:]), what


@pytest.mark.parametrize("name", NAMES)
def test_spmv_dot_kernels_exact(tz, gpu, name):
    """csr_spmv_dot and csr_spmv_dot2 with 1, 2 and 4 lanes per row on the zoo made square: q / w
    equal the reference, and the partials sum to exactly its p . q (r . r and r . w)"""
    kn = tz._tz.kernels
    case, rp, ci = _structure(name, True)
    n = case.nrows
    val, x, _ = sr.exact_data(case, seed=13)
    v, p = _dev(val, torch.float32), _x_dev(case, x, poison=False)
    q_ref = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)
    xx, xq = float(np.dot(x.astype(np.float64), x)), float(np.dot(x.astype(np.float64), q_ref))
    assert xx < 2 ** 50 and np.abs(x.astype(np.float64) * q_ref).sum() < 2 ** 50  # eighths: exact in f64
    for W in (1, 2, 4):
        cnt = kn.spmv_dot_partial_count(n, ILP + W)
        assert cnt == min(SLAB, max(1, -(-n * W // 1024)))
        q, pq = _nan32(n + GUARD), _nan64(SLAB + GUARD)
        kn.csr_spmv_dot(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), p.data_ptr(), q.data_ptr(), ILP + W,
                        pq.data_ptr(), 0, 0, 0, _stream())
        torch.cuda.synchronize()
        assert torch.equal(q[:n].double().cpu(), _f64(q_ref)), (name, W)
        assert _untouched(q[n:])
        _check_partials(pq, cnt, xq, (name, W, "p.q"))
        w, pg, pd = _nan32(n + GUARD), _nan64(SLAB + GUARD), _nan64(SLAB + GUARD)
        kn.csr_spmv_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), p.data_ptr(), w.data_ptr(), ILP + W,
                         pg.data_ptr(), pd.data_ptr(), 0, 0, 0, 0, _stream())
        torch.cuda.synchronize()
        assert torch.equal(w[:n].double().cpu(), _f64(q_ref)), (name, W)
        assert _untouched(w[n:])
        _check_partials(pg, cnt, xx, (name, W, "r.r"))
        _check_partials(pd, cnt, xq, (name, W, "r.w"))


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_spmm_dot2_exact(tz, gpu, name, k):
    """csr_spmm_dot2 on k interleaved right-hand sides: every column of W equals the reference
    on its own x column, and slab j of each partial array sums to that column's dot products"""
    kn = tz._tz.kernels
    case, rp, ci = _structure(name, True)
    n = case.nrows
    val, x, _ = sr.exact_data(case, k=k, seed=14)
    assert x.shape == (n, k) and len({x[:, j].tobytes() for j in range(k)}) == k  # columns differ
    v, r = _dev(val, torch.float32), _x_dev(case, x, poison=False)
    assert r.data_ptr() % 16 == 0
    w_ref = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)
    x64 = x.astype(np.float64)
    rr, rw = (x64 * x64).sum(axis=0), (x64 * w_ref).sum(axis=0)
    assert np.abs(x64 * w_ref).sum(axis=0).max() < 2 ** 50
    for W in (1, 2, 4):
        cnt = kn.spmv_dot_partial_count(n, ILP + W)
        w, pg, pd = _nan32(n * k + GUARD), _nan64(k * SLAB + GUARD), _nan64(k * SLAB + GUARD)
        assert w.data_ptr() % 16 == 0
        kn.csr_spmm_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), r.data_ptr(), w.data_ptr(), k, ILP + W,
                         pg.data_ptr(), pd.data_ptr(), 0, 0, 0, 0, _stream())
        torch.cuda.synchronize()
        assert torch.equal(w[:n * k].view(n, k).double().cpu(), _f64(w_ref)), (name, k, W)
        assert _untouched(w[n * k:])
        _check_partials(pg, cnt, rr, (name, k, W, "r.r"))
        _check_partials(pd, cnt, rw, (name, k, W, "r.w"))


def _halo(tz, order):
    """the geometry of an 8 x 8 x 8 halo with ghost 2, 3 quantities and 26 directions"""
    a = tz.HaloArgs()
    a.nx = a.ny = a.nz = 8
    a.ghost, a.nq, a.neighbors, a.order = 2, 3, 26, order
    return tz.HaloExchange(a)


# (moves M, SpMV workgroups S, lanes per row W, stride): one move is one workgroup at this size
INTERLEAVES = [(1, 1, 4, 1),     # all = 2: the even quotient 2 becomes stride 1
               (26, 1, 1, 27),   # one SpMV workgroup, then every move
               (6, 6, 2, 1),     # S = M: quotient 2, stride 1, all SpMV workgroups first
               (26, 13, 4, 3),   # (M + S) / S = 3
               (21, 3, 1, 7),    # (M + S) / S = 8 becomes 7: the moves after the last SpMV slot shift by S
               (26, 5, 2, 5),    # 31 / 5 = 6 becomes 5
               (2, 7, 4, 1)]     # S > 3 M: stride 1


@pytest.mark.parametrize("order", ["xyzq", "qxyz"])
@pytest.mark.parametrize("M,S,W,stride", INTERLEAVES)
def test_box_move_spmv_interleave(tz, gpu, order, M, S, W, stride):
    """the branches of the interleave: the grid is exactly what the shape binding reports, every
    ghost equals the torch strided copy and the rest of the grid is untouched, and y equals the
    reference, plain and accumulating (a workgroup served twice would add its rows twice, one
    never served would leave the payload)"""
    kn = tz._tz.kernels
    h = _halo(tz, order)
    g = torch.Generator(device="cpu").manual_seed(3)
    grid = torch.randn(h.grid_elems(), generator=g, dtype=torch.float64).cuda()
    out, exp = grid.clone(), grid.clone()
    moves = []
    for i in range(h.ndirs())[:M]:
        s, d = h.pack_box(i), h.unpack_box(h.opposite(i))
        moves.append(dict(src=out.data_ptr(), dst=out.data_ptr(), src_off=s["grid_off"], dst_off=d["grid_off"],
                          s1=s["s1"], s2=s["s2"], s3=s["s3"], len=s["len"], n1=s["n1"], n2=s["n2"], n3=s["n3"]))
        for i3 in range(s["n3"]):
            for i2 in range(s["n2"]):
                so = s["grid_off"] + i2 * s["s2"] + i3 * s["s3"]
                do = d["grid_off"] + i2 * s["s2"] + i3 * s["s3"]
                exp.as_strided((s["n1"], s["len"]), (s["s1"], 1), do).copy_(
                    grid.as_strided((s["n1"], s["len"]), (s["s1"], 1), so))
    assert len(moves) == M and not torch.equal(exp, grid)
    n = S * 256 // W - 3  # a ragged last SpMV workgroup
    case = sr.lengths_case(n)
    assert kn.box_move_spmv_shape(moves, n, ILP + W) == dict(move_blocks=M, spmv_blocks=S, stride=stride)
    val, x, y0 = sr.exact_data(case, seed=15)
    rp, ci, v = _dev(case.row_ptr, torch.int32), _dev(case.col_ind, torch.int32), _dev(val, torch.float32)
    xd = _x_dev(case, x)
    assert xd.isnan().any()
    y = _nan32(n + GUARD)
    args = (n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), xd.data_ptr(), y.data_ptr(), ILP + W)
    kn.box_move_spmv(moves, *args, False, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out, exp)
    assert torch.equal(y[:n].double().cpu(), _f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)))
    y[:n] = torch.from_numpy(y0).cuda()
    kn.box_move_spmv(moves, *args, True, _stream())
    torch.cuda.synchronize()
    assert torch.equal(out, exp)
    assert torch.equal(y[:n].double().cpu(), _f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x, y0)))
    assert _untouched(y[n:])


def test_gather_grid_stride(tz, gpu):
    """more elements than 2048 workgroups of 256 cover at once: the grid-stride loop runs"""
    n = 2048 * 256 + 777
    g = torch.Generator(device="cpu").manual_seed(5)
    src = torch.randn(1000, generator=g)
    idx = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32)
    dst = _nan32(n + GUARD)
    tz._tz.kernels.gather_f32(n, src.cuda().data_ptr(), idx.cuda().data_ptr(), dst.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(dst[:n].cpu(), torch.from_numpy(src.numpy()[idx.numpy()]))
    assert _untouched(dst[n:])


def test_vector_add_grid_stride(tz, gpu):
    """more 16-byte quads than 2048 workgroups cover at once, and 3 tail elements"""
    n = 2048 * 1024 + 1027
    assert n // 4 > 2048 * 256 and n % 4 == 3
    g = torch.Generator(device="cpu").manual_seed(6)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd, y = a.cuda(), b.cuda(), _nan32(n + GUARD)
    tz._tz.kernels.vector_add_f32(n, ad.data_ptr(), bd.data_ptr(), y.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(y[:n].cpu(), (a.double() + b.double()).float())  # one rounding either way
    assert _untouched(y[n:])


def test_vector_add_rejects_misaligned_pointers(tz, gpu):
    """the throw only: nothing is launched on a misaligned pointer"""
    from tenzing_amd import ops

    kn = tz._tz.kernels
    t = [torch.ones(64, device="cuda") for _ in range(3)]
    y = _nan32(64)
    ptr = [t[0].data_ptr(), t[1].data_ptr(), y.data_ptr()]
    assert all(p % 16 == 0 for p in ptr)
    for i in range(3):
        for off in (4, 8, 12):
            bad = list(ptr)
            bad[i] += off
            with pytest.raises(Exception, match="16-byte aligned"):
                kn.vector_add_f32(8, *bad, _stream())
    torch.cuda.synchronize()
    assert _untouched(y)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.vector_add(t[0][1:], t[1][:-1])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.vector_add(t[0][:-1], t[1][1:])
    # a slice that starts on a 16-byte boundary is fine
    assert torch.equal(ops.vector_add(t[0][4:], t[1][:60]), torch.full((60,), 2.0, device="cuda"))


@pytest.mark.parametrize("W,name", [(1, "lengths"), (2, "dups"), (4, "narrow")])
def test_ops_csr_spmv_accepts_the_ilp_lanes(tz, gpu, W, name):
    from tenzing_amd import ops

    case, rp, ci = _structure(name)
    val, x, y0 = sr.exact_data(case, seed=16)
    v, xd = _dev(val, torch.float32), _x_dev(case, x)
    y = ops.csr_spmv(rp, ci, v, xd, lanes=ILP + W)
    torch.cuda.synchronize()
    assert torch.equal(y.double().cpu(), _f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)))
    y = ops.csr_spmv(rp, ci, v, xd, y=torch.from_numpy(y0).cuda(), lanes=ILP + W,
                     accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(y.double().cpu(), _f64(sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x, y0)))
    for bad in (3, ILP, ILP + 3, ILP + 8, -2):
        with pytest.raises(ValueError, match="SPMV_ILP"):
            ops.csr_spmv(rp, ci, v, xd, lanes=bad)
