"""The numpy stencil reference (tenzing_amd/utils/stencil_ref.py) on its own: the premise that
makes bit-exact GPU comparisons legitimate, the error bound for the default coefficients, and the
identities that show what the affine field of `stencil_check` can and cannot see."""
import numpy as np
import pytest

from tenzing_amd.utils import stencil_ref as sr


def _box(layout, xs, nx, ny, nz, m0=0, m1=0, **kw):
    """'q' QXYZ-like (nouter 1, row xs * nx), 'x' XYZQ-like (xs 1, nouter 3). Returns (box, n)"""
    if layout == "q":
        return sr.padded_box(xs * nx, ny, nz, xs, 1, m0, m1, **kw)
    return sr.padded_box(nx, ny, nz, 1, 3, m0, m1, **kw)


def _coords(b, e):
    """(o, z, y, i) of flat indices e relative to the box (negative / beyond: outside it)"""
    # padded_box puts the box's first element 4 into the pitched row, one row and one plane into
    # its padded volume: count from that volume's first element
    r = e - b["base"]
    lead = b["sz"] + b["sy"] + 4
    o = np.floor_divide(r + lead, b["so"]) if b["so"] else np.zeros_like(r)
    r = r - o * b["so"]
    z = np.floor_divide(r + lead, b["sz"]) - 1
    r = r - z * b["sz"]
    y = np.floor_divide(r + b["sy"] + 4, b["sy"]) - 1
    return o, z, y, r - y * b["sy"]


def test_exact_inputs_make_every_evaluation_order_exact():
    """integers in [-2^20, 2^20] with c0 = 1/2, c1 = 1/8: the source's order, a pairwise order
    with c1 distributed, and integer arithmetic agree on every one of 2 * 10^6 samples, so a
    kernel may be held to torch.equal whatever order or contraction the compiler picks"""
    rng = np.random.default_rng(1)
    v = sr.exact_field(rng, (7, 2_000_000))
    assert v.min() >= -sr.EXACT_RANGE and v.max() <= sr.EXACT_RANGE and np.array_equal(v, np.rint(v))
    c, xm, xp, ym, yp, zm, zp = v
    c0, c1 = sr.C0_EXACT, sr.C1_EXACT
    a = c0 * c + c1 * (xm + xp + ym + yp + zm + zp)
    b = ((c1 * zp + c1 * zm) + (c1 * yp + c1 * ym)) + ((c1 * xp + c1 * xm) + c0 * c)
    vi = v.astype(np.int64)
    num = 4 * vi[0] + vi[1:].sum(axis=0)
    assert int(np.abs(num).max()) < 1 << 24
    k = num.astype(np.float64) / 8.0  # an integer below 2^24 over a power of two: exact
    assert np.array_equal(a, b) and np.array_equal(a, k)
    # the extreme of the range as well
    top = float(sr.EXACT_RANGE)
    assert c0 * top + c1 * (6 * top) == 1.25 * top


def test_default_coefficients_bound_holds_between_honest_orders():
    """c0 = 0.4, c1 = 0.1 on standard-normal data: two float64 orders differ by well under
    2^-49 A, and each is within 2^-49 A of an extended-precision evaluation"""
    rng = np.random.default_rng(2)
    v = rng.standard_normal((7, 2_000_000))
    c, xm, xp, ym, yp, zm, zp = v
    c0, c1 = sr.C0_DEFAULT, sr.C1_DEFAULT
    a = c0 * c + c1 * (xm + xp + ym + yp + zm + zp)
    b = ((c1 * zp + c1 * zm) + (c1 * yp + c1 * ym)) + ((c1 * xp + c1 * xm) + c0 * c)
    A = abs(c0) * np.abs(c) + abs(c1) * np.abs(v[1:]).sum(axis=0)
    assert float((np.abs(a - b) / A).max()) < 2.0 ** -50
    if np.finfo(np.longdouble).nmant > 52:
        L = v.astype(np.longdouble)
        w = np.longdouble(c0) * L[0] + np.longdouble(c1) * L[1:].sum(axis=0)
        for got in (a, b):
            assert float((np.abs(got - w) / A).max()) < 2.0 ** -50


@pytest.mark.parametrize("layout,xs", [("q", 3), ("x", 1)])
@pytest.mark.parametrize("m0,m1", [(0, 0), (1, 0), (4, 2)])
def test_apply_matches_a_cell_by_cell_loop(layout, xs, m0, m1):
    """the vectorised reference against a loop over cells written from the contract's words"""
    b, n = _box(layout, xs, 5, 3, 2, m0, m1)
    rng = np.random.default_rng(3)
    f = sr.poisoned_input([b], n, rng)
    mask, val = sr.apply(b, f)
    want = np.full(n, np.nan)
    cnt = 0
    for o in range(b["nouter"]):
        for z in range(b["nz"]):
            for y in range(b["ny"]):
                for i in range(m0, b["row"] - m1):
                    e = b["base"] + o * b["so"] + z * b["sz"] + y * b["sy"] + i
                    want[e] = 0.4 * f[e] + 0.1 * (f[e - b["xs"]] + f[e + b["xs"]] + f[e - b["sy"]] +
                                                  f[e + b["sy"]] + f[e - b["sz"]] + f[e + b["sz"]])
                    cnt += 1
    assert int(mask.sum()) == cnt == sr.cells(b).size
    assert np.isfinite(val).all(), "the reference read a cell that is not needed"
    assert np.array_equal(want[mask], val) and np.isnan(want[~mask]).all()
    assert np.array_equal(sr.magnitude(b, f) >= np.abs(val), np.ones(cnt, dtype=bool))


@pytest.mark.parametrize("layout,xs", [("q", 1), ("q", 2), ("q", 4), ("x", 1)])
def test_needed_is_the_cells_and_their_face_neighbours(layout, xs):
    b, n = _box(layout, xs, 6, 4, 3)
    nd = sr.needed(b, n)
    o, z, y, i = _coords(b, np.flatnonzero(nd))
    inx, iny, inz = (i >= 0) & (i < b["row"]), (y >= 0) & (y < b["ny"]), (z >= 0) & (z < b["nz"])
    # never two axes outside at once (no edge or corner apron), and never further than one cell
    assert (inx.astype(int) + iny + inz >= 2).all()
    assert (i >= -b["xs"]).all() and (i < b["row"] + b["xs"]).all()
    assert (y >= -1).all() and (y <= b["ny"]).all() and (z >= -1).all() and (z <= b["nz"]).all()
    per = (b["row"] * b["ny"] * b["nz"] + 2 * b["xs"] * b["ny"] * b["nz"]
           + 2 * b["row"] * b["nz"] + 2 * b["row"] * b["ny"])
    assert int(nd.sum()) == per * b["nouter"]
    # a corner of the apron and an element two planes below are not needed
    assert not nd[b["base"] - b["sz"] - b["sy"]] and not nd[b["base"] - b["sy"] - 1]


@pytest.mark.parametrize("layout,xs", [("q", 3), ("q", 4), ("x", 1)])
def test_masked_box_needs_nothing_beside_its_rows(layout, xs):
    """m0 = m1 = xs (the workload's ghost-free interior): no element left of a row's start or
    right of its end is needed; a mask narrower than xs still needs part of the x apron"""
    bx = xs if layout == "q" else 1
    b, n = _box(layout, xs, 6, 4, 3, bx, bx)
    _, _, _, i = _coords(b, np.flatnonzero(sr.needed(b, n)))
    assert i.min() == 0 and i.max() == b["row"] - 1
    if b["xs"] > 1:
        b1, _ = _box(layout, xs, 6, 4, 3, 1, 0)
        _, _, _, i = _coords(b1, np.flatnonzero(sr.needed(b1, n)))
        assert i.min() == 1 - b1["xs"] and i.max() == b1["row"] + b1["xs"] - 1
    # a box masked away entirely needs, and writes, nothing
    gone, _ = _box(layout, xs, 6, 4, 3, b["row"], 0)
    assert sr.cells(gone).size == 0 and not sr.needed(gone, n).any()
    empty = dict(b, nz=0)
    assert sr.cells(empty).size == 0 and not sr.needed(empty, n).any()


def test_needed_rejects_an_apron_outside_the_array():
    b, n = _box("q", 2, 6, 4, 3)
    with pytest.raises(ValueError):
        sr.needed(dict(b, base=b["sz"] - 1), n)
    with pytest.raises(ValueError):
        sr.needed(b, n - 2 * b["sz"])
    with pytest.raises(ValueError):  # rows that run into each other
        sr.apply(dict(b, sy=b["row"] - 1), np.zeros(n))


def test_constant_and_affine_fields():
    """a constant field gives (c0 + 6 c1) times the constant. An affine field reproduces itself
    when c0 + 6 c1 = 1 -- and does so for WRONG stencils too, as long as they read a symmetric
    pair on each axis: the field of halo_init cannot tell them from the right one, random data
    can"""
    # c0 + 6 c1 = 1, exact on integers; masked like the workload's interior, so that the wrong
    # stencils below stay inside the pitched rows
    b, n = _box("q", 3, 7, 5, 4, 3, 3, c0=0.25, c1=0.125)
    mask, val = sr.apply(b, np.full(n, 3.0))
    assert np.array_equal(val, np.full(val.size, 3.0))
    _, val = sr.apply(dict(b, c0=0.5), np.full(n, 3.0))
    assert np.array_equal(val, np.full(val.size, (0.5 + 6 * 0.125) * 3.0))

    e = np.arange(n, dtype=np.int64)
    _, z, y, i = _coords(b, e)
    x, q = np.floor_divide(i, 3), np.mod(i, 3)
    affine = (x + 64.0 * y + 4096.0 * z + 262144.0 * q).astype(np.float64)
    mask, val = sr.apply(b, affine)
    assert np.array_equal(val, affine[mask])

    def wrong(f, offs):
        c = np.flatnonzero(mask)
        return 0.25 * f[c] + 0.125 * sum(f[c + d] for d in offs)
    xs, sy, sz = b["xs"], b["sy"], b["sz"]
    rng = np.random.default_rng(4)
    rnd = sr.exact_field(rng, n)
    _, right = sr.apply(b, rnd)
    assert np.array_equal(wrong(rnd, (-xs, xs, -sy, sy, -sz, sz)), right)
    for offs in ((-xs, xs, -xs, xs, -sz, sz),          # x read twice instead of y
                 (-2 * xs, 2 * xs, -sy, sy, -sz, sz),  # +-2 instead of +-1
                 (-xs, xs, -sz, sz, -sz, sz)):         # z read twice instead of y
        assert np.array_equal(wrong(affine, offs), affine[mask]), "the affine field sees this error"
        assert not np.array_equal(wrong(rnd, offs), right), "random data misses this error"
