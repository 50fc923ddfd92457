"""The numpy SpMV reference (tenzing_amd/utils/spmv_ref.py) checked against itself and against
dense float64 products, without a GPU: the reference product, the zoo's claims about its own
cases, the exactness of `exact_data` under three f32 summation orders, and `abs_bound`."""
import functools

import numpy as np
import pytest

from tenzing_amd.utils import spmv_ref as sr


@functools.lru_cache(maxsize=None)
def _zoo():
    return tuple(sr.zoo())


NAMES = ["tiny_1", "tiny_63", "tiny_64", "tiny_65", "tiny_257", "empty_all", "empty_runs", "lengths",
         "long_row", "cap", "narrow", "wide", "dups", "band"]


def _get(name):
    return next(c for c in _zoo() if c.name == name)


def _dense(case, val):
    """the matrix as a dense float64 array (duplicates add up)"""
    a = np.zeros((case.nrows, case.ncols), dtype=np.float64)
    rp = case.row_ptr
    for r in range(case.nrows):
        for j in range(rp[r], rp[r + 1]):
            a[r, case.col_ind[j]] += np.float64(val[j])
    return a


def _seq(p):
    """f32 sum of p (entries, k) in storage order (cumsum accumulates left to right)"""
    return np.cumsum(p, axis=0, dtype=np.float32)[-1] if len(p) else np.zeros(p.shape[1:], np.float32)


def _pairwise(p):
    """f32 sum of p by repeated halving: neighbours first, then pairs of pairs, .."""
    if not len(p):
        return np.zeros(p.shape[1:], np.float32)
    while len(p) > 1:
        if len(p) % 2:
            p = np.concatenate((p, np.zeros((1,) + p.shape[1:], np.float32)))
        p = p[0::2] + p[1::2]
        assert p.dtype == np.float32
    return p[0]


def _f32_products(case, val, x, order):
    """per row, the f32 sum in `order` of the f32-rounded products; shaped like the reference"""
    xs = x.reshape(x.shape[0], -1)
    out = np.zeros((case.nrows, xs.shape[1]), dtype=np.float32)
    rp = case.row_ptr
    for r in range(case.nrows):
        p = val[rp[r]:rp[r + 1], None] * xs[case.col_ind[rp[r]:rp[r + 1]]]
        assert p.dtype == np.float32
        out[r] = order(p)
    return out.reshape((case.nrows,) + x.shape[1:])


def test_zoo_is_complete_and_small():
    assert [c.name for c in _zoo()] == NAMES
    for c in _zoo():
        assert 1 <= c.nrows <= sr.MAX_ROWS and len(c.col_ind) <= sr.MAX_NNZ
        assert max(c.nrows, c.ncols) <= sr.MAX_ROWS  # `squared` stays within the limit too
        assert c.row_ptr.dtype == np.int32 and c.col_ind.dtype == np.int32 and c.val.dtype == np.float32
        assert c.row_ptr[0] == 0 and c.row_ptr[-1] == len(c.col_ind) == len(c.val)
        assert len(c.row_ptr) == c.nrows + 1 and (np.diff(c.row_ptr) >= 0).all()
        if len(c.col_ind):
            assert 0 <= c.col_ind.min() and c.col_ind.max() < c.ncols
    # deterministic in the seed
    for a, b in zip(_zoo(), sr.zoo()):
        assert all(np.array_equal(u, v) for u, v in zip(a[3:], b[3:]))


@pytest.mark.parametrize("name", NAMES)
def test_premises_hold(name):
    case = _get(name)
    got = sr.premises(case)
    for claim in sr.claims(name):
        assert got[claim], (name, claim, got)


def test_every_premise_is_claimed_and_shapes_are_as_named():
    claimed = {c for n in NAMES for c in sr.claims(n)}
    assert claimed == set(sr.premises(_get("tiny_1")))
    length = {n: np.diff(_get(n).row_ptr) for n in NAMES}
    assert _get("tiny_1").nrows == 1 and len(_get("tiny_1").col_ind) == 1
    assert [_get(f"tiny_{n}").nrows for n in (63, 64, 65, 257)] == [63, 64, 65, 257]
    assert len(_get("empty_all").col_ind) == 0
    # a run of at least 130 empty rows, so a whole stream block inside it whatever its phase
    runs = "".join("e" if v == 0 else "x" for v in length["empty_runs"])
    assert max(len(r) for r in runs.split("x")) >= 130
    # every length 0..70 and 127..129, not in sorted order
    assert sorted(length["lengths"]) == list(range(71)) + [127, 128, 129]
    assert (np.diff(length["lengths"]) < 0).any() and (np.diff(length["lengths"]) > 0).any()
    # the long row: 9000 entries, starts off a multiple of the pass size, spans three passes of
    # its block (which starts at entry 0), short rows before and after
    c = _get("long_row")
    r = int(np.argmax(length["long_row"]))
    lo, hi = int(c.row_ptr[r]), int(c.row_ptr[r + 1])
    assert hi - lo == 9000 and lo % sr.STREAM_CAP != 0 and 0 < r < c.nrows - 1 and r < sr.STREAM_ROWS
    assert lo // sr.STREAM_CAP == 0 and (hi - 1) // sr.STREAM_CAP == 2 and hi % sr.STREAM_CAP != 0
    # blocks of exactly these sizes around the pass size and the unrolled loop's hand-over
    assert list(sr.block_entries(_get("cap"))[:6]) == [4095, 4096, 4097, 1023, 1024, 1025]
    assert _get("cap").nrows % sr.STREAM_ROWS != 0
    assert (_get("narrow").nrows, _get("narrow").ncols) == (300, 7)
    assert (_get("wide").nrows, _get("wide").ncols) == (65, 5000)
    assert length["narrow"].sum() > 100 * 7  # each x entry gathered hundreds of times
    assert (_get("band").nrows, _get("band").ncols, len(_get("band").col_ind)) == (5000, 5000, 50_000)


@pytest.mark.parametrize("name", NAMES)
def test_csr_matvec_f64_matches_dense(name):
    """on exact data, where the dense product (another order, duplicates merged first) is exact
    too: equality, no tolerance"""
    case = _get(name)
    rng = np.random.default_rng(5)
    for k in (1, 3):
        val, x, y0 = sr.exact_data(case, k=k, seed=1)
        got = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)
        assert got.shape == (case.nrows,) + x.shape[1:] and got.dtype == np.float64
        assert np.array_equal(got, _dense(case, val) @ x.astype(np.float64))
        got0 = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x, y0)
        assert np.array_equal(got0, got + y0) and (got0 != got).all()
    sq = sr.squared(case)
    assert sq.nrows == sq.ncols == max(case.nrows, case.ncols)
    xs = rng.standard_normal(sq.ncols)
    ys = sr.csr_matvec_f64(sq.row_ptr, sq.col_ind, sq.val, xs)
    assert np.array_equal(ys[:case.nrows], sr.csr_matvec_f64(case.row_ptr, case.col_ind, case.val, xs[:case.ncols]))
    assert not ys[case.nrows:].any()


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_exact_data_is_exact_in_f32_in_any_order(name, k):
    case = _get(name)
    val, x, y0 = sr.exact_data(case, k=k, seed=3)
    assert val.dtype == x.dtype == y0.dtype == np.float32
    assert x.shape == ((case.ncols,) if k == 1 else (case.ncols, k)) and y0.shape == (case.nrows,) + x.shape[1:]
    m = val * 8
    assert (m == np.round(m)).all() and (np.abs(m) >= 1).all() and (np.abs(m) <= 8).all()
    assert (x == np.round(x)).all() and (np.abs(x) >= 1).all() and (np.abs(x) <= 16).all()
    assert (y0 == np.round(y0)).all() and (np.abs(y0) >= 1).all() and (np.abs(y0) <= 64).all()
    ref = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)
    assert (ref * 8 == np.round(ref * 8)).all()
    for order in (_seq, _pairwise, lambda p: _seq(p[::-1])):
        got = _f32_products(case, val, x, order)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref)
    # y0 + 2 A x as two accumulating f32 launches form it
    acc = (y0 + _f32_products(case, val, x, _seq)) + _f32_products(case, val, x, _pairwise)
    assert acc.dtype == np.float32
    assert np.array_equal(acc.astype(np.float64), sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, 2 * x, y0))
    # different seeds and k draw different data
    assert not np.array_equal(sr.exact_data(case, k=k, seed=4)[1], x)


@pytest.mark.parametrize("name", NAMES)
def test_abs_bound_holds_and_is_not_vacuous(name):
    case = _get(name)
    val, x = sr.normal_data(case, k=2, seed=9)
    assert val.dtype == x.dtype == np.float32 and x.shape == (case.ncols, 2)
    ref = sr.csr_matvec_f64(case.row_ptr, case.col_ind, val, x)
    bound = sr.abs_bound(case.row_ptr, case.col_ind, val, x)
    mag = sr.abs_sum(case.row_ptr, case.col_ind, val, x)
    assert bound.shape == ref.shape == mag.shape
    length = np.diff(case.row_ptr)
    assert np.array_equal(bound, (length[:, None] + 2.0) * 2.0 ** -24 * mag)
    assert (bound <= 1e-3 * mag).all() and (bound[length > 0] > 0).all() and not bound[length == 0].any()
    for order in (_seq, _pairwise):
        err = np.abs(_f32_products(case, val, x, order).astype(np.float64) - ref)
        assert (err <= bound).all(), (name, float((err - bound).max()))
    if len(case.col_ind):  # and it bites: an entry dropped from the longest row breaks it
        r = int(np.argmax(length))
        lo, hi = case.row_ptr[r], case.row_ptr[r + 1]
        j = lo + int(np.argmax(np.abs(val[lo:hi] * x[case.col_ind[lo:hi], 0])))
        v2 = val.copy()
        v2[j] = 0
        err = np.abs(sr.csr_matvec_f64(case.row_ptr, case.col_ind, v2, x) - ref)
        assert err[r, 0] > bound[r, 0]
