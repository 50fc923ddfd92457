"""A plain numpy reference for the CSR SpMV kernels (csrc/kernels/spmv_kernels.hip,
spmv_device.hpp, the SpMV + dot kernels of cg_kernels.hip), and the matrices to hold them to it.

It shares nothing with the native code and calls neither scipy nor torch sparse:

- `csr_matvec_f64` is the product in float64 by plain accumulation;
- `abs_bound` is the derived error bound of an f32 dot product, the only tolerance the tests of
  random data use;
- `zoo` yields small named matrices with the row shapes at which the kernels change path (the
  CSR-stream kernel's 64-row blocks and 4096-product passes, the 16-entry passes of the ILP
  kernels, rows shorter than a lane group, empty rows and blocks, rectangular shapes, repeated
  and unsorted columns); `premises` measures what each case claims about itself (`CLAIMS`), so a
  test can prove it is not void;
- `exact_data` draws values on which every summation order is exact in f32, fused or not
  (tests/test_spmv_ref.py proves it), so a kernel's output must equal the reference bit for bit
  and any dropped, duplicated or misattributed entry changes it.
"""
from __future__ import annotations

from typing import Iterator, NamedTuple

import numpy as np

STREAM_ROWS = 64    # rows per workgroup of the CSR-stream kernel
STREAM_CAP = 4096   # products it stages per pass
ILP_PASS = 16       # entries per pass of an ILP lane group (W * K)
MAX_ROWS, MAX_NNZ = 10_000, 60_000
U32 = 2.0 ** -24    # unit roundoff of f32


class Case(NamedTuple):
    name: str
    nrows: int
    ncols: int
    row_ptr: np.ndarray  # int32, nrows + 1
    col_ind: np.ndarray  # int32
    val: np.ndarray      # float32, random normal (exact_data replaces it)


def _rows(row_ptr) -> np.ndarray:
    """the row of every entry"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def csr_matvec_f64(row_ptr, col_ind, val, x, y0=None) -> np.ndarray:
    """y = A x (+ y0) in float64, one np.add.at over the entries in storage order. `x` is
    (ncols,) or (ncols, k); the result (and y0) is (nrows,) or (nrows, k) accordingly."""
    x = np.asarray(x, dtype=np.float64)
    xs = x.reshape(x.shape[0], -1)
    nrows = len(row_ptr) - 1
    col = np.asarray(col_ind, dtype=np.int64)
    prod = np.asarray(val, dtype=np.float64)[:, None] * xs[col]
    y = np.zeros((nrows, xs.shape[1]), dtype=np.float64)
    np.add.at(y, _rows(row_ptr), prod)
    y = y.reshape((nrows,) + x.shape[1:])
    if y0 is not None:
        y = y + np.asarray(y0, dtype=np.float64)
    return y


def abs_sum(row_ptr, col_ind, val, x) -> np.ndarray:
    """per row, sum_j |a_j| |x_j| in float64 (shaped as csr_matvec_f64's result)"""
    return csr_matvec_f64(row_ptr, col_ind, np.abs(np.asarray(val, dtype=np.float64)),
                          np.abs(np.asarray(x, dtype=np.float64)))


def abs_bound(row_ptr, col_ind, val, x) -> np.ndarray:
    """per row, (L + 2) 2^-24 sum_j |a_j| |x_j| with L the row length: the bound of an L-term
    f32 dot product summed in any order, with or without fma. Higham (Accuracy and Stability of
    Numerical Algorithms, section 3.1) gives |error| <= gamma_L sum |a_j x_j| with gamma_L =
    L u / (1 - L u) = L u + O(L^2 u^2); Jeannerod and Rump (Improved error bounds for inner
    products in floating-point arithmetic, SIAM J. Matrix Anal. Appl. 34, 2013) show that L u
    itself bounds it, for every L and every order, which (L + 2) u covers. Additions of the exact
    zeros that idle lanes contribute round nothing. Derived, not measured (underflow aside: the
    data here stays far from it)."""
    s = abs_sum(row_ptr, col_ind, val, x)
    length = np.diff(np.asarray(row_ptr, dtype=np.int64)).astype(np.float64)
    return (length + 2.0).reshape((-1,) + (1,) * (s.ndim - 1)) * U32 * s


def _case(name: str, lengths, ncols: int, rng, holes=None, dups: bool = False) -> Case:
    """a matrix with the given row lengths. Columns come from all but `holes` (default: the
    middle column, so that one column at least is referenced by nobody); sorted and unique in a
    row, or with `dups` drawn with repetition and left unsorted."""
    lengths = np.asarray(lengths, dtype=np.int64)
    holes = [ncols // 2] if holes is None else list(holes)
    allowed = np.setdiff1d(np.arange(ncols, dtype=np.int64), holes)
    cols = []
    for n in lengths:
        if dups or n > len(allowed):
            cols.append(rng.choice(allowed, size=int(n), replace=True))
        else:
            cols.append(np.sort(rng.choice(allowed, size=int(n), replace=False)))
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    rp = np.concatenate(([0], np.cumsum(lengths)))
    val = rng.standard_normal(len(col)).astype(np.float32)
    return Case(name, len(lengths), ncols, rp.astype(np.int32), col.astype(np.int32), val)


def _split(total: int, parts: int, rng) -> np.ndarray:
    """`parts` row lengths, uneven and with empty rows among them, that add up to `total`"""
    w = rng.random(parts) ** 3
    w[rng.integers(0, parts, size=parts // 8)] = 0.0
    return rng.multinomial(total, w / w.sum())


def lengths_case(nrows: int, seed: int = 7, ncols: int = 200) -> Case:
    """a matrix of any row count in the style of the `lengths` case: its rows run through a
    shuffle of the lengths 0..70, 127, 128, 129 again and again (74 rows hold all of them)"""
    rng = np.random.default_rng([seed, nrows])
    base = rng.permutation(np.concatenate((np.arange(71), [127, 128, 129])))
    return _case(f"lengths_{nrows}", np.resize(base, nrows), ncols, rng)


CAP_BLOCKS =(STREAM_CAP - 1, STREAM_CAP, STREAM_CAP + 1, 1023, 1024, 1025)


def _band() -> Case:
    from .. import _tz  # the generator of the ordinary case is the project's own (host code)

    n = 5000
    rp, ci, val = _tz.random_band_matrix(n, 300, 10 * n, 7)
    return Case("band", n, n, np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32),
                np.asarray(val, dtype=np.float32))


def zoo(seed: int = 2024) -> Iterator[Case]:
    """the named cases, deterministic in `seed`; every one within MAX_ROWS rows and MAX_NNZ entries"""
    rng = np.random.default_rng(seed)
    # one entry; then mixed short rows around the stream block of 64 rows and the 4 rows per
    # workgroup of 64 lanes per row, with a ragged last workgroup
    yield _case("tiny_1", [1], 3, rng)
    for n in (63, 64, 65, 257):
        yield _case(f"tiny_{n}", rng.integers(0, 7, size=n), n, rng)
    yield _case("empty_all", np.zeros(200, dtype=np.int64), 50, rng)
    # first row, last row and rows 100..239 empty: the stream block of rows 128..191 has a == b
    ln = rng.integers(1, 9, size=400)
    ln[0] = ln[-1] = 0
    ln[100:240] = 0
    yield _case("empty_runs", ln, 400, rng)
    # every length 0..70, then 127, 128, 129, in an order that is not sorted by length
    yield _case("lengths", rng.permutation(np.concatenate((np.arange(71), [127, 128, 129]))), 200, rng)
    # 17 entries in 5 short rows, then 9000 in one: it starts off a multiple of 4096, is clipped
    # at the end of the first stream pass, fills the second and is clipped at the start of the third
    yield _case("long_row", np.concatenate(([3, 0, 5, 2, 7], [9000], rng.integers(0, 12, size=30))), 10_000, rng)
    # 64-row blocks holding exactly these many entries, then a ragged block of 20 rows
    yield _case("cap", np.concatenate([_split(t, STREAM_ROWS, rng) for t in CAP_BLOCKS]
                                      + [rng.integers(0, 9, size=20)]), 2000, rng)
    # rectangular: 7 columns, each gathered hundreds of times; 5000 columns over 65 rows
    yield _case("narrow", rng.integers(0, 7, size=300), 7, rng)
    yield _case("wide", rng.integers(0, 41, size=65), 5000, rng)
    # repeated and unsorted columns (40 columns, rows of up to 50 entries)
    yield _case("dups", rng.integers(0, 51, size=130), 40, rng, dups=True)
    yield _band()


# what each case claims about itself (keys of `premises`); every case but the ordinary one also
# has a column that no entry references
CLAIMS = {"long_row": ("long_row",), "cap": ("cap_block",), "empty_all": ("empty_block",),
          "empty_runs": ("empty_block", "empty_ends"), "dups": ("dup_cols", "unsorted_cols"),
          "band": ()}


def claims(name: str) -> tuple:
    return CLAIMS.get(name, ()) + (() if name == "band" else ("unreferenced_col",))


def block_entries(case: Case) -> np.ndarray:
    """entries per STREAM_ROWS-row block (the last block may be ragged)"""
    rp = np.asarray(case.row_ptr, dtype=np.int64)
    edges = np.minimum(np.arange(0, case.nrows + STREAM_ROWS, STREAM_ROWS), case.nrows)
    return np.diff(rp[edges])


def premises(case: Case) -> dict:
    """measured on the case: the facts its name stands for"""
    rp = np.asarray(case.row_ptr, dtype=np.int64)
    length = np.diff(rp)
    per_block = block_entries(case)
    whole = per_block[:case.nrows // STREAM_ROWS]
    used = np.zeros(case.ncols, dtype=bool)
    used[case.col_ind] = True
    dup = unsorted = False
    for r in np.nonzero(length > 1)[0]:
        c = case.col_ind[rp[r]:rp[r + 1]]
        dup = dup or len(np.unique(c)) < len(c)
        unsorted = unsorted or bool((np.diff(c) < 0).any())
    return dict(long_row=bool(length.max(initial=0) > 2 * STREAM_CAP),
                cap_block=bool((whole == STREAM_CAP).any()),
                empty_block=bool((whole == 0).any()),
                empty_ends=bool(case.nrows > 1 and length[0] == 0 and length[-1] == 0),
                unreferenced_col=bool((~used).any()), dup_cols=dup, unsorted_cols=unsorted)


def squared(case: Case) -> Case:
    """the case made square, for the kernels that need x and y of one length: empty rows are
    appended, or columns that nobody references; the entries and their order stay"""
    n = max(case.nrows, case.ncols)
    rp = np.concatenate((case.row_ptr, np.full(n - case.nrows, case.row_ptr[-1], dtype=np.int32)))
    return case._replace(nrows=n, ncols=n, row_ptr=rp)


def exact_data(case: Case, k: int = 1, seed: int = 0):
    """(val, x, y0), all float32: values m / 8 with m in +-{1..8}, x integers in +-{1..16}
    ((ncols,) or, with k > 1, (ncols, k)), y0 integers in +-{1..64} shaped like the product.
    Every product is a multiple of 1/8 of magnitude at most 16, so while a row's sum of
    magnitudes stays below 2^24 eighths every partial sum, in any order, fused or not, is a
    multiple of 1/8 below 2^24 eighths: exact in f32. Asserted here for the case, with room for
    y0 + 2 A x (two accumulating launches). No value and no x entry is zero."""
    rng = np.random.default_rng([seed, k, case.nrows, len(case.col_ind)])
    nnz = len(case.col_ind)

    def signed(hi, shape):
        return (rng.integers(1, hi + 1, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float32)

    val = signed(8, nnz) / np.float32(8)
    shape = (case.ncols,) if k == 1 else (case.ncols, k)
    x = signed(16, shape)
    y0 = signed(64, (case.nrows,) + shape[1:])
    worst = float(abs_sum(case.row_ptr, case.col_ind, val, x).max(initial=0.0))
    assert worst * 8 < 2 ** 24, (case.name, worst)
    assert (2 * worst + 64) * 8 < 2 ** 24, (case.name, worst)
    return val, x, y0


def normal_data(case: Case, k: int = 1, seed: int = 0):
    """(val, x): the case's own random-normal values and a random-normal float32 x"""
    rng = np.random.default_rng([seed, k, case.ncols])
    shape = (case.ncols,) if k == 1 else (case.ncols, k)
    return case.val, rng.standard_normal(shape).astype(np.float32)


def referenced(case: Case) -> np.ndarray:
    """mask over the columns: True where some entry references the column"""
    used = np.zeros(case.ncols, dtype=bool)
    used[case.col_ind] = True
    return used
