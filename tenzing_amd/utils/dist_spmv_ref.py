"""A plain numpy model of the distributed SpMV workload (csrc/workloads/spmv.cpp): the row
partition, the local / remote split, the receive and send plans, and the product itself.

It shares nothing with the native code. Everything is built from the global CSR matrix `A =
(row_ptr, col_ind, val)` alone, written from the definitions:

- rank r of P owns a contiguous run of rows (and the x entries of the same indices); the runs
  are as even as can be, the n mod P ranks of lowest number holding one row more;
- an entry of one of my rows is local when I own its column, else remote; the remote-x buffer
  has one slot per distinct remote column, in increasing column order;
- rank p sends rank q the x entries of the columns of p that q's rows use, in q's slot order.

`y_ref` and `bound` are `spmv_ref.csr_matvec_f64` and `spmv_ref.abs_bound` over whole rows of
the whole matrix with the whole x. The split form (two partial dots and one add), the accumulate
form and any library order are each some summation order of a row's L products, so the derived
(L + 2) u bound of an L-term dot product holds for the full row unchanged.
"""
from __future__ import annotations

import numpy as np

from . import spmv_ref

GENERATIONS = 4
GEN_STRIDE = 1000003  # 1000003 mod 2000 = 3: a generation shifts the hash's residues


def x_gen(g, gen: int) -> np.ndarray:
    """x of global index (or indices) g in value generation gen, float32: the multiplicative hash
    ((g + gen * 1000003) * 2654435761 mod 2000 - 1000) / 1000, thousandths in [-1, 1). Generation
    0 is the x of every ordinary run. 2654435761 * 1000003 * gen mod 2000 is 1283, 566, 1849 for
    gen 1, 2, 3: no two generations agree anywhere."""
    k = (np.asarray(g, dtype=np.int64) + np.int64(gen) * GEN_STRIDE) * np.int64(2654435761) % 2000
    return (k - 1000).astype(np.float32) / np.float32(1000)


def row_starts(n: int, size: int) -> np.ndarray:
    """first row of every rank, and n at the end (size + 1 entries)"""
    counts = np.full(size, n // size, dtype=np.int64)
    counts[:n % size] += 1
    return np.concatenate(([0], np.cumsum(counts)))


def row_partition(n: int, rank: int, size: int):
    s = row_starts(n, size)
    return int(s[rank]), int(s[rank + 1])


def owner_of(cols, n: int, size: int) -> np.ndarray:
    """the rank whose run of rows holds each index"""
    return np.searchsorted(row_starts(n, size), np.asarray(cols, dtype=np.int64), side="right") - 1


def as_csr(A):
    rp, ci, val = A
    return (np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64),
            np.asarray(val, dtype=np.float32))


def rows_of(A, r0: int, r1: int):
    """rows [r0, r1) of A as a CSR of their own (global columns)"""
    rp, ci, val = as_csr(A)
    return rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], val[rp[r0]:rp[r1]]


def _select(rp, mask):
    """row pointers of the entries that `mask` keeps"""
    kept = np.concatenate(([0], np.cumsum(mask)))
    return kept[rp]


def plan_ref(A, rank: int, size: int) -> dict:
    """what DistSpmv.plan() of this rank must return (same keys; int64 / float32 arrays)"""
    rp, ci, val = as_csr(A)
    n = len(rp) - 1
    starts = row_starts(n, size)
    r0, r1 = int(starts[rank]), int(starts[rank + 1])
    brp, bci, bval = rows_of(A, r0, r1)
    mine = (bci >= r0) & (bci < r1)
    remote_cols = np.unique(bci[~mine])
    local = (_select(brp, mine), bci[mine] - r0, bval[mine])
    remote = (_select(brp, ~mine), np.searchsorted(remote_cols, bci[~mine]), bval[~mine])
    recv_count = np.bincount(owner_of(remote_cols, n, size), minlength=size)
    send_count, send_off, send_idx = [], [], []
    at = 0
    for q in range(size):
        need = np.zeros(0, dtype=np.int64)
        if q != rank:
            _, qci, _ = rows_of(A, int(starts[q]), int(starts[q + 1]))
            need = np.unique(qci[(qci >= r0) & (qci < r1)])
        send_off.append(at)
        send_count.append(len(need))
        send_idx.append(need - r0)
        at += len(need)
    return dict(r0=r0, r1=r1, local=local, remote=remote, remote_cols=remote_cols,
                recv_count=recv_count, recv_off=np.cumsum(recv_count) - recv_count,
                send_count=np.asarray(send_count, dtype=np.int64),
                send_off=np.asarray(send_off, dtype=np.int64),
                send_idx=np.concatenate(send_idx) if send_idx else np.zeros(0, dtype=np.int64))


def y_ref(A, gen: int, r0: int, r1: int) -> np.ndarray:
    """rows [r0, r1) of A x_gen in float64"""
    n = len(A[0]) - 1
    rp, ci, val = rows_of(A, r0, r1)
    return spmv_ref.csr_matvec_f64(rp, ci, val, x_gen(np.arange(n), gen))


def bound(A, gen: int, r0: int, r1: int) -> np.ndarray:
    """per row of [r0, r1), (L + 2) 2^-24 sum |a| |x|: spmv_ref.abs_bound of the whole rows"""
    n = len(A[0]) - 1
    rp, ci, val = rows_of(A, r0, r1)
    return spmv_ref.abs_bound(rp, ci, val, x_gen(np.arange(n), gen))


class Rows:
    """rows [r0, r1) of A held against device results: y_ref and bound per generation, computed
    once each and never changed"""

    def __init__(self, A, r0: int, r1: int):
        self.A, self.r0, self.r1 = as_csr(A), r0, r1
        self.lengths = np.diff(rows_of(self.A, r0, r1)[0])
        self._gens = {}

    def ref(self, gen: int):
        """(y_ref, bound) of the generation"""
        if gen not in self._gens:
            pair = y_ref(self.A, gen, self.r0, self.r1), bound(self.A, gen, self.r0, self.r1)
            for a in pair:
                a.setflags(write=False)
            self._gens[gen] = pair
        return self._gens[gen]

    def outside(self, y_dev, gen: int) -> np.ndarray:
        """mask over the rows: |y_dev - y_ref| <= bound does not hold (a NaN is outside)"""
        y = np.asarray(y_dev, dtype=np.float64)
        ref, b = self.ref(gen)
        assert y.shape == ref.shape, (y.shape, ref.shape)
        return ~(np.abs(y - ref) <= b)

    def ratio(self, y_dev, gen: int) -> float:
        """max over the rows of |y_dev - y_ref| / bound, with 0 / 0 = 0 (an empty row computed as
        0) and inf for a non-finite y: at most 1 exactly when no row is outside"""
        y = np.asarray(y_dev, dtype=np.float64)
        ref, b = self.ref(gen)
        assert y.shape == ref.shape, (y.shape, ref.shape)
        err = np.abs(y - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / b)
        r[~np.isfinite(y)] = np.inf
        return float(r.max(initial=0.0))


def default_band(m: int, size: int, bw: int = 0, nnz: int = 0, seed: int = 1):
    """the global matrix of a workload left at SpmvConfig's defaults (bw 0 = m / size, at least 1;
    nnz 0 = 10 m), from the project's generator: host code that tests/test_matrix_market.py pins"""
    from .. import _tz

    return as_csr(_tz.random_band_matrix(m, bw if bw > 0 else max(1, m // size),
                                         nnz if nnz > 0 else 10 * m, seed))
