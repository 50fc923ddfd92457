"""What the tests of the refined CG solve share (test_cg_refine_graph.py, test_gpu_cg_refine.py and
test_gpu_cg_refine_kernels.py): a numpy model of mixed-precision iterative refinement around the
f32 single-reduction recurrence, the cap on its outer steps, and the f64 error bounds.

The inner solves are ``HostSrCg`` / ``HostPcg`` in their f32 form (f32 vectors, f64 dot products,
coefficients rounded to f32), imported from the tests of those forms. The outer loop keeps x64 in
f64, forms r64 = b - A x64 in f64 and restarts the inner model on f32(r64).
"""
import math

import numpy as np

from test_gpu_cg_sr import HostSrCg
from test_gpu_pcg import HostPcg

SHAPES = [(50, 8), (1037, 0), (20_011, 0)]
SYSTEMS = [("none", 0), ("jacobi", 2)]  # (precond, diag_scale)
TOLS = [1e-3, 1e-5]
REFINE_TOLS = [1e-9, 1e-12]
U64 = 2.0 ** -53


def cap(tol, refine_tol):
    """refine_step() calls a refined solve may take: every step cuts the true residual by about
    the inner tol, so ceil(log(refine_tol) / log(tol)) of them and one more. The quotient is
    rounded to 9 digits first: log(1e-9) / log(1e-3) is 3, not 3.0000000000000004."""
    return math.ceil(round(math.log(refine_tol) / math.log(tol), 9)) + 1


def row_counts(rp):
    return np.diff(np.asarray(rp, dtype=np.int64))


def abs_row_sums(rp, ci, val, b, x64):
    """|b_i| + sum_j |a_ij| |x64_j|, in f64"""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    prod = np.abs(np.asarray(val, dtype=np.float64)) * np.abs(np.asarray(x64, dtype=np.float64))[ci]
    return np.abs(np.asarray(b, dtype=np.float64)) + np.add.reduceat(prod, rp[:-1])


def residual64(rp, ci, val, b, x64):
    """b - A x64 in numpy f64 (row sums by np.add.reduceat)"""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    prod = np.asarray(val, dtype=np.float64) * np.asarray(x64, dtype=np.float64)[ci]
    return np.asarray(b, dtype=np.float64) - np.add.reduceat(prod, rp[:-1])


def residual_bound(rp, ci, val, b, x64):
    """per row: (K_i + 2) 2^-53 (|b_i| + sum_j |a_ij| |x64_j|), the standard bound of an f64 dot
    product of K_i terms in any order followed by one subtraction; not a measured constant (the
    device's worst error on the tests' systems is below half of it)"""
    return (row_counts(rp) + 2) * U64 * abs_row_sums(rp, ci, val, b, x64)


def check_floor(rp, ci, val, b, x64):
    """what evaluating ||b - A x64|| / ||b|| in f64 can itself be off by: the norm of the row
    bounds with K the largest row count"""
    k = int(row_counts(rp).max())
    nb = float(np.linalg.norm(np.asarray(b, dtype=np.float64)))
    return (k + 2) * U64 * float(np.linalg.norm(abs_row_sums(rp, ci, val, b, x64))) / nb


class HostRefine:
    """x64 = 0; inner f32 solve of A d = rhat from d = 0 until its recurrence has r.r <= tol^2
    rhat.rhat (tested before every iteration, as the device's update tests the slab of the r it is
    about to change); x64 += d in f64; r64 = b - A x64 in f64; refined once r64.r64 <= refine_tol^2
    b.b, else rhat = f32(r64) and again."""

    def __init__(self, rp, ci, val, b, dinv, tol, refine_tol):
        self.sys = (rp, ci, val)
        self.b = np.asarray(b, dtype=np.float32)
        self.dinv, self.tol, self.refine_tol = dinv, tol, refine_tol
        self.x64 = np.zeros(len(self.b), dtype=np.float64)
        b64 = self.b.astype(np.float64)
        self.bb = float(np.dot(b64, b64))
        self.steps = self.inner_iters = 0
        self.refined = False
        self.history = [1.0]  # ||r64|| / ||b|| after every step

    def _inner(self, rhs):
        if self.dinv is None:
            return HostSrCg(*self.sys, rhs, True)
        return HostPcg(*self.sys, rhs, self.dinv, True)

    def solve(self, max_steps, max_inner=400):
        rhs = self.b
        while self.steps < max_steps and not self.refined:
            h = self._inner(rhs)
            thresh = self.tol * self.tol * h.rr
            while h.rr > thresh and self.inner_iters < max_inner:
                h.step()
                self.inner_iters += 1
            self.x64 = self.x64 + h.x.astype(np.float64)
            r64 = residual64(*self.sys, self.b, self.x64)
            rr64 = float(np.dot(r64, r64))
            self.steps += 1
            self.history.append(math.sqrt(rr64 / self.bb) if self.bb > 0 else math.sqrt(rr64))
            self.refined = rr64 <= self.refine_tol * self.refine_tol * self.bb
            rhs = r64.astype(np.float32)
        return self
