"""Conjugate gradient on one rank: one schedule run is one CG iteration on A x = b.

Not in the reference (its SpMV workload is the single product y = A x). A is a symmetric,
strictly diagonally dominant band matrix (``spd_band_matrix``: m = 150,000 rows, 5 m random
off-diagonal draws mirrored across the diagonal) or a symmetric Matrix Market file; b is a fixed
pseudo-random vector. The search chooses between the plain form (8 launches) and the fused form
(4 launches) and places the x update beside the r -> r.r -> beta -> p chain. ``form="sr"`` is
the single-reduction (Chronopoulos-Gear) recurrence in 2 launches: an SpMV of r that also forms
r.r and r.(A r), then one update of p, s, x and r; ``form="all"`` offers all three to the search.
With ``nrhs`` = 2, 4 or 8 the single-reduction form solves that many right-hand sides in the same
two launches: one matrix stream and one gather per entry serve every column. With ``tol`` > 0
that form stops each column on the device at r.r <= tol^2 b.b and freezes it; ``solve`` drives a
prepared runtime until every column has stopped. ``precond="jacobi"`` runs that form preconditioned
by diag(A), still in two launches; ``diag_scale`` poses the same problem in badly chosen units.
``refine_tol`` > 0 wraps that f32 solve in f64 iterative refinement: the solution is kept in f64
(``x64``), ``refine_step`` forms b - A x64 in f64 on the device and restarts the f32 recurrence on
it, and ``solve`` repeats that until the f64 residual is below ``refine_tol`` ||b||. The step is
not part of the searched schedule, batched refinement and an f64 matrix are not built.
"""
from __future__ import annotations

import dataclasses

from .. import _tz


@dataclasses.dataclass
class CgConfig:
    m: int = 150_000
    bw: int = 0         # 0 = m
    nnz: int = 0        # 0 = 5 m (before mirroring)
    seed: int = 1
    matrix: str = ""    # symmetric Matrix Market file instead of the band matrix
    # plain (one kernel per step) | fused (4 launches) | choice (plain | fused) |
    # sr (single reduction, 2 launches) | all (plain | fused | sr)
    form: str = "choice"
    lanes: int = _tz.kernels.SPMV_ILP + 4  # csr_spmv variant of the plain form's SpMV
    rhs: str = "random"  # random: b in [-1, 1) from seed | zero: b = 0 (the degenerate system)
    # right-hand sides solved side by side on interleaved vectors (1, 2, 4 or 8; more than one needs
    # form="sr"): numbers rhs_first .. rhs_first + nrhs - 1 of the sequence derived from seed, of
    # which number 0 is the b of a single solve. Column j has the bits of a single solve of
    # right-hand side rhs_first + j; read it with x(j), r(j), p(j), b(j), rr(j), residual(j).
    nrhs: int = 1
    rhs_first: int = 0
    # > 0 (form="sr" only): column j stops at r_j.r_j <= tol^2 b_j.b_j, decided on the device, and
    # stays frozen however many more iterations are launched; iterations(j), converged(j) and
    # threshold(j) report, set_armed(False) switches the test off for timing loops. 0: no test
    tol: float = 0.0
    # none | jacobi: M = diag(A), the preconditioned single-reduction recurrence in the same two
    # launches (form="sr" and nrhs=1 only). The stopping test stays r.r <= tol^2 b.b; u() and dinv()
    # read the stored u = f32(dinv * r) and dinv = 1 / a_ii
    precond: str = "none"
    # d in 0..8: the same problem in badly chosen units, (S A S) y = S b with S = diag(2^e_i), e_i
    # uniform in [-d, d] from seed; exact in f32. scale() returns S's diagonal. 0: as generated / read
    diag_scale: int = 0
    # > 0 (form="sr", nrhs=1, tol > 0, refine_tol < tol): f64 iterative refinement around the f32
    # solve. tol becomes the inner solve's relative tolerance (it stops at r.r <= tol^2 rhat.rhat,
    # rhat the f32 right-hand side it was restarted with); refine_step() adds x to x64, forms
    # r64 = b - A x64 in f64 and restarts, until r64.r64 <= refine_tol^2 b.b. x64(), r64(),
    # outer_steps(), refined(), inner_threshold() and residual64() report. 0: off
    refine_tol: float = 0.0
    prefix: str = "cg_"

    def args(self, rank: int = 0, size: int = 1, device: int = -1) -> "_tz.CgArgs":
        a = _tz.CgArgs()
        a.m, a.bw, a.nnz, a.seed = self.m, self.bw, self.nnz, self.seed
        a.matrix, a.form, a.lanes, a.rhs, a.prefix = self.matrix, self.form, self.lanes, self.rhs, self.prefix
        a.nrhs, a.rhs_first, a.tol = self.nrhs, self.rhs_first, self.tol
        a.precond, a.diag_scale, a.refine_tol = self.precond, self.diag_scale, self.refine_tol
        a.rank, a.size, a.device = rank, size, device
        return a


def build_cg(cfg: CgConfig, ctrl=None, device: int = -1, setup: bool = True, graph=None):
    """(ConjugateGradient, Graph). One rank only: a control plane of several ranks raises."""
    rank = ctrl.rank if ctrl is not None else 0
    size = ctrl.size if ctrl is not None else 1
    c = _tz.ConjugateGradient(cfg.args(rank, size, device))
    if setup:
        c.setup()
    g = graph if graph is not None else _tz.Graph()
    c.add_to_graph(g)
    return c, g


@dataclasses.dataclass
class CgSolve:
    iterations: list   # per column: iterations taken before it stopped (or until max_iters)
    converged: list    # per column: r.r <= tol^2 b.b was reached
    launched: int      # iterations launched: at most max(iterations) + check_every, and max_iters
    residual: list     # per column: the true residual ||b - A x|| / ||b|| of the x it ended with
    #                    (formed on the host; empty with solve(..., residual=False))
    # refine_tol > 0 only (the defaults otherwise):
    outer_steps: int = 0        # restarts of the inner solve (refine_step calls that did not end it)
    refined: bool = False       # a step found r64.r64 <= refine_tol^2 b.b
    residual64: float = None    # ||b - A x64|| / ||b|| in f64 (None with residual=False)


def solve(cg, rt, max_iters: int, check_every: int = 8, residual: bool = True, max_outer: int = 20) -> CgSolve:
    """Iterate a ``tol`` > 0 workload from its current state until every column has converged or
    ``max_iters`` iterations were launched. ``rt`` must have a schedule of this workload's graph
    prepared. The host looks at the device's flags only every ``check_every`` iterations; the
    iterations launched past a column's stop leave it untouched, so x, r, p and ``iterations`` do
    not depend on ``check_every``.

    With ``refine_tol`` > 0, a look that finds the inner solve converged takes a ``refine_step()``;
    the solve ends once that finds it refined, after ``max_iters`` inner iterations launched, or
    once the inner solve has been restarted ``max_outer`` times. ``iterations`` then counts inner
    iterations over the whole solve, ``converged`` and ``residual`` describe the last inner solve
    (its x is a correction, 0 after a step), and x64 and the step counts do not depend on
    ``check_every`` either."""
    if cg.args.tol <= 0:
        raise ValueError("solve needs a workload built with tol > 0")
    if max_iters < 0 or check_every < 1:
        raise ValueError("solve: max_iters >= 0 and check_every >= 1")
    refine = cg.args.refine_tol > 0
    if refine and max_outer < 1:
        raise ValueError("solve: max_outer >= 1")
    cols = range(cg.args.nrhs)
    launched = 0
    while launched < max_iters:
        n = min(check_every, max_iters - launched)
        rt.run(n)
        launched += n
        rt.device_sync()
        if all(cg.converged(j) for j in cols):
            if not refine:
                break
            cg.refine_step()
            if cg.refined() or cg.outer_steps() >= max_outer:
                break
    sol = CgSolve([cg.iterations(j) for j in cols], [cg.converged(j) for j in cols], launched,
                  [cg.residual(j) for j in cols] if residual else [])
    if refine:
        sol.outer_steps, sol.refined = cg.outer_steps(), cg.refined()
        sol.residual64 = cg.residual64() if residual else None
    return sol
