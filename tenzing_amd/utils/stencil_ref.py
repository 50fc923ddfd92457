"""A plain numpy model of the 7-point stencil over a `StencilBox` (csrc/kernels/kernels.hpp).

`stencil_check` verifies stencil-mode runs against the field `halo_init` writes, which is affine
in the cell coordinates: with c0 + 6 c1 = 1 the stencil of that field is the field itself, for any
kernel that reads a symmetric pair of neighbours on each axis. Which neighbours a kernel reads
has to be checked on data without that symmetry; this module is the reference for it
(tests/test_gpu_stencil_kernels.py), and shares nothing with the native code:

- a box is a dict of the `StencilBox` fields (``base row ny nz nouter sy sz so xs``, optional
  ``m0 m1 c0 c1``) over one flat array; element (i, y, z, o) is at
  ``base + o*so + z*sz + y*sy + i``;
- `cells` lists the output cells (row positions in [m0, row - m1)), `needed` marks what the
  contract entitles a kernel to use, `apply` evaluates the stencil in float64 in the order the
  source writes it, `magnitude` gives the sum of absolute terms that error bounds scale with;
- `exact_field` draws data on which every evaluation order is exact (tests/test_stencil_ref.py
  proves it), so a kernel's output must equal `apply`'s bit for bit.
"""
from __future__ import annotations

import numpy as np

C0_DEFAULT, C1_DEFAULT = 0.4, 0.1  # StencilBox defaults
C0_EXACT, C1_EXACT = 0.5, 0.125    # with exact_field: three fractional bits, no rounding
EXACT_RANGE = 1 << 20


def padded_box(row: int, ny: int, nz: int, xs: int = 1, nouter: int = 1, m0: int = 0, m1: int = 0,
               shift: int = 0, **fields):
    """(box, n): a box inside padded volumes of its own in a flat array of n elements. Rows are
    pitched to an even stride with 4 elements before the box's first and at least 5 after its
    last, planes hold ny + 2 rows, a volume nz + 2 planes (XYZQ-like boxes, nouter > 1, stack
    one volume per outer index), and one whole plane of margin lies before and after, so nothing
    a kernel could plausibly touch is outside the array. Every stride and `base` are even;
    `shift` = 1 moves the box one element on (odd base: no 16-B alignment of its rows)"""
    sy = (row + 11) // 2 * 2
    sz = sy * (ny + 2)
    so = sz * (nz + 2) if nouter > 1 else 0
    box = dict(base=2 * sz + sy + 4 + shift, row=row, ny=ny, nz=nz, nouter=nouter, sy=sy, sz=sz, so=so,
               xs=xs, m0=m0, m1=m1, **fields)
    return box, sz * (2 + nouter * (nz + 2))


def cells(box: dict) -> np.ndarray:
    """flat indices (int64, in box order o, z, y, i) of the box's output cells"""
    lo, hi = int(box.get("m0", 0)), int(box["row"]) - int(box.get("m1", 0))
    n = [max(int(box[k]), 0) for k in ("nouter", "nz", "ny")]
    i = np.arange(lo, max(hi, lo), dtype=np.int64)
    o, z, y = (np.arange(k, dtype=np.int64) for k in n)
    e = (int(box["base"]) + o[:, None, None, None] * int(box["so"]) + z[None, :, None, None] * int(box["sz"])
         + y[None, None, :, None] * int(box["sy"]) + i[None, None, None, :])
    return e.reshape(-1)


def _offsets(box: dict):
    xs, sy, sz = int(box["xs"]), int(box["sy"]), int(box["sz"])
    return (-xs, xs, -sy, sy, -sz, sz)


def needed(box: dict, n: int) -> np.ndarray:
    """bool mask over a flat array of n elements: the output cells and their six neighbours.
    Everything else (edge and corner aprons, the x apron on a side masked by at least xs, what
    lies beyond) is none of the kernel's business"""
    m = np.zeros(n, dtype=bool)
    e = cells(box)
    if e.size == 0:
        return m
    for d in (0,) + _offsets(box):
        idx = e + d
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError("the box's apron leaves the array")
        m[idx] = True
    return m


def _coeffs(box: dict):
    return float(box.get("c0", C0_DEFAULT)), float(box.get("c1", C1_DEFAULT))


def _cell_mask(e: np.ndarray, n: int) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    m[e] = True
    if int(m.sum()) != e.size:
        raise ValueError("the box's output cells overlap")
    return m


def apply(box: dict, flat_in: np.ndarray):
    """(mask, values): the bool mask of the output cells over flat_in, and the stencil of each in
    float64, ``c0*cur + c1*(xm + xp + ym + yp + zm + zp)`` as the kernels' source writes it, in
    ascending flat order (``out[mask]`` is what to compare them with)"""
    flat_in = np.asarray(flat_in, dtype=np.float64)
    e = np.sort(cells(box))
    mask = _cell_mask(e, flat_in.size)
    c0, c1 = _coeffs(box)
    xm, xp, ym, yp, zm, zp = (flat_in[e + d] for d in _offsets(box))
    return mask, c0 * flat_in[e] + c1 * (xm + xp + ym + yp + zm + zp)


def magnitude(box: dict, flat_in: np.ndarray) -> np.ndarray:
    """A = |c0||cur| + |c1| sum |neighbour| per output cell (ascending flat order): two honest
    float64 evaluations of the stencil differ by at most 2^-49 A (derivation at stencil_check_k
    in csrc/kernels/check_kernels.hip: at most 7 roundings on each side)"""
    flat_in = np.abs(np.asarray(flat_in, dtype=np.float64))
    e = np.sort(cells(box))
    c0, c1 = _coeffs(box)
    return abs(c0) * flat_in[e] + abs(c1) * sum(flat_in[e + d] for d in _offsets(box))


def exact_field(rng: np.random.Generator, size) -> np.ndarray:
    """integers drawn uniformly from [-2^20, 2^20] as float64. With c0 = 0.5 and c1 = 0.125 every
    partial sum is an integer below 2^23 and every product a multiple of 1/8 below 2^21, so any
    evaluation order, with or without FMA contraction, is exact"""
    return rng.integers(-EXACT_RANGE, EXACT_RANGE + 1, size=size).astype(np.float64)


def poisoned_input(boxes, n: int, rng: np.random.Generator, normal: bool = False) -> np.ndarray:
    """a flat input of n elements for a list of boxes: data (exact_field, or standard normal)
    where any box needs it, NaN everywhere else, so that an output cell computed from anything
    the contract does not grant comes out NaN"""
    m = np.zeros(n, dtype=bool)
    for b in boxes:
        m |= needed(b, n)
    a = np.full(n, np.nan)
    k = int(m.sum())
    a[m] = rng.standard_normal(k) if normal else exact_field(rng, k)
    return a
