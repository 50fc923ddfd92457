"""The 7-point stencil kernels (csrc/kernels/stencil_kernels.hip) on random data against the numpy
reference (tenzing_amd/utils/stencil_ref.py): masks, tile edges, both element widths, every
tuning, thin boxes and their batches, and the regions the halo workload launches.

`stencil_check` cannot see which neighbours a kernel reads: its field is affine, and any symmetric
pair of neighbours reproduces it (tests/test_stencil_ref.py). Here the input holds integers on
which every evaluation order is exact, so the output must EQUAL the reference, and NaN wherever
the contract in kernels.hpp grants the kernel nothing, so an output computed from such a cell is
NaN. The output is prefilled with a NaN of a fixed payload and compared as bits: every element
that is no output cell, masked cells included, must still hold it."""
import contextlib
import math

import numpy as np
import pytest

from tenzing_amd.utils import stencil_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x7FF8_0000_0BAD_C0DE  # a quiet NaN no arithmetic produces
EXACT = dict(c0=sr.C0_EXACT, c1=sr.C1_EXACT)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Case:
    """one flat `in` (poisoned outside what the boxes need) and one flat `out` for a list of boxes
    with disjoint output cells; the reference is computed once, on construction"""

    def __init__(self, boxes, n, seed, normal=False):
        rng = np.random.default_rng(seed)
        self.n = n
        host = sr.poisoned_input(boxes, n, rng, normal)
        mask, want = np.zeros(n, dtype=bool), np.zeros(n)
        self.bound = np.zeros(n)
        for b in boxes:
            m, v = sr.apply(b, host)
            assert not (mask & m).any(), "the boxes' output cells overlap"
            mask |= m
            want[m] = v
            self.bound[m] = 2.0 ** -49 * sr.magnitude(b, host)
        assert np.isfinite(want[mask]).all()
        self.mask = mask
        self.want_host = want[mask]
        self.bound = self.bound[mask]
        self.inp = _cuda(host)
        self.cells = _cuda(np.flatnonzero(mask))
        self.rest = _cuda(np.flatnonzero(~mask))
        self.want = _cuda(self.want_host)
        self.out = torch.empty(n, dtype=torch.float64, device="cuda")
        assert self.inp.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0
        self.reset()

    def reset(self):
        self.out.view(torch.int64).fill_(SENTINEL)

    def untouched(self):
        return bool((self.out.view(torch.int64) == SENTINEL).all())

    def check(self, what, exact=True):
        """output cells equal the reference (exact) or lie within 2^-49 A of it; all else is
        sentinel. Resets `out` for the next launch"""
        torch.cuda.synchronize()
        got = self.out[self.cells]
        stray = self.out.view(torch.int64)[self.rest] != SENTINEL
        if exact:
            ok = torch.equal(got, self.want)  # a NaN equals nothing
        else:
            err = np.abs(got.cpu().numpy() - self.want_host)
            ok = bool((err <= self.bound).all())  # a NaN fails
        strays = self.rest[stray].cpu().numpy()
        self.reset()
        if ok and strays.size == 0:
            return
        g = got.cpu().numpy()
        bad = np.flatnonzero(~(g == self.want_host) if exact else ~(err <= self.bound))
        first = bad[:6]
        pytest.fail(f"{what}: {bad.size} of {g.size} output cells wrong, {int(np.isnan(g[bad]).sum())} of them "
                    f"NaN (a poisoned cell was used, or the cell was never written); first at flat "
                    f"{self.cells.cpu().numpy()[first].tolist()}: got {g[first].tolist()}, want "
                    f"{self.want_host[first].tolist()}. {strays.size} elements that are no output cell were "
                    f"written, first at flat {strays[:6].tolist()}")


def _run7(k, case, b, lds):
    k.stencil7(case.inp.data_ptr(), case.out.data_ptr(), b["base"], b["row"], b["ny"], b["nz"], b["nouter"],
               b["sy"], b["sz"], b["so"], b["xs"], b.get("c0", sr.C0_DEFAULT), b.get("c1", sr.C1_DEFAULT),
               lds, _stream(), m0=b["m0"], m1=b["m1"])


def _vx(b):
    """elements per thread, by the rule documented at stencil7: two when row, base and every
    stride are even and both pointers 16-B aligned (Case asserts the pointers)"""
    return 2 if all(b[f] % 2 == 0 for f in ("row", "base", "sy", "sz", "so")) else 1


def _tiles(b, ty, zc):
    return (math.ceil(b["row"] / (64 * _vx(b))) * math.ceil(b["ny"] / ty) * math.ceil(b["nz"] / zc)
            * b["nouter"])


@contextlib.contextmanager
def _tuning(k, ty=16, zc=64, pf=1, db=True, xcd=True):
    prev = k.get_stencil_xcd_tiles()
    k.set_stencil_tuning(ty, zc, pf, db)
    k.set_stencil_xcd_tiles(xcd)
    try:
        yield
    finally:
        k.set_stencil_tuning()
        k.set_stencil_xcd_tiles(prev)


# ----------------------------------------------------------------------------- A: z-march kernels
MASKS = {"none": lambda xs: (0, 0), "xs": lambda xs: (xs, xs), "lo1": lambda xs: (1, 0),
         "hi1": lambda xs: (0, 1), "xs+1,2": lambda xs: (xs + 1, 2)}
# (layout, xs, row, ny, nz, mask): 'q' QXYZ-like (nouter 1, row = xs * nx), 'x' XYZQ-like (xs 1,
# nouter 3). Rows sit one element either side of a 64- and a 128-wide tile, ny one either side of
# TY = 8 and 16, nz one either side of ZC = 16 and 64 (the two tunings of TUNINGS_AB). Even rows
# run with two elements per thread at `base` and with one at `base + 1`; odd rows only with one
BOXES = [
    ("q", 2, 32, 4, 4, "none"),      # the smallest box that is not thin
    ("q", 4, 64, 7, 15, "xs"),       # rlo 4, rhi 60
    ("x", 1, 128, 8, 16, "lo1"),     # rlo 1: the first pair straddles
    ("q", 2, 130, 17, 65, "hi1"),    # rhi 129: the last pair straddles; 2 x 2 x 2 tiles
    ("x", 1, 64, 15, 63, "xs+1,2"),  # rlo 2, rhi 62
    ("q", 3, 132, 16, 64, "xs"),     # rlo 3, rhi 129: both ends straddle (no even row above is 3 * nx)
    ("x", 1, 32, 9, 17, "none"),
    ("q", 4, 128, 16, 64, "xs+1,2"),  # rlo 5, rhi 126
    ("q", 3, 63, 8, 16, "xs"),
    ("q", 1, 65, 17, 65, "lo1"),     # 2 x 2 x 2 tiles of 64
    ("q", 3, 129, 9, 17, "hi1"),
    ("x", 1, 129, 4, 4, "xs+1,2"),
]
BOX_IDS = ["%s-xs%d-row%d-ny%d-nz%d-%s" % b for b in BOXES]
TUNINGS_AB = [dict(), dict(ty=8, zc=16, pf=2, db=False)]  # the default (16, 64, 1, True) and one more


def _make(spec, shift, **fields):
    layout, xs, row, ny, nz, mask = spec
    m0, m1 = MASKS[mask](xs)
    assert layout == "x" or row % xs == 0
    return sr.padded_box(row, ny, nz, xs, 1 if layout == "q" else 3, m0, m1, shift, **fields)


def test_box_list_covers_every_edge_for_both_widths():
    """every listed row, ny, nz, xs and mask occurs with one and with two elements per thread (odd
    rows cannot take two), both mask ends occur odd and even with two, both layouts occur, and
    the XCD-ordered launch runs with and without padding workgroups"""
    seen = {1: [], 2: []}
    for spec in BOXES:
        for shift in (0, 1):
            b, _ = _make(spec, shift)
            assert _vx(b) == (2 if spec[2] % 2 == 0 and shift == 0 else 1)
            seen[_vx(b)].append((spec, b))
    for vx, rows in ((1, {32, 63, 64, 65, 128, 129, 130}), (2, {32, 64, 128, 130})):
        specs = [s for s, _ in seen[vx]]
        assert rows <= {s[2] for s in specs}
        assert {s[3] for s in specs} >= {4, 7, 8, 9, 15, 16, 17}   # 4, TY - 1, TY, TY + 1
        assert {s[4] for s in specs} >= {4, 15, 16, 17, 63, 64, 65}  # 4, ZC - 1, ZC, ZC + 1
        assert {s[1] for s in specs} == {1, 2, 3, 4}
        assert {s[5] for s in specs} == set(MASKS)
        assert {s[0] for s in specs} == {"q", "x"}
        for t in TUNINGS_AB:
            pad = {_tiles(b, t.get("ty", 16), t.get("zc", 64)) % 8 == 0 for _, b in seen[vx]}
            assert pad == {True, False}
    ends = [(b["m0"] % 2, (b["row"] - b["m1"]) % 2) for _, b in seen[2]]
    assert {e[0] for e in ends} == {0, 1} and {e[1] for e in ends} == {0, 1}
    for spec in BOXES:
        assert not (spec[2] < 32 or spec[3] < 4 or spec[4] < 4)


@pytest.mark.parametrize("spec", BOXES, ids=BOX_IDS)
def test_stencil7_boxes_exact(tz, gpu, spec):
    """each box at an even base (two elements per thread when the row is even) and one element
    on (one per thread), LDS-tiled and straight from global memory, at two tunings"""
    k = tz._tz.kernels
    for shift in (0, 1):
        b, n = _make(spec, shift, **EXACT)
        assert not k.stencil_thin(b["row"], b["ny"], b["nz"])
        case = Case([b], n, seed=10 + shift)
        for t in TUNINGS_AB:
            with _tuning(k, **t):
                for lds in (True, False):
                    _run7(k, case, b, lds)
                    case.check(f"vx{_vx(b)} lds={lds} tuning={t or 'default'}")


ALL_TUNINGS = [(ty, zc, pf, db, xcd) for ty in (8, 16)
               for zc, pf in ((16, 1), (16, 2), (32, 1), (32, 2), (64, 1), (64, 2), (128, 1))
               for db in (True, False) for xcd in (True, False)]


@pytest.mark.parametrize("spec,shift,vx", [(("x", 1, 65, 17, 130, "none"), 0, 1),
                                           (("q", 3, 132, 17, 130, "xs"), 0, 2)], ids=["vx1", "vx2-masked"])
def test_stencil7_every_tuning(tz, gpu, spec, shift, vx):
    """all 56 launch shapes (rows per tile, planes per chunk and in flight, double buffering,
    tile order) on 130 planes (two chunks even at zc = 128): one unmasked box with one element per
    thread, and the workload's interior form (m0 = m1 = xs = 3) with two"""
    assert len(ALL_TUNINGS) == 56
    k = tz._tz.kernels
    b, n = _make(spec, shift, **EXACT)
    assert _vx(b) == vx
    case = Case([b], n, seed=20)
    for ty, zc, pf, db, xcd in ALL_TUNINGS:
        with _tuning(k, ty, zc, pf, db, xcd):
            for lds in (True, False):
                _run7(k, case, b, lds)
                case.check(f"lds={lds} ty={ty} zc={zc} pf={pf} db={db} xcd_tiles={xcd}")


@pytest.mark.parametrize("spec,shift", [(("q", 3, 132, 17, 65, "xs"), 0), (("x", 1, 130, 9, 17, "lo1"), 1),
                                        (("q", 3, 27, 5, 6, "hi1"), 0)], ids=["vx2", "vx1", "thin"])
def test_stencil7_default_coefficients_within_bound(tz, gpu, spec, shift):
    """c0 = 0.4, c1 = 0.1 on standard-normal data: |got - ref| <= 2^-49 A with A = |c0||cur| +
    |c1| sum |nb| (at most 7 roundings on each side, 16 u in all: the derivation at
    stencil_check_k)"""
    k = tz._tz.kernels
    b, n = _make(spec, shift)
    case = Case([b], n, seed=30, normal=True)
    for lds in (True, False):
        _run7(k, case, b, lds)
        torch.cuda.synchronize()
        err = np.abs(case.out[case.cells].cpu().numpy() - case.want_host)
        print(f"vx{_vx(b)} lds={lds}: max |got - ref| / A = {float((err / case.bound).max()) * 2.0 ** -49:.3e}"
              f" (bound {2.0 ** -49:.3e})")
        case.check(f"lds={lds}", exact=False)


def test_stencil7_argument_errors(tz, gpu):
    """xs outside 1..4 and null pointers raise before anything is launched; an empty extent is a
    no-op (even with a bad xs or null pointers, as the workload's degenerate regions rely on)"""
    k = tz._tz.kernels
    b, n = _make(("q", 2, 32, 4, 4, "none"), 0, **EXACT)
    case = Case([b], n, seed=40)
    for xs in (0, 5, -1):
        with pytest.raises(RuntimeError, match="x neighbour distance"):
            _run7(k, case, dict(b, xs=xs), True)
    args = [b[f] for f in ("base", "row", "ny", "nz", "nouter", "sy", "sz", "so", "xs")]
    for inp, out in ((0, case.out.data_ptr()), (case.inp.data_ptr(), 0)):
        with pytest.raises(RuntimeError, match="null grid"):
            k.stencil7(inp, out, *args)
        thin = [b["base"], 8, 2, 2, 1, b["sy"], b["sz"], 0, 2]
        with pytest.raises(RuntimeError, match="null grid"):
            k.stencil7(inp, out, *thin)
    for f in ("row", "ny", "nz", "nouter"):
        for lds in (True, False):
            _run7(k, case, dict(b, **{f: 0}), lds)
    k.stencil7(0, 0, *[0 if i == 1 else a for i, a in enumerate(args)])
    k.stencil7_thin_many(0, 0, [dict(b, nz=0)], _stream())
    with pytest.raises(RuntimeError, match="null grid"):
        k.stencil7_thin_many(0, case.out.data_ptr(), [b], _stream())
    torch.cuda.synchronize()
    assert case.untouched()
    # the keyword-only newcomers default to no mask, and positional calls still work
    k.stencil7(case.inp.data_ptr(), case.out.data_ptr(), *args, sr.C0_EXACT, sr.C1_EXACT, True, _stream())
    case.check("positional call")


# ----------------------------------------------------------------------------------- B: thin boxes
def test_stencil_thin_boundaries(tz):
    k = tz._tz.kernels
    assert not k.stencil_thin(32, 4, 4)
    assert k.stencil_thin(31, 4, 4) and k.stencil_thin(32, 3, 4) and k.stencil_thin(32, 4, 3)
    assert k.stencil_thin(1, 500, 500) and not k.stencil_thin(5000, 500, 500)


@pytest.mark.parametrize("spec", [("q", 1, 31, 5, 6, "lo1"), ("q", 3, 66, 3, 6, "xs"), ("x", 1, 40, 5, 3, "xs+1,2"),
                                  ("q", 4, 4, 1, 1, "none"), ("x", 1, 1, 9, 7, "none"), ("q", 2, 300, 1, 70, "hi1")],
                         ids=lambda s: "%s-xs%d-row%d-ny%d-nz%d-%s" % s)
def test_stencil7_thin_box_exact(tz, gpu, spec):
    """a box thin along any one axis takes the one-thread-per-element kernel under either `lds`;
    the last one has more items than one pass of its blocks' threads covers four at a time"""
    k = tz._tz.kernels
    for shift in (0, 1):
        b, n = _make(spec, shift, **EXACT)
        assert k.stencil_thin(b["row"], b["ny"], b["nz"])
        case = Case([b], n, seed=50 + shift)
        for lds in (True, False):
            _run7(k, case, b, lds)
            case.check(f"shift={shift} lds={lds}")
        k.stencil7_thin_many(case.inp.data_ptr(), case.out.data_ptr(), [b], _stream())
        case.check(f"shift={shift} thin_many")


def _shell(layout, copies=3, X=20, Y=7, Z=6, nq=3):
    """the six one-cell slabs around an X x Y x Z interior (HaloExchange::stencil's region 1), in
    `copies` separate padded volumes of one flat array; the second and third copies mask some"""
    xs = nq if layout == "q" else 1
    sy = (xs * X + 11) // 2 * 2
    sz = sy * (Y + 2)
    so = sz * (Z + 2) if layout == "x" else 0
    vol = sz * (Z + 2) * (nq if layout == "x" else 1)
    slabs = [(0, X, 0, Y, 0, 1), (0, X, 0, Y, Z - 1, Z), (0, X, 0, 1, 1, Z - 1), (0, X, Y - 1, Y, 1, Z - 1),
             (0, 1, 1, Y - 1, 1, Z - 1), (X - 1, X, 1, Y - 1, 1, Z - 1)]
    masks = [["none"] * 6, ["xs", "lo1", "hi1", "xs+1,2", "none", "lo1" if xs > 1 else "none"],
             ["hi1", "xs", "xs+1,2", "none", "hi1" if xs > 1 else "none", "none"]]
    boxes = []
    for c in range(copies):
        org = sz + c * vol + sz + sy + 4
        for (x0, x1, y0, y1, z0, z1), m in zip(slabs, masks[c]):
            m0, m1 = MASKS[m](xs)
            boxes.append(dict(base=org + z0 * sz + y0 * sy + x0 * xs, row=(x1 - x0) * xs, ny=y1 - y0, nz=z1 - z0,
                              nouter=1 if layout == "q" else nq, sy=sy, sz=sz, so=so, xs=xs, m0=m0, m1=m1, **EXACT))
    return boxes, 2 * sz + copies * vol


@pytest.mark.parametrize("layout", ["q", "x"])
def test_stencil7_thin_many_batches(tz, gpu, layout):
    """batches of 1, 6, 8, 9, 17 and 18 boxes: within one launch's kMaxFlat = 8, and split over
    two and three launches; empty boxes (row = 0, nz = 0) at index 0 and 8 shift the split. Every
    box writes a region of its own, so a box dropped at a batch boundary leaves sentinels and a
    box launched over another's cells breaks them. (A box launched twice writes the same values
    twice: the batching loop's `k` carrying over from the inner loop is verified by reading it.
    The 8192-block cap needs 8.4 M items in one box, ten times the largest shell slab of a
    512^3 x 3 grid: not reached here.)"""
    k = tz._tz.kernels
    pool, n = _shell(layout)
    assert len(pool) == 18 and all(k.stencil_thin(b["row"], b["ny"], b["nz"]) for b in pool)
    e0, e8 = dict(pool[0], row=0), dict(pool[3], nz=0)
    batches = [pool[:1], pool[:6], pool[:8], [e0] + pool[:7] + [e8], [e0] + pool[:7] + [e8] + pool[7:15], pool,
               [e0, e8], []]
    assert [len(b) for b in batches] == [1, 6, 8, 9, 17, 18, 2, 0]
    for boxes in batches:
        case = Case(boxes, n, seed=60 + len(boxes))
        assert int(case.mask.sum()) == sum(sr.cells(b).size for b in boxes)
        k.stencil7_thin_many(case.inp.data_ptr(), case.out.data_ptr(), boxes, _stream())
        case.check(f"batch of {len(boxes)}")


# --------------------------------------------------------------------- C: the workload's regions
GEOMETRIES = [(70, 20, 9, 3, 1), (70, 20, 9, 3, 3), (5, 4, 3, 2, 1),   # (nx, ny, nz, nq, ghost)
              (6, 5, 1, 2, 1), (6, 5, 2, 2, 1), (6, 1, 4, 2, 1), (6, 2, 4, 2, 1), (1, 5, 4, 2, 1),
              (2, 5, 4, 2, 1), (3, 3, 3, 3, 1)]


class Regions:
    """a one-rank HaloExchange in stencil mode with its grid and output driven from the host"""

    def __init__(self, tz, order, geo):
        from tenzing_amd.models import HaloConfig

        self.k = tz._tz.kernels
        self.X, self.Y, self.Z, self.nq, self.g = geo
        a = HaloConfig(order=order, stencil=True).args(0, 1, 0)
        a.nx, a.ny, a.nz, a.nq, a.ghost = geo
        self.h = tz.HaloExchange(a)
        self.h.setup(tz.SelfCtrl())
        assert self.h.stencil_out_ptr() != 0 and self.h.stencil_out_ptr() != self.h.grid_ptr()
        lay = self.h.layout()
        self.n = self.h.grid_elems()
        st = lay["strides_qzyx"]
        ax = [np.arange(m, dtype=np.int64) * s for m, s in zip(lay["shape_qzyx"], st)]
        idx = (lay["x_offset_cells"] * st[3] + ax[0][:, None, None, None] + ax[1][None, :, None, None]
               + ax[2][None, None, :, None] + ax[3][None, None, None, :])
        assert int(idx.min()) >= 0 and int(idx.max()) < self.n and np.unique(idx).size == idx.size
        self.idx = idx  # flat storage index of logical (q, z, y, x), ghosts included
        g = self.g
        self.interior = idx[:, g:-g, g:-g, g:-g]
        rng = np.random.default_rng(70)
        self.data = sr.exact_field(rng, self.interior.shape)
        # the interior, and the interior with exactly what the whole stencil needs beside it: the
        # face ghosts next to it, filled periodically. Deeper ghosts, edges, corners and the row
        # padding are NaN in both
        L = np.full(lay["shape_qzyx"], np.nan)
        L[:, g:-g, g:-g, g:-g] = self.data
        self.bare = np.full(self.n, np.nan)
        self.bare[idx.reshape(-1)] = L.reshape(-1)
        L[:, g - 1, g:-g, g:-g], L[:, -g, g:-g, g:-g] = self.data[:, -1], self.data[:, 0]
        L[:, g:-g, g - 1, g:-g], L[:, g:-g, -g, g:-g] = self.data[:, :, -1], self.data[:, :, 0]
        L[:, g:-g, g:-g, g - 1], L[:, g:-g, g:-g, -g] = self.data[:, :, :, -1], self.data[:, :, :, 0]
        self.wrapped = np.full(self.n, np.nan)
        self.wrapped[idx.reshape(-1)] = L.reshape(-1)
        # the reference, from the logical grid alone (default coefficients: the workload's)
        c = L[:, g:-g, g:-g, g:-g]
        nb = [L[:, g - 1:-g - 1, g:-g, g:-g], L[:, g + 1:L.shape[1] - g + 1, g:-g, g:-g],
              L[:, g:-g, g - 1:-g - 1, g:-g], L[:, g:-g, g + 1:L.shape[2] - g + 1, g:-g],
              L[:, g:-g, g:-g, g - 1:-g - 1], L[:, g:-g, g:-g, g + 1:L.shape[3] - g + 1]]
        self.want = sr.C0_DEFAULT * c + sr.C1_DEFAULT * (nb[4] + nb[5] + nb[2] + nb[3] + nb[0] + nb[1])
        self.bound = 2.0 ** -49 * (sr.C0_DEFAULT * np.abs(c) + sr.C1_DEFAULT * sum(np.abs(v) for v in nb))
        assert np.isfinite(self.want).all()
        self.fill = torch.full((self.n,), SENTINEL, dtype=torch.int64, device="cuda")
        self.got = torch.empty(self.n, dtype=torch.float64, device="cuda")

    def run(self, grid, regions):
        """out (host, flat) after the regions ran on `grid` into a sentinel-filled output"""
        src = _cuda(grid)
        torch.cuda.synchronize()
        self.h.write_grid(src.data_ptr(), _stream())
        self.k.copy_bytes(self.h.stencil_out_ptr(), self.fill.data_ptr(), 8 * self.n, _stream())
        for r in regions:
            self.h.stencil(r, _stream())
        self.k.copy_bytes(self.got.data_ptr(), self.h.stencil_out_ptr(), 8 * self.n, _stream())
        torch.cuda.synchronize()
        return self.got.cpu().numpy()

    def written(self, out):
        return out.view(np.int64) != SENTINEL

    def check(self, out, cells, what):
        """`cells`: bool over the interior (q, z, y, x). Those are within the bound of the
        reference (and finite), everything else in the storage is sentinel"""
        got = out[self.interior]
        err = np.abs(got - self.want)
        bad = cells & ~(err <= self.bound)
        assert not bad.any(), (f"{what}: {int(bad.sum())} cells wrong ({int((np.isnan(got) & cells).sum())} NaN), "
                               f"first (q, z, y, x) {np.argwhere(bad)[:5].tolist()}")
        allowed = np.zeros(self.n, dtype=bool)
        allowed[self.interior[cells]] = True
        stray = self.written(out) & ~allowed
        assert not stray.any(), f"{what}: {int(stray.sum())} elements written outside, first {np.flatnonzero(stray)[:5]}"
        missing = allowed & ~self.written(out)
        assert not missing.any(), f"{what}: {int(missing.sum())} cells never written"


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "x".join(map(str, g[:3])) + f"-q{g[3]}-g{g[4]}")
@pytest.mark.parametrize("order", ["qxyz", "xyzq"])
def test_workload_regions_on_random_data(tz, gpu, order, geo):
    """HaloExchange.stencil on integer data (default coefficients, which are not dyadic: cells are
    held to 2^-49 A, against errors of order c1 = 0.1 and more from any wrong neighbour).

    - region 2 with only the adjacent face ghosts filled (periodically), all else NaN: every
      interior cell right, nothing else written;
    - region 0 with EVERY ghost NaN: the cells one in from each face are right and finite, so the
      interior reads no ghost and may run beside the exchange; nothing else written;
    - region 1: exactly the remaining cells; 0 then 1 into one output: bit-identical to region 2.

    The small geometries take each branch of HaloExchange::stencil: Z = 1 and 2, Y = 1 and 2,
    X = 1 and 2 (no interior, a shell that lacks slabs), 3^3 (an interior of one cell)."""
    r = Regions(tz, order, geo)
    everything = np.ones(r.data.shape, dtype=bool)
    inner = np.zeros_like(everything)
    inner[:, 1:-1, 1:-1, 1:-1] = True  # empty when an extent is below 3
    whole = r.run(r.wrapped, [2])
    r.check(whole, everything, "region 2")
    r.check(r.run(r.bare, [0]), inner, "region 0 with NaN ghosts")
    r.check(r.run(r.wrapped, [0]), inner, "region 0")
    r.check(r.run(r.wrapped, [1]), everything & ~inner, "region 1")
    both = r.run(r.wrapped, [0, 1])
    r.check(both, everything, "regions 0 then 1")
    assert np.array_equal(both.view(np.int64), whole.view(np.int64)), "regions 0 + 1 differ from region 2 in bits"


def test_stencil_out_ptr_is_zero_outside_stencil_mode(tz, gpu):
    a = tz.HaloArgs()
    a.nx = a.ny = a.nz = 8
    assert tz.HaloExchange(a).stencil_out_ptr() == 0
    a.stencil = True
    assert tz.HaloExchange(a).stencil_out_ptr() == 0  # not set up yet
