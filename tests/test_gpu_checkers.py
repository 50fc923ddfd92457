"""The device-side checkers (halo_init, halo_check, stencil_check) against numpy: they are the
oracle of every multi-rank run, where they are only ever seen returning 0. Here the expected grids
come from a wrap-padded global field sliced per rank, and every planted error must be counted
exactly once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NX, NY, NZ, G, NQ = 12, 10, 8, 2, 3
C0, C1 = 0.4, 0.1  # StencilBox defaults, which stencil_check uses
# one rank, and ranks 5 and 7 of a 2 x 2 x 2 rank grid (coordinates (1, 0, 1) and (1, 1, 1): the
# global wrap crosses rank boundaries)
RANKS = [(0, 1), (5, 2), (7, 2)]
RANK_IDS = ["1rank", "rank5of8", "rank7of8"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _halo(tz, order, neighbors, rank, p):
    a = tz.HaloArgs()
    a.nx, a.ny, a.nz, a.nq, a.ghost = NX, NY, NZ, NQ, G
    a.neighbors, a.order = neighbors, order
    a.rank, a.size, a.px, a.py, a.pz = rank, p ** 3, p, p, p
    return tz.HaloExchange(a)  # geometry only: never set up


def _field(p, gen):
    """the global field (q, gz, gy, gx) that halo_init encodes, exact in float64"""
    q, gz, gy, gx = np.meshgrid(np.arange(NQ, dtype=np.int64), np.arange(NZ * p, dtype=np.int64),
                                np.arange(NY * p, dtype=np.int64), np.arange(NX * p, dtype=np.int64),
                                indexing="ij")
    v = ((q * 65536 + gz) * 65536 + gy) * 65536 + gx + (np.int64(gen) << 51)
    assert int(v.max()) < 1 << 53
    return v.astype(np.float64)


def _block(padded, h, lo, hi):
    """this rank's block of a global array padded by G: logical cells [lo, n + 2 G - hi) per axis"""
    cx, cy, cz = h.coords()
    return padded[:, cz * NZ + lo:cz * NZ + NZ + 2 * G - hi, cy * NY + lo:cy * NY + NY + 2 * G - hi,
                  cx * NX + lo:cx * NX + NX + 2 * G - hi]


def _ghost_rank():
    """per logical cell (z, y, x): on how many axes it lies in the ghost layer (0: interior)"""
    def axis(n):
        i = np.arange(n + 2 * G)
        return ((i < G) | (i >= n + G)).astype(np.int64)
    return axis(NZ)[:, None, None] + axis(NY)[None, :, None] + axis(NX)[None, None, :]


def _exchanged(h, p, gen, neighbors):
    """the logical grid (q, z, y, x) of this rank after a complete exchange"""
    pad = np.pad(_field(p, gen), ((0, 0), (G, G), (G, G), (G, G)), mode="wrap")
    e = _block(pad, h, 0, 0).copy()
    if neighbors == 6:  # only the faces are filled
        e[:, _ghost_rank() > 1] = -1.0
    return e


def _logical(h, t):
    """the storage t as a (q, z, y, x) view over the logical grid, ghosts included"""
    lay = h.layout()
    st = lay["strides_qzyx"]
    return t.as_strided(lay["shape_qzyx"], st, lay["x_offset_cells"] * st[3])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _garbage(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)


def _padding(h):
    """storage elements outside the logical grid (row padding)"""
    m = torch.ones(h.grid_elems(), dtype=torch.bool, device="cuda")
    _logical(h, m).fill_(False)
    return m


@pytest.fixture(params=[(o, nb, r) for o in ("xyzq", "qxyz") for nb in (6, 26) for r in range(len(RANKS))],
                ids=lambda t: f"{t[0]}-{t[1]}-{RANK_IDS[t[2]]}")
def geo(tz, gpu, request):
    order, neighbors, r = request.param
    rank, p = RANKS[r]
    h = _halo(tz, order, neighbors, rank, p)
    if p == 2:
        assert tuple(h.coords()) == (rank & 1, rank >> 1 & 1, rank >> 2)
    assert bool(_padding(h).any()), "no row padding: the padding checks are void"
    return h, p, neighbors


@pytest.mark.parametrize("gen", [0, 1, 2, 3])
def test_halo_init_matches_numpy(tz, geo, gen):
    h, p, _ = geo
    k = tz._tz.kernels
    grid = _garbage(h.grid_elems(), 1)
    exp = grid.clone()
    want = np.full((NQ, NZ + 2 * G, NY + 2 * G, NX + 2 * G), -1.0)
    want[:, G:-G, G:-G, G:-G] = _block(_field(p, gen), h, 0, 2 * G)
    _logical(h, exp).copy_(_cuda(want))
    k.halo_init(h, gen, grid.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = _logical(h, grid).cpu().numpy()
    assert np.array_equal(got[:, G:-G, G:-G, G:-G], want[:, G:-G, G:-G, G:-G]), "interior"
    assert np.array_equal(got, want), "ghosts must be -1"
    assert torch.equal(grid.view(torch.int64), exp.view(torch.int64)), "row padding was written"


def _cells(neighbors):
    """7 logical cells (q, z, y, x): a face, an edge and a corner ghost, an interior cell, the
    first and the last logical element (corner ghosts too), one more face ghost; every q occurs"""
    Z, Y, X = NZ + 2 * G, NY + 2 * G, NX + 2 * G
    return [(0, G + 1, G + 2, 0),          # -x face ghost
            (1, Z - 1, 1, G + 3),          # +z -y edge ghost
            (2, 1, Y - 2, X - 1),          # corner ghost
            (1, G, G, G),                  # first interior cell
            (0, 0, 0, 0),                  # first logical element
            (NQ - 1, Z - 1, Y - 1, X - 1),  # last logical element
            (2, G + 3, Y - 1, G + 5)]      # +y face ghost


@pytest.mark.parametrize("gen", [0, 1, 2, 3])
def test_halo_check_counts_exactly(tz, geo, gen):
    h, p, neighbors = geo
    k = tz._tz.kernels
    good_l = _exchanged(h, p, gen, neighbors)
    good = _garbage(h.grid_elems(), 2)
    _logical(h, good).copy_(_cuda(good_l))
    s = _stream()
    assert k.halo_check(h, gen, good.data_ptr(), s) == 0
    # row padding is nobody's business
    bad = good.clone()
    bad[_padding(h)] = 12345.0
    assert k.halo_check(h, gen, bad.data_ptr(), s) == 0
    # one wrong value at a time, then all seven
    cells = _cells(neighbors)
    assert {c[0] for c in cells} == set(range(NQ))
    every = good.clone()
    for c in cells:
        one = good.clone()
        for t in (one, every):
            lv = _logical(h, t)
            lv[c] = lv[c] + 1.0  # -1 -> 0, a coordinate -> its x neighbour's
        assert k.halo_check(h, gen, one.data_ptr(), s) == 1, f"cell {c}"
    assert k.halo_check(h, gen, every.data_ptr(), s) == 7
    # a -1 where a value belongs, and the right value of the wrong generation
    other = _exchanged(h, p, (gen + 1) % 4, neighbors)
    interior = cells[3]
    for v in (-1.0, float(other[interior])):
        one = good.clone()
        _logical(h, one)[interior] = v
        assert k.halo_check(h, gen, one.data_ptr(), s) == 1
    stale = good.clone()
    _logical(h, stale).copy_(_cuda(other))
    assert k.halo_check(h, gen, stale.data_ptr(), s) == int((other != -1.0).sum())
    assert k.halo_check(h, (gen + 1) % 4, stale.data_ptr(), s) == 0
    # before the exchange every ghost an exchange fills is wrong
    k.halo_init(h, gen, stale.data_ptr(), s)
    assert k.halo_check(h, gen, stale.data_ptr(), s) == int((good_l[:, _ghost_rank() > 0] != -1.0).sum())


def _stencils(h, p, gen):
    """the 7-point stencil of this rank's interior from the wrap-padded global field, in float64,
    in two addition orders: the checker's own and a pairwise one with c1 distributed"""
    pad = np.pad(_field(p, gen), ((0, 0), (G, G), (G, G), (G, G)), mode="wrap")

    def v(dz, dy, dx):
        return _block(pad, h, G, G)[...] if (dz, dy, dx) == (0, 0, 0) else \
            _block(np.roll(pad, (-dz, -dy, -dx), axis=(1, 2, 3)), h, G, G)
    c, xm, xp, ym, yp, zm, zp = (v(0, 0, 0), v(0, 0, -1), v(0, 0, 1), v(0, -1, 0), v(0, 1, 0), v(-1, 0, 0),
                                 v(1, 0, 0))
    a = C0 * c + C1 * (xm + xp + ym + yp + zm + zp)
    b = ((C1 * zp + C1 * zm) + (C1 * yp + C1 * ym)) + ((C1 * xp + C1 * xm) + C0 * c)
    return a, b


@pytest.mark.parametrize("gen", [0, 1, 2, 3])
def test_stencil_check_counts_exactly(tz, geo, gen):
    """stencil_check accepts |out - want| <= 2^-49 want: both honest evaluation orders count 0,
    a wrong y neighbour (off by c1 * 65536) or z neighbour (c1 * 2^32) is counted at the cell of
    the largest value of every generation. With the former 1e-12 |want| + 1e-9 the y case passed
    unnoticed at generation 3 (want 7.3e15, tolerance 7318 against 6553.6)"""
    h, p, _ = geo
    k = tz._tz.kernels
    s = _stream()
    a, b = _stencils(h, p, gen)
    assert float(np.abs(a - b).max() / a.max()) < 2.0 ** -49  # the two orders themselves agree
    outs = []
    for want in (a, b):
        out = torch.full((h.grid_elems(),), float("nan"), dtype=torch.float64, device="cuda")
        _logical(h, out)[:, G:-G, G:-G, G:-G] = _cuda(want)
        assert k.stencil_check(h, gen, out.data_ptr(), s) == 0
        outs.append(out)
    out = outs[0]
    top = tuple(int(i) for i in np.unravel_index(np.argmax(a), a.shape))
    cell = (top[0], top[1] + G, top[2] + G, top[3] + G)
    for err in (C1 * 65536, -C1 * 65536, C1 * 2.0 ** 32):
        assert abs(err) > 2.0 ** -49 * a[top] and abs(err) > 4 * np.spacing(a[top])
        one = out.clone()
        _logical(h, one)[cell] = float(a[top]) + err
        assert k.stencil_check(h, gen, one.data_ptr(), s) == 1, f"deviation {err} at {cell} not counted"
    # a NaN is no match
    one = out.clone()
    _logical(h, one)[cell] = float("nan")
    assert k.stencil_check(h, gen, one.data_ptr(), s) == 1
    # three deviations, three counts; ghosts and padding of `out` are never read (they are NaN)
    three = out.clone()
    for c in ((0, G, G, G), (1, G + 3, G + 4, G + 5), (NQ - 1, NZ + G - 1, NY + G - 1, NX + G - 1)):
        _logical(h, three)[c] += C1 * 2.0 ** 32
    assert k.stencil_check(h, gen, three.data_ptr(), s) == 3
    if gen == 0:
        # a wrong x neighbour (off by c1 * 1) is below one ulp of `out` at generations 1-3; it can
        # be resolved where the value is small: generation 0, q = 0, z = 0
        low = (0, 0, 0, 0)
        assert C1 > 2.0 ** -49 * a[low] and C1 > 4 * np.spacing(a[low])
        one = out.clone()
        _logical(h, one)[0, G, G, G] = float(a[low]) + C1
        assert k.stencil_check(h, gen, one.data_ptr(), s) == 1
    else:
        assert C1 < np.spacing(a.min())
