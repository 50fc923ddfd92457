"""Every launch shape of the box kernels against the torch strided-copy references of
test_gpu_kernels.py: the three pack / unpack template instances (BoxTuning::unroll 1-3, 4-7, 8+),
both cache policies, block caps that make a lane loop many times (with max_blocks = 1 one block
walks a whole face, so the unrolled head loop and the tail loop both run), widen_unpack off, and
the move's unroll / items / peel / cap / XCD-order settings. The defaults alone never leave the
first pass of any loop."""
import contextlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- references (shared helpers)

def _halo(tz, shape, order, neighbors=26, ghost=3, nq=3, ghost_align=None):
    a = tz.HaloArgs()
    a.nx, a.ny, a.nz = shape
    a.nq, a.ghost, a.neighbors, a.order = nq, ghost, neighbors, order
    if ghost_align is not None:
        a.ghost_align = ghost_align
    return tz.HaloExchange(a)


def _count(b):
    return b["len"] * b["n1"] * b["n2"] * b["n3"]


def _view(t, b, off):
    """the box's rows at element offset `off` of the pitched array t, as (n3, n2, n1, len)"""
    return t.as_strided((b["n3"], b["n2"], b["n1"], b["len"]), (b["s3"], b["s2"], b["s1"], 1), off)


def _pack_ref(grid, box):
    """what a pack of `box` must leave in its dense buffer"""
    return _view(grid, box, box["grid_off"]).contiguous().reshape(-1)


def _unpack_ref(exp, box, src):
    """unpack the dense buffer src into the pitched array exp (exactly the box)"""
    _view(exp, box, box["grid_off"]).copy_(src.view(box["n3"], box["n2"], box["n1"], box["len"]))


def _box_moves(h, src, dst):
    """slab facing d -> ghost on side -d, as test_box_move_matches_torch builds them"""
    moves = []
    for i in range(h.ndirs()):
        s, d = h.pack_box(i), h.unpack_box(h.opposite(i))
        moves.append(dict(src=src, dst=dst, src_off=s["grid_off"], dst_off=d["grid_off"], s1=s["s1"],
                          s2=s["s2"], s3=s["s3"], len=s["len"], n1=s["n1"], n2=s["n2"], n3=s["n3"]))
    return moves


def _move_ref(exp, grid, moves):
    """apply the moves (row pairs: both runs) to exp, reading the pristine grid"""
    for m in moves:
        runs = [(m["src_off"], m["dst_off"])]
        if m.get("pair"):
            delta, ln = m["dst_off"] - m["src_off"], m["len"]
            runs.append((m["src_off"] + ln + delta, m["src_off"] + ln))
        for so, do in runs:
            _view(exp, m, do).copy_(_view(grid, m, so))


def _mask(n, boxes, widened):
    """the elements of an n-element storage that the boxes' rows cover (widened: with the row
    padding their lead / trail allow an unpack to write)"""
    m = torch.zeros(n, dtype=torch.bool)
    for b in boxes:
        lead, trail = (b["lead"], b["trail"]) if widened else (0, 0)
        _view(m, dict(b, len=lead + b["len"] + trail), b["grid_off"] - lead).fill_(True)
    return m.to("cuda")


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _guarded(grid):
    """a copy of the storage with as many NaNs behind it: a lane that runs one item past a box
    decodes a row of the plane after the last one, which must show as a failed assertion"""
    return torch.cat([grid, _nan(grid.numel())])


@contextlib.contextmanager
def _tuning(k, unroll=None, nt=None, max_blocks=None, widen=None, move_unroll=None, move_items=None,
            peel=None, remap=None):
    """set the given BoxTuning fields; every setting is restored on exit"""
    prev = (k.get_box_tuning(), k.get_widen_unpack(), k.get_move_unroll(), k.get_move_items(),
            k.get_peel_moves(), k.get_xcd_remap())
    t = list(prev[0])
    try:
        if unroll is not None:
            t[0] = unroll
        if nt is not None:
            t[1] = t[2] = nt
        if max_blocks is not None:
            t[3] = max_blocks
        k.set_box_tuning(*t)
        if widen is not None:
            k.set_widen_unpack(widen)
        if move_unroll is not None:
            k.set_move_unroll(move_unroll)
        if move_items is not None:
            k.set_move_items(move_items)
        if peel is not None:
            k.set_peel_moves(peel)
        if remap is not None:
            k.set_xcd_remap(remap)
        yield
    finally:
        k.set_box_tuning(*prev[0])
        k.set_widen_unpack(prev[1])
        k.set_move_unroll(prev[2])
        k.set_move_items(prev[3])
        k.set_peel_moves(prev[4])
        k.set_xcd_remap(prev[5])


# ---------------------------------------------------------------- pack / unpack

SMALL, BIG = (20, 12, 9), (64, 40, 24)
GUARD = 2  # doubles (one 16-B item) of NaN on either side of every dense buffer

_COPY_CASES = {}


def _copy_case(tz, order, shape):
    """grid, boxes, buffers and references of one storage order: computed once, never written"""
    if (order, shape) in _COPY_CASES:
        return _COPY_CASES[order, shape]
    h = _halo(tz, shape, order)
    n = h.grid_elems()
    gen = torch.Generator(device="cuda").manual_seed(20 + len(order) + shape[0])
    # (the grid is the first half of its allocation, as _guarded's copies are)
    grid = torch.randn(2 * n, dtype=torch.float64, device="cuda", generator=gen)[:n]
    pb = [h.pack_box(i) for i in range(h.ndirs())]
    ub = [h.unpack_box(i) for i in range(h.ndirs())]
    assert any(b["lead"] > 0 or b["trail"] > 0 for b in ub), "no widened box: the test is void"
    srcs = [torch.randn(_count(b) + GUARD, dtype=torch.float64, device="cuda", generator=gen)[:_count(b)]
            for b in ub]
    c = dict(h=h, n=n, grid=grid, pb=pb, ub=ub, srcs=srcs, names=[h.dir_name(i) for i in range(h.ndirs())])
    c["pack_ref"] = [_pack_ref(grid, b) for b in pb]
    c["unpack_ref"], exp_all = [], grid.clone()
    for b, s in zip(ub, srcs):
        e = grid.clone()
        _unpack_ref(e, b, s)
        _unpack_ref(exp_all, b, s)
        c["unpack_ref"].append(e)
    c["unpack_all_ref"] = exp_all
    c["mine"] = [_mask(n, [b], False) for b in ub]
    c["allowed"] = [_mask(n, [b], True) for b in ub]
    c["mine_all"], c["allowed_all"] = _mask(n, ub, False), _mask(n, ub, True)
    # the widening covers row padding only
    logical = _mask(n, ub + pb, False)
    assert not (c["allowed_all"] & ~c["mine_all"] & logical).any(), "widened over a logical cell"
    _COPY_CASES[order, shape] = c
    return c


def _bits(t):
    return t.view(torch.int64)


def _run_copies(k, c, which):
    """pack every slab and unpack every ghost box, the boxes in `which` also one per launch;
    returns what the launches left (nothing is compared before the one synchronize)"""
    grid = c["grid"]
    r = dict(single_pack={}, single_unpack={})
    for i in which:
        t = _nan(_count(c["pb"][i]) + 2 * GUARD)
        k.box_copy(grid.data_ptr(), dict(c["pb"][i], buf=t.data_ptr() + 8 * GUARD), False, _stream())
        g2 = _guarded(grid)
        k.box_copy(g2.data_ptr(), dict(c["ub"][i], buf=c["srcs"][i].data_ptr()), True, _stream())
        r["single_pack"][i], r["single_unpack"][i] = t, g2
    r["many_pack"] = [_nan(_count(b) + 2 * GUARD) for b in c["pb"]]
    k.box_copy_many(grid.data_ptr(), [dict(b, buf=t.data_ptr() + 8 * GUARD)
                                      for b, t in zip(c["pb"], r["many_pack"])], False, _stream())
    r["many_unpack"] = _guarded(grid)
    k.box_copy_many(r["many_unpack"].data_ptr(), [dict(b, buf=s.data_ptr()) for b, s in zip(c["ub"], c["srcs"])],
                    True, _stream())
    torch.cuda.synchronize()
    return r


def _check_pack(c, i, buf, what):
    name = c["names"][i]
    assert torch.equal(buf[GUARD:-GUARD], c["pack_ref"][i]), f"pack mismatch, {what}, dir {name}"
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), \
        f"pack wrote outside its buffer, {what}, dir {name}"


def _check_unpack(c, big, exp, mine, allowed, what, exact):
    n, grid = c["n"], c["grid"]
    assert bool(torch.isnan(big[n:]).all()), f"unpack wrote past the grid, {what}"
    g2 = big[:n]
    if exact:  # widen_unpack off: exactly the boxes, row padding included
        assert torch.equal(g2, exp), f"unpack differs from exactly the box, {what}"
    else:
        assert torch.equal(g2[mine], exp[mine]), f"ghost cells wrong, {what}"
        assert torch.equal(g2[~allowed], grid[~allowed]), f"unpack wrote outside its widened rows, {what}"


def _check_copies(c, r, exact=False):
    for i, t in r["single_pack"].items():
        _check_pack(c, i, t, "single")
    for i, t in enumerate(r["many_pack"]):
        _check_pack(c, i, t, "batch")
    for i, big in r["single_unpack"].items():
        _check_unpack(c, big, c["unpack_ref"][i], c["mine"][i], c["allowed"][i], "box " + c["names"][i], exact)
    _check_unpack(c, r["many_unpack"], c["unpack_all_ref"], c["mine_all"], c["allowed_all"], "batch", exact)


@pytest.mark.parametrize("max_blocks", [1, 2, 4096])
@pytest.mark.parametrize("nt", [True, False], ids=["nt", "plain"])
@pytest.mark.parametrize("unroll", [1, 3, 4, 8])
@pytest.mark.parametrize("order", ["xyzq", "qxyz"])
def test_pack_unpack_launch_shapes(tz, gpu, order, unroll, nt, max_blocks):
    """pack of every slab, unpack of every ghost box (the x ghosts widened over row padding), one
    box per launch and all 26 in one, under every template instance, cache policy and block cap.
    20 x 12 x 9 x 3, ghost 3: with one block of 256 lanes a z face is 1080 16-B items: 5 passes of
    the one-item loop (unroll 1 and 3), one pass of the 4-wide head loop and a 56-item tail
    (unroll 4), tail passes only (unroll 8; its head loop: test_pack_unpack_many_passes)"""
    k, c = tz._tz.kernels, _copy_case(tz, order, SMALL)
    g0 = c["grid"].clone()
    with _tuning(k, unroll=unroll, nt=nt, max_blocks=max_blocks):
        r = _run_copies(k, c, range(len(c["pb"])))
    assert torch.equal(_bits(c["grid"]), _bits(g0)), "a pack wrote into the grid"
    _check_copies(c, r)


@pytest.mark.parametrize("unroll,nt", [(1, True), (3, False), (4, True), (8, False), (8, True)])
@pytest.mark.parametrize("order", ["xyzq", "qxyz"])
def test_pack_unpack_many_passes(tz, gpu, order, unroll, nt):
    """64 x 40 x 24 x 3 with one block per box: a z face is 11 520 items, so a lane makes 45 passes
    of the one-item loop, 11 of the 4-wide head loop plus a tail pass, or 5 of the 8-wide head
    loop plus 5 tail passes. All boxes in one launch, the 6 faces also one per launch"""
    k, c = tz._tz.kernels, _copy_case(tz, order, BIG)
    faces = [i for i in range(len(c["pb"])) if sum(map(abs, c["h"].dir(i))) == 1]
    assert len(faces) == 6
    with _tuning(k, unroll=unroll, nt=nt, max_blocks=1):
        r = _run_copies(k, c, faces)
    _check_copies(c, r)


@pytest.mark.parametrize("unroll,max_blocks", [(1, 4096), (3, 1), (4, 2), (8, 1)])
@pytest.mark.parametrize("order", ["xyzq", "qxyz"])
def test_unwidened_unpack_is_exactly_the_box(tz, gpu, order, unroll, max_blocks):
    """widen_unpack = false: the boxes that carry lead / trail are written as exactly the box:
    the ghost cells are exact and the rest of the storage, row padding included, is unchanged"""
    k, c = tz._tz.kernels, _copy_case(tz, order, SMALL)
    with _tuning(k, unroll=unroll, max_blocks=max_blocks, widen=False):
        r = _run_copies(k, c, range(len(c["pb"])))
    _check_copies(c, r, exact=True)


# ---------------------------------------------------------------- moves

_MOVE_CASES = {}


def _move_case(tz, layout, shape):
    """(grid, moves with null pointers, expected grid): computed once per layout and shape.
    Layouts: the two default ones (slab -> opposite ghost, 26 boxes) and XYZQ with x = 0 at the
    row start (ghost_align -1): the exchange's own moves, the x self-wrap as row pairs, every
    other row starting one element past a 16-B boundary (the peeled path)"""
    key = (layout, shape)
    if key in _MOVE_CASES:
        return _MOVE_CASES[key]
    if layout == "xyzq-rowstart":
        h = _halo(tz, shape, "xyzq", ghost_align=-1)
        moves = h.direct_moves(list(range(h.ndirs())))
        moves = [{f: m[f] for f in ("src_off", "dst_off", "s1", "s2", "s3", "len", "n1", "n2", "n3", "pair")}
                 for m in moves]
        assert any(m["pair"] for m in moves), "no row pair: the test is void"
    else:
        h = _halo(tz, shape, layout)
        moves = _box_moves(h, 0, 0)
    gen = torch.Generator(device="cuda").manual_seed(7 + shape[0])
    grid = torch.randn(h.grid_elems(), dtype=torch.float64, device="cuda", generator=gen)
    exp = grid.clone()
    _move_ref(exp, grid, moves)
    _MOVE_CASES[key] = (grid, moves, exp)
    return _MOVE_CASES[key]


@pytest.mark.parametrize("layout,shape,peel,max_blocks,remap", [
    ("xyzq", SMALL, True, 4096, 0),
    ("xyzq", BIG, True, 1, 2),
    ("qxyz", SMALL, True, 1, 0),
    ("qxyz", BIG, True, 4096, 2),
    ("xyzq-rowstart", SMALL, True, 1, 0),
    ("xyzq-rowstart", SMALL, False, 4096, 2),
    ("xyzq-rowstart", BIG, True, 4096, 2),
    ("xyzq-rowstart", BIG, False, 1, 0),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("move_items", [1, 2, 4])
@pytest.mark.parametrize("move_unroll", [1, 2, 4])
def test_move_launch_shapes(tz, gpu, move_unroll, move_items, layout, shape, peel, max_blocks, remap):
    """box_move_many under every unroll instance (1, 2, 4 in flight) and items per lane, with the
    peeled path on and off, one block per box (a lane walks the whole box) and uncapped, in
    launch order and in the per-box XCD order; the whole grid against the torch strided copy"""
    k = tz._tz.kernels
    grid, moves, exp = _move_case(tz, layout, shape)
    out = grid.clone()
    ms = [dict(m, src=out.data_ptr(), dst=out.data_ptr()) for m in moves]
    with _tuning(k, max_blocks=max_blocks, move_unroll=move_unroll, move_items=move_items, peel=peel,
                 remap=remap):
        kinds = set(k.move_kinds(ms))
        k.box_move_many(ms, _stream())
        torch.cuda.synchronize()
    if layout == "xyzq-rowstart":
        assert "pair" in kinds and ("peeled" in kinds) == peel, kinds
    assert torch.equal(out, exp)
