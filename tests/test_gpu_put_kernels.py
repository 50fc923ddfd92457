"""The signalling put kernels and their counters in one process on one device: what a put must
do (the data, one signal per box per launch, block counters back at zero, every block cap),
ipc_signal / ipc_wait, gather_put_signal, copy_many and copy_bytes. Flags and counters are plain
torch tensors, a second tensor stands in for the peer's grid or receive buffer.

No launch here waits for anything that is not already there: a counter is set before the wait
is launched, or its writer is an earlier launch on the same stream. timeout_s = 1.0 is never
reached and err stays 0."""
import numpy as np
import pytest

from test_gpu_box_tuning import _bits, _box_moves, _count, _halo, _move_ref, _nan, _pack_ref, _stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# the smallest grid in use whose z face (11 520 16-B items, 15 blocks of 3 x 256) exceeds a cap
# while a corner (81 elements) is a quarter of one block: nb = 1, nb = cap and nb < cap at once
SHAPE = (64, 40, 24)
LAYOUTS = [("xyzq", None), ("qxyz", None), ("xyzq", -1)]
LAYOUT_IDS = ["xyzq", "qxyz", "xyzq-rowstart"]
CAPS = [1, 2, 0, 4096]  # 0: BoxTuning::put_max_blocks (64)
GUARD_FLAG = -0x0123456789ABCDEF
PROBE = 1 << 20  # a block counter that starts here never reaches nb - 1: it only counts blocks


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


class _Flags:
    """n flags of arbitrary initial values with a guard slot on either side"""

    def __init__(self, init):
        self.init = list(init)
        self.t = _i64([GUARD_FLAG] + self.init + [GUARD_FLAG])

    def ptrs(self):
        return [self.t.data_ptr() + 8 * (1 + i) for i in range(len(self.init))]

    def values(self):
        v = self.t.tolist()
        assert v[0] == GUARD_FLAG and v[-1] == GUARD_FLAG, "a signal landed beside the flag array"
        return v[1:-1]


def _case(tz, layout):
    order, align = layout
    h = _halo(tz, SHAPE, order, ghost_align=align)
    gen = torch.Generator(device="cuda").manual_seed(5)
    # (grid A is the first half of its allocation: a lane that ran one item past a box would read
    # a row of the plane after the last one; the guard behind every buffer shows its store)
    a = torch.randn(2 * h.grid_elems(), dtype=torch.float64, device="cuda", generator=gen)[:h.grid_elems()]
    return h, a


def _buffers(boxes):
    """one NaN tensor holding every box's dense buffer, 2 doubles (16 B) of guard around each"""
    offs, o = [], 2
    for b in boxes:
        offs.append(o)
        o += _count(b) + 2 + _count(b) % 2  # buffers stay 16-B aligned
    return _nan(o), offs


def _pack_expected(a, boxes, offs, total):
    exp = _nan(total)
    for b, o in zip(boxes, offs):
        exp[o:o + _count(b)] = _pack_ref(a, b)
    return exp


# ---------------------------------------------------------------- signalling moves and packs

@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_move_signal(tz, gpu, layout, cap):
    """26 moves from grid A into grid B, three launches on the same tensors"""
    k = tz._tz.kernels
    h, a = _case(tz, layout)
    nd = h.ndirs()
    b = _nan(h.grid_elems())
    moves = _box_moves(h, a.data_ptr(), b.data_ptr())
    if layout[1] == -1:
        assert "peeled" in k.move_kinds(moves), "no peeled box: the peeled signal path did not run"
    exp = _nan(h.grid_elems())
    _move_ref(exp, a, moves)
    a0 = a.clone()
    flags = _Flags(5 + i for i in range(nd))
    done = torch.zeros(nd + 1, dtype=torch.int32, device="cuda")
    for launch in range(1, 4):
        k.box_move_many_signal(moves, done.data_ptr(), flags.ptrs(), cap, _stream())
        torch.cuda.synchronize()
        assert torch.equal(_bits(b), _bits(exp)), f"launch {launch}: grid B differs"
        assert flags.values() == [5 + i + launch for i in range(nd)], f"launch {launch}"
        assert not done.any(), f"launch {launch}: block counters not back at zero: {done.tolist()}"
        b.copy_(_nan(h.grid_elems()))  # the next launch must deliver everything again
    assert torch.equal(_bits(a), _bits(a0))


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_pack_signal(tz, gpu, layout, cap):
    """26 packs of grid A into dense (peer) buffers, three launches; then three in store mode:
    the boxes in store_mask publish ++count[i] instead of adding 1"""
    k = tz._tz.kernels
    h, a = _case(tz, layout)
    nd = h.ndirs()
    boxes = [h.pack_box(i) for i in range(nd)]
    bufs, offs = _buffers(boxes)
    exp = _pack_expected(a, boxes, offs, bufs.numel())
    boxes = [dict(b, buf=bufs.data_ptr() + 8 * o) for b, o in zip(boxes, offs)]
    flags = _Flags(5 + i for i in range(nd))
    done = torch.zeros(nd + 1, dtype=torch.int32, device="cuda")
    for launch in range(1, 4):
        k.box_pack_many_signal(a.data_ptr(), boxes, done.data_ptr(), flags.ptrs(), max_blocks=cap,
                               stream=_stream())
        torch.cuda.synchronize()
        assert torch.equal(_bits(bufs), _bits(exp)), f"launch {launch}: buffers differ"
        assert flags.values() == [5 + i + launch for i in range(nd)], f"launch {launch}"
        assert not done.any(), f"launch {launch}: block counters not back at zero: {done.tolist()}"
        bufs.copy_(_nan(bufs.numel()))
    # store mode on alternate boxes; their flags start at garbage
    mask = sum(1 << i for i in range(0, nd, 2))
    masked = [bool(mask >> i & 1) for i in range(nd)]
    flags = _Flags(-99 - i if masked[i] else 5 + i for i in range(nd))
    count = _Flags(100 + i for i in range(nd))
    for launch in range(1, 4):
        k.box_pack_many_signal(a.data_ptr(), boxes, done.data_ptr(), flags.ptrs(), count.ptrs()[0], mask, cap,
                               _stream())
        torch.cuda.synchronize()
        assert torch.equal(_bits(bufs), _bits(exp)), f"store launch {launch}: buffers differ"
        assert flags.values() == [100 + i + launch if masked[i] else 5 + i + launch for i in range(nd)]
        assert count.values() == [100 + i + (launch if masked[i] else 0) for i in range(nd)]
        assert not done.any()
        bufs.copy_(_nan(bufs.numel()))


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_put_block_caps(tz, gpu, layout):
    """workgroups per box under every cap. A block counter that starts far above any block count
    never sees `nb - 1`, so nobody resets it or signals: after the launch it has counted the
    box's blocks. Uncapped counts come from cap 4096; every other cap must give min(uncapped,
    cap), the launch's own cap taking precedence over BoxTuning::put_max_blocks"""
    k = tz._tz.kernels
    h, a = _case(tz, layout)
    nd = h.ndirs()
    b = _nan(h.grid_elems())
    moves = _box_moves(h, a.data_ptr(), b.data_ptr())
    boxes = [h.pack_box(i) for i in range(nd)]
    bufs, offs = _buffers(boxes)
    boxes = [dict(bx, buf=bufs.data_ptr() + 8 * o) for bx, o in zip(boxes, offs)]
    flags = _Flags(5 + i for i in range(nd))

    def blocks(cap, pack):
        done = torch.full((nd,), PROBE, dtype=torch.int32, device="cuda")
        if pack:
            k.box_pack_many_signal(a.data_ptr(), boxes, done.data_ptr(), flags.ptrs(), max_blocks=cap,
                                   stream=_stream())
        else:
            k.box_move_many_signal(moves, done.data_ptr(), flags.ptrs(), cap, _stream())
        torch.cuda.synchronize()
        assert flags.values() == [5 + i for i in range(nd)], "a box signalled before its count was complete"
        return [v - PROBE for v in done.tolist()]

    face_z = next(i for i in range(nd) if h.dir(i) == (0, 0, 1))
    corner = next(i for i in range(nd) if h.dir(i) == (1, 1, 1))
    prev = k.get_put_max_blocks()
    try:
        for pack in (False, True):
            free = blocks(4096, pack)
            assert free[corner] == 1 and min(free) == 1
            if layout[1] is None:  # 16-B items: 11 520 of them, 3 x 256 per block
                assert free[face_z] == 15, free
            assert max(free) > 2
            assert blocks(1, pack) == [1] * nd
            assert blocks(2, pack) == [min(f, 2) for f in free]
            assert blocks(0, pack) == [min(f, 64) for f in free]
            k.set_put_max_blocks(3)  # the global cap: taken with max_blocks 0, overridden otherwise
            assert blocks(0, pack) == [min(f, 3) for f in free]
            assert blocks(4096, pack) == free
            k.set_put_max_blocks(prev)
    finally:
        k.set_put_max_blocks(prev)


def test_put_signal_bad_arguments(tz, gpu):
    k = tz._tz.kernels
    h, a = _case(tz, LAYOUTS[0])
    b = _nan(h.grid_elems())
    moves = _box_moves(h, a.data_ptr(), b.data_ptr())[:3]
    boxes = [h.pack_box(i) for i in range(3)]
    bufs, offs = _buffers(boxes)
    boxes = [dict(bx, buf=bufs.data_ptr() + 8 * o) for bx, o in zip(boxes, offs)]
    flags = _Flags([5, 6, 7])
    count = _Flags([100, 101, 102])
    done = torch.zeros(4, dtype=torch.int32, device="cuda")
    d, f, s = done.data_ptr(), flags.ptrs(), _stream()
    null_flag = [f[0], 0, f[2]]
    with pytest.raises(RuntimeError, match="null flag"):
        k.box_move_many_signal(moves, d, null_flag, 0, s)
    with pytest.raises(RuntimeError, match="null buffer/flag"):
        k.box_pack_many_signal(a.data_ptr(), boxes, d, null_flag, stream=s)
    with pytest.raises(RuntimeError, match="empty box"):
        k.box_move_many_signal([moves[0], dict(moves[1], len=0), moves[2]], d, f, 0, s)
    with pytest.raises(RuntimeError, match="empty box"):
        k.box_pack_many_signal(a.data_ptr(), [boxes[0], dict(boxes[1], n1=0), boxes[2]], d, f, stream=s)
    with pytest.raises(RuntimeError, match="without counters"):
        k.box_pack_many_signal(a.data_ptr(), boxes, d, f, 0, 0b101, 0, s)
    with pytest.raises(RuntimeError, match="row pairs"):
        k.box_move_many_signal([dict(moves[0], pair=True)] + moves[1:], d, f, 0, s)
    with pytest.raises(RuntimeError, match="null block counters"):
        k.box_move_many_signal(moves, 0, f, 0, s)
    # MoveSignal::count / store_mask are the pack's: the move refuses them instead of ignoring them
    with pytest.raises(RuntimeError, match="store mode is for packs only"):
        k.box_move_many_signal(moves, d, f, 0, s, count=count.ptrs()[0], store_mask=0b010)
    torch.cuda.synchronize()
    # nothing was launched
    assert flags.values() == [5, 6, 7] and count.values() == [100, 101, 102] and not done.any()
    assert bool(torch.isnan(b).all()) and bool(torch.isnan(bufs).all())


# ---------------------------------------------------------------- ipc_signal and ipc_wait

@pytest.mark.parametrize("n", [1, 26, 64])
def test_ipc_signal(tz, gpu, n):
    k = tz._tz.kernels
    c = _Flags(7 + 3 * i for i in range(n))
    for launch in range(1, 3):
        k.ipc_signal(c.ptrs(), stream=_stream())
        torch.cuda.synchronize()
        assert c.values() == [7 + 3 * i + launch for i in range(n)]
    # store mode: counters[k] = ++count[k]; the counters start at garbage
    c = _Flags(-5 - i for i in range(n))
    count = _Flags(50 + 2 * i for i in range(n))
    for launch in range(1, 3):
        k.ipc_signal(c.ptrs(), count.ptrs()[0], _stream())
        torch.cuda.synchronize()
        assert count.values() == [50 + 2 * i + launch for i in range(n)]
        assert c.values() == count.values()


def test_ipc_signal_bad_arguments(tz, gpu):
    k = tz._tz.kernels
    c = _Flags(range(65))
    with pytest.raises(RuntimeError, match="too many counters"):
        k.ipc_signal(c.ptrs(), stream=_stream())
    with pytest.raises(RuntimeError, match="null counter"):
        k.ipc_signal([c.ptrs()[0], 0], stream=_stream())
    torch.cuda.synchronize()
    assert c.values() == list(range(65))


NSLOTS = 80


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("n", [1, 26, 64])
def test_ipc_wait_satisfied(tz, gpu, n, lag):
    """lag 0: arrive[s] = expected[s] + 1; lag 1: arrive[s] = expected[s]. The counters are set
    before the launch, so nothing spins. Slots outside the subset hold unsatisfied values: the
    kernel must not look at them"""
    k = tz._tz.kernels
    rng = np.random.default_rng(100 * n + lag)
    slots = [int(s) for s in rng.permutation(NSLOTS)[:n]]
    exp0 = [3 + 2 * s for s in range(NSLOTS)]
    expected = _Flags(exp0)
    arrive = _Flags(exp0[s] + 1 - lag if s in slots else 0 for s in range(NSLOTS))
    # every third waiter forwards nothing
    sig = _Flags(1000 + i for i in range(n))
    forward = [p if i % 3 != 2 else 0 for i, p in enumerate(sig.ptrs())]
    err = torch.zeros(3, dtype=torch.int32, device="cuda")
    for launch in range(1, 3):
        k.ipc_wait(arrive.ptrs()[0], expected.ptrs()[0], slots, err.data_ptr() + 4, 1.0, lag, forward, _stream())
        torch.cuda.synchronize()
        assert err.tolist() == [0, 0, 0]
        assert expected.values() == [e + launch if s in slots else e for s, e in enumerate(exp0)]
        assert sig.values() == [1000 + i + (launch if i % 3 != 2 else 0) for i in range(n)]
        assert arrive.values() == [exp0[s] + launch - lag if s in slots else 0 for s in range(NSLOTS)]
        arrive.t[1:-1] += _i64([1 if s in slots else 0 for s in range(NSLOTS)])  # the next arrival
    # without signal counters
    k.ipc_wait(arrive.ptrs()[0], expected.ptrs()[0], slots, err.data_ptr() + 4, 1.0, lag, None, _stream())
    torch.cuda.synchronize()
    assert err.tolist() == [0, 0, 0]
    assert expected.values() == [e + 3 if s in slots else e for s, e in enumerate(exp0)]
    assert sig.values() == [1000 + i + (2 if i % 3 != 2 else 0) for i in range(n)]


def test_ipc_wait_bad_arguments(tz, gpu):
    k = tz._tz.kernels
    c = _Flags([1] * NSLOTS)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="too many slots"):
        k.ipc_wait(c.ptrs()[0], c.ptrs()[0], list(range(65)), err.data_ptr(), 1.0, 0, None, _stream())
    with pytest.raises(RuntimeError, match="lag must be 0 or 1"):
        k.ipc_wait(c.ptrs()[0], c.ptrs()[0], [0], err.data_ptr(), 1.0, 2, None, _stream())
    with pytest.raises(RuntimeError, match="null pointer"):
        k.ipc_wait(c.ptrs()[0], c.ptrs()[0], [0], 0, 1.0, 0, None, _stream())
    torch.cuda.synchronize()
    assert c.values() == [1] * NSLOTS and err.item() == 0


def _logical(h, t):
    """the storage t as a (q, z, y, x) view over the logical grid, ghosts included"""
    lay = h.layout()
    st = lay["strides_qzyx"]
    return t.as_strided(lay["shape_qzyx"], st, lay["x_offset_cells"] * st[3])


@pytest.mark.parametrize("order", ["xyzq", "qxyz"])
def test_put_wait_unpack_chain(tz, gpu, order):
    """one exchange the way the buffers-mode IPC transport runs it, on one stream: the signalling
    pack puts every slab into a receive buffer and bumps its arrival counter, ipc_wait (lag 0)
    waits for those counters (their writer is the launch before it), box_copy_many unpacks the
    buffers into a second grid, whose ghosts must be the periodic images of the interior"""
    k = tz._tz.kernels
    h = _halo(tz, (20, 12, 9), order)
    nd, g = h.ndirs(), 3
    gen = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn(2 * h.grid_elems(), dtype=torch.float64, device="cuda", generator=gen)[:h.grid_elems()]
    b = a.clone()
    lb = _logical(h, b)
    interior = lb[:, g:-g, g:-g, g:-g].clone()
    lb.fill_(float("nan"))
    lb[:, g:-g, g:-g, g:-g] = interior
    want = np.pad(interior.cpu().numpy(), ((0, 0), (g, g), (g, g), (g, g)), mode="wrap")
    # slab facing d -> receive buffer d -> the ghost on side -d
    packs = [h.pack_box(i) for i in range(nd)]
    bufs, offs = _buffers(packs)
    packs = [dict(p, buf=bufs.data_ptr() + 8 * o) for p, o in zip(packs, offs)]
    unpacks = [dict(h.unpack_box(h.opposite(i)), buf=bufs.data_ptr() + 8 * o) for i, o in zip(range(nd), offs)]
    rng = np.random.default_rng(3)
    slots = [int(s) for s in rng.permutation(NSLOTS)[:nd]]
    exp0 = [40 + s for s in range(NSLOTS)]
    arrive, expected = _Flags(exp0), _Flags(exp0)
    done = torch.zeros(nd, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = _stream()
    k.box_pack_many_signal(a.data_ptr(), packs, done.data_ptr(), [arrive.ptrs()[x] for x in slots], stream=s)
    k.ipc_wait(arrive.ptrs()[0], expected.ptrs()[0], slots, err.data_ptr(), 1.0, 0, None, s)
    k.box_copy_many(b.data_ptr(), unpacks, True, s)
    torch.cuda.synchronize()
    assert err.item() == 0 and not done.any()
    bumped = [e + 1 if x in slots else e for x, e in enumerate(exp0)]
    assert arrive.values() == bumped and expected.values() == bumped
    got = _logical(h, b).cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} wrong cells"


# ---------------------------------------------------------------- gather_put_signal

def _gather_case(sizes, seed):
    """segments of the given sizes at non-zero offsets into a random index list, each with its
    own destination inside one NaN tensor (a guard element after every dst) and its own flag"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randn(50_000, dtype=torch.float32, device="cuda", generator=gen)
    offs, o = [], 3
    for n in sizes:
        offs.append(o)
        o += n + 5
    idx = torch.randint(0, src.numel(), (o,), dtype=torch.int32, device="cuda", generator=gen)
    dsts, d = [], 1
    for n in sizes:
        dsts.append(d)
        d += n + 1
    dst = torch.full((d,), float("nan"), dtype=torch.float32, device="cuda")
    exp = dst.clone()
    for n, so, do in zip(sizes, offs, dsts):
        exp[do:do + n] = src[idx[so:so + n].long()]
    flags = _Flags(9 + 2 * i for i in range(len(sizes)))
    segs = [dict(dst=dst.data_ptr() + 4 * do, off=so, n=n, flag=p)
            for n, so, do, p in zip(sizes, offs, dsts, flags.ptrs())]
    return src, idx, dst, exp, flags, segs


SEG_SIZES = [1, 255, 1024, 1025, 70_001]  # 1, 1, 1, 2 and 64 blocks (69 uncapped: the lanes loop)


def test_gather_put_signal(tz, gpu):
    k = tz._tz.kernels
    src, idx, dst, exp, flags, segs = _gather_case(SEG_SIZES, 1)
    done = torch.zeros(64, dtype=torch.int32, device="cuda")
    for launch in range(1, 3):
        k.gather_put_signal(src.data_ptr(), idx.data_ptr(), segs, done.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert torch.equal(dst.view(torch.int32), exp.view(torch.int32)), f"launch {launch}"
        assert flags.values() == [9 + 2 * i + launch for i in range(len(segs))]
        assert not done.any(), done.tolist()
        dst.fill_(float("nan"))
    # blocks per segment (see test_put_block_caps): 4 x 256 elements per block, 64 at most
    done.fill_(PROBE)
    k.gather_put_signal(src.data_ptr(), idx.data_ptr(), segs, done.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert [v - PROBE for v in done.tolist()[:5]] == [1, 1, 1, 2, 64]
    assert flags.values() == [9 + 2 * i + 2 for i in range(len(segs))]


def test_gather_put_signal_64_segments(tz, gpu):
    k = tz._tz.kernels
    src, idx, dst, exp, flags, segs = _gather_case([3] * 64, 2)
    done = torch.zeros(65, dtype=torch.int32, device="cuda")
    k.gather_put_signal(src.data_ptr(), idx.data_ptr(), segs, done.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int32), exp.view(torch.int32))
    assert flags.values() == [9 + 2 * i + 1 for i in range(64)]
    assert not done.any()
    with pytest.raises(RuntimeError, match="too many peers"):
        k.gather_put_signal(src.data_ptr(), idx.data_ptr(), segs + segs[:1], done.data_ptr(), _stream())
    with pytest.raises(RuntimeError, match="bad segment"):
        k.gather_put_signal(src.data_ptr(), idx.data_ptr(), [segs[0], dict(segs[1], n=0)], done.data_ptr(),
                            _stream())
    torch.cuda.synchronize()
    assert flags.values() == [9 + 2 * i + 1 for i in range(64)] and not done.any()


# ---------------------------------------------------------------- copy_many and copy_bytes

COPY_MANY_BYTES = [8, 16, 24, 4096, 16 * 4 * 256 * 3 + 8]  # the last: 3 blocks, one 4-wide pass, a tail


def test_copy_many(tz, gpu):
    k = tz._tz.kernels
    copies, o = [], 2
    for nbytes in COPY_MANY_BYTES:
        copies.append((o, nbytes // 8))
        o += nbytes // 8 + 2 + (nbytes // 8) % 2  # 16-B aligned, 2 or 3 doubles of guard between
    gen = torch.Generator(device="cuda").manual_seed(4)
    src = torch.randn(o, dtype=torch.float64, device="cuda", generator=gen)
    dst = _nan(o)
    exp = _nan(o)
    for off, n in copies:
        exp[off:off + n] = src[off:off + n]
    k.copy_many([dict(dst=dst.data_ptr() + 8 * off, src=src.data_ptr() + 8 * off, bytes=8 * n)
                 for off, n in copies], _stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(exp))
    # one copy, and a zero-length entry among others
    dst.copy_(_nan(o))
    off, n = copies[3]
    k.copy_many([dict(dst=dst.data_ptr() + 8 * off, src=src.data_ptr() + 8 * off, bytes=8 * n),
                 dict(dst=0, src=0, bytes=0)], _stream())
    torch.cuda.synchronize()
    exp = _nan(o)
    exp[off:off + n] = src[off:off + n]
    assert torch.equal(_bits(dst), _bits(exp))
    d, s = dst.data_ptr(), src.data_ptr()
    for bad in (dict(dst=d + 8, src=s, bytes=16), dict(dst=d, src=s + 8, bytes=16), dict(dst=d, src=s, bytes=12)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            k.copy_many([bad], _stream())
    with pytest.raises(RuntimeError, match="too many copies"):
        k.copy_many([dict(dst=d, src=s, bytes=16)] * 33, _stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(exp))


@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4096 + 7])
def test_copy_bytes(tz, gpu, nbytes):
    k = tz._tz.kernels
    gen = torch.Generator(device="cuda").manual_seed(nbytes)
    src = torch.randint(0, 256, (nbytes + 32,), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    exp = dst.clone()
    exp[16:16 + nbytes] = src[16:16 + nbytes]
    k.copy_bytes(dst.data_ptr() + 16, src.data_ptr() + 16, nbytes, _stream())
    torch.cuda.synchronize()
    assert torch.equal(dst, exp)
    for dd, ss in ((17, 16), (16, 24)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            k.copy_bytes(dst.data_ptr() + dd, src.data_ptr() + ss, nbytes, _stream())
    torch.cuda.synchronize()
    assert torch.equal(dst, exp)
