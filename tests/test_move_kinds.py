"""How the direct-move kernel moves each box (kernels.move_kinds, host only): the x self-wrap of
the reference's XYZQ layout (x = 0 at the row start) as one row pair, odd-offset rows peeled."""


def _pair_moves(tz, nx, g, ghost_align=-1, base=1 << 20):
    """the +x / -x self-wrap of one (dy, dz) = (0, 0) as one row-pair move (geometry from a
    HaloExchange that is not set up; `base` stands in for the grid pointer)"""
    a = tz.HaloArgs()
    a.nx = a.ny = a.nz = nx
    a.nq, a.ghost, a.neighbors, a.order, a.ghost_align = 3, g, 26, "xyzq", ghost_align
    h = tz.HaloExchange(a)
    plus = next(i for i in range(h.ndirs()) if h.dir(i) == (1, 0, 0))
    s, d = h.pack_box(plus), h.unpack_box(h.opposite(plus))
    m = dict(src=base, dst=base, src_off=s["grid_off"], dst_off=d["grid_off"], s1=s["s1"],
             s2=s["s2"], s3=s["s3"], len=s["len"], n1=s["n1"], n2=s["n2"], n3=s["n3"], pair=True)
    return h, m


def test_box_move_spmv_shape(tz):
    """the grid of the fused move + SpMV launch (kernels.box_move_spmv_shape, host only): S =
    ceil(rows W / 256) SpMV workgroups, one every (M + S) / S workgroups, an even quotient less one"""
    import pytest

    k = tz._tz.kernels
    a = tz.HaloArgs()
    a.nx = a.ny = a.nz = 8
    a.nq, a.ghost, a.neighbors, a.order = 3, 2, 26, "qxyz"
    h = tz.HaloExchange(a)
    moves = []
    for i in range(h.ndirs()):
        s, d = h.pack_box(i), h.unpack_box(h.opposite(i))
        moves.append(dict(src=1 << 20, dst=1 << 20, src_off=s["grid_off"], dst_off=d["grid_off"], s1=s["s1"],
                          s2=s["s2"], s3=s["s3"], len=s["len"], n1=s["n1"], n2=s["n2"], n3=s["n3"]))
    ilp = k.SPMV_ILP

    def shape(m, rows, w):
        got = k.box_move_spmv_shape(moves[:m], rows, ilp + w)
        return got["move_blocks"], got["spmv_blocks"], got["stride"]

    assert shape(26, 256, 1) == (26, 1, 27)  # every face of this halo is one workgroup
    assert shape(26, 257, 1) == (26, 2, 13)  # 28 / 2 = 14, made odd
    assert shape(26, 64, 4) == (26, 1, 27) and shape(26, 65, 4) == (26, 2, 13) and shape(26, 129, 2) == (26, 2, 13)
    assert shape(1, 1, 1) == (1, 1, 1) and shape(6, 6 * 64, 4) == (6, 6, 1)  # quotient 2
    assert shape(26, 13 * 256, 1) == (26, 13, 3) and shape(21, 3 * 256, 1) == (21, 3, 7)
    assert shape(2, 7 * 256, 1) == (2, 7, 1)
    assert shape(0, 700, 1) == (0, 3, 1) and shape(3, 0, 1) == (3, 0, 4) and shape(0, 0, 4) == (0, 0, 1)
    assert k.box_move_spmv_shape(moves, 256)["spmv_blocks"] == 4  # lanes default: SPMV_ILP + 4
    with pytest.raises(Exception, match="lanes"):
        k.box_move_spmv_shape(moves, 256, 8)
    with pytest.raises(Exception, match="bad SpMV job"):
        k.box_move_spmv_shape(moves, -1, ilp + 1)
    with pytest.raises(Exception, match="too many boxes"):
        k.box_move_spmv_shape(moves + moves[:7], 256, ilp + 1)
    assert shape(0, 2 ** 31 - 1, 4) == (0, 2 ** 25, 1)  # the largest job: no overflow


def test_kinds_of_the_row_start_layout(tz):
    h, m = _pair_moves(tz, 512, 3)
    plain = dict(m, pair=False)
    # the +x slab starts at x = 512 (16-B aligned), the -x slab at x = 3 (peeled)
    minus = next(i for i in range(h.ndirs()) if h.dir(i) == (-1, 0, 0))
    s, d = h.pack_box(minus), h.unpack_box(h.opposite(minus))
    peeled = dict(plain, src_off=s["grid_off"], dst_off=d["grid_off"])
    k = tz._tz.kernels
    assert k.move_kinds([m, plain, peeled]) == ["pair", "vec8", "peeled"]
    prev = k.get_peel_moves()
    k.set_peel_moves(False)
    try:
        assert k.move_kinds([peeled]) == ["vec8"]
    finally:
        k.set_peel_moves(prev)
