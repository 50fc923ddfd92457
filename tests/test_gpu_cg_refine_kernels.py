"""The three kernels of a refinement step (cg_refine_kernels.hip) on raw device memory:
``cg_refine_accumulate``, ``cg_refine_residual`` and ``cg_refine_decide``.

Oracles: numpy in f64. The accumulate is one IEEE add per element, so numpy's bits. The f64
residual is held to the standard bound of an f64 dot product in any order,
|r64_dev - r64_ref|_i <= (K_i + 2) 2^-53 (|b_i| + sum_j |a_ij| |x64_j|) with K_i the row's entry
count (not a measured constant), and everything derived from it (r, p, u) to the bits of numpy's
conversions of the device's r64. A slab's sum in the kernels' order is within (n + 2) 2^-53
relative of numpy's f64 sum of squares. The decide kernel is held to the bits of the host formula.

Sizes: 1, 3, 4, 5 (a hand-made dense matrix), 255, 1024, 1037, 20 011 (the band matrix), and
70 001 rows with half-width 16, the smallest case in which 4 lanes per row take a second, ragged
grid-stride pass (as test_gpu_cg_batch_kernels.py); the accumulate's 256-thread blocks take
several passes from n = 1037 on. f32 vectors are tested 16-byte aligned and 4 bytes past that.
Every output lies between NaN guard regions that must stay NaN.

Measured on an MI355X: worst |r64_dev - r64_ref| / bound 0.47 (n = 70 001), worst relative slab
error 5.5e-16 (n = 70 001, bound 7.8e-12); the slab nearest its bound is at 0.23 of it (n = 4).
"""
import functools

import numpy as np
import pytest

from cg_kernel_helpers import NAN, SLAB, _nan, _nan_slab, _rand, _same_bits, _stream, _tree_sum
from cg_refine_model import U64, residual64, residual_bound

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [(1, 0), (3, 0), (4, 0), (5, 0), (255, 255), (1024, 1024), (1037, 1037), (20_011, 20_011), (70_001, 16)]
G = 8  # guard elements on either side of a vector


@functools.lru_cache(maxsize=None)
def _matrix(tz, n, bw):
    """(rowPtr, colInd, val) on the host (numpy) and on the device, once per shape, never changed.
    bw = 0: a dense symmetric n x n matrix with every entry stored."""
    if bw:
        rp, ci, v = (np.asarray(a) for a in tz._tz.spd_band_matrix(n, bw, 5 * n, 1))
    else:
        a = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
        a = a + a.T + 2 * n * np.eye(n, dtype=np.float32)
        rp, ci, v = np.arange(0, n * n + 1, n), np.tile(np.arange(n), n), a.reshape(-1)
    host = (rp.astype(np.int64), ci.astype(np.int64), v.astype(np.float32))
    dev = (torch.tensor(rp, dtype=torch.int32).cuda(), torch.tensor(ci, dtype=torch.int32).cuda(),
           torch.tensor(v, dtype=torch.float32).cuda())
    return host, dev


def _guarded(n, dtype, mis=False, fill=None):
    """(buffer, view): n elements between two NaN guard regions; `mis` starts an f32 view 4 bytes
    past a 16-byte boundary; `fill`: the view's contents (a tensor), NaN otherwise"""
    buf = _nan(n + 2 * G + 1, dtype)
    off = G + (1 if mis else 0)
    view = buf[off:off + n]
    assert view.data_ptr() % 16 == (4 if mis else 0)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(torch.isnan(buf[:off]).all() and torch.isnan(buf[off + view.numel():]).all())


def _flag(v):
    """an int32 flag between two sentinels"""
    t = torch.tensor([-7, v, -7], dtype=torch.int32, device="cuda")
    return t, t[1:2]


def _np(t):
    return t.cpu().numpy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("n", [n for n, _ in SIZES] + [300_007])
def test_accumulate(tz, gpu, n, mis):
    kn = tz._tz.kernels
    x0, s0, x640 = _rand(n, 1), _rand(n, 2), _rand(n, 3, torch.float64)
    bx, x = _guarded(n, torch.float32, mis, x0)
    bs, s = _guarded(n, torch.float32, mis, s0)
    b64, x64 = _guarded(n, torch.float64, False, x640)
    fbuf, flag = _flag(0)
    kn.cg_refine_accumulate(n, x.data_ptr(), s.data_ptr(), x64.data_ptr(), flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    want = _np(x640) + _np(x0).astype(np.float64)
    assert _bits_equal(_np(x64), want)
    zero = np.zeros(n, dtype=np.float32)
    assert _bits_equal(_np(x), zero) and _bits_equal(_np(s), zero)  # +0.0, not -0.0
    assert _guards_intact(bx, x) and _guards_intact(bs, s) and _guards_intact(b64, x64)
    assert _np(fbuf).tolist() == [-7, 0, -7]
    # a refined state is written by nothing
    x.copy_(x0)
    s.copy_(s0)
    fbuf, flag = _flag(1)
    kn.cg_refine_accumulate(n, x.data_ptr(), s.data_ptr(), x64.data_ptr(), flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _bits_equal(_np(x64), want) and _same_bits(x, x0) and _same_bits(s, s0)
    if n == 300_007:
        assert n > SLAB * 256  # past the first pass of a full grid


def _residual(kn, dev, n, b, x64, dinv, mis, done=0):
    rp, ci, v = dev
    out = {"r64": _guarded(n, torch.float64), "r": _guarded(n, torch.float32, mis),
           "p": _guarded(n, torch.float32, mis), "u": _guarded(n, torch.float32, mis)}
    p64, p32 = _nan_slab(), _nan_slab()
    fbuf, flag = _flag(done)
    pc = dinv is not None
    kn.cg_refine_residual(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), b.data_ptr(), x64.data_ptr(),
                          dinv.data_ptr() if pc else 0, out["r64"][1].data_ptr(), out["r"][1].data_ptr(),
                          out["p"][1].data_ptr(), out["u"][1].data_ptr() if pc else 0, p64.data_ptr(),
                          p32.data_ptr(), flag.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _np(fbuf).tolist() == [-7, done, -7]
    for buf, view in out.values():
        assert _guards_intact(buf, view)
    return {k: view for k, (_, view) in out.items()}, p64, p32


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("pc", [False, True])
@pytest.mark.parametrize("n,bw", SIZES)
def test_residual(tz, gpu, n, bw, pc, mis):
    kn = tz._tz.kernels
    (rp, ci, v), dev = _matrix(tz, n, bw)
    _, b = _guarded(n, torch.float32, mis, _rand(n, 11))
    x64 = _rand(n, 12, torch.float64)
    dinv = _guarded(n, torch.float32, mis, _rand(n, 13).abs() + 0.25)[1] if pc else None
    out, p64, p32 = _residual(kn, dev, n, b, x64, dinv, mis)
    cnt = kn.cg_refine_partial_count(n)
    assert cnt == min(SLAB, max(1, -(-n * 4 // 1024)))
    r64 = _np(out["r64"])
    ref = residual64(rp, ci, v, _np(b), _np(x64))
    bound = residual_bound(rp, ci, v, _np(b), _np(x64))
    err = np.abs(r64 - ref)
    print(f"residual n={n} pc={pc} mis={mis}: worst |err| / bound = {(err / bound).max():.3f}")
    assert np.isfinite(r64).all() and (err <= bound).all()
    r = r64.astype(np.float32)
    assert _bits_equal(_np(out["r"]), r)
    if pc:
        u = _np(dinv) * r  # numpy's f32 product: one rounding
        assert _bits_equal(_np(out["u"]), u) and _bits_equal(_np(out["p"]), u)
    else:
        assert _bits_equal(_np(out["p"]), r)
        assert torch.isnan(out["u"]).all()  # never touched
    # the slabs: `cnt` partials each and NaN beyond, summed in the kernels' order
    for slab, vec in ((p64, r64), (p32, r.astype(np.float64))):
        part = _np(slab)
        assert not np.isnan(part[:cnt]).any() and np.isnan(part[cnt:]).all()
        want = float(np.dot(vec, vec))
        got = _tree_sum(part[:cnt])
        print(f"  slab: |sum - ref| / ref = {abs(got - want) / want:.3e} bound {(n + 2) * U64:.3e}")
        assert abs(got - want) <= (n + 2) * U64 * want
    # the same bits on every call
    out2, p642, p322 = _residual(kn, dev, n, b, x64, dinv, mis)
    assert all(_same_bits(out[k], out2[k]) for k in out) and _same_bits(p64, p642) and _same_bits(p32, p322)
    # a refined state is written by nothing
    out3, p643, p323 = _residual(kn, dev, n, b, x64, dinv, mis, done=1)
    assert all(torch.isnan(t).all() for t in out3.values()) and torch.isnan(p643).all() and torch.isnan(p323).all()
    if n == 70_001:
        assert n * 4 > SLAB * 1024 and (n * 4) % (SLAB * 1024) != 0  # a second, ragged pass


class _Decide:
    """the state a decide launch touches, laid out as the workload keeps it: the stop state
    [thresh f64 | iters i64 | done i32 | all_done i32], the five scalars and the outer state, every
    f64 a NaN sentinel, done = 7, iters = 41, outer steps = 5"""

    def __init__(self, cnt, seed, outer_thresh, outer_done=0):
        self.cnt = cnt
        self.p64, self.p32 = _nan_slab(), _nan_slab()
        self.p64[:cnt] = _rand(cnt, seed, torch.float64).abs() + 0.1
        self.p32[:cnt] = _rand(cnt, seed + 1, torch.float64).abs() + 0.1
        self.stop = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.thresh = self.stop[0:1].view(torch.float64)
        self.thresh.fill_(NAN)
        self.iters = self.stop[1:2]
        self.iters.fill_(41)
        self.flags = self.stop[2:3].view(torch.int32)  # done, all_done
        self.flags.copy_(torch.tensor([7, -3], dtype=torch.int32))
        self.scal = _nan(7)  # gamma, alpha, beta, gamma_prev, alpha_prev and two guards
        self.outer = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.o_thresh = self.outer[0:1].view(torch.float64)
        self.o_thresh.fill_(outer_thresh)
        self.o_rr = self.outer[1:2].view(torch.float64)
        self.o_rr.fill_(NAN)
        self.o_steps = self.outer[2:3]
        self.o_steps.fill_(5)
        self.o_flags = self.outer[3:4].view(torch.int32)  # outer_done, pad
        self.o_flags.copy_(torch.tensor([outer_done, -9], dtype=torch.int32))

    def args(self, tol2):
        sc = [self.scal[i:i + 1].data_ptr() for i in range(5)]
        return (self.p64.data_ptr(), self.p32.data_ptr(), self.cnt, tol2, self.thresh.data_ptr(),
                self.flags.data_ptr(), *sc, self.o_thresh.data_ptr(), self.o_flags.data_ptr(),
                self.o_steps.data_ptr(), self.o_rr.data_ptr(), _stream())

    def launch(self, kn, tol2):
        kn.cg_refine_decide(*self.args(tol2))
        torch.cuda.synchronize()
        return self

    def sums(self):
        return _tree_sum(_np(self.p64)[:self.cnt]), _tree_sum(_np(self.p32)[:self.cnt])

    def untouched_inner(self):
        return bool(torch.isnan(self.scal).all() and torch.isnan(self.thresh).all()
                    and _np(self.flags).tolist() == [7, -3] and self.iters.item() == 41)


@pytest.mark.parametrize("cnt", [1, 5, 64, 70, SLAB])
def test_decide(tz, gpu, cnt):
    kn = tz._tz.kernels
    tol2 = 1e-5 * 1e-5
    s64, s32 = _Decide(cnt, 20 + cnt, 0.0).sums()
    # below the outer threshold, and exactly on it: refined, and the inner solve is not touched
    for outer_thresh in (2.0 * s64, s64):
        d = _Decide(cnt, 20 + cnt, outer_thresh).launch(kn, tol2)
        assert _np(d.o_flags).tolist() == [1, -9] and d.untouched_inner()
        assert d.o_steps.item() == 5 and d.o_rr.item() == s64 and d.o_thresh.item() == outer_thresh
    # above it: the inner solve restarts
    for outer_thresh in (np.nextafter(s64, 0.0), 0.0, -1.0):
        d = _Decide(cnt, 20 + cnt, outer_thresh).launch(kn, tol2)
        assert _np(d.o_flags).tolist() == [0, -9] and d.o_steps.item() == 6 and d.o_rr.item() == s64
        assert d.thresh.item() == tol2 * s32  # bit for bit: == on two f64 values
        assert _np(d.flags).tolist() == [0, -3] and d.iters.item() == 41
        five = _np(d.scal)
        assert _bits_equal(five[:5], np.zeros(5)) and np.isnan(five[5:]).all()  # +0.0 each
    # a NaN sum never refines
    d = _Decide(cnt, 20 + cnt, 1e300)
    d.p64[cnt - 1] = NAN
    d.launch(kn, tol2)
    assert _np(d.o_flags).tolist() == [0, -9] and d.o_steps.item() == 6 and np.isnan(d.o_rr.item())
    assert d.thresh.item() == tol2 * s32 and _np(d.flags).tolist() == [0, -3]
    # a NaN threshold neither
    d = _Decide(cnt, 20 + cnt, NAN).launch(kn, tol2)
    assert _np(d.o_flags).tolist() == [0, -9] and d.o_steps.item() == 6
    # a refined state is written by nothing, whatever the slabs say
    d = _Decide(cnt, 20 + cnt, 0.0, outer_done=1).launch(kn, tol2)
    assert _np(d.o_flags).tolist() == [1, -9] and d.untouched_inner()
    assert d.o_steps.item() == 5 and np.isnan(d.o_rr.item())
    # slots past the count are not read (they hold NaN) and the slabs are not written
    assert torch.isnan(d.p64[cnt:]).all() and torch.isnan(d.p32[cnt:]).all()


def test_bad_arguments_raise(tz, gpu):
    kn = tz._tz.kernels
    n = 1037
    (rp, ci, v), dev = _matrix(tz, n, n)
    x, s, b, r, p, u, dinv = (_rand(n, i) for i in range(7))
    x64, r64 = _rand(n, 8, torch.float64), _rand(n, 9, torch.float64)
    _, flag = _flag(0)
    f = flag.data_ptr()

    def acc(**kw):
        a = {"n": n, "x": x.data_ptr(), "s": s.data_ptr(), "x64": x64.data_ptr(), "outer_done": f}
        a.update(kw)
        kn.cg_refine_accumulate(**a, stream=_stream())

    with pytest.raises(Exception, match="n must be positive"):
        acc(n=0)
    for name in ("x", "s", "x64", "outer_done"):
        with pytest.raises(Exception, match="null pointer"):
            acc(**{name: 0})
    with pytest.raises(Exception, match="4-byte aligned"):
        acc(x=x.data_ptr() + 2)
    with pytest.raises(Exception, match="8-byte aligned"):
        acc(x64=x64.data_ptr() + 4)
    with pytest.raises(Exception, match="must not overlap"):
        acc(s=x.data_ptr() + 4 * (n - 1))

    p64, p32 = _nan_slab(), _nan_slab()

    def res(**kw):
        a = {"n_rows": n, "row_ptr": dev[0].data_ptr(), "col_ind": dev[1].data_ptr(), "val": dev[2].data_ptr(),
             "b": b.data_ptr(), "x64": x64.data_ptr(), "dinv": dinv.data_ptr(), "r64": r64.data_ptr(),
             "r": r.data_ptr(), "p": p.data_ptr(), "u": u.data_ptr(), "partials64": p64.data_ptr(),
             "partials32": p32.data_ptr(), "outer_done": f}
        a.update(kw)
        kn.cg_refine_residual(**a, stream=_stream())

    with pytest.raises(Exception, match="nRows must be positive"):
        res(n_rows=0)
    for name in ("row_ptr", "col_ind", "val", "b", "x64", "r64", "r", "p", "partials64", "partials32", "outer_done"):
        with pytest.raises(Exception, match="null pointer"):
            res(**{name: 0})
    for name in ("dinv", "u"):
        with pytest.raises(Exception, match="dinv and u come together or not at all"):
            res(**{name: 0})
    with pytest.raises(Exception, match="4-byte aligned"):
        res(r=r.data_ptr() + 2)
    with pytest.raises(Exception, match="8-byte aligned"):
        res(r64=r64.data_ptr() + 4)
    with pytest.raises(Exception, match="must not overlap"):
        res(p=r.data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        res(r64=x64.data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        res(partials32=p64.data_ptr() + 8)

    d = _Decide(5, 3, 1.0)
    names = ("partials64", "partials32", "np", "tol2", "thresh", "done", "gamma", "alpha", "beta", "gamma_prev",
             "alpha_prev", "outer_thresh", "outer_done", "outer_steps", "outer_rr64")

    def dec(**kw):
        a = dict(zip(names, d.args(1e-10)[:-1]))
        a.update(kw)
        kn.cg_refine_decide(**a, stream=_stream())

    for bad in (0, SLAB + 1):
        with pytest.raises(Exception, match="1..256 partials"):
            dec(np=bad)
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(Exception, match="tol2 must be positive"):
            dec(tol2=bad)
    for name in names:
        if name not in ("np", "tol2"):
            with pytest.raises(Exception, match="null pointer"):
                dec(**{name: 0})
    with pytest.raises(Exception, match="8-byte aligned"):
        dec(thresh=d.thresh.data_ptr() + 4)
    # the outer state shares no byte with the inner solve's scalars and stop state
    with pytest.raises(Exception, match="must not overlap"):
        dec(outer_thresh=d.thresh.data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        dec(outer_done=d.flags.data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        dec(outer_rr64=d.scal[0:1].data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        dec(outer_steps=d.scal[3:4].data_ptr())
    with pytest.raises(Exception, match="must not overlap"):
        dec(gamma=d.scal[1:2].data_ptr())
    torch.cuda.synchronize()
    assert d.untouched_inner() and _np(d.o_flags).tolist() == [0, -9]  # nothing was launched
