"""The Jacobi-preconditioned pair of the single-reduction CG form (cg_kernels.hip):
``pcg_spmv_dot3``, ``pcg_update`` and their ``_stop`` forms.

Three oracles. With a unit diagonal (dinv = 1, u = r) the pair is the unpreconditioned pair, bit for
bit. With a general dinv (random in [2^-3, 2^3]) the SpMV has the bits of ``csr_spmv`` applied to u
and its three slabs are f64 dot products, and the update is the composition ``kernels.hpp`` states:
torch's f32 ``dinv * r``, ``xpay_dev_f32`` twice, ``axpy_dev_f32`` twice, torch's ``dinv * r_new``,
with beta and alpha from the host formula on the tree sums of the slabs. A stopping kernel is its
parent when it does not stop and writes nothing but gamma and ``done`` when it does.

Sizes: n % 4 in {0, 1, 3}, fewer elements than a quad, one block, 1024 (one full block of the
SpMV at one lane per row), several blocks, and 20 011; every vector aligned, and every vector 4
bytes past a 16-byte boundary."""
import numpy as np
import pytest

from cg_kernel_helpers import (NAN, SLAB, _check_dot, _f64, _host_scalars, _misaligned, _nan, _rand, _same_bits,
                               _stream, _tree_sum)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INF = float("inf")
SIZES = [1, 3, 4, 5, 255, 1024, 1037, 20_011]
GP0, AP0 = 0.8123, 0.37454011884736254  # gamma_prev, alpha_prev: the generic case of the parents' tests
DONE0, ITERS0 = 7, 41  # what done and iters hold before a launch
G_OUT0, A_OUT0 = 0.7310585786300049, 3.0e-9


def _i32(v):
    return torch.tensor(np.atleast_1d(v), dtype=torch.int32, device="cuda")


def _i64(v):
    return torch.tensor(np.atleast_1d(v), dtype=torch.int64, device="cuda")


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _place(t, misaligned):
    return _misaligned(t) if misaligned else t.clone()


def _matrix(tz, n):
    rp, ci, v = tz._tz.spd_band_matrix(n, min(n, 1037), min(5 * n, max(1, n * n // 2)), 1)
    return (torch.tensor(rp, dtype=torch.int32).cuda(), torch.tensor(ci, dtype=torch.int32).cuda(),
            torch.tensor(v, dtype=torch.float32).cuda())


def _dinv(n, seed=40):
    """random in [2^-3, 2^3]"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.exp2(6.0 * torch.rand(n, generator=g, dtype=torch.float64) - 3.0).float().cuda()


def _spmv3(kn, mat, r, u, lanes, done=None):
    """one pcg_spmv_dot3 (or _stop) launch into poisoned outputs: w, the three slabs, the prev pair"""
    n = r.numel()
    w, slabs = _nan(n, torch.float32), [_nan(SLAB + 8) for _ in range(3)]
    g_out, a_out, g_prev, a_prev = _f64(G_OUT0), _f64(A_OUT0), _nan(1), _nan(1)
    args = (n, *_ptrs(mat), r.data_ptr(), u.data_ptr(), w.data_ptr(), lanes, *_ptrs(slabs), g_out.data_ptr(),
            a_out.data_ptr(), g_prev.data_ptr(), a_prev.data_ptr())
    if done is None:
        kn.pcg_spmv_dot3(*args, _stream())
    else:
        kn.pcg_spmv_dot3_stop(*args, done.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert g_out.item() == G_OUT0 and a_out.item() == A_OUT0  # read only
    return w, *slabs, g_prev, a_prev


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_spmv_with_a_unit_diagonal_is_csr_spmv_dot2(tz, gpu, n, misaligned):
    kn = tz._tz.kernels
    mat = _matrix(tz, n)
    r = _place(_rand(n, 5), misaligned)
    u = _place(r, misaligned)
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W
        w0, pg0, pd0 = _nan(n, torch.float32), _nan(SLAB + 8), _nan(SLAB + 8)
        g_out, a_out, g_prev0, a_prev0 = _f64(G_OUT0), _f64(A_OUT0), _nan(1), _nan(1)
        kn.csr_spmv_dot2(n, *_ptrs(mat), r.data_ptr(), w0.data_ptr(), lanes, pg0.data_ptr(), pd0.data_ptr(),
                         g_out.data_ptr(), a_out.data_ptr(), g_prev0.data_ptr(), a_prev0.data_ptr(), _stream())
        torch.cuda.synchronize()
        w, pg, pd, pr, g_prev, a_prev = _spmv3(kn, mat, r, u, lanes)
        assert _same_bits(w, w0) and _same_bits(pg, pg0) and _same_bits(pd, pd0), W
        cnt = kn.spmv_dot_partial_count(n, lanes)
        assert _same_bits(pr[:cnt], pg[:cnt]) and torch.isnan(pr[cnt:]).all(), W
        assert _same_bits(g_prev, g_prev0) and _same_bits(a_prev, a_prev0) and g_prev.item() == G_OUT0


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_spmv_with_a_general_diagonal(tz, gpu, n, misaligned):
    kn = tz._tz.kernels
    mat = _matrix(tz, n)
    r = _place(_rand(n, 5), misaligned)
    u = _place(_dinv(n) * r, misaligned)
    assert not _same_bits(u, r)
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W
        ref = _nan(n, torch.float32)
        kn.csr_spmv(n, *_ptrs(mat), u.data_ptr(), ref.data_ptr(), lanes, False, _stream())
        runs = [_spmv3(kn, mat, r, u, lanes) for _ in range(2)]
        w, pg, pd, pr, g_prev, a_prev = runs[0]
        assert _same_bits(w, ref), W
        cnt = kn.spmv_dot_partial_count(n, lanes)
        _check_dot(pg, cnt, r, u, n)  # also: slots past the count are untouched NaN
        _check_dot(pd, cnt, u, w, n)
        _check_dot(pr, cnt, r, r, n)
        assert g_prev.item() == G_OUT0 and a_prev.item() == A_OUT0
        assert all(_same_bits(a, b) for a, b in zip(runs[0], runs[1]))  # two launches, the same bits


def _slabs(kn, n):
    """gamma, delta and rho slabs with known sums; slots past the count are NaN and must not be read"""
    cnt = kn.spmv_dot_partial_count(n, 4)
    pg, pd, pr = _nan(SLAB + 8), _nan(SLAB + 8), _nan(SLAB + 8)
    pg[:cnt] = _rand(cnt, 31, torch.float64).abs() + 0.1
    pd[:cnt] = _rand(cnt, 32, torch.float64).abs() + 2.0
    pr[:cnt] = _rand(cnt, 33, torch.float64).abs() + 0.5
    sums = [_tree_sum(t[:cnt].cpu().numpy()) for t in (pg, pd, pr)]
    return cnt, pg, pd, pr, sums


def _vectors(n, dinv, misaligned=False, only=None):
    """w, dinv, r, p, s, x, u with u poisoned: the update must not read it"""
    vs = [_rand(n, 20), dinv, _rand(n, 21), _rand(n, 22), _rand(n, 23), _rand(n, 24), _nan(n, torch.float32)]
    return [_place(t, misaligned and (only is None or only == i)) for i, t in enumerate(vs)]


def _update(kn, n, cnt, pg, pd, vecs, gp0=GP0, ap0=AP0):
    out = [_nan(1) for _ in range(3)]
    g_prev, a_prev = _f64(gp0), _f64(ap0)
    kn.pcg_update(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(), *_ptrs(vecs),
                  *_ptrs(out), _stream())
    torch.cuda.synchronize()
    assert g_prev.item() == gp0 and a_prev.item() == ap0  # read only
    return out


def _update_stop(kn, n, cnt, pg, pd, pr, vecs, thresh):
    out = [_nan(1) for _ in range(3)]
    g_prev, a_prev, th = _f64(GP0), _f64(AP0), _f64(thresh)
    done, iters = _i32(DONE0), _i64(ITERS0)
    kn.pcg_update_stop(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(), *_ptrs(vecs),
                       *_ptrs(out), pr.data_ptr(), th.data_ptr(), done.data_ptr(), iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert g_prev.item() == GP0 and a_prev.item() == AP0 and _same_bits(th, _f64(thresh))
    return out, done.item(), iters.item()


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_update_with_a_unit_diagonal_is_cg_sr_update(tz, gpu, n, misaligned):
    kn = tz._tz.kernels
    cnt, pg, pd, pr, sums = _slabs(kn, n)
    for gp0, ap0 in ((GP0, AP0), (0.0, 0.0)):
        got = _vectors(n, torch.ones(n, device="cuda"), misaligned)
        out = _update(kn, n, cnt, pg, pd, got, gp0, ap0)
        w, _, r, p, s, x, _ = _vectors(n, torch.ones(n, device="cuda"))
        want_out = [_nan(1) for _ in range(3)]
        g_prev, a_prev = _f64(gp0), _f64(ap0)
        kn.cg_sr_update(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(),
                        *_ptrs([w, r, p, s, x]), *_ptrs(want_out), _stream())
        torch.cuda.synchronize()
        assert all(_same_bits(a, b) for a, b in zip(out, want_out)), (gp0, ap0)
        for i, t in zip((0, 2, 3, 4, 5), (w, r, p, s, x)):
            assert _same_bits(got[i], t), (gp0, ap0, i)
        assert _same_bits(got[6], r)  # u = 1 * r
        assert _same_bits(got[1], torch.ones(n, device="cuda"))


@pytest.mark.parametrize("n", SIZES)
def test_update_with_a_general_diagonal_is_the_composition(tz, gpu, n):
    kn = tz._tz.kernels
    cnt, pg, pd, pr, (gamma, delta, rho) = _slabs(kn, n)
    dinv = _dinv(n)
    for gp0, ap0 in ((GP0, AP0), (0.0, AP0), (GP0, 0.0), (0.0, 0.0)):
        base = _vectors(n, dinv)
        got = [t.clone() for t in base]
        g_out, a_out, b_out = _update(kn, n, cnt, pg, pd, got, gp0, ap0)
        beta, alpha = _host_scalars(gamma, delta, gp0, ap0)
        assert g_out.item() == gamma and b_out.item() == beta and a_out.item() == alpha, (gp0, ap0)
        assert np.isfinite(alpha) and alpha != 0
        w, _, r, p, s, x, _ = [t.clone() for t in base]
        u_old = dinv * r  # torch's f32 product: one rounding
        kn.xpay_dev_f32(n, b_out.data_ptr(), u_old.data_ptr(), p.data_ptr(), _stream())
        kn.xpay_dev_f32(n, b_out.data_ptr(), w.data_ptr(), s.data_ptr(), _stream())
        kn.axpy_dev_f32(n, a_out.data_ptr(), 1, p.data_ptr(), x.data_ptr(), _stream())
        kn.axpy_dev_f32(n, a_out.data_ptr(), -1, s.data_ptr(), r.data_ptr(), _stream())
        torch.cuda.synchronize()
        u_new = dinv * r
        for i, t in zip((0, 1, 2, 3, 4, 5, 6), (w, dinv, r, p, s, x, u_new)):
            assert _same_bits(got[i], t), (gp0, ap0, "wdrpsxu"[i])
        assert not _same_bits(got[5], base[5]) and not _same_bits(got[2], base[2])
        assert not _same_bits(got[6], got[2])  # u is not r
        if gp0 == 0.0:  # the guard: beta = 0, so p = u_old and s = w
            assert beta == 0.0 and _same_bits(got[3], u_old) and _same_bits(got[4], w)
    # every vector in turn, and all of them, 4 bytes past a 16-byte boundary: the same bits
    want = [t.clone() for t in _vectors(n, dinv)]
    _update(kn, n, cnt, pg, pd, want)
    for only in (None, 0, 1, 2, 3, 4, 5, 6):
        got = _vectors(n, dinv, True, only)
        assert got[6 if only is None else only].data_ptr() % 16 == 4
        _update(kn, n, cnt, pg, pd, got)
        assert all(_same_bits(a, b) for a, b in zip(got, want)), only


@pytest.mark.parametrize("n", SIZES)
def test_update_stop_that_does_not_stop_is_the_parent(tz, gpu, n):
    kn = tz._tz.kernels
    cnt, pg, pd, pr, (gamma, delta, rho) = _slabs(kn, n)
    dinv = _dinv(n)
    want = _vectors(n, dinv)
    want_out = _update(kn, n, cnt, pg, pd, want)
    # the largest f64 below rho, zero, a disarmed threshold, NaN (which compares false), and, when it
    # lies below rho, gamma: the test is on rho = r . r, not on gamma = r . u
    for thresh in (np.nextafter(rho, 0.0), 0.0, -1.0, NAN) + ((gamma,) if gamma < rho else ()):
        for misaligned in (False, True):
            got = _vectors(n, dinv, misaligned)
            out, done, iters = _update_stop(kn, n, cnt, pg, pd, pr, got, thresh)
            assert all(_same_bits(a, b) for a, b in zip(got, want)), thresh
            assert all(_same_bits(a, b) for a, b in zip(out, want_out)), thresh
            assert done == 0 and iters == ITERS0 + 1, thresh
    # a NaN rho never stops, whatever the threshold
    pr[0] = NAN
    got = _vectors(n, dinv)
    out, done, iters = _update_stop(kn, n, cnt, pg, pd, pr, got, INF)
    assert all(_same_bits(a, b) for a, b in zip(got, want)) and all(_same_bits(a, b) for a, b in zip(out, want_out))
    assert done == 0 and iters == ITERS0 + 1


@pytest.mark.parametrize("n", SIZES)
def test_update_stop_that_stops_writes_nothing(tz, gpu, n):
    kn = tz._tz.kernels
    cnt, pg, pd, pr, (gamma, delta, rho) = _slabs(kn, n)
    dinv = _dinv(n)
    # rho itself (<= stops), the next f64 above, and, when it lies at or above rho, gamma
    for thresh in (rho, np.nextafter(rho, INF), 2.0 * rho, INF) + ((gamma,) if gamma >= rho else ()):
        for misaligned in (False, True):
            base = _vectors(n, dinv, misaligned)
            base[6].copy_(_rand(n, 25))  # a stopped update leaves u as it is
            got = [_place(t, misaligned) for t in base]
            out, done, iters = _update_stop(kn, n, cnt, pg, pd, pr, got, thresh)
            assert all(_same_bits(a, b) for a, b in zip(got, base)), thresh
            assert out[0].item() == gamma
            assert np.isnan(out[1].item()) and np.isnan(out[2].item())  # alpha and beta not published
            assert done == 1 and iters == ITERS0, thresh
    # zero slabs against a zero threshold (the system b = 0): 0 <= 0 stops
    for t in (pg, pd, pr):
        t[:cnt] = 0
    base = _vectors(n, dinv)
    got = [t.clone() for t in base]
    out, done, iters = _update_stop(kn, n, cnt, pg, pd, pr, got, 0.0)
    assert all(_same_bits(a, b) for a, b in zip(got, base))
    assert out[0].item() == 0.0 and done == 1 and iters == ITERS0


@pytest.mark.parametrize("n", [50, 1037, 20_011])
def test_spmv_stop(tz, gpu, n):
    """flag clear: pcg_spmv_dot3 bit for bit; flag set (by a stopped update): nothing is written"""
    kn = tz._tz.kernels
    mat = _matrix(tz, n)
    r = _rand(n, 5)
    u = _dinv(n) * r
    # a stopped update's flag, as the workload chains them
    cnt, pg, pd, pr, (gamma, delta, rho) = _slabs(kn, 65)
    out, done, iters = _update_stop(kn, 65, cnt, pg, pd, pr, _vectors(65, _dinv(65)), rho)
    assert done == 1
    done1 = _i32(done)
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W
        want = _spmv3(kn, mat, r, u, lanes)
        assert not torch.isnan(want[0]).any() and want[4].item() == G_OUT0
        clear = _i32(0)
        assert all(_same_bits(a, b) for a, b in zip(_spmv3(kn, mat, r, u, lanes, clear), want)), W
        assert clear.item() == 0  # read only
        for t in _spmv3(kn, mat, r, u, lanes, done1):  # w, the slabs and the previous scalars keep their poison
            assert torch.isnan(t).all(), W
        assert done1.item() == 1


def test_bad_arguments_raise(tz, gpu):
    kn = tz._tz.kernels
    n = 8
    vec = [torch.zeros(n, device="cuda") for _ in range(7)]  # w, dinv, r, p, s, x, u
    vp = _ptrs(vec)
    ap = vp[0]
    s = torch.zeros(3 * SLAB + 128, dtype=torch.float64, device="cuda")
    sp = s.data_ptr()
    pg, pd, pr = sp, sp + 8 * SLAB, sp + 16 * SLAB
    sc = [sp + 8 * (3 * SLAB + 8 * i) for i in range(8)]
    prev, outs, th, dn, it = sc[0:2], sc[2:5], sc[5], sc[6], sc[7]
    L = kn.SPMV_ILP + 4
    st = _stream()
    mat = [ap, ap, ap]  # never read: every call below raises before any launch
    r, u, w = vp[2], vp[6], vp[0]
    # pcg_spmv_dot3(n, rowPtr, colInd, val, r, u, w, lanes, slabs x 3, scalars x 4)
    kn_ok = (n, *mat, r, u, w, L, pg, pd, pr, outs[0], outs[1], prev[0], prev[1])
    for i in (4, 5, 6, 8, 9, 10):  # r, u, w and each slab null
        bad = list(kn_ok)
        bad[i] = 0
        with pytest.raises(Exception, match="pcg_spmv_dot3: .*null"):
            kn.pcg_spmv_dot3(*bad, st)
    with pytest.raises(Exception, match="pcg_spmv_dot3: lanes"):
        kn.pcg_spmv_dot3(n, *mat, r, u, w, 8, pg, pd, pr, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="null"):  # the four scalars come together
        kn.pcg_spmv_dot3(n, *mat, r, u, w, L, pg, pd, pr, outs[0], outs[1], prev[0], 0, st)
    for rr, uu in ((w, u), (r, w), (r, w + 4)):  # w on r, w on u, w one element into u
        with pytest.raises(Exception, match="pcg_spmv_dot3: .*overlap"):
            kn.pcg_spmv_dot3(n, *mat, rr, uu, w, L, pg, pd, pr, 0, 0, 0, 0, st)
    for slabs in ((pg, pd, pg), (pg, pd, pd), (pg, pg, pr)):
        with pytest.raises(Exception, match="overlap"):
            kn.pcg_spmv_dot3(n, *mat, r, u, w, L, *slabs, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="pcg_spmv_dot3_stop: .*null"):
        kn.pcg_spmv_dot3_stop(*kn_ok, 0, st)
    with pytest.raises(Exception, match="pcg_spmv_dot3_stop: .*alias"):
        kn.pcg_spmv_dot3_stop(*kn_ok, prev[1] + 4, st)
    # pcg_update(n, slabs x 2, np, prev x 2, w, dinv, r, p, s, x, u, out x 3)
    for i in range(7):
        bad = list(vp)
        bad[i] = 0
        with pytest.raises(Exception, match="pcg_update: .*null"):
            kn.pcg_update(n, pg, pd, 1, *prev, *bad, *outs, st)
    for i in range(7):  # every vector on each written one (r, p, s, x, u), whole or by one element
        for j in (2, 3, 4, 5, 6):
            if i != j:
                for off in (0, 4 * (n - 1)):
                    bad = list(vp)
                    bad[i] = vp[j] + off
                    with pytest.raises(Exception, match="pcg_update: .*overlap"):
                        kn.pcg_update(n, pg, pd, 1, *prev, *bad, *outs, st)
    for cnt in (0, SLAB + 1):
        with pytest.raises(Exception, match="pcg_update: .*partials"):
            kn.pcg_update(n, pg, pd, cnt, *prev, *vp, *outs, st)
    with pytest.raises(Exception, match="partials"):  # a null slab
        kn.pcg_update(n, 0, pd, 1, *prev, *vp, *outs, st)
    with pytest.raises(Exception, match="pcg_update: .*alias"):
        kn.pcg_update(n, pg, pd, 1, *prev, *vp, prev[0], outs[1], outs[2], st)
    with pytest.raises(Exception, match="pcg_update: .*alias"):
        kn.pcg_update(n, pg, pd, 1, *prev, *vp, outs[0], outs[0], outs[2], st)
    # pcg_update_stop(.., out x 3, partials_rho, thresh, done, iters)
    with pytest.raises(Exception, match="pcg_update_stop: .*partials"):
        kn.pcg_update_stop(n, pg, pd, 1, *prev, *vp, *outs, 0, th, dn, it, st)
    for i in range(3):
        own = [th, dn, it]
        own[i] = 0
        with pytest.raises(Exception, match="pcg_update_stop: .*null"):
            kn.pcg_update_stop(n, pg, pd, 1, *prev, *vp, *outs, pr, *own, st)
    for other in prev + outs:  # thresh, done and iters against each of the five scalars
        for i in range(3):
            own = [th, dn, it]
            own[i] = other + (4 if i == 1 else 0)
            with pytest.raises(Exception, match="alias"):
                kn.pcg_update_stop(n, pg, pd, 1, *prev, *vp, *outs, pr, *own, st)
    with pytest.raises(Exception, match="alias each other"):
        kn.pcg_update_stop(n, pg, pd, 1, *prev, *vp, *outs, pr, th, th + 4, it, st)
    torch.cuda.synchronize()
    assert not s.any() and not any(t.any() for t in vec)  # nothing was launched
