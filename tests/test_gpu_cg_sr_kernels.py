"""The two kernels of the single-reduction CG form (cg_kernels.hip): ``csr_spmv_dot2`` against
``csr_spmv`` (bit for bit) and f64 dot products, ``cg_sr_update`` against the host formula for
beta and alpha (bit for bit) and against the plain kernels it replaces (bit for bit).

Sizes as in test_gpu_cg_kernels.py: 70 001 rows is the smallest case in which 4 lanes per row
take a second, ragged grid-stride pass; 300 007 elements the smallest second pass of the vector
layout."""
import numpy as np
import pytest

from cg_kernel_helpers import (SLAB, _check_dot, _f64, _host_scalars, _misaligned, _nan_slab, _rand, _same_bits,
                               _stream, _tree_sum)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [1, 63, 64, 65, 257, 1037, 300_007]


@pytest.mark.parametrize("n,bw", [(50, 8), (257, 16), (1037, 1037), (70_001, 16)])
def test_csr_spmv_dot2(tz, gpu, n, bw):
    k = tz._tz.kernels
    rp, ci, v = tz._tz.spd_band_matrix(n, bw, 5 * n, 1)
    rp = torch.tensor(rp, dtype=torch.int32).cuda()
    ci = torch.tensor(ci, dtype=torch.int32).cuda()
    v = torch.tensor(v, dtype=torch.float32).cuda()
    r = _rand(n, 5)
    g_out0, a_out0 = 0.7310585786300049, 3.0e-9
    for W in (1, 2, 4):
        lanes = k.SPMV_ILP + W
        ref = torch.full((n,), float("nan"), device="cuda")
        k.csr_spmv(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), r.data_ptr(), ref.data_ptr(), lanes, False,
                   _stream())
        g_out, a_out = _f64(g_out0), _f64(a_out0)
        runs = []
        for _ in range(2):
            w = torch.full((n,), float("nan"), device="cuda")
            pg, pd = _nan_slab(), _nan_slab()
            g_prev, a_prev = _f64(float("nan")), _f64(float("nan"))
            k.csr_spmv_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), r.data_ptr(), w.data_ptr(), lanes,
                            pg.data_ptr(), pd.data_ptr(), g_out.data_ptr(), a_out.data_ptr(), g_prev.data_ptr(),
                            a_prev.data_ptr(), _stream())
            torch.cuda.synchronize()
            runs.append((w, pg, pd, g_prev, a_prev))
        w, pg, pd, g_prev, a_prev = runs[0]
        assert _same_bits(w, ref)
        cnt = k.spmv_dot_partial_count(n, lanes)
        assert cnt == min(SLAB, max(1, -(-n * W // 1024)))
        _check_dot(pg, cnt, r, r, n)
        _check_dot(pd, cnt, r, w, n)
        # the scalar move is bit-exact and leaves its sources alone
        assert _same_bits(g_prev, g_out) and _same_bits(a_prev, a_out)
        assert g_out.item() == g_out0 and a_out.item() == a_out0
        # two launches give the same bits
        assert all(_same_bits(a, b) for a, b in zip(runs[0], runs[1]))
        # without the scalar pointers nothing else changes
        w2, pg2, pd2 = torch.full((n,), float("nan"), device="cuda"), _nan_slab(), _nan_slab()
        k.csr_spmv_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), r.data_ptr(), w2.data_ptr(), lanes,
                        pg2.data_ptr(), pd2.data_ptr(), 0, 0, 0, 0, _stream())
        torch.cuda.synchronize()
        assert _same_bits(w, w2) and _same_bits(pg, pg2) and _same_bits(pd, pd2)
    if n == 70_001:
        assert n * 4 > SLAB * 1024  # the second pass exists


def _update(k, n, pg, pd, cnt, g_prev, a_prev, w, r, p, s, x):
    """one cg_sr_update launch on the given tensors (r, p, s, x are updated in place); returns
    the published (gamma, alpha, beta) tensors"""
    out = [_f64(float("nan")) for _ in range(3)]
    k.cg_sr_update(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(), w.data_ptr(),
                   r.data_ptr(), p.data_ptr(), s.data_ptr(), x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                   out[2].data_ptr(), _stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", SIZES)
def test_cg_sr_update(tz, gpu, n):
    k = tz._tz.kernels
    w, r, p, s, x = (_rand(n, 20 + i) for i in range(5))
    cnt = k.spmv_dot_partial_count(n, 4)
    pg, pd = _nan_slab(), _nan_slab()  # slots past the count must not be read
    pg[:cnt] = _rand(cnt, 31, torch.float64).abs() + 0.1
    pd[:cnt] = _rand(cnt, 32, torch.float64).abs() + 2.0
    gamma, delta = _tree_sum(pg[:cnt].cpu().numpy()), _tree_sum(pd[:cnt].cpu().numpy())
    for gp0, ap0 in ((0.8123, 0.37454011884736254), (0.0, 0.37454011884736254), (0.8123, 0.0), (0.0, 0.0)):
        g_prev, a_prev = _f64(gp0), _f64(ap0)
        r1, p1, s1, x1 = r.clone(), p.clone(), s.clone(), x.clone()
        g_out, a_out, b_out = _update(k, n, pg, pd, cnt, g_prev, a_prev, w, r1, p1, s1, x1)
        # the published scalars are the host formula on the kernels' sums, bit for bit
        beta, alpha = _host_scalars(gamma, delta, gp0, ap0)
        assert g_out.item() == gamma
        assert b_out.item() == beta, (gp0, ap0)
        assert a_out.item() == alpha, (gp0, ap0)
        assert np.isfinite(alpha) and alpha != 0
        assert g_prev.item() == gp0 and a_prev.item() == ap0  # read only
        # the vectors are the plain kernels' with the published scalars
        r2, p2, s2, x2 = r.clone(), p.clone(), s.clone(), x.clone()
        k.xpay_dev_f32(n, b_out.data_ptr(), r2.data_ptr(), p2.data_ptr(), _stream())
        k.xpay_dev_f32(n, b_out.data_ptr(), w.data_ptr(), s2.data_ptr(), _stream())
        k.axpy_dev_f32(n, a_out.data_ptr(), 1, p2.data_ptr(), x2.data_ptr(), _stream())
        k.axpy_dev_f32(n, a_out.data_ptr(), -1, s2.data_ptr(), r2.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert _same_bits(p1, p2) and _same_bits(s1, s2) and _same_bits(x1, x2) and _same_bits(r1, r2)
        assert not _same_bits(x1, x) and not _same_bits(r1, r)
        if gp0 == 0.0:  # the guard: beta = 0, so p = r and s = w
            assert beta == 0.0 and _same_bits(p1, r) and _same_bits(s1, w)
        else:
            assert not _same_bits(p1, r) and not _same_bits(s1, w)
    # misaligned copies of each vector give the same bits (generic scalars: the last r1.. hold
    # the (0, 0) case, so run the generic one again as the reference)
    g_prev, a_prev = _f64(0.8123), _f64(0.37454011884736254)
    want = [t.clone() for t in (w, r, p, s, x)]
    _update(k, n, pg, pd, cnt, g_prev, a_prev, *want)
    for i in range(5):
        got = [t.clone() for t in (w, r, p, s, x)]
        got[i] = _misaligned(got[i])
        _update(k, n, pg, pd, cnt, g_prev, a_prev, *got)
        assert all(_same_bits(a, b) for a, b in zip(got, want)), i
    # zero slabs: alpha = 0 (guarded), x and r unchanged
    pg[:cnt] = 0
    pd[:cnt] = 0
    got = [t.clone() for t in (w, r, p, s, x)]
    g_out, a_out, b_out = _update(k, n, pg, pd, cnt, g_prev, a_prev, *got)
    assert g_out.item() == 0.0 and a_out.item() == 0.0 and b_out.item() == 0.0
    assert _same_bits(got[1], r) and _same_bits(got[4], x)
    if n == 300_007:
        assert n // 4 > SLAB * 256  # the second pass exists


def test_bad_arguments_raise(tz, gpu):
    k = tz._tz.kernels
    a = torch.zeros(8, device="cuda")
    s = torch.zeros(SLAB + 8, dtype=torch.float64, device="cuda")
    ap, sp = a.data_ptr(), s.data_ptr()
    sc = [sp + 8 * (SLAB + i) for i in range(5)]  # five distinct scalars past the slab
    s2 = torch.zeros(SLAB, dtype=torch.float64, device="cuda").data_ptr()
    with pytest.raises(Exception, match="lanes"):
        k.csr_spmv_dot2(8, ap, ap, ap, ap, ap, 8, sp, s2, 0, 0, 0, 0, _stream())
    with pytest.raises(Exception, match="null"):
        k.csr_spmv_dot2(8, ap, ap, ap, ap, ap, k.SPMV_ILP + 4, sp, 0, 0, 0, 0, 0, _stream())
    with pytest.raises(Exception, match="null"):  # the four scalars come together
        k.csr_spmv_dot2(8, ap, ap, ap, ap, ap, k.SPMV_ILP + 4, sp, s2, sc[0], sc[1], sc[2], 0, _stream())
    with pytest.raises(Exception, match="partials"):
        k.cg_sr_update(8, sp, s2, SLAB + 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[3], sc[4], _stream())
    with pytest.raises(Exception, match="null"):
        k.cg_sr_update(8, sp, s2, 1, sc[0], sc[1], ap, ap, ap, 0, ap, sc[2], sc[3], sc[4], _stream())
    with pytest.raises(Exception, match="null"):
        k.cg_sr_update(8, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[3], 0, _stream())
    with pytest.raises(Exception, match="alias"):
        k.cg_sr_update(8, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[0], sc[3], sc[4], _stream())
