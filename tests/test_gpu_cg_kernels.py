"""The conjugate-gradient kernels (cg_kernels.hip) against f64 references: dot-product partials,
the one-block scalar kernels, vector updates with a device scalar, the fused SpMV + dot and the
fused updates against the plain kernels they replace (bit for bit).

Sizes: one lane, either side of a wave, a partial block, fewer elements than partial slots, and
several grid-stride passes with a ragged tail (300 007 > 256 blocks x 1024 elements)."""
import math

import numpy as np
import pytest

from cg_kernel_helpers import SLAB, _check_dot, _misaligned, _nan_slab, _rand, _same_bits, _stream, _tree_sum

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [1, 63, 64, 65, 257, 1037, 300_007]


@pytest.mark.parametrize("n", SIZES)
def test_dot_partials(tz, gpu, n):
    k = tz._tz.kernels
    u, v = _rand(n, 1), _rand(n, 2)
    cnt = k.dot_partial_count(n)
    assert cnt == min(SLAB, max(1, -(-n // 1024)))
    a, b = _nan_slab(), _nan_slab()
    k.dot_partials_f32(n, u.data_ptr(), v.data_ptr(), a.data_ptr(), _stream())
    k.dot_partials_f32(n, u.data_ptr(), v.data_ptr(), b.data_ptr(), _stream())
    torch.cuda.synchronize()
    _check_dot(a, cnt, u, v, n)
    assert _same_bits(a, b)
    # the same partials from vectors that are not 16-byte aligned, and for u . u
    c = _nan_slab()
    k.dot_partials_f32(n, _misaligned(u).data_ptr(), v.data_ptr(), c.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _same_bits(a, c)
    d = _nan_slab()
    k.dot_partials_f32(n, u.data_ptr(), u.data_ptr(), d.data_ptr(), _stream())
    torch.cuda.synchronize()
    _check_dot(d, cnt, u, u, n)


@pytest.mark.parametrize("cnt", [1, 5, 64, 147, 256])
def test_alpha_beta_match_host_arithmetic(tz, gpu, cnt):
    k = tz._tz.kernels
    slab = _nan_slab()  # slots past the count must not be read: they would poison the sum
    part = _rand(cnt, 10 + cnt, torch.float64)
    slab[:cnt] = part
    want = _tree_sum(part.cpu().numpy())
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    k.sum_partials_f64(slab.data_ptr(), cnt, out.data_ptr(), _stream())
    assert out.item() == want
    for rr0 in (0.7310585786300049, 3.0e-9, 0.0):
        rr = torch.tensor([rr0], dtype=torch.float64, device="cuda")
        alpha = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        k.cg_alpha(slab.data_ptr(), cnt, rr.data_ptr(), alpha.data_ptr(), _stream())
        assert alpha.item() == (rr0 / want if want != 0 else 0.0)
        assert rr.item() == rr0
        beta = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        k.cg_beta(slab.data_ptr(), cnt, rr.data_ptr(), beta.data_ptr(), _stream())
        assert beta.item() == (want / rr0 if rr0 != 0 else 0.0)  # the rr == 0 guard
        assert rr.item() == want
    # the pq == 0 guard
    slab[:cnt] = 0
    rr = torch.tensor([2.5], dtype=torch.float64, device="cuda")
    alpha = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    k.cg_alpha(slab.data_ptr(), cnt, rr.data_ptr(), alpha.data_ptr(), _stream())
    assert alpha.item() == 0.0
    beta = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    k.cg_beta(slab.data_ptr(), cnt, rr.data_ptr(), beta.data_ptr(), _stream())
    assert beta.item() == 0.0 and rr.item() == 0.0


def _ulps(a, b):
    def ordered(t):
        i = t.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs().max().item()


@pytest.mark.parametrize("n", SIZES)
def test_axpy_xpay_with_a_device_scalar(tz, gpu, n):
    k = tz._tz.kernels
    x, y = _rand(n, 3), _rand(n, 4)
    for s0 in (0.37454011884736254, -1.9507143064099162):
        s = torch.tensor([s0], dtype=torch.float64, device="cuda")
        sf = float(np.float32(s0))
        for sign in (1, -1):
            got = y.clone()
            k.axpy_dev_f32(n, s.data_ptr(), sign, x.data_ptr(), got.data_ptr(), _stream())
            ref = (y.double() + sign * sf * x.double()).float()
            assert _ulps(got, ref) <= 1  # one fma rounding against a double rounding
            off = y.clone()
            k.axpy_dev_f32(n, s.data_ptr(), sign, _misaligned(x).data_ptr(), off.data_ptr(), _stream())
            assert _same_bits(got, off)
            dst = _misaligned(y)
            k.axpy_dev_f32(n, s.data_ptr(), sign, x.data_ptr(), dst.data_ptr(), _stream())
            assert _same_bits(got, dst)
        got = y.clone()
        k.xpay_dev_f32(n, s.data_ptr(), x.data_ptr(), got.data_ptr(), _stream())
        ref = (x.double() + sf * y.double()).float()
        assert _ulps(got, ref) <= 1
        off = y.clone()
        k.xpay_dev_f32(n, s.data_ptr(), _misaligned(x).data_ptr(), off.data_ptr(), _stream())
        assert _same_bits(got, off)


# the generator shapes of test_cg_graph.py, and one whose rows x 4 lanes exceed 256 blocks of
# 1024 threads, so that csr_spmv_dot's grid-stride loop takes a second, ragged pass
@pytest.mark.parametrize("n,bw", [(50, 8), (257, 16), (1037, 1037), (70_001, 16)])
def test_csr_spmv_dot(tz, gpu, n, bw):
    k = tz._tz.kernels
    rp, ci, v = tz._tz.spd_band_matrix(n, bw, 5 * n, 1)
    rp = torch.tensor(rp, dtype=torch.int32).cuda()
    ci = torch.tensor(ci, dtype=torch.int32).cuda()
    v = torch.tensor(v, dtype=torch.float32).cuda()
    p = _rand(n, 5)
    prr = _nan_slab()
    rr_part = _rand(7, 6, torch.float64).abs()
    prr[:7] = rr_part
    for W in (1, 2, 4):
        lanes = k.SPMV_ILP + W
        ref = torch.full((n,), float("nan"), device="cuda")
        k.csr_spmv(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), p.data_ptr(), ref.data_ptr(), lanes, False,
                   _stream())
        q = torch.full((n,), float("nan"), device="cuda")
        pq = _nan_slab()
        rr = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        k.csr_spmv_dot(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), p.data_ptr(), q.data_ptr(), lanes,
                       pq.data_ptr(), prr.data_ptr(), 7, rr.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert _same_bits(q, ref)
        cnt = k.spmv_dot_partial_count(n, lanes)
        assert cnt == min(SLAB, max(1, -(-n * W // 1024)))
        _check_dot(pq, cnt, p, q, n)
        assert rr.item() == _tree_sum(rr_part.cpu().numpy())
        # without the rr slab nothing else changes, and rr is left alone
        q2, pq2 = torch.full((n,), float("nan"), device="cuda"), _nan_slab()
        k.csr_spmv_dot(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), p.data_ptr(), q2.data_ptr(), lanes,
                       pq2.data_ptr(), 0, 0, 0, _stream())
        torch.cuda.synchronize()
        assert _same_bits(q, q2) and _same_bits(pq, pq2)
    if n == 70_001:
        assert n * 4 > SLAB * 1024  # the second pass exists


@pytest.mark.parametrize("n", SIZES)
def test_fused_updates_equal_their_plain_compositions(tz, gpu, n):
    k = tz._tz.kernels
    p, q, x, r = _rand(n, 7), _rand(n, 8), _rand(n, 9), _rand(n, 10)
    cnt = k.spmv_dot_partial_count(n, 4)
    pq = _nan_slab()
    pq[:cnt] = _rand(cnt, 11, torch.float64).abs() + 0.1
    rr = torch.tensor([0.8123], dtype=torch.float64, device="cuda")
    alpha = torch.zeros(1, dtype=torch.float64, device="cuda")
    k.cg_alpha(pq.data_ptr(), cnt, rr.data_ptr(), alpha.data_ptr(), _stream())
    assert math.isfinite(alpha.item()) and alpha.item() != 0
    # x += alpha p
    x1, x2 = x.clone(), x.clone()
    k.axpy_dev_f32(n, alpha.data_ptr(), 1, p.data_ptr(), x1.data_ptr(), _stream())
    k.cg_fused_x(n, pq.data_ptr(), cnt, rr.data_ptr(), p.data_ptr(), x2.data_ptr(), _stream())
    assert _same_bits(x1, x2) and not _same_bits(x1, x)
    # r -= alpha q and the partials of the new r . r
    r1, r2, s1, s2 = r.clone(), r.clone(), _nan_slab(), _nan_slab()
    k.axpy_dev_f32(n, alpha.data_ptr(), -1, q.data_ptr(), r1.data_ptr(), _stream())
    k.dot_partials_f32(n, r1.data_ptr(), r1.data_ptr(), s1.data_ptr(), _stream())
    k.cg_fused_r(n, pq.data_ptr(), cnt, rr.data_ptr(), q.data_ptr(), r2.data_ptr(), s2.data_ptr(), _stream())
    assert _same_bits(r1, r2) and not _same_bits(r1, r)
    assert _same_bits(s1, s2)
    nv = k.dot_partial_count(n)
    _check_dot(s2, nv, r2, r2, n)
    # p = r + beta p; the fused kernel leaves rr alone, cg_beta moves it on
    p1, p2 = p.clone(), p.clone()
    rr1 = rr.clone()
    beta = torch.zeros(1, dtype=torch.float64, device="cuda")
    k.cg_beta(s1.data_ptr(), nv, rr1.data_ptr(), beta.data_ptr(), _stream())
    k.xpay_dev_f32(n, beta.data_ptr(), r1.data_ptr(), p1.data_ptr(), _stream())
    k.cg_fused_p(n, s2.data_ptr(), nv, rr.data_ptr(), r2.data_ptr(), p2.data_ptr(), _stream())
    assert _same_bits(p1, p2) and not _same_bits(p1, p)
    assert rr.item() == 0.8123 and rr1.item() == _tree_sum(s1[:nv].cpu().numpy())
    # both guards: a zero pq slab leaves x and r unchanged, a zero rr leaves p = r
    pq[:cnt] = 0
    x3, r3, s3 = x.clone(), r.clone(), _nan_slab()
    k.cg_fused_x(n, pq.data_ptr(), cnt, rr.data_ptr(), p.data_ptr(), x3.data_ptr(), _stream())
    k.cg_fused_r(n, pq.data_ptr(), cnt, rr.data_ptr(), q.data_ptr(), r3.data_ptr(), s3.data_ptr(), _stream())
    assert _same_bits(x3, x) and _same_bits(r3, r)
    zero = torch.zeros(1, dtype=torch.float64, device="cuda")
    p3 = p.clone()
    k.cg_fused_p(n, s3.data_ptr(), nv, zero.data_ptr(), r.data_ptr(), p3.data_ptr(), _stream())
    assert _same_bits(p3, r)


def test_bad_arguments_raise(tz, gpu):
    k = tz._tz.kernels
    a = torch.zeros(8, device="cuda")
    s = torch.zeros(SLAB, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception, match="partials"):
        k.cg_alpha(s.data_ptr(), SLAB + 1, s.data_ptr(), s.data_ptr(), _stream())
    with pytest.raises(Exception, match="sign"):
        k.axpy_dev_f32(8, s.data_ptr(), 2, a.data_ptr(), a.data_ptr(), _stream())
    with pytest.raises(Exception, match="lanes"):
        k.csr_spmv_dot(8, a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), 8,
                       s.data_ptr(), 0, 0, 0, _stream())
