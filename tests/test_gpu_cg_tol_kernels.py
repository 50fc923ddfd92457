"""The four stopping kernels of the single-reduction CG form (cg_kernels.hip): ``cg_sr_update_stop``,
``csr_spmv_dot2_stop`` and their batched forms. The oracle is the kernel each one extends, bit for
bit: with the threshold below gamma (or the flag clear) every output equals the parent kernel's;
with the threshold at or above gamma (or the flag set) nothing but ``done`` and gamma is written,
which poisoned outputs show. The parents are held to their own references by
test_gpu_cg_sr_kernels.py and test_gpu_cg_batch_kernels.py, whose helpers and shapes these tests use.

Sizes: n % 4 in {1, 2, 3}, one block (n <= 1024 elements), several blocks, and 300 007 elements
(150 005 / 75 003 / 37 503 rows for k = 2 / 4 / 8), the smallest second pass of 256 blocks; for the
SpMV 70 001 rows, the smallest ragged second pass of 4 lanes per row."""
import numpy as np
import pytest

from cg_kernel_helpers import NAN, SLAB, _f64, _misaligned, _nan, _rand, _same_bits, _stream, _tree_sum
from test_gpu_cg_batch_kernels import KS, SECOND_PASS, _matrix, _slabs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INF = float("inf")
SIZES = [1, 63, 65, 1038, 300_007]  # n % 4 = 1, 3, 1, 2, 3
GP0, AP0 = 0.8123, 0.37454011884736254  # gamma_prev, alpha_prev: the generic case of the parents' tests
DONE0, ITERS0 = 7, 41  # what done and iters hold before a launch


def _i32(v):
    return torch.tensor(np.atleast_1d(v), dtype=torch.int32, device="cuda")


def _i64(v):
    return torch.tensor(np.atleast_1d(v), dtype=torch.int64, device="cuda")


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _update_stop(kn, n, pg, pd, cnt, vecs, thresh):
    """one cg_sr_update_stop launch on `vecs` = (w, r, p, s, x), in place; returns the published
    (gamma, alpha, beta), NaN before the launch, and done, iters"""
    out = [_nan(1) for _ in range(3)]
    g_prev, a_prev, th = _f64(GP0), _f64(AP0), _f64(thresh)
    done, iters = _i32(DONE0), _i64(ITERS0)
    kn.cg_sr_update_stop(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(), *_ptrs(vecs),
                         *_ptrs(out), th.data_ptr(), done.data_ptr(), iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert g_prev.item() == GP0 and a_prev.item() == AP0  # read only
    assert _same_bits(th, _f64(thresh))
    return out, done.item(), iters.item()


def _update_parent(kn, n, pg, pd, cnt, vecs):
    out = [_nan(1) for _ in range(3)]
    g_prev, a_prev = _f64(GP0), _f64(AP0)
    kn.cg_sr_update(n, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(), *_ptrs(vecs),
                    *_ptrs(out), _stream())
    torch.cuda.synchronize()
    return out


def _single_case(kn, n):
    base = [_rand(n, 20 + i) for i in range(5)]  # w, r, p, s, x
    cnt = kn.spmv_dot_partial_count(n, 4)
    pg, pd = _nan(SLAB + 8), _nan(SLAB + 8)  # slots past the count must not be read
    pg[:cnt] = _rand(cnt, 31, torch.float64).abs() + 0.1
    pd[:cnt] = _rand(cnt, 32, torch.float64).abs() + 2.0
    return base, cnt, pg, pd, _tree_sum(pg[:cnt].cpu().numpy())


@pytest.mark.parametrize("n", SIZES)
def test_update_with_the_threshold_below_gamma_is_the_parent(tz, gpu, n):
    kn = tz._tz.kernels
    base, cnt, pg, pd, gamma = _single_case(kn, n)
    want = [t.clone() for t in base]
    want_out = _update_parent(kn, n, pg, pd, cnt, want)
    assert want_out[0].item() == gamma
    assert not _same_bits(want[4], base[4]) and not _same_bits(want[1], base[1])
    # the largest f64 below gamma, zero, a disarmed threshold, and NaN (which compares false)
    for thresh in (np.nextafter(gamma, 0.0), 0.0, -1.0, NAN):
        got = [t.clone() for t in base]
        out, done, iters = _update_stop(kn, n, pg, pd, cnt, got, thresh)
        assert all(_same_bits(a, b) for a, b in zip(got, want)), thresh
        assert all(_same_bits(a, b) for a, b in zip(out, want_out)), thresh
        assert done == 0 and iters == ITERS0 + 1, thresh
    # a misaligned copy of each vector gives the same bits
    for i in range(5):
        got = [t.clone() for t in base]
        got[i] = _misaligned(got[i])
        out, done, iters = _update_stop(kn, n, pg, pd, cnt, got, 0.0)
        assert all(_same_bits(a, b) for a, b in zip(got, want)), i
    # a NaN gamma never stops, whatever the threshold
    pg[0] = NAN
    want = [t.clone() for t in base]
    want_out = _update_parent(kn, n, pg, pd, cnt, want)
    got = [t.clone() for t in base]
    out, done, iters = _update_stop(kn, n, pg, pd, cnt, got, INF)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(_same_bits(a, b) for a, b in zip(out, want_out)) and np.isnan(out[0].item())
    assert done == 0 and iters == ITERS0 + 1
    if n == 300_007:
        assert n // 4 > SLAB * 256  # the second pass exists


@pytest.mark.parametrize("n", SIZES)
def test_update_with_the_threshold_at_or_above_gamma_writes_nothing(tz, gpu, n):
    kn = tz._tz.kernels
    base, cnt, pg, pd, gamma = _single_case(kn, n)
    for thresh in (gamma, np.nextafter(gamma, INF), 2.0 * gamma, INF):  # gamma itself: <= stops
        got = [t.clone() for t in base]
        out, done, iters = _update_stop(kn, n, pg, pd, cnt, got, thresh)
        assert all(_same_bits(a, b) for a, b in zip(got, base)), thresh  # w, r, p, s, x
        assert out[0].item() == gamma
        assert np.isnan(out[1].item()) and np.isnan(out[2].item())  # alpha and beta not published
        assert done == 1 and iters == ITERS0, thresh
    # zero slabs against a zero threshold (the system b = 0): 0 <= 0 stops
    pg[:cnt] = 0
    pd[:cnt] = 0
    got = [t.clone() for t in base]
    out, done, iters = _update_stop(kn, n, pg, pd, cnt, got, 0.0)
    assert all(_same_bits(a, b) for a, b in zip(got, base))
    assert out[0].item() == 0.0 and done == 1 and iters == ITERS0


@pytest.mark.parametrize("n,bw", [(50, 8), (1037, 1037), (70_001, 16)])
def test_spmv_stop(tz, gpu, n, bw):
    """flag clear: csr_spmv_dot2 bit for bit; flag set (by a stopped update): nothing is written"""
    kn = tz._tz.kernels
    rp, ci, v = _matrix(tz, n, bw)
    r = _rand(n, 5)
    g_out, a_out = _f64(0.7310585786300049), _f64(3.0e-9)
    # a stopped update's flag, as the workload chains them
    base, cnt1, pg1, pd1, gamma1 = _single_case(kn, 65)
    done1 = _i32(DONE0)
    keep = [_f64(GP0), _f64(AP0), *base, _nan(1), _nan(1), _nan(1), _f64(gamma1), done1, _i64(0)]
    kn.cg_sr_update_stop(65, pg1.data_ptr(), pd1.data_ptr(), cnt1, *_ptrs(keep), _stream())
    torch.cuda.synchronize()
    assert done1.item() == 1
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W

        def launch(stop):
            w, pg, pd = _nan(n, torch.float32), _nan(SLAB + 8), _nan(SLAB + 8)
            g_prev, a_prev = _nan(1), _nan(1)
            args = (n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), r.data_ptr(), w.data_ptr(), lanes, pg.data_ptr(),
                    pd.data_ptr(), g_out.data_ptr(), a_out.data_ptr(), g_prev.data_ptr(), a_prev.data_ptr())
            if stop is None:
                kn.csr_spmv_dot2(*args, _stream())
            else:
                kn.csr_spmv_dot2_stop(*args, stop.data_ptr(), _stream())
            torch.cuda.synchronize()
            return w, pg, pd, g_prev, a_prev

        want = launch(None)
        assert not torch.isnan(want[0]).any() and want[3].item() == g_out.item()
        clear = _i32(0)
        assert all(_same_bits(a, b) for a, b in zip(launch(clear), want)), W
        assert clear.item() == 0  # read only
        for t in launch(done1):  # w, both slabs and the previous scalars keep their poison
            assert torch.isnan(t).all(), W
        assert done1.item() == 1
    if n == 70_001:
        assert n * 4 > SLAB * 1024 and (n * 4) % (SLAB * 1024) != 0  # a ragged second pass


def _batch_stop(kn, n, k, pg, pd, cnt, vecs, thresh):
    """one cg_sr_update_batch_stop launch; every array has two guard slots past k"""
    out = [_nan(k + 2) for _ in range(3)]
    g_prev, a_prev = _f64([GP0] * k), _f64([AP0] * k)
    th = _f64(list(thresh) + [NAN, NAN])
    done, iters, all_done = _i32([DONE0] * (k + 2)), _i64([ITERS0 + j for j in range(k + 2)]), _i32([DONE0, DONE0])
    kn.cg_sr_update_batch_stop(n, k, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(),
                               *_ptrs(vecs), *_ptrs(out), th.data_ptr(), done.data_ptr(), iters.data_ptr(),
                               all_done.data_ptr(), _stream())
    torch.cuda.synchronize()
    for o in out:
        assert torch.isnan(o[k:]).all()
    assert done[k:].tolist() == [DONE0, DONE0] and iters[k:].tolist() == [ITERS0 + k, ITERS0 + k + 1]
    assert all_done[1].item() == DONE0
    return [o[:k] for o in out], done[:k].tolist(), iters[:k].tolist(), all_done[0].item()


@pytest.mark.parametrize("k,n", [(k, n) for k in KS for n in (1, 63, 64, 65, 1037, SECOND_PASS[k])])
def test_update_batch_stop(tz, gpu, k, n):
    """per-column thresholds: a stopped column is untouched, a running one is what the single
    stopping kernel makes of its contiguous copy, all_done is the AND. n odd with k = 2 leaves a
    two-element tail, one element per column."""
    kn = tz._tz.kernels
    base = [_rand((n, k), 20 + i) for i in range(5)]  # w, r, p, s, x
    cnt = kn.spmv_dot_partial_count(n, 4)
    pg, pd = _slabs(k, cnt, 31)
    gamma = [_tree_sum(pg[j * SLAB:j * SLAB + cnt].cpu().numpy()) for j in range(k)]
    # the running columns' oracle, once per column: the single kernel with the threshold below gamma
    single = []
    for j in range(k):
        cols = [t[:, j].clone(memory_format=torch.contiguous_format) for t in base]
        out, done, iters = _update_stop(kn, n, pg[j * SLAB:], pd[j * SLAB:], cnt, cols, np.nextafter(gamma[j], 0.0))
        assert done == 0 and iters == ITERS0 + 1
        single.append((cols, out))
    masks = [[j % 2 == 0 for j in range(k)], [j % 2 == 1 for j in range(k)], [j != k - 1 for j in range(k)],
             [False] * k, [True] * k]  # True: the column stops
    for stop in masks:
        # a stopping column's threshold is its gamma exactly, a running one's the next f64 below
        thresh = [gamma[j] if stop[j] else np.nextafter(gamma[j], 0.0) for j in range(k)]
        got = [t.clone() for t in base]
        (g_out, a_out, b_out), done, iters, all_done = _batch_stop(kn, n, k, pg, pd, cnt, got, thresh)
        assert _same_bits(got[0], base[0])  # w is read only
        assert done == [int(s) for s in stop]
        assert iters == [ITERS0 + j + (0 if stop[j] else 1) for j in range(k)]
        assert all_done == int(all(stop))
        for j in range(k):
            assert g_out[j].item() == gamma[j], (stop, j)
            if stop[j]:
                for i in (1, 2, 3, 4):
                    assert _same_bits(got[i][:, j], base[i][:, j]), (stop, j, "wrpsx"[i])
                assert np.isnan(a_out[j].item()) and np.isnan(b_out[j].item())
            else:
                cols, out = single[j]
                for i in (1, 2, 3, 4):
                    assert _same_bits(got[i][:, j], cols[i]), (stop, j, "wrpsx"[i])
                    assert not _same_bits(got[i][:, j], base[i][:, j])
                assert _same_bits(a_out[j:j + 1], out[1]) and _same_bits(b_out[j:j + 1], out[2])
    if n == SECOND_PASS[k]:
        assert n % 2 == 1 and n * k // 4 > SLAB * 256  # the second pass exists


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,bw", [(50, 8), (1037, 1037), (70_001, 16)])
def test_spmm_stop(tz, gpu, n, bw, k):
    """all_done clear: csr_spmm_dot2 bit for bit; all_done set: nothing is written"""
    kn = tz._tz.kernels
    rp, ci, v = _matrix(tz, n, bw)
    R = _rand((n, k), 5 + k)
    g_out = _f64([0.7310585786300049 + j for j in range(k)])
    a_out = _f64([3.0e-9 * (j + 1) for j in range(k)])
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W

        def launch(flag):
            w, pg, pd = _nan(n * k, torch.float32).view(n, k), _nan(k * SLAB + 8), _nan(k * SLAB + 8)
            g_prev, a_prev = _nan(k + 2), _nan(k + 2)
            args = (n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), R.data_ptr(), w.data_ptr(), k, lanes,
                    pg.data_ptr(), pd.data_ptr(), g_out.data_ptr(), a_out.data_ptr(), g_prev.data_ptr(),
                    a_prev.data_ptr())
            if flag is None:
                kn.csr_spmm_dot2(*args, _stream())
            else:
                all_done = _i32(flag)
                kn.csr_spmm_dot2_stop(*args, all_done.data_ptr(), _stream())
            torch.cuda.synchronize()
            return w, pg, pd, g_prev, a_prev

        want = launch(None)
        assert not torch.isnan(want[0]).any() and _same_bits(want[3][:k], g_out)
        assert all(_same_bits(a, b) for a, b in zip(launch(0), want)), W
        for t in launch(1):
            assert torch.isnan(t).all(), W


def test_bad_arguments_raise(tz, gpu):
    kn = tz._tz.kernels
    a = torch.zeros(64, device="cuda")
    s = torch.zeros(8 * SLAB + 128, dtype=torch.float64, device="cuda")
    s2 = torch.zeros(8 * SLAB, dtype=torch.float64, device="cuda").data_ptr()
    ap, sp = a.data_ptr(), s.data_ptr()
    sc = [sp + 8 * (8 * SLAB + 8 * i) for i in range(9)]  # nine distinct arrays of 8 past the slabs
    prev, outs, th, dn, it, ad = sc[0:2], sc[2:5], sc[5], sc[6], sc[7], sc[8]
    L = kn.SPMV_ILP + 4
    st = _stream()
    vec = [ap] * 5
    # csr_spmv_dot2_stop(n, rowPtr, colInd, val, r, w, lanes, slabs.., scalars.., done)
    with pytest.raises(Exception, match="null"):
        kn.csr_spmv_dot2_stop(8, ap, ap, ap, ap, ap, L, sp, s2, 0, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="lanes"):
        kn.csr_spmv_dot2_stop(8, ap, ap, ap, ap, ap, 8, sp, s2, 0, 0, 0, 0, dn, st)
    with pytest.raises(Exception, match="null"):  # the four scalars come together
        kn.csr_spmv_dot2_stop(8, ap, ap, ap, ap, ap, L, sp, s2, outs[0], outs[1], prev[0], 0, dn, st)
    with pytest.raises(Exception, match="alias"):
        kn.csr_spmv_dot2_stop(8, ap, ap, ap, ap, ap, L, sp, s2, outs[0], outs[1], prev[0], prev[1], prev[1] + 4, st)
    # cg_sr_update_stop(n, slabs.., np, prev.., w, r, p, s, x, out.., thresh, done, iters)
    for i in range(3):
        own = [th, dn, it]
        own[i] = 0
        with pytest.raises(Exception, match="null"):
            kn.cg_sr_update_stop(8, sp, s2, 1, *prev, *vec, *outs, *own, st)
    with pytest.raises(Exception, match="partials"):
        kn.cg_sr_update_stop(8, sp, s2, SLAB + 1, *prev, *vec, *outs, th, dn, it, st)
    with pytest.raises(Exception, match="alias"):  # the parent's check
        kn.cg_sr_update_stop(8, sp, s2, 1, *prev, *vec, prev[0], outs[1], outs[2], th, dn, it, st)
    for other in prev + outs:  # thresh, done and iters against each of the five scalars
        for i in range(3):
            own = [th, dn, it]
            own[i] = other + (4 if i == 1 else 0)  # done: the upper half of the double
            with pytest.raises(Exception, match="alias"):
                kn.cg_sr_update_stop(8, sp, s2, 1, *prev, *vec, *outs, *own, st)
    with pytest.raises(Exception, match="alias each other"):
        kn.cg_sr_update_stop(8, sp, s2, 1, *prev, *vec, *outs, th, th + 4, it, st)
    # csr_spmm_dot2_stop(n, rowPtr, colInd, val, R, Wout, k, lanes, slabs.., scalars.., all_done)
    with pytest.raises(Exception, match="2, 4 or 8"):
        kn.csr_spmm_dot2_stop(8, ap, ap, ap, ap, ap + 128, 3, L, sp, s2, 0, 0, 0, 0, ad, st)
    with pytest.raises(Exception, match="null"):
        kn.csr_spmm_dot2_stop(8, ap, ap, ap, ap, ap + 128, 2, L, sp, s2, 0, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="aligned"):
        kn.csr_spmm_dot2_stop(8, ap, ap, ap, ap + 4, ap + 128, 2, L, sp, s2, 0, 0, 0, 0, ad, st)
    with pytest.raises(Exception, match="alias"):  # inside the k-wide array of previous alphas
        kn.csr_spmm_dot2_stop(8, ap, ap, ap, ap, ap + 128, 4, L, sp, s2, outs[0], outs[1], prev[0], prev[1],
                              prev[1] + 24, st)
    # cg_sr_update_batch_stop(n, k, slabs.., np, prev.., w, r, p, s, x, out.., thresh, done, iters, all_done)
    with pytest.raises(Exception, match="2, 4 or 8"):
        kn.cg_sr_update_batch_stop(8, 3, sp, s2, 1, *prev, *vec, *outs, th, dn, it, ad, st)
    for i in range(4):
        own = [th, dn, it, ad]
        own[i] = 0
        with pytest.raises(Exception, match="null"):
            kn.cg_sr_update_batch_stop(8, 2, sp, s2, 1, *prev, *vec, *outs, *own, st)
    with pytest.raises(Exception, match="aligned"):
        kn.cg_sr_update_batch_stop(8, 2, sp, s2, 1, *prev, ap, ap + 4, ap, ap, ap, *outs, th, dn, it, ad, st)
    with pytest.raises(Exception, match="alias"):  # overlapping by one element of a k-wide array
        kn.cg_sr_update_batch_stop(8, 4, sp, s2, 1, *prev, *vec, *outs, outs[2] + 24, dn, it, ad, st)
    with pytest.raises(Exception, match="alias"):
        kn.cg_sr_update_batch_stop(8, 4, sp, s2, 1, *prev, *vec, *outs, th, dn, it, dn + 12, st)
