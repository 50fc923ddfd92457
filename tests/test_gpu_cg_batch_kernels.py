"""The two batched kernels of the single-reduction CG form (cg_kernels.hip): ``csr_spmm_dot2``
and ``cg_sr_update_batch`` on k = 2, 4, 8 interleaved right-hand sides. The oracle is the
single-RHS kernels, bit for bit: column j of every output equals what ``csr_spmv_dot2`` /
``cg_sr_update`` give on a contiguous copy of column j (those are held to ``csr_spmv``, f64 dot
products, the host formula and the plain kernels by test_gpu_cg_sr_kernels.py).

Sizes as there: 70 001 rows is the smallest case in which 4 lanes per row take a second, ragged
grid-stride pass; an odd n with n k // 4 > 65 536 quads (150 005 / 75 003 / 37 503 rows for k =
2 / 4 / 8, about the 300 007 elements used there) gives the vector layout a second pass."""
import functools

import numpy as np
import pytest

from cg_kernel_helpers import SLAB,_f64, _host_scalars, _nan, _rand, _same_bits, _stream, _tree_sum

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = [2, 4, 8]
SECOND_PASS = {2: 150_005, 4: 75_003, 8: 37_503}
# (gamma_prev, alpha_prev): the four guard cases of test_gpu_cg_sr_kernels.py
GUARDS = ((0.8123, 0.37454011884736254), (0.0, 0.37454011884736254), (0.8123, 0.0), (0.0, 0.0))


@functools.lru_cache(maxsize=None)
def _matrix(tz, n, bw):
    """the system matrix on the device, built once per shape and never changed"""
    rp, ci, v = tz._tz.spd_band_matrix(n, bw, 5 * n, 1)
    return (torch.tensor(rp, dtype=torch.int32).cuda(), torch.tensor(ci, dtype=torch.int32).cuda(),
            torch.tensor(v, dtype=torch.float32).cuda())


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,bw", [(50, 8), (257, 16), (1037, 1037), (70_001, 16)])
def test_csr_spmm_dot2(tz, gpu, n, bw, k):
    kn = tz._tz.kernels
    rp, ci, v = _matrix(tz, n, bw)
    R = _rand((n, k), 5 + k)
    assert R.data_ptr() % 16 == 0
    g_out0 = np.array([0.7310585786300049 + j for j in range(k)])
    a_out0 = np.array([3.0e-9 * (j + 1) for j in range(k)])
    for W in (1, 2, 4):
        lanes = kn.SPMV_ILP + W
        cnt = kn.spmv_dot_partial_count(n, lanes)
        assert cnt == min(SLAB, max(1, -(-n * W // 1024)))
        g_out, a_out = _f64(g_out0), _f64(a_out0)

        def launch(scalars=True):
            w, pg, pd = _nan(n * k, torch.float32).view(n, k), _nan(k * SLAB + 8), _nan(k * SLAB + 8)
            g_prev, a_prev = _nan(k + 2), _nan(k + 2)
            sc = (g_out.data_ptr(), a_out.data_ptr(), g_prev.data_ptr(), a_prev.data_ptr()) if scalars else (0,) * 4
            kn.csr_spmm_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), R.data_ptr(), w.data_ptr(), k, lanes,
                             pg.data_ptr(), pd.data_ptr(), *sc, _stream())
            torch.cuda.synchronize()
            return w, pg, pd, g_prev, a_prev

        w, pg, pd, g_prev, a_prev = first = launch()
        for j in range(k):
            rj = R[:, j].contiguous()
            wr, pgr, pdr = _nan(n, torch.float32), _nan(SLAB), _nan(SLAB)
            kn.csr_spmv_dot2(n, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), rj.data_ptr(), wr.data_ptr(), lanes,
                             pgr.data_ptr(), pdr.data_ptr(), 0, 0, 0, 0, _stream())
            torch.cuda.synchronize()
            assert not torch.isnan(wr).any() and not torch.isnan(pgr[:cnt]).any() and not torch.isnan(pdr[:cnt]).any()
            assert _same_bits(w[:, j], wr), (W, j)
            # the whole slab: the partials in use, and NaN in every slot past the count
            assert _same_bits(pg[j * SLAB:(j + 1) * SLAB], pgr), (W, j)
            assert _same_bits(pd[j * SLAB:(j + 1) * SLAB], pdr), (W, j)
            assert torch.isnan(pg[j * SLAB + cnt:(j + 1) * SLAB]).all()
            assert torch.isnan(pd[j * SLAB + cnt:(j + 1) * SLAB]).all()
        assert torch.isnan(pg[k * SLAB:]).all() and torch.isnan(pd[k * SLAB:]).all()
        # the k-wide scalar move is bit-exact, stays inside its arrays and leaves its sources alone
        assert _same_bits(g_prev[:k], g_out) and _same_bits(a_prev[:k], a_out)
        assert torch.isnan(g_prev[k:]).all() and torch.isnan(a_prev[k:]).all()
        assert np.array_equal(g_out.cpu().numpy(), g_out0) and np.array_equal(a_out.cpu().numpy(), a_out0)
        # two launches give the same bits
        assert all(_same_bits(a, b) for a, b in zip(first, launch()))
        # without the scalar pointers nothing else changes, and nothing is moved
        w2, pg2, pd2, g_prev2, a_prev2 = launch(scalars=False)
        assert _same_bits(w, w2) and _same_bits(pg, pg2) and _same_bits(pd, pd2)
        assert torch.isnan(g_prev2).all() and torch.isnan(a_prev2).all()
    if n == 70_001:
        assert n * 4 > SLAB * 1024  # the second pass exists, and it is ragged
        assert (n * 4) % (SLAB * 1024) != 0


def _slabs(k, cnt, seed):
    """k slabs of random positive partials up to the count, NaN beyond it (and past the last)"""
    pg, pd = _nan(k * SLAB + 8), _nan(k * SLAB + 8)
    for j in range(k):
        pg[j * SLAB:j * SLAB + cnt] = _rand(cnt, seed + 2 * j, torch.float64).abs() + 0.1
        pd[j * SLAB:j * SLAB + cnt] = _rand(cnt, seed + 2 * j + 1, torch.float64).abs() + 2.0
    return pg, pd


def _update_batch(kn, n, k, pg, pd, cnt, g_prev, a_prev, vecs):
    """one cg_sr_update_batch launch (r, p, s, x of `vecs` = (w, r, p, s, x) are updated in
    place); returns the published (gamma, alpha, beta) arrays, each with two NaN guard slots"""
    out = [_nan(k + 2) for _ in range(3)]
    kn.cg_sr_update_batch(n, k, pg.data_ptr(), pd.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(),
                          *(t.data_ptr() for t in vecs), *(o.data_ptr() for o in out), _stream())
    torch.cuda.synchronize()
    for o in out:
        assert torch.isnan(o[k:]).all()
    return [o[:k] for o in out]


def _update_single(kn, n, pg_j, pd_j, cnt, gp, ap, cols):
    """cg_sr_update on contiguous vectors with slab views pg_j, pd_j; returns (gamma, alpha, beta)"""
    out = [_nan(1) for _ in range(3)]
    g_prev, a_prev = _f64(gp), _f64(ap)
    kn.cg_sr_update(n, pg_j.data_ptr(), pd_j.data_ptr(), cnt, g_prev.data_ptr(), a_prev.data_ptr(),
                    *(t.data_ptr() for t in cols), *(o.data_ptr() for o in out), _stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k,n", [(k, n) for k in KS for n in (1, 63, 64, 65, 257, 1037, SECOND_PASS[k])])
def test_cg_sr_update_batch(tz, gpu, k, n):
    kn = tz._tz.kernels
    base = [_rand((n, k), 20 + i) for i in range(5)]  # w, r, p, s, x
    assert all(t.data_ptr() % 16 == 0 for t in base)
    w, r, p, s, x = base
    cnt = kn.spmv_dot_partial_count(n, 4)
    pg, pd = _slabs(k, cnt, 31)
    gamma = [_tree_sum(pg[j * SLAB:j * SLAB + cnt].cpu().numpy()) for j in range(k)]
    delta = [_tree_sum(pd[j * SLAB:j * SLAB + cnt].cpu().numpy()) for j in range(k)]
    for shift in range(4):  # the four guard cases mixed across the columns of one launch
        case = [GUARDS[(j + shift) % 4] for j in range(k)]
        g_prev, a_prev = _f64([c[0] for c in case]), _f64([c[1] for c in case])
        got = [t.clone() for t in base]
        g_out, a_out, b_out = _update_batch(kn, n, k, pg, pd, cnt, g_prev, a_prev, got)
        assert _same_bits(got[0], w)  # w is read only
        assert np.array_equal(g_prev.cpu().numpy(), [c[0] for c in case])  # read only
        assert np.array_equal(a_prev.cpu().numpy(), [c[1] for c in case])
        for j in range(k):
            gp0, ap0 = case[j]
            # the published scalars are the host formula on the kernels' sums, bit for bit
            beta, alpha = _host_scalars(gamma[j], delta[j], gp0, ap0)
            assert g_out[j].item() == gamma[j], (shift, j)
            assert b_out[j].item() == beta, (shift, j)
            assert a_out[j].item() == alpha, (shift, j)
            assert np.isfinite(alpha) and alpha != 0
            # column j is what cg_sr_update gives on contiguous copies with slab j and its scalars
            # (copies: with n = 1 a column already is contiguous, and the launch writes in place)
            cols = [t[:, j].clone(memory_format=torch.contiguous_format) for t in base]
            g1, a1, b1 = _update_single(kn, n, pg[j * SLAB:], pd[j * SLAB:], cnt, gp0, ap0, cols)
            assert _same_bits(g1, g_out[j:j + 1]) and _same_bits(a1, a_out[j:j + 1]) and _same_bits(b1, b_out[j:j + 1])
            for i in (1, 2, 3, 4):
                assert _same_bits(got[i][:, j], cols[i]), (shift, j, "wrpsx"[i])
            assert not _same_bits(got[4][:, j], x[:, j]) and not _same_bits(got[1][:, j], r[:, j])
            if gp0 == 0.0:  # the guard: beta = 0, so p = r and s = w
                assert beta == 0.0 and _same_bits(got[2][:, j], r[:, j]) and _same_bits(got[3][:, j], w[:, j])
            else:
                assert not _same_bits(got[2][:, j], r[:, j]) and not _same_bits(got[3][:, j], w[:, j])
    # one column with zero slabs: alpha = beta = 0 (guarded), its x and r unchanged; the others move
    z = k - 1
    pg[z * SLAB:z * SLAB + cnt] = 0
    pd[z * SLAB:z * SLAB + cnt] = 0
    g_prev, a_prev = _f64([GUARDS[0][0]] * k), _f64([GUARDS[0][1]] * k)
    got = [t.clone() for t in base]
    g_out, a_out, b_out = _update_batch(kn, n, k, pg, pd, cnt, g_prev, a_prev, got)
    assert g_out[z].item() == 0.0 and a_out[z].item() == 0.0 and b_out[z].item() == 0.0
    assert _same_bits(got[1][:, z], r[:, z]) and _same_bits(got[4][:, z], x[:, z])
    for j in range(k - 1):
        assert a_out[j].item() != 0.0 and b_out[j].item() != 0.0
        assert not _same_bits(got[1][:, j], r[:, j]) and not _same_bits(got[4][:, j], x[:, j])
    if n == SECOND_PASS[k]:
        assert n % 2 == 1 and n * k // 4 > SLAB * 256  # the second pass exists


def test_bad_arguments_raise(tz, gpu):
    kn = tz._tz.kernels
    a = torch.zeros(64, device="cuda")
    s = torch.zeros(8 * SLAB + 64, dtype=torch.float64, device="cuda")
    s2 = torch.zeros(8 * SLAB, dtype=torch.float64, device="cuda").data_ptr()
    ap, sp = a.data_ptr(), s.data_ptr()
    assert ap % 16 == 0
    sc = [sp + 8 * (8 * SLAB + 8 * i) for i in range(5)]  # five distinct arrays of 8 past the slabs
    L = kn.SPMV_ILP + 4
    st = _stream()
    # csr_spmm_dot2(n, rowPtr, colInd, val, R, Wout, k, lanes, slabs.., scalars..)
    with pytest.raises(Exception, match="2, 4 or 8"):
        kn.csr_spmm_dot2(8, ap, ap, ap, ap, ap + 128, 3, L, sp, s2, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="lanes"):
        kn.csr_spmm_dot2(8, ap, ap, ap, ap, ap + 128, 2, 8, sp, s2, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="aligned"):
        kn.csr_spmm_dot2(8, ap, ap, ap, ap + 4, ap + 128, 2, L, sp, s2, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="aligned"):
        kn.csr_spmm_dot2(8, ap, ap, ap, ap, ap + 128 + 8, 2, L, sp, s2, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="null"):
        kn.csr_spmm_dot2(8, ap, ap, ap, 0, ap + 128, 2, L, sp, s2, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="null"):
        kn.csr_spmm_dot2(8, ap, ap, ap, ap, ap + 128, 2, L, sp, 0, 0, 0, 0, 0, st)
    with pytest.raises(Exception, match="null"):  # the four scalar arrays come together
        kn.csr_spmm_dot2(8, ap, ap, ap, ap, ap + 128, 2, L, sp, s2, sc[0], sc[1], sc[2], 0, st)
    # cg_sr_update_batch(n, k, slabs.., np, prev.., w, r, p, s, x, out..)
    with pytest.raises(Exception, match="2, 4 or 8"):
        kn.cg_sr_update_batch(8, 3, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[3], sc[4], st)
    for i in range(5):  # each of the five vectors
        vecs = [ap] * 5
        vecs[i] = ap + 4
        with pytest.raises(Exception, match="aligned"):
            kn.cg_sr_update_batch(8, 2, sp, s2, 1, sc[0], sc[1], *vecs, sc[2], sc[3], sc[4], st)
        vecs[i] = 0
        with pytest.raises(Exception, match="null"):
            kn.cg_sr_update_batch(8, 2, sp, s2, 1, sc[0], sc[1], *vecs, sc[2], sc[3], sc[4], st)
    with pytest.raises(Exception, match="null"):
        kn.cg_sr_update_batch(8, 2, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[3], 0, st)
    with pytest.raises(Exception, match="partials"):
        kn.cg_sr_update_batch(8, 2, sp, s2, SLAB + 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[3], sc[4], st)
    with pytest.raises(Exception, match="alias"):
        kn.cg_sr_update_batch(8, 2, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[0], sc[3], sc[4], st)
    with pytest.raises(Exception, match="alias"):  # overlapping by one element of a k-wide array
        kn.cg_sr_update_batch(8, 4, sp, s2, 1, sc[0], sc[1], ap, ap, ap, ap, ap, sc[2], sc[1] + 24, sc[4], st)
