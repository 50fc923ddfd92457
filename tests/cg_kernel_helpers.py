"""What the tests of the conjugate-gradient kernels share (test_gpu_cg_kernels.py and its sr,
batch and tol siblings): device tensors with known contents, bit comparisons, and the host side
of the kernels' arithmetic (the slab sum's order, the guarded divisions)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

SLAB = 256  # kernels.CG_MAX_PARTIALS
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(shape, seed, dtype=torch.float32):
    """`shape`: a length n or a tuple, (n, k) for a batch"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=dtype).cuda()


def _nan(n, dtype=torch.float64):
    return torch.full((n,), NAN, dtype=dtype, device="cuda")


def _nan_slab():
    return _nan(SLAB + 8)


def _bits(t):
    """a column of a batch is a strided view: compared through a contiguous copy"""
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _f64(v):
    """a scalar, or one value per column"""
    return torch.tensor(np.atleast_1d(v), dtype=torch.float64, device="cuda")


def _tree_sum(part):
    """the order every prologue sums a slab in (kernels.sum_partials_f64): thread t of 256 holds
    partial t (+0.0 past the count), xor butterfly over each 64, then the four groups in order"""
    v = np.zeros(256, dtype=np.float64)
    v[:len(part)] = part
    v = v.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    s = v[0, 0]
    for w in (1, 2, 3):
        s = s + v[w, 0]
    return float(s)


def _misaligned(t):
    """a copy of t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()]
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def _check_dot(part, n_used, u, v, n):
    """partials summed in index order on the host against the f64 dot product: the only error
    is the n - 1 f64 additions (the products are exact); x 2 for the reference's own rounding"""
    p = part.cpu().numpy()
    assert not np.isnan(p[:n_used]).any(), "a partial slot in use was not written"
    assert np.isnan(p[n_used:]).all(), "a slot past the documented count was touched"
    s = 0.0
    for x in p[:n_used]:
        s += float(x)
    ud, vd = u.double(), v.double()
    ref = torch.dot(ud, vd).item()
    bound = 2.0 * (n - 1) * 2.0 ** -53 * (ud * vd).abs().sum().item()
    print(f"dot n={n}: |err|={abs(s - ref):.3e} bound={bound:.3e}")
    assert abs(s - ref) <= bound


def _gdiv(a, b):
    return a / b if b != 0 else 0.0


def _host_scalars(gamma, delta, gamma_prev, alpha_prev):
    """beta and alpha as the recurrence defines them, in IEEE f64 (Python floats: the product
    and the difference round separately)"""
    beta = _gdiv(gamma, gamma_prev)
    alpha = _gdiv(gamma, delta - beta * _gdiv(gamma, alpha_prev))
    return beta, alpha
