"""d3d_amd.math on the GPU (bessel.hip): the reference's bits from tests/golden/math_ref_cases.npz, the numpy model of
tests/math_reference.py on 2^22-element draws that put wavefronts on either side of |x| = 8 and across it, scipy for fp64,
mpmath for the accuracy figure, every shape and alignment of the launch, a stream of the caller's, n past 2^31, and both
backward modes of I0Exp.  Reads nothing outside the repository."""
import os

import numpy as np
import pytest
import torch

import math_reference as mr
from golden_io import GOLDEN

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(GOLDEN, "math_ref_cases.npz"))
DTYPES = [("f32", np.float32), ("f64", np.float64)]
MODEL = {0: mr.model_i0e, 1: mr.model_i1e}


def fns():
    from d3d_amd import math as dmath
    return {"cc": (dmath.i0e_cc, dmath.i1e_cc), "cuda": (dmath.i0e_cuda, dmath.i1e_cuda), "public": (dmath.i0e, dmath.i1e)}


def raw(order, x, out=None, n=None):
    """the C entry on device tensors"""
    from d3d_amd import _lib
    out = torch.empty_like(x) if out is None else out
    n = x.numel() if n is None else n
    rc = _lib.load().d3d_bessel_e(order, _lib.ptr(x), n, _lib.F32 if x.dtype == torch.float32 else _lib.F64, _lib.ptr(out),
                                  _lib.stream_ptr())
    assert rc == _lib.OK
    return out


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag,T", DTYPES)
def test_golden_bits(tag, T, order):
    x, want = Z[tag + "/x"], Z["%s/i%de" % (tag, order)]
    xd = torch.from_numpy(x).cuda()
    got = raw(order, xd).cpu().numpy()
    assert mr.same_bits(got, want), "raw entry: %d of %d differ" % (np.sum(mr.bits(got) != mr.bits(want)), len(x))
    for name, pair in fns().items():
        got = pair[order](xd)
        assert got.is_cuda and got.dtype == xd.dtype and got.shape == xd.shape
        assert mr.same_bits(got.cpu().numpy(), want), name


def big_draw(T):
    """2^22 values: stretches inside (-8, 8), stretches outside, stretches across (whole wavefronts of each kind and mixed
    ones), plus single outliers inside uniform stretches and specials"""
    rng = np.random.default_rng(99 + np.dtype(T).itemsize)
    n = 1 << 22
    x = rng.uniform(-20, 20, n)
    x[: n // 4] = rng.uniform(-8, 8, n // 4)
    x[n // 4: n // 2] = rng.uniform(8, 1e3, n // 4) * rng.choice([-1.0, 1.0], n // 4)
    x[rng.integers(0, n // 4, 64)] = 9.5                    # one lane on the other side
    x[rng.integers(n // 4, n // 2, 64)] = -0.25
    x = x.astype(T)
    x[-4096:] = mr.log_uniform(rng, 4096, T)
    x[1000:1008] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 8.0, -8.0, np.nextafter(T(8), T(9))], T)
    return x


@pytest.mark.parametrize("tag,T", DTYPES)
def test_big_draw_equals_model_and_scipy(tag, T):
    from scipy import special
    x = big_draw(T)
    assert np.sum(np.abs(x) <= 8) > 1 << 20 and np.sum(np.abs(x) > 8) > 1 << 20
    xd = torch.from_numpy(x).cuda()
    for order in (0, 1):
        got = raw(order, xd).cpu().numpy()
        want = MODEL[order](x)
        bad = ~(np.isnan(got) & np.isnan(want)) & (mr.bits(got) != mr.bits(want))
        assert not bad.any(), "i%de %s: %d differ, first at x = %r" % (order, tag, bad.sum(), x[np.argmax(bad)])
        if T is np.float64:
            assert mr.same_bits(got, (special.i0e, special.i1e)[order](x))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag,T", DTYPES)
def test_distance_from_mpmath_within_the_references(tag, T, order):
    """bit equality with the reference implies it; kept so that a deliberate deviation one day is held to the same figure"""
    s = mr.ulp_sample(T)
    got = raw(order, torch.from_numpy(s).cuda()).cpu().numpy()
    d = mr.ulp_distance(got, mr.exact(order, s))
    recorded = float(Z["%s/i%de_max_ulp" % (tag, order)][0])
    print(tag, "i%de" % order, "largest distance %.4f ulp, the reference's %.4f" % (d.max(), recorded))
    assert d.max() <= recorded


@pytest.mark.parametrize("tag,T", DTYPES)
def test_shapes_and_layouts(tag, T):
    from d3d_amd import math as dmath
    rng = np.random.default_rng(5)
    for order, fn in ((0, dmath.i0e_cc), (1, dmath.i1e_cc)):
        x = np.array(rng.uniform(-12, 12), T)                                   # 0-d
        got = fn(torch.from_numpy(x).cuda())
        assert got.shape == () and mr.same_bits(got.cpu().numpy(), MODEL[order](x))
        for shape in ((0,), (3, 0, 2)):                                         # empty
            got = fn(torch.empty(shape, dtype=torch.from_numpy(x).dtype, device="cuda"))
            assert got.shape == shape and got.is_cuda
        x = rng.uniform(-12, 12, (3, 5, 7)).astype(T)
        got = fn(torch.from_numpy(x).cuda())
        assert got.shape == (3, 5, 7) and got.is_contiguous() and mr.same_bits(got.cpu().numpy(), MODEL[order](x))
        x = rng.uniform(-12, 12, (33, 17)).astype(T)                            # a transposed view
        xt = torch.from_numpy(x).cuda().t()
        assert not xt.is_contiguous()
        got = fn(xt)
        assert got.shape == (17, 33) and mr.same_bits(got.cpu().numpy(), MODEL[order](x.T))
        xs = torch.from_numpy(x).cuda()[::2, 1::3]                              # strided rows and columns
        assert mr.same_bits(fn(xs).cpu().numpy(), MODEL[order](x[::2, 1::3]))


@pytest.mark.parametrize("tag,T", DTYPES)
def test_every_small_n_at_every_alignment_and_nothing_beyond_n(tag, T):
    """n = 1 .. 70 with the input and the output each 0 .. 3 elements (fp32; 0 .. 1 for fp64) past a 16-byte boundary, the
    4-bytes-past case of a sliced view among them: the single elements in front of and behind the vectors, the unaligned loads,
    and a NaN-poisoned output that must keep every element outside [0, n); then every n in place at every alignment"""
    rng = np.random.default_rng(6)
    per16 = 16 // np.dtype(T).itemsize
    x_all = rng.uniform(-12, 12, 96).astype(T)
    x_all[::7] = rng.uniform(8, 50, len(x_all[::7])).astype(T)
    base = torch.from_numpy(x_all).cuda()
    assert base.data_ptr() % 16 == 0
    for order in (0, 1):
        for n in range(1, 71):
            for xo in range(per16):
                for oo in range(per16):
                    x = base[xo: xo + n]
                    assert x.data_ptr() % 16 == (xo * x.element_size()) % 16
                    buf = torch.full((96,), float("nan"), dtype=base.dtype, device="cuda")
                    out = buf[4 + oo: 4 + oo + n]
                    raw(order, x, out)
                    got = buf.cpu().numpy()
                    want = MODEL[order](x_all[xo: xo + n])
                    assert mr.same_bits(got[4 + oo: 4 + oo + n], want), (order, n, xo, oo)
                    assert np.all(np.isnan(got[: 4 + oo])) and np.all(np.isnan(got[4 + oo + n:])), (order, n, xo, oo)
            for xo in range(per16):                         # in place: the output is the input
                buf = base.clone()
                v = buf[xo: xo + n]
                raw(order, v, v)
                got = buf.cpu().numpy()
                assert mr.same_bits(got[xo: xo + n], MODEL[order](x_all[xo: xo + n])), (order, n, xo, "in place")
                assert mr.same_bits(got[:xo], x_all[:xo]) and mr.same_bits(got[xo + n:], x_all[xo + n:]), (order, n, xo)
    from d3d_amd import math as dmath
    view = base[1:]                                         # the Python layer on a view 4 (8) bytes past the boundary
    assert view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
    assert mr.same_bits(dmath.i0e_cc(view).cpu().numpy(), mr.model_i0e(x_all[1:]))
    buf = torch.full((80,), float("nan"), dtype=base.dtype, device="cuda")       # n smaller than the buffers
    raw(1, base, buf, n=37)
    got = buf.cpu().numpy()
    assert mr.same_bits(got[:37], mr.model_i1e(x_all[:37])) and np.all(np.isnan(got[37:]))


def test_result_on_a_side_stream_without_device_synchronisation():
    from d3d_amd import math as dmath
    x = np.random.default_rng(7).uniform(-20, 20, 1 << 20).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        filler = torch.rand(2048, 2048, device="cuda")
        for _ in range(8):
            filler = (filler @ filler) * 1e-3               # the stream is busy when the launches are queued behind it
        y = dmath.i1e_cc(dmath.i0e_cc(xd))                  # the second launch consumes the first, on the same stream
        host = y.cpu()                                      # a copy on the side stream; waits for that stream alone
    assert mr.same_bits(host.numpy(), mr.model_i1e(mr.model_i0e(x)))
    side.synchronize()


@pytest.mark.parametrize("tag,T", DTYPES)
def test_cpu_tensor_in_cpu_tensor_out(tag, T):
    x = Z[tag + "/x"][:500]
    for name, pair in fns().items():
        for order in (0, 1):
            got = pair[order](torch.from_numpy(x))
            assert got.device.type == "cpu" and mr.same_bits(got.numpy(), Z["%s/i%de" % (tag, order)][:500]), name


def test_n_past_2_to_31():
    n = (1 << 31) + 4099
    free, _ = torch.cuda.mem_get_info()
    if free < 20 * (1 << 30):
        pytest.skip("needs 20 GB of free device memory")
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    chunk = 1 << 26
    g = torch.Generator(device="cuda").manual_seed(11)
    for a in range(0, n, chunk):                            # uniform in +-20, filled by pieces
        b = min(a + chunk, n)
        x[a:b].uniform_(-20, 20, generator=g)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    raw(0, x, out)
    idx = np.concatenate([[0, 1, 2, 3, n - 1, n - 2, n - 3, n - 4, (1 << 31) - 1, 1 << 31, (1 << 31) + 1],
                          np.random.default_rng(12).integers(0, n, 100000)])
    it = torch.from_numpy(idx).cuda()
    xs, got = x[it].cpu().numpy(), out[it].cpu().numpy()
    assert mr.same_bits(got, mr.model_i0e(xs))
    assert not bool(torch.isnan(out[-(1 << 20):]).any()) and not bool(torch.isnan(out[(1 << 31) - 4096: (1 << 31) + 4096]).any())
    del x, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("tag,T", DTYPES)
def test_autograd_reference_compat_returns_i1e_of_the_gradient(tag, T):
    from d3d_amd import math as dmath
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-12, 12, (40, 25)).astype(T)).cuda().requires_grad_()
    g = rng.uniform(-12, 12, (40, 25)).astype(T)
    for y in (dmath.i0e(x), dmath.i0e(x, reference_compat=True), dmath.I0Exp.apply(x)):
        x.grad = None
        y.backward(torch.from_numpy(g).cuda())
        assert mr.same_bits(x.grad.cpu().numpy(), mr.model_i1e(g))
        assert mr.same_bits(y.detach().cpu().numpy(), mr.model_i0e(x.detach().cpu().numpy()))


@pytest.mark.parametrize("tag,T", DTYPES)
def test_autograd_true_derivative(tag, T):
    from d3d_amd import math as dmath
    rng = np.random.default_rng(9)
    xn = rng.uniform(-20, 20, 5000).astype(T)
    xn[:6] = np.array([0.0, -0.0, 8.0, -8.0, 1e-30, -1e-30], T)
    gn = rng.uniform(-3, 3, 5000).astype(T)
    x = torch.from_numpy(xn).cuda().requires_grad_()
    g = torch.from_numpy(gn).cuda()
    y = dmath.i0e(x, reference_compat=False)
    y.backward(g)
    i0, i1 = dmath.i0e_cc(x.detach()), dmath.i1e_cc(x.detach())
    want = g * (i1 - torch.sign(x.detach()) * i0)           # IEEE multiplies and subtracts in the kernel's order
    assert mr.same_bits(x.grad.cpu().numpy(), want.cpu().numpy())
    assert mr.same_bits(x.grad.cpu().numpy(), mr.model_backward(xn, gn))
    assert float(x.grad[0]) == 0.0 and float(x.grad[1]) == 0.0                  # the kink: sign(0) = 0
    xc = torch.from_numpy(xn[:64]).requires_grad_()                             # CPU tensors in, CPU gradient out
    dmath.i0e(xc, reference_compat=False).backward(torch.from_numpy(gn[:64]))
    assert xc.grad.device.type == "cpu" and mr.same_bits(xc.grad.numpy(), mr.model_backward(xn[:64], gn[:64]))


def test_gradcheck_fp64():
    from d3d_amd import math as dmath
    rng = np.random.default_rng(10)
    v = rng.uniform(1e-2, 6, 40) * rng.choice([-1.0, 1.0], 40)                  # away from the kink at 0
    x = torch.from_numpy(v).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: dmath.i0e(t, reference_compat=False), (x,))


def test_raw_backward_entry_unaligned_and_poisoned():
    from d3d_amd import _lib
    rng = np.random.default_rng(13)
    xn, gn = rng.uniform(-20, 20, 200).astype(np.float32), rng.uniform(-3, 3, 200).astype(np.float32)
    xb, gb = torch.from_numpy(xn).cuda(), torch.from_numpy(gn).cuda()
    for n in (1, 2, 3, 5, 64, 131):
        for xo, go, oo in ((0, 0, 0), (1, 0, 0), (0, 3, 1), (2, 1, 3)):
            buf = torch.full((160,), float("nan"), dtype=torch.float32, device="cuda")
            x, g, out = xb[xo: xo + n], gb[go: go + n], buf[8 + oo: 8 + oo + n]
            rc = _lib.load().d3d_i0e_backward(_lib.ptr(x), _lib.ptr(g), n, _lib.F32, _lib.ptr(out), _lib.stream_ptr())
            assert rc == _lib.OK
            got = buf.cpu().numpy()
            assert mr.same_bits(got[8 + oo: 8 + oo + n], mr.model_backward(xn[xo: xo + n], gn[go: go + n])), (n, xo, go, oo)
            assert np.all(np.isnan(got[: 8 + oo])) and np.all(np.isnan(got[8 + oo + n:]))
        for o in (0, 1):                                    # in place: grad_x over x, then over grad
            want = mr.model_backward(xn[o: o + n], gn[o: o + n])
            for over_x in (True, False):
                xc, gc = xb.clone(), gb.clone()
                x, g = xc[o: o + n], gc[o: o + n]
                dst, src = (xc, xn) if over_x else (gc, gn)
                rc = _lib.load().d3d_i0e_backward(_lib.ptr(x), _lib.ptr(g), n, _lib.F32, _lib.ptr(dst[o: o + n]), _lib.stream_ptr())
                assert rc == _lib.OK
                got = dst.cpu().numpy()
                assert mr.same_bits(got[o: o + n], want), (n, o, over_x)
                assert mr.same_bits(got[:o], src[:o]) and mr.same_bits(got[o + n:], src[o + n:]), (n, o, over_x)
