"""GPU: the paired box operators (box2d_iou_paired / box3d_iou_paired, boxpair.hip) -- values against the CPU reference
(paired_reference.py: 1e-9 fp64, 1e-3 fp32) and, bit for bit, against the diagonal of the library's own matrix operators;
gradients against central differences of the reference (every parameter of every pair) and against the matrix operators'
autograd; the launch boundaries, degenerate pairs and the plumbing around the call."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import paired_reference as pr
from call_opts import set_opts
from test_oracle_box import _loss_cases

pytestmark = pytest.mark.gpu

COMBOS = ((np.float64, True), (np.float64, False), (np.float32, True), (np.float32, False))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases(dims):
    """the 40 seeded pairs, then the pairs of _loss_cases (identical boxes, a shared edge, corner contact, containment ...)"""
    b1, b2, c1, c2, _ = pr.seeded_pairs()
    l1, l2 = _loss_cases()
    n = min(len(l1), len(l2))
    l1, l2 = l1[:n], l2[:n]
    if dims == 2:
        return np.concatenate([b1, l1]), np.concatenate([b2, l2])
    z1, z2 = pr.with_z(l1, l2, 25)
    return np.concatenate([c1, z1]), np.concatenate([c2, z2])


def _n60(dims):
    """60 pairs for the comparisons with the matrix operators: random ones, the tie cases of _loss_cases in front"""
    b1, b2 = pr.rand_boxes(60, 31, 6.0), pr.rand_boxes(60, 32, 6.0)
    l1, l2 = _loss_cases()
    b1[:9], b2[:9] = l1[-9:], l2[-9:]
    return (b1, b2) if dims == 2 else tuple(pr.with_z(b1, b2, 33))


def _call(dims):
    from d3d_amd.box import box2d_iou_paired, box3d_iou_paired
    return box2d_iou_paired if dims == 2 else box3d_iou_paired


@pytest.mark.parametrize("dims,method", [(2, m) for m in pr.METHODS_2D] + [(3, m) for m in pr.METHODS_3D])
def test_forward_vs_cpu_reference(dims, method):
    b1, b2 = _cases(dims)
    ref = (pr.iou2d if dims == 2 else pr.iou3d)(b1, b2, method)
    assert np.array_equal(ref[:pr.N], pr.reference(dims, method)[0])
    for dtype, precise in COMBOS:
        got = _call(dims)(T(b1.astype(dtype)), T(b2.astype(dtype)), method=method, precise=precise)
        assert got.shape == (len(b1),) and got.dtype == (torch.float64 if dtype == np.float64 else torch.float32) and got.is_cuda
        err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
        print(dims, method, dtype.__name__, precise, "max |got - ref| = %.3e" % err)
        assert err < (1e-9 if dtype == np.float64 else 1e-3), (dtype, precise, err)
        if dims == 3 and dtype == np.float32:                     # the evaluator's fp32 measure
            o = np.diag(oracle.iou3d(b1.astype(np.float32), b2.astype(np.float32), method))
            assert np.max(np.abs(got.cpu().numpy() - o)) < 1e-3


@pytest.mark.parametrize("method", pr.METHODS_2D)
def test_forward_is_the_matrix_diagonal_bit_for_bit(method):
    """N = 60: the matrix operators' single-launch routes (k_iou_small, k_loss_iou) -- parent code, so a yardstick"""
    from d3d_amd.box import box2d_iou, box2d_iou_paired
    b1, b2 = _n60(2)
    for dtype, precise in COMBOS:
        t1, t2 = T(b1.astype(dtype)), T(b2.astype(dtype))
        paired, matrix = box2d_iou_paired(t1, t2, method=method, precise=precise), box2d_iou(t1, t2, method=method, precise=precise)
        assert paired.dtype == matrix.dtype
        assert torch.equal(paired, matrix.diagonal()), (dtype, precise, float((paired - matrix.diagonal()).abs().max()))


@pytest.mark.parametrize("method", pr.METHODS_3D)
def test_forward_3d_is_the_iou3d_diagonal_bit_for_bit(method):
    from d3d_amd.box import box3d_iou_paired, iou3d
    c1, c2 = _n60(3)
    t1, t2 = T(c1.astype(np.float32)), T(c2.astype(np.float32))
    paired = box3d_iou_paired(t1, t2, method=method, precise=False)
    assert torch.equal(paired, iou3d(t1, t2, method).diagonal()) and int((paired > 0).sum()) > 5


def _grads(dims, method, b1, b2, w, dtype, precise, which=(True, True)):
    t1, t2 = T(b1.astype(dtype)).requires_grad_(which[0]), T(b2.astype(dtype)).requires_grad_(which[1])
    (_call(dims)(t1, t2, method=method, precise=precise) * T(w.astype(dtype))).sum().backward()
    return t1.grad, t2.grad


@pytest.mark.parametrize("dims,method", [(2, m) for m in pr.METHODS_2D] + [(3, m) for m in pr.METHODS_3D])
def test_gradients_vs_central_differences(dims, method):
    """every parameter of every seeded pair, both inputs (the z and lz columns of the 3D boxes like the others)"""
    b1, b2, c1, c2, w = pr.seeded_pairs()
    x1, x2 = (b1, b2) if dims == 2 else (c1, c2)
    _, f1, f2 = pr.reference(dims, method)
    g1, g2 = _grads(dims, method, x1, x2, w, np.float64, True)
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    assert g1.dtype == np.float64 and g1.shape == x1.shape and g2.shape == x2.shape
    for fd, g in ((f1, g1), (f2, g2)):
        excess = np.abs(fd - g) - 2e-5 * np.maximum(1.0, np.abs(fd))
        print(dims, method, "max |fd - g| = %.3e" % np.abs(fd - g).max())
        assert np.all(excess < 0), (np.argwhere(excess >= 0)[:5], np.abs(fd - g).max())
    assert np.abs(g1).max() > 0.05
    # fp32 arithmetic and fp64 arithmetic on fp32 boxes agree with the fp64 gradients
    for precise in (False, True):
        h1, h2 = _grads(dims, method, x1, x2, w, np.float32, precise)
        assert h1.dtype == torch.float32 and h2.dtype == torch.float32
        for h, g in ((h1, g1), (h2, g2)):
            assert np.max(np.abs(h.cpu().numpy() - g)) < 2e-2 * max(1.0, np.abs(g).max()), precise


@pytest.mark.parametrize("method", pr.METHODS_2D)
def test_gradients_vs_the_matrix_operator(method):
    from d3d_amd.box import box2d_iou
    b1, b2 = _n60(2)
    w = np.random.default_rng(34).random(60)
    g1, g2 = _grads(2, method, b1, b2, w, np.float64, True)
    t1, t2 = T(b1).requires_grad_(True), T(b2).requires_grad_(True)
    (box2d_iou(t1, t2, method=method).diagonal() * T(w)).sum().backward()
    for g, r in ((g1, t1.grad), (g2, t2.grad)):
        assert torch.isfinite(g).all()
        assert float((g - r).abs().max()) < 1e-9 * max(1.0, float(r.abs().max()))


@pytest.mark.parametrize("dims,method", [(2, "rbox"), (2, "grbox"), (3, "rbox")])
def test_launch_boundaries(dims, method):
    """a pair's value and gradient do not depend on its position, its workgroup or on whether a gradient was asked for; output
    and gradient buffers are NaN-poisoned before every launch"""
    b1, b2 = pr.rand_boxes(1000, 41), pr.rand_boxes(1000, 42)
    if dims == 3:
        b1, b2 = pr.with_z(b1, b2, 43)
    set_opts(poison=True)
    call = _call(dims)
    full = call(T(b1), T(b2), method=method)
    assert not torch.isnan(full).any() and int((full != 0).sum()) > 100
    t1, t2 = T(b1).requires_grad_(True), T(b2).requires_grad_(True)
    vfull = call(t1, t2, method=method)
    vfull.sum().backward()
    assert torch.equal(vfull.detach(), full)
    gfull = (t1.grad, t2.grad)
    assert not torch.isnan(gfull[0]).any() and not torch.isnan(gfull[1]).any()
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        assert torch.equal(call(T(b1[:n]), T(b2[:n]), method=method), full[:n]), n
        t1, t2 = T(b1[:n]).requires_grad_(True), T(b2[:n]).requires_grad_(True)
        v = call(t1, t2, method=method)
        v.sum().backward()
        assert torch.equal(v.detach(), full[:n]), n
        assert torch.equal(t1.grad, gfull[0][:n]) and torch.equal(t2.grad, gfull[1][:n]), n


def test_degenerate_pairs():
    """no area: 0, never NaN -- value and gradient; contact cases: finite.  ('box' measures the bounding boxes, which have an area
    even where the rectangle has none, so a rectangle of negative size is no degenerate case for it: it follows the matrix.)"""
    from d3d_amd.box import box2d_iou, box2d_iou_paired, box3d_iou_paired
    #              zero width       negative height   disjoint          identical           shared edge       corner contact
    a = np.array([[0, 0, 0, 2, 0.3], [1, 1, -1, 2, 0], [0, 0, 2, 2, 0.1], [1, 2, 3, 2, 0.4], [0, 0, 2, 2, 0], [0, 0, 2, 2, 0]], np.float64)
    b = np.array([[0, 0, 2, 2, 0.1], [1, 1, 2, 2, 0.2], [9, 9, 2, 2, 0.5], [1, 2, 3, 2, 0.4], [2, 0, 2, 2, 0], [2, 2, 2, 2, 0]], np.float64)
    for x1, x2 in ((a, b), (b, a)):
        for method in pr.METHODS_2D:
            for dtype, precise in COMBOS:
                t1, t2 = T(x1.astype(dtype)).requires_grad_(True), T(x2.astype(dtype)).requires_grad_(True)
                v = box2d_iou_paired(t1, t2, method=method, precise=precise)
                v.sum().backward()
                v = v.detach()
                assert torch.isfinite(v).all() and torch.isfinite(t1.grad).all() and torch.isfinite(t2.grad).all()
                assert torch.equal(v, box2d_iou(t1.detach(), t2.detach(), method=method, precise=precise).diagonal())
                zero = [0, 1] if method != "box" else []            # no area -> 0 and no gradient
                if method in ("box", "rbox"):
                    zero += [2, 4, 5]                               # apart, or touching only: identically 0 around the point
                    assert abs(float(v[3]) - 1) < 1e-6
                assert torch.count_nonzero(v[zero]) == 0 and torch.count_nonzero(t1.grad[zero]) == 0 and torch.count_nonzero(t2.grad[zero]) == 0
                if method in ("grbox", "drbox"):
                    assert float(v[2]) < -0.5 and float(t1.grad[2].abs().max()) > 0 and abs(float(v[3]) - 1) < 1e-6
    # 3D: (x, y, z, lx, ly, lz, rz)
    #              z touching               z apart                  both heights 0           no BEV area            BEV apart                identical
    c = np.array([[0, 0, 0, 2, 2, 1, 0.1], [0, 0, 0, 2, 2, 1, 0.1], [0, 0, 0, 2, 2, 0, 0.1], [0, 0, 0, 0, 2, 1, 0.1], [0, 0, 0, 2, 2, 1, 0.1], [1, 2, 3, 2, 3, 4, 0.5]], np.float64)
    d = np.array([[.1, 0, 1, 2, 2, 1, 0.2], [.1, 0, 5, 2, 2, 1, 0.2], [.1, 0, 0, 2, 2, 0, 0.2], [.1, 0, 0, 2, 2, 1, 0.2], [9, 9, 0, 2, 2, 1, 0.2], [1, 2, 3, 2, 3, 4, 0.5]], np.float64)
    for x1, x2 in ((c, d), (d, c)):
        for method in pr.METHODS_3D:
            for dtype, precise in COMBOS:
                t1, t2 = T(x1.astype(dtype)).requires_grad_(True), T(x2.astype(dtype)).requires_grad_(True)
                v = box3d_iou_paired(t1, t2, method=method, precise=precise)
                v.sum().backward()
                v = v.detach()
                assert torch.isfinite(v).all() and torch.isfinite(t1.grad).all() and torch.isfinite(t2.grad).all()
                zero = [0, 1, 2, 4] + ([3] if method == "rbox" else [])
                assert torch.count_nonzero(v[zero]) == 0 and torch.count_nonzero(t1.grad[zero]) == 0 and torch.count_nonzero(t2.grad[zero]) == 0
                assert abs(float(v[5]) - 1) < 1e-6
    # the floor of the z union active with a positive overlap: the union does not move, the overlap does
    e = np.array([[0, 0, 0, 2, 2, 4e-7, 0.1]])
    f = np.array([[0, 0, 1e-7, 2, 2, 4e-7, 0.1]])
    t1, t2 = T(e).requires_grad_(True), T(f).requires_grad_(True)
    v = box3d_iou_paired(t1, t2)
    v.sum().backward()
    v = v.detach()
    assert abs(float(v[0]) - 0.3) < 1e-9                             # bev 1, overlap 3e-7 over the floor 1e-6
    assert abs(float(t1.grad[0, 2]) - 1e6) < 1e-2 and abs(float(t1.grad[0, 5]) - 0.5e6) < 1e-2       # d overlap / d z1 = 1, / d lz1 = 1/2
    assert abs(float(t2.grad[0, 2]) + 1e6) < 1e-2 and abs(float(t2.grad[0, 5]) - 0.5e6) < 1e-2


def test_plumbing():
    from d3d_amd import _lib
    from d3d_amd.box import IouType, box2d_iou_paired, box3d_iou_paired
    b1, b2, c1, c2, w = pr.seeded_pairs()
    ref2 = box2d_iou_paired(T(b1), T(b2), method="grbox")
    ref3 = box3d_iou_paired(T(c1), T(c2))
    # numpy in, numpy out; CPU tensors come back on the CPU
    out = box2d_iou_paired(b1, b2, method="grbox")
    assert isinstance(out, np.ndarray) and np.array_equal(out, ref2.cpu().numpy())
    out = box3d_iou_paired(torch.from_numpy(c1), torch.from_numpy(c2))
    assert not out.is_cuda and torch.equal(out, ref3.cpu())
    t1, t2 = torch.from_numpy(b1).requires_grad_(True), torch.from_numpy(b2)
    (box2d_iou_paired(t1, t2, method="grbox") * torch.from_numpy(w)).sum().backward()
    g1, _ = _grads(2, "grbox", b1, b2, w, np.float64, True)
    assert not t1.grad.is_cuda and torch.equal(t1.grad, g1.cpu()) and t2.grad is None
    # views: columns of a wider tensor, every second row
    wide = torch.zeros((pr.N, 8), dtype=torch.float64, device="cuda")
    wide[:, :5] = T(b1)
    assert not wide[:, :5].is_contiguous() and torch.equal(box2d_iou_paired(wide[:, :5], T(b2), method="grbox"), ref2)
    twice = torch.zeros((2 * pr.N, 7), dtype=torch.float64, device="cuda")
    twice[::2] = T(c1)
    assert torch.equal(box3d_iou_paired(twice[::2], T(c2)), ref3)
    # the current stream
    s = torch.cuda.Stream()
    x1, x2 = T(b1), T(b2)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_s = box2d_iou_paired(x1, x2, method="grbox")
    s.synchronize()
    assert torch.equal(on_s, ref2)
    # one input needs a gradient: that one gets it, the other's stays None
    for which in ((True, False), (False, True)):
        for dims, x1, x2 in ((2, b1, b2), (3, c1, c2)):
            both = _grads(dims, "rbox", x1, x2, w, np.float64, True)
            one = _grads(dims, "rbox", x1, x2, w, np.float64, True, which)
            for k in range(2):
                assert (one[k] is not None and torch.equal(one[k], both[k])) if which[k] else one[k] is None
    # twice differentiable it is not
    t1 = T(b1).requires_grad_(True)
    g, = torch.autograd.grad(box2d_iou_paired(t1, T(b2)).sum(), t1, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # the C entries: jac = NULL, n = 0, and jac in the arithmetic's type for the widened form
    lib = _lib.load()
    f1, f2 = T(b1.astype(np.float32)), T(b2.astype(np.float32))
    ious = torch.full((pr.N,), float("nan"), dtype=torch.float32, device="cuda")
    null = ctypes.c_void_p(0)
    assert lib.d3d_iou2d_paired(_lib.ptr(f1), _lib.ptr(f2), pr.N, int(IouType.RBOX), _lib.F32_WIDE, _lib.ptr(ious), null, _lib.stream_ptr()) == 0
    assert torch.equal(ious, box2d_iou_paired(f1, f2))
    jac = torch.full((pr.N, 10), float("nan"), dtype=torch.float64, device="cuda")
    ious.fill_(float("nan"))
    assert lib.d3d_iou2d_paired(_lib.ptr(f1), _lib.ptr(f2), pr.N, int(IouType.RBOX), _lib.F32_WIDE, _lib.ptr(ious), _lib.ptr(jac), _lib.stream_ptr()) == 0
    assert torch.equal(ious, box2d_iou_paired(f1, f2)) and torch.isfinite(jac).all() and int(torch.count_nonzero(jac[:, 0])) > 5
    assert lib.d3d_iou2d_paired(null, null, 0, int(IouType.RBOX), _lib.F32, null, null, _lib.stream_ptr()) == 0
    g1, g2 = T(c1), T(c2)
    out = torch.full((pr.N,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.d3d_iou3d_paired(_lib.ptr(g1), _lib.ptr(g2), pr.N, 1, _lib.F64, _lib.ptr(out), null, _lib.stream_ptr()) == 0
    assert torch.equal(out, ref3)
    assert lib.d3d_iou3d_paired(null, null, 0, 0, _lib.F64, null, null, _lib.stream_ptr()) == 0
