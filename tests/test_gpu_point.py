"""aligned_scatter on the GPU, both launch routes (point.hip: plain = one lane per (point, channel) on the [B, C, D..] map;
channels-last = the map transposed into the workspace through 32 x 32 LDS tiles, taken for C >= 8 when a workspace that
holds the map is passed), against the C oracle (forward: bit for bit) and the fp64 model of tests/point_reference.py
(every element of forward and backward, bounds of point_reference.forward_bound / backward_bound; no element is skipped
or masked, no tolerance is a constant).

The bounds count (K + 3 dim + 4) u A for the backward and (2^dim + 3 dim + 2) u S for the forward, PLUS the term E of
point_reference: the first operation of a LINEAR factor, 1 + x or 1 - x, rounds to the spacing of 1 +- x and not of the factor,
an absolute error of up to u |1 +- x| per factor that a count of relative roundings of the term does not hold.  The real
reference's recorded outputs miss the count without E (tests/test_point.py::test_model_matches_reference_forward: 5.7 x on
c1), the C oracle misses it by up to 800 x on the (1000,) map in fp32; with E the worst forward element stands at 0.99 of
its bound.  E is zero for MEAN.

Grid (point_reference.grid()): a covering subset of atype x dtype x C x map x B x n.  Every C in (1, 5, 7, 8, 9, 31, 32, 33,
64, 100) meets every one of the 12 maps once; method, dtype, B, the point count and a started image_grad rotate along both
axes, so each C and each map sees both methods, both dtypes and B = 1, 2, 3.  Left out: the other three (method, dtype)
pairs of each (C, map) cell; n C = 255 / 256 / 257 at C other than 1, 5, 8, 32, 64; 70 001 points on maps other than (1000,),
(40, 50), (32, 32), (8, 8, 8), (7, 11, 13); 200 000 points in fp32 on (7, 11, 13) (a corner cell collects 7000 contributions,
past the fp32 cap K <= 4000; fp64 there) and hot cells at C other than 5, 8, 9, 32, 33, 64.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import point_reference as pr

pytestmark = pytest.mark.gpu

GRID = pr.grid()
F32, F64 = np.float32, np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def poison_arena(shape, dtype):
    """the Python layer's arena for this map, dirty: the backward's staging buffer must be cleared by the operator"""
    from d3d_amd import _lib
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize + 512
    _lib.workspace(nbytes, torch.device("cuda", torch.cuda.current_device()))[:nbytes].fill_(0x5a)


def worst(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def check_forward(got, coord, image, atype, what):
    """every element: the oracle's bits, and the model within forward_bound"""
    want = oracle.aligned_scatter_forward(coord, image, atype)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, "bits differ from the oracle at", int(np.sum(got != want)), "elements")
    u, dim = pr.unit(image.dtype), coord.shape[1] - 1
    out, S, E = pr.forward_terms(coord, image, atype, u)
    err, bound = np.abs(got - out), pr.forward_bound(S, dim, u, E)
    print(what, "forward worst error / bound %.3f" % worst(err, bound))
    assert np.all(err <= bound), (what, worst(err, bound))


def check_backward(got, coord, grad, atype, init, what, cap=True):
    """every element of image_grad: |got - exact| <= (K + 3 dim + 4) u A + E"""
    u, dim = pr.unit(grad.dtype), coord.shape[1] - 1
    exact, K, A, E = pr.backward_terms(coord, grad, atype, got.shape, init, u)
    if cap and grad.dtype == F32 and K.size:
        assert K.max() <= pr.K_CAP, what                        # keeps the bound below 2^-12 A + E
    err, bound = np.abs(got - exact), pr.backward_bound(K, A, dim, u, E)
    print(what, "backward worst error / bound %.3f, K max %d" % (worst(err, bound), K.max() if K.size else 0))
    assert got.dtype == grad.dtype and np.all(err <= bound), (what, worst(err, bound), int(np.sum(~(err <= bound))))


def raw(fn, coord, a, b, shape, atype, ws, wsb, dtype=None, n=None, dim=None, dims=None, stream=None):
    """the C entry as it is: fn = "forward" (a = image, b = out) or "backward" (a = grad, b = image_grad)"""
    from d3d_amd import _lib
    lib = _lib.load()
    dims = list(shape[2:]) if dims is None else dims
    dims_h = (ctypes.c_int64 * max(len(dims), 1))(*dims)
    code = dtype if dtype is not None else (_lib.F64 if a.dtype == torch.float64 else _lib.F32)
    return getattr(lib, "d3d_aligned_scatter_" + fn)(
        _lib.ptr(coord), coord.shape[0] if n is None else n, len(shape) - 2 if dim is None else dim, _lib.ptr(a), shape[0], shape[1],
        ctypes.cast(dims_h, ctypes.c_void_p), int(atype), code, _lib.ptr(b), _lib.ptr(ws) if ws is not None else None, wsb, stream)


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_grid(case):
    from d3d_amd import _lib
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    coord, image, grad, init = case.make()
    c, f, g = dev(coord), dev(image), dev(grad)
    at = AlignType(case.atype)
    poison_arena(case.shape, case.dtype)
    got = host(aligned_scatter_forward(c, f, at))
    check_forward(got, coord, image, case.atype, case.id)
    if case.C >= 8 and case.n:                                   # the same call without a workspace: plain route, same bits
        out = torch.full((case.n, case.C), float("nan"), dtype=f.dtype, device="cuda")
        assert raw("forward", c, f, out, case.shape, at, None, 0) == _lib.OK
        assert np.array_equal(host(out), got), case.id
    poison_arena(case.shape, case.dtype)
    ig = dev(init) if case.init else torch.zeros(case.shape, dtype=f.dtype, device="cuda")
    aligned_scatter_backward(c, g, at, ig)
    check_backward(host(ig), coord, grad, case.atype, init, case.id)


# ------------------------------------------------------------------------------------------------------- the raw C entry
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("atype", [pr.MEAN, pr.LINEAR], ids=["mean", "linear"])
def test_raw_entry_routes_by_workspace(dtype, atype):
    """full workspace (channels-last), NULL and one byte short of the map (plain): same forward bits, backward within the
    bound into a started image_grad, and a workspace the call may not use keeps its poison"""
    from d3d_amd import _lib
    lib = _lib.load()
    case = pr.Case(atype, dtype, 33, (7, 11, 13), 2, 5000, init=True, seed=7)
    coord, image, grad, init = case.make()
    c, f, g = dev(coord), dev(image), dev(grad)
    dims_h = (ctypes.c_int64 * 3)(*case.dims)
    wsb = lib.d3d_aligned_scatter_workspace_bytes(case.B, case.C, ctypes.cast(dims_h, ctypes.c_void_p), 3, _lib.F64 if dtype == F64 else _lib.F32)
    map_bytes = image.size * image.itemsize
    assert wsb >= map_bytes
    fwd = []
    for name, nbytes, passed in (("full", wsb, wsb), ("null", wsb, None), ("short", map_bytes - 1, map_bytes - 1)):
        ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda")
        out = torch.full((case.n, case.C), float("nan"), dtype=f.dtype, device="cuda")
        assert raw("forward", c, f, out, case.shape, atype, ws if passed else None, passed or 0) == _lib.OK
        check_forward(host(out), coord, image, atype, name)
        fwd.append(host(out))
        if name != "full":
            assert bool((ws == 0x5a).all()), name
        ws.fill_(0x5a)
        ig = dev(init)
        assert raw("backward", c, g, ig, case.shape, atype, ws if passed else None, passed or 0) == _lib.OK
        check_backward(host(ig), coord, grad, atype, init, name)
        if name != "full":
            assert bool((ws == 0x5a).all()), name
    assert np.array_equal(fwd[0], fwd[1]) and np.array_equal(fwd[0], fwd[2])


def test_raw_entry_workspace_query_and_status_codes():
    from d3d_amd import _lib
    lib = _lib.load()
    query = lib.d3d_aligned_scatter_workspace_bytes
    d3 = (ctypes.c_int64 * 3)(7, 11, 13)
    p3 = ctypes.cast(d3, ctypes.c_void_p)
    for args in ((0, 33, p3, 3, _lib.F32), (2, 0, p3, 3, _lib.F32), (2, 33, None, 3, _lib.F32), (2, 33, p3, 0, _lib.F32),
                 (2, 33, p3, 4, _lib.F32), (-1, 33, p3, 3, _lib.F64)):
        assert query(*args) == 256, args
    assert query(2, 33, p3, 3, _lib.F32) >= 2 * 33 * 1001 * 4 and query(2, 33, p3, 3, _lib.F64) >= 2 * 33 * 1001 * 8
    assert query(1, 1, p3, 1, _lib.F32) >= 7 * 4
    shape = (2, 33, 7, 11, 13)
    c = torch.zeros((4, 4), device="cuda")
    f = torch.zeros(shape, device="cuda")
    g = torch.zeros((4, 33), device="cuda")
    for fn, a, b in (("forward", f, g), ("backward", g, f)):
        for dim in (0, 4):
            assert raw(fn, c, a, b, shape, 1, None, 0, dim=dim, dims=[7, 11, 13, 2][:max(dim, 1)]) == _lib.ERR_UNSUPPORTED
        for atype in (0, 3, 4):
            assert raw(fn, c, a, b, shape, atype, None, 0) == _lib.ERR_UNSUPPORTED
        assert raw(fn, c, a, b, shape, 2, None, 0, dtype=7) == _lib.ERR_BAD_ARG
        assert raw(fn, c, a, b, shape, 2, None, 0, dtype=_lib.F64_M32) == _lib.ERR_BAD_ARG
        assert raw(fn, c, a, b, shape, 2, None, 0, n=-1) == _lib.ERR_BAD_ARG
        for dims in ([0, 11, 13], [7, -1, 13], [7, 11, 0]):
            assert raw(fn, c, a, b, shape, 2, None, 0, dims=dims) == _lib.ERR_BAD_ARG
        assert raw(fn, None, None, None, shape, 2, None, 0, n=0, dtype=_lib.F32) == _lib.OK
        assert raw(fn, None, None, None, (2, 0, 7, 11, 13), 1, None, 0, n=4, dtype=_lib.F64) == _lib.OK
    torch.cuda.synchronize()
    assert not f.any() and not g.any()                           # no refused call wrote anything


# ------------------------------------------------------------------------------------------------------ the Python layer
LAYER = [pr.Case(at, dt, C, (3, 4, 5), 2, 200, init=True, seed=11) for at in (pr.MEAN, pr.LINEAR) for dt in (F32, F64) for C in (3, 9)]


@pytest.mark.parametrize("case", LAYER, ids=lambda c: c.id)
def test_non_contiguous_arguments_and_copy_back(case):
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    coord, image, grad, init = case.make()
    at = AlignType(case.atype)
    c = dev(np.concatenate([coord, coord], 1))[:, :case.dim + 1]                 # a column slice of a wider tensor
    f = dev(np.ascontiguousarray(np.moveaxis(image, 1, -1))).permute(0, 4, 1, 2, 3)       # channels-last memory
    g = dev(np.ascontiguousarray(grad.T)).t()
    assert not c.is_contiguous() and not f.is_contiguous() and not g.is_contiguous()
    check_forward(host(aligned_scatter_forward(c, f, at)), coord, image, case.atype, case.id)
    ig = dev(np.ascontiguousarray(np.moveaxis(init, 1, -1))).permute(0, 4, 1, 2, 3)       # a view: the result must reach it
    base = ig.data_ptr()
    assert not ig.is_contiguous()
    aligned_scatter_backward(c, g, at, ig)
    assert ig.data_ptr() == base and not ig.is_contiguous()
    check_backward(host(ig), coord, grad, case.atype, init, case.id)


@pytest.mark.parametrize("case", LAYER, ids=lambda c: c.id)
def test_cpu_tensors_in_and_out(case):
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    coord, image, grad, init = case.make()
    at = AlignType(case.atype)
    out = aligned_scatter_forward(torch.from_numpy(coord), torch.from_numpy(image), at)
    assert out.device.type == "cpu"
    check_forward(out.numpy(), coord, image, case.atype, case.id)
    ig = torch.from_numpy(init.copy())
    aligned_scatter_backward(torch.from_numpy(coord), torch.from_numpy(grad), at, ig)
    assert ig.device.type == "cpu"
    check_backward(ig.numpy(), coord, grad, case.atype, init, case.id)


@pytest.mark.parametrize("case", [pr.Case(pr.LINEAR, F32, 33, (40, 50), 2, 20000, init=True, seed=12),
                                  pr.Case(pr.MEAN, F64, 5, (7, 11, 13), 3, 20000, init=True, seed=12)], ids=lambda c: c.id)
def test_non_default_stream(case):
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    coord, image, grad, init = case.make()
    c, f, g, ig = dev(coord), dev(image), dev(grad), dev(init)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = aligned_scatter_forward(c, f, AlignType(case.atype))
        aligned_scatter_backward(c, g, AlignType(case.atype), ig)
    s.synchronize()
    check_forward(host(out), coord, image, case.atype, case.id)
    check_backward(host(ig), coord, grad, case.atype, init, case.id)


@pytest.mark.parametrize("case", LAYER, ids=lambda c: c.id)
def test_two_backward_calls_accumulate(case):
    from d3d_amd.point import AlignType, aligned_scatter_backward
    coord, image, grad, init = case.make()
    rng = np.random.default_rng(13)
    coord2 = np.concatenate([coord[::2], coord[1::4]])
    grad2 = rng.standard_normal((len(coord2), case.C)).astype(case.dtype)
    ig = dev(init)
    aligned_scatter_backward(dev(coord), dev(grad), AlignType(case.atype), ig)
    first = host(ig).copy()
    aligned_scatter_backward(dev(coord2), dev(grad2), AlignType(case.atype), ig)
    # the second call starts from the first's result, rounded where it stands; both calls' terms count
    check_backward(host(ig), coord2, grad2, case.atype, first, case.id)
    exact, K, A, E = pr.backward_terms(np.concatenate([coord, coord2]), np.concatenate([grad, grad2]), case.atype, case.shape, init, case.u)
    # ... and against both calls' terms at once, each call with its own 3 dim + 4
    assert np.all(np.abs(host(ig) - exact) <= pr.backward_bound(K + 3 * case.dim + 4, A, case.dim, case.u, E))


@pytest.mark.parametrize("case", LAYER, ids=lambda c: c.id)
def test_autograd_backward_with_a_random_gradient(case):
    from d3d_amd.point import aligned_scatter
    coord, image, grad, _ = case.make()
    c = dev(coord).requires_grad_(True)
    f = dev(image).requires_grad_(True)
    out = aligned_scatter(c, f, "mean" if case.atype == pr.MEAN else "linear")
    check_forward(host(out), coord, image, case.atype, case.id)
    out.backward(dev(grad))
    assert c.grad is None and f.grad.shape == f.shape
    check_backward(host(f.grad), coord, grad, case.atype, None, case.id)


@pytest.mark.parametrize("method", ["mean", "linear"])
@pytest.mark.parametrize("C", [3, 9], ids=["plain", "channels-last"])
def test_gradcheck_fp64(method, C):
    from d3d_amd.point import aligned_scatter
    case = pr.Case(pr.MEAN if method == "mean" else pr.LINEAR, F64, C, (3, 4, 5), 2, 24, init=False, seed=14)
    coord, image, _, _ = case.make()
    eps = 2.0 ** -10
    # the operator is linear in the map, so a central difference errs by rounding alone: two forward errors over 2 eps
    # (forward_bound on the map moved by eps); the analytic column is one backward of at most 8 n terms of at most 1 each,
    # whose weights carry at most dim u max(D) of absolute error
    _, S, E = pr.forward_terms(coord, np.abs(image) + eps, case.atype, case.u)
    terms = 8 * case.n
    atol = float(np.max(pr.forward_bound(S, case.dim, case.u, E))) / eps \
        + pr.backward_bound(terms, terms, case.dim, case.u, terms * case.dim * case.u * max(case.dims))
    f = dev(image).requires_grad_(True)
    c = dev(coord)
    assert torch.autograd.gradcheck(lambda m: aligned_scatter(c, m, method), (f,), eps=eps, atol=atol, rtol=0.0, nondet_tol=atol)


def test_forward_is_bit_identical_run_to_run():
    """(not asserted for the fp32 backward: the atomics reorder)"""
    from d3d_amd.point import AlignType, aligned_scatter_forward
    for case in (pr.Case(pr.LINEAR, F32, 64, (40, 50), 2, 100000, init=False, seed=15), pr.Case(pr.MEAN, F64, 7, (7, 11, 13), 3, 50000, init=False, seed=15)):
        coord, image, _, _ = case.make()
        c, f = dev(coord), dev(image)
        first = host(aligned_scatter_forward(c, f, AlignType(case.atype)))
        for _ in range(3):
            poison_arena(case.shape, case.dtype)
            assert np.array_equal(host(aligned_scatter_forward(c, f, AlignType(case.atype))), first)


# ----------------------------------------------------------------------------------------------------------- index width
WIDE_SHAPE = (2, 64, 256, 256, 256)                              # 2^31 elements: the last channel planes of the last batch lie
WIDE_MUL, WIDE_MASK = 2654435761, (1 << 24) - 1                  # past every 32-bit product of batch, channel and volume


def wide_value(flat):
    """element `flat` of the large map: ((flat 2654435761) mod 2^24) / 2^24, exact in fp32 -- the host evaluates any cell
    without holding the map"""
    return ((np.asarray(flat).astype(np.uint64) * np.uint64(WIDE_MUL)) & np.uint64(WIDE_MASK)).astype(np.float64) / 2.0 ** 24


def test_flat_offsets_past_2_31_on_both_routes():
    """about 26 GB of device memory: the map, its channels-last copy in the arena, and image_grad"""
    from d3d_amd import _lib
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    B, C = WIDE_SHAPE[:2]
    vol = 256 ** 3
    total = B * C * vol
    image = torch.empty(WIDE_SHAPE, dtype=torch.float32, device="cuda")
    flat_view, step = image.view(-1), 1 << 26
    for lo in range(0, total, step):                             # (2^31 - 1) 2654435761 < 2^63
        i = torch.arange(lo, lo + step, dtype=torch.int64, device="cuda")
        flat_view[lo:lo + step] = ((i * WIDE_MUL) & WIDE_MASK).to(torch.float32) / float(1 << 24)
        del i
    probe = np.array([0, 1, 12345678901 % total, total - 2, total - 1])
    assert np.array_equal(host(flat_view[torch.from_numpy(probe).cuda()]).astype(np.float64), wide_value(probe))
    case = pr.Case(pr.LINEAR, F32, C, WIDE_SHAPE[2:], B, 100000, init=False, seed=16)
    coord, _, grad, _ = case.make_points()
    coord[len(coord) // 4:, 0] = B - 1                           # three quarters of the points read the last batch
    coord[[4, 7], 0] = B - 1                                     # ... the rows past the far corner among them
    assert np.any(np.all(coord[:, 1:] > 255, 1) & (coord[:, 0] == B - 1))        # ... one of them the map's last element
    c, g = dev(coord), dev(grad)
    fetch = lambda b, ch, cell: wide_value((b * C + ch) * vol + cell)  # noqa: E731
    out, S, E = pr.forward_terms(coord, fetch, pr.LINEAR, case.u, dims=(C,) + WIDE_SHAPE[2:])
    bound = pr.forward_bound(S, 3, case.u, E)
    got = host(aligned_scatter_forward(c, image, AlignType.LINEAR))                  # channels-last
    assert np.all(np.abs(got - out) <= bound), worst(np.abs(got - out), bound)
    plain = torch.full((case.n, C), float("nan"), dtype=torch.float32, device="cuda")
    assert raw("forward", c, image, plain, WIDE_SHAPE, 2, None, 0) == _lib.OK
    assert np.array_equal(host(plain), got)
    del image, flat_view, plain

    flat, exact, K, A, E = pr.backward_sparse(coord, grad, pr.LINEAR, WIDE_SHAPE, case.u)
    assert flat.max() == total - 1 and K.max() <= pr.K_CAP
    bound = pr.backward_bound(K, A, 3, case.u, E)
    where = torch.from_numpy(flat).cuda()
    ig = torch.zeros(WIDE_SHAPE, dtype=torch.float32, device="cuda")
    for route in ("channels-last", "plain"):
        if route == "plain":
            ig.zero_()
            assert raw("backward", c, g, ig, WIDE_SHAPE, 2, None, 0) == _lib.OK
        else:
            poison_arena(WIDE_SHAPE, F32)
            aligned_scatter_backward(c, g, AlignType.LINEAR, ig)
        vals = ig.view(-1)[where]
        err = np.abs(host(vals).astype(np.float64) - exact)
        assert np.all(err <= bound), (route, worst(err, bound))
        # everything else is exactly zero: as many non-zero elements in the whole map as among the model's
        everywhere = sum(int(torch.count_nonzero(ig.view(-1)[lo:lo + (1 << 28)])) for lo in range(0, total, 1 << 28))
        assert everywhere == int(torch.count_nonzero(vals)), route
        assert everywhere >= int(np.sum(np.abs(exact) > bound)), route      # an element whose sum exceeds its bound cannot be zero
