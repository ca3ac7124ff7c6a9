"""GPU: the one call frame and the one egress of the box fronts (d3d_amd.box), and `_lib.ship`.  Every operator takes the same
inputs as numpy arrays (where the front takes arrays), as host tensors and as CUDA tensors; each result comes back as the same kind
on the same side, all hold the same bits, and so do the gradients, which land where the inputs live.  Then one host result of 1 MiB
and more per egress that moved onto `_lib.to_caller` (page-locked, the values of the CUDA call), the layout of `_lib.ship`, and
the refusals that answer only once the library is loaded or a GPU is at hand, word for word.

Sizes: 0, 1 and 65 rows a side (65 crosses the 64-row tile of the pair kernels), 4096 points x 2 boxes for the one-launch crop.

The gradient kernels of the IoU family and of pdist sum with float atomics, whose order is not fixed: a sum of three or more terms
has different bits from run to run (tests/test_gpu_box.py says the same of them).  The upstream gradient of the matrix operators
here has one nonzero entry per row and per column, so every sum has one nonzero term and its bits are a function of the inputs:
what is compared is the front -- staging, launch, egress -- not the order of a kernel's sums.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIDES = [(0, 65), (65, 0), (1, 1), (65, 65)]
F64 = {True: np.float64, False: np.float32}


def boxes5(rng, n, dtype=np.float32):
    return np.concatenate([rng.uniform(0, 12, (n, 2)), rng.uniform(0.5, 4, (n, 2)), rng.uniform(-3.2, 3.2, (n, 1))], 1).astype(dtype)


def boxes7(rng, n, dtype=np.float32):
    return np.concatenate([rng.uniform(0, 12, (n, 3)), rng.uniform(0.5, 4, (n, 3)), rng.uniform(-3.2, 3.2, (n, 1))], 1).astype(dtype)


def points(rng, n, cols, dtype=np.float32):
    return rng.uniform(-1, 13, (n, cols)).astype(dtype)


def flat(res):
    if isinstance(res, dict):
        return [res[k] for k in sorted(res)]
    return list(res) if isinstance(res, (tuple, list)) else [res]


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return a.numel() == 0 or torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def one_per_row_and_column(rng, shape, dtype):
    up = torch.zeros(shape, dtype=dtype)
    if len(shape) == 1:
        return torch.from_numpy(rng.normal(size=shape)).to(dtype)
    k = min(shape)
    up[torch.arange(k), torch.from_numpy(rng.permutation(shape[1])[:k])] = torch.from_numpy(rng.normal(size=k)).to(dtype)
    return up


def three_ways(fn, arrays, numpy_ok, differentiable, rng, empty_on_cpu=False):
    """fn on numpy arrays, host tensors and CUDA tensors -> the CUDA call's flat results; asserts kind, side and bits"""
    runs, grads = [], []
    if numpy_ok:
        out = flat(fn(*[a.copy() for a in arrays]))
        assert all(isinstance(o, torch.Tensor if empty_on_cpu else np.ndarray) for o in out)
        runs.append([torch.as_tensor(o) for o in out])
    upstream = None
    for device in ("cpu", "cuda"):
        xs = [torch.from_numpy(a.copy()).to(device) for a in arrays]
        for x in xs[:differentiable]:
            x.requires_grad_()
        out = flat(fn(*xs))
        for o in out:
            assert isinstance(o, torch.Tensor) and o.device == (torch.device("cpu") if empty_on_cpu else xs[0].device)
        if differentiable:
            if upstream is None:
                upstream = one_per_row_and_column(rng, tuple(out[0].shape), out[0].dtype)
            out[0].backward(upstream.to(out[0].device))
            for x in xs[:differentiable]:
                assert x.grad.device == x.device and x.grad.dtype == x.dtype and x.grad.shape == x.shape
            grads.append([x.grad for x in xs[:differentiable]])
        runs.append(out)
    for other in runs[:-1]:
        assert len(other) == len(runs[-1]) and all(same_bits(a, b) for a, b in zip(other, runs[-1]))
    if differentiable:
        assert all(same_bits(a, b) for a, b in zip(grads[0], grads[1]))
        if min(len(arrays[0]), len(arrays[1])) > 1:                         # (65 weighted pairs: some of them overlap)
            assert all(bool(g.abs().sum() > 0) for g in grads[1])
    return runs[-1]


@pytest.mark.parametrize("n,m", SIDES)
@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("method", ["box", "rbox", "grbox", "drbox"])
def test_box2d_iou(method, precise, n, m):
    from d3d_amd.box import box2d_iou
    rng = np.random.default_rng(n * 100 + m)
    for dtype in (np.float32, np.float64):
        out, = three_ways(lambda a, b: box2d_iou(a, b, method=method, precise=precise), (boxes5(rng, n, dtype), boxes5(rng, m, dtype)), True, 2, rng)
        assert out.shape == (n, m) and out.dtype == torch.from_numpy(np.zeros(0, dtype)).dtype


@pytest.mark.parametrize("n,m", SIDES)
def test_matrix_operators_without_a_gradient(n, m):
    from d3d_amd import box
    rng = np.random.default_rng(n * 100 + m + 1)
    b5, c5, b7, c7 = boxes5(rng, n), boxes5(rng, m), boxes7(rng, n), boxes7(rng, m)
    for method in ("rbox", "box"):
        out, = three_ways(lambda a, b: box.iou3d(a, b, method), (b7, c7), True, 0, rng)
        assert out.shape == (n, m) and out.dtype == torch.float32
        three_ways(lambda a, b: box.iou3d_sparse(a, b, method, 0.01, return_offsets=True), (b7, c7), True, 0, rng)
        for precise in (True, False):
            pairs, values, offsets = three_ways(lambda a, b: box.box2d_iou_sparse(a, b, method, 0.01, precise, True), (b5, c5), True, 0, rng)
            assert pairs.dtype == torch.int64 and values.dtype == torch.float32 and offsets.shape == (n + 1,)
    flags = three_ways(lambda a, b: box.iou2dr_flags(a, b, which=("nx", "xflags", "nm", "mflags", "far")), (b5, c5), False, 0, rng)
    assert [tuple(f.shape) for f in flags] == [(n, m, 2), (n, m, 8), (n, m), (n, m), (n, m, 8)] and all(f.dtype == torch.uint8 for f in flags)
    for dtype in (np.float32, np.float64):                                  # points [m] against boxes [n]
        mask, = three_ways(box.crop_2dr, (points(rng, m, 2, dtype), boxes5(rng, n, dtype)), False, 0, rng)
        assert mask.shape == (n, m) and mask.dtype == torch.bool
    for axis in (0, 1, 2):                                                  # (below 4096 points: the composition around crop_2dr)
        mask, = three_ways(lambda p, b: box.box3dp_crop(p, b, axis), (points(rng, m, 3), b7), False, 0, rng)
        assert mask.shape == (n, m) and mask.dtype == torch.bool


@pytest.mark.parametrize("n", [0, 1, 65])
def test_paired_operators(n):
    from d3d_amd import box
    rng = np.random.default_rng(n + 7)
    grads = 2 if n else 0                                                   # (no pair: the fronts answer without a graph)
    for precise in (True, False):
        for dtype in (np.float32, np.float64):
            a5, a7 = boxes5(rng, n, dtype), boxes7(rng, n, dtype)
            b5, b7 = (a5 + rng.normal(size=a5.shape) * 0.3).astype(dtype), (a7 + rng.normal(size=a7.shape) * 0.3).astype(dtype)
            for method in ("box", "rbox", "grbox", "drbox"):
                out, = three_ways(lambda a, b: box.box2d_iou_paired(a, b, method, precise), (a5, b5), True, grads, rng)
                assert out.shape == (n,)
            for method in ("box", "rbox"):
                out, = three_ways(lambda a, b: box.box3d_iou_paired(a, b, method, precise), (a7, b7), True, grads, rng)
                assert out.shape == (n,)


@pytest.mark.parametrize("n", [0, 1, 65])
def test_nms_fronts(n):
    """(the empty case answers with a CPU tensor whatever came in: box2d_nms's, from the reference)"""
    from d3d_amd import box
    rng = np.random.default_rng(n + 11)
    b, s, g = boxes5(rng, n), rng.uniform(size=n).astype(np.float32), rng.integers(-2, 2, size=n)
    for precise in (True, False):
        for method in ("box", "rbox"):
            keep, = three_ways(lambda x, y: box.box2d_nms(x, y, method, "hard", 0.3, 0.1, 0, precise), (b, s), True, 0, rng, empty_on_cpu=n == 0)
            assert keep.shape == (n,) and keep.dtype == torch.bool
            keep, = three_ways(lambda x, y, z: box.box2d_nms_batched(x, y, z, method, "hard", 0.3, 0.1, 0, precise), (b, s, g), True, 0, rng,
                               empty_on_cpu=n == 0)
            assert keep.shape == (n,) and keep.dtype == torch.bool
    soft, = three_ways(lambda x, y: box.box2d_nms(x, y, "rbox", "gaussian", 0.3, 0.1, 0.5), (b, s), True, 0, rng, empty_on_cpu=n == 0)
    assert soft.shape == (n,)


@pytest.mark.parametrize("n,m", SIDES)
def test_pdist_operators(n, m):
    from d3d_amd import box
    rng = np.random.default_rng(n * 100 + m + 3)
    for dtype in (np.float32, np.float64):
        out, = three_ways(box.box2dr_pdist, (points(rng, m, 2, dtype), boxes5(rng, n, dtype)), False, 2, rng)
        assert out.shape == (n, m)
        for axis in (0, 1, 2):
            # box3dr_pdist composes the planar kernel with tensor arithmetic on the caller's device; its corner branch (a point
            # outside both in the plane and along the axis) takes torch.sqrt of a sum of squares, which the host and the GPU
            # round differently.  The boxes here span every point along the axis, so the composition is exact on both sides.
            b7 = boxes7(rng, n, dtype)
            b7[:, 3 + axis] += 30
            out, = three_ways(lambda p, b: box.box3dr_pdist(p, b, axis), (points(rng, m, 3, dtype), b7), False, 2, rng)
            assert out.shape == (n, m)


def test_one_launch_crop_4096_points_by_2_boxes():
    from d3d_amd import box
    rng = np.random.default_rng(4)
    p, b = points(rng, 4096, 4), boxes7(rng, 2)
    b[:, 3:6] *= 3                                                          # (large enough to hold points)
    mask, = three_ways(box.box3dp_crop, (p, b), False, 0, rng)
    assert mask.shape == (2, 4096) and mask.dtype == torch.bool and bool(mask.any())
    composed = box.crop_2dr(torch.from_numpy(p[:, :2].copy()).cuda(), torch.from_numpy(b[:, [0, 1, 3, 4, 6]].copy()).cuda())
    assert not bool((mask.cuda() & ~composed).any())                        # (inside the box: inside its footprint)


def test_host_results_of_1_mib_and_more_are_page_locked_and_equal():
    """the four egresses that moved onto _lib.to_caller, each with a host result above the threshold against the CUDA call"""
    from d3d_amd import _lib, box
    rng = np.random.default_rng(9)
    big = _lib._PINNED_RESULT_MIN_BYTES

    def check(host, dev, pinned, summed=False):
        host, dev = flat(host), flat(dev)
        assert len(host) == len(dev)
        for h, d, pin in zip(host, dev, pinned):
            assert h.device.type == "cpu" and d.is_cuda and h.dtype == d.dtype and h.shape == d.shape
            assert (h.numel() * h.element_size() >= big) == pin and h.is_pinned() == pin
            if pin or not summed:
                assert same_bits(h, d)
            else:   # the one partner's gradient: 26400 fp64 terms t in an order that is not fixed; two orders differ by less than
                    # n * 2^-52 * sum |t| < 26400 * 2.3e-16 * (26400 * 8) = 1.3e-6 (the upstream is clamped to +-4, |derivative| < 2)
                assert float((h - d.cpu()).abs().max()) < 1.3e-6

    p, b = torch.from_numpy(points(rng, 400, 2, np.float64)), torch.from_numpy(boxes5(rng, 400, np.float64))
    check(box.pdist2dr_forward(p, b), box.pdist2dr_forward(p.cuda(), b.cuda()), (True, False))          # 1.28 MB of fp64, 160 kB of uint8
    which = ("xflags", "nx")
    check(box.iou2dr_flags(b, b, which), box.iou2dr_flags(b.cuda(), b.cuda(), which), (False, True))    # sorted names: nx 160 kB, xflags 1.28 MB
    # [26400, 5] fp64 = 1.056 MB against ONE partner: a single term per sum, whose bits no order of the atomics changes
    many, one_p, one_b = torch.from_numpy(boxes5(rng, 26400, np.float64)), p[:1] * 0 + 6, b[:1].clone()
    one_b[0, :4] = torch.tensor([6.0, 6.0, 14.0, 14.0], dtype=torch.float64)
    g = torch.from_numpy(rng.normal(size=(26400, 1))).clamp(-4, 4)
    check(box.pdist2dr_backward(one_p, many, g), box.pdist2dr_backward(one_p.cuda(), many.cuda(), g.cuda()), (True, False), summed=True)
    check(box._iou_backward(many, one_b, g, box.IouType.RBOX), box._iou_backward(many.cuda(), one_b.cuda(), g.cuda(), box.IouType.RBOX),
          (True, False), summed=True)


def test_host_results_of_the_point_and_transform_fronts_above_1_mib():
    """crop_points, transform_points, project_points_to_camera and aligned_scatter_forward leave through _lib.to_caller as well: a
    host result above the threshold each, page-locked, with the bits of the CUDA call; numpy in still gives numpy out"""
    from d3d_amd import _lib
    from d3d_amd.abstraction import TransformSet, crop_points
    from d3d_amd.point import AlignType, aligned_scatter_forward
    rng = np.random.default_rng(13)
    big = _lib._PINNED_RESULT_MIN_BYTES

    def check(host, dev, pinned):
        host, dev = flat(host), flat(dev)
        assert len(host) == len(dev)
        for h, d, pin in zip(host, dev, pinned):
            assert h.device.type == "cpu" and d.is_cuda and same_bits(h, d)
            assert (h.numel() * h.element_size() >= big) == pin and h.is_pinned() == pin

    cloud = np.concatenate([rng.uniform(5, 50, (600000, 1)), rng.uniform(-2, 2, (600000, 2))], 1).astype(np.float32)       # in front, in view
    boxes = np.array([[20, 0, 0, 30, 3, 3, 0.3], [40, 1, 0, 8, 2, 5, -1.0]], np.float32)
    pts, bx = torch.from_numpy(cloud), torch.from_numpy(boxes)
    inside = crop_points(bx, pts)                                            # bool [2, 600000]: 1.2 MB
    check(inside, crop_points(bx.cuda(), pts.cuda()), (True,))
    assert bool(inside.any()) and not bool(inside.all())
    as_numpy = crop_points(boxes, cloud)
    assert isinstance(as_numpy, np.ndarray) and np.array_equal(as_numpy, inside.numpy())

    ts = TransformSet("base")
    ts.set_intrinsic_lidar("lidar")
    ts.set_extrinsic(np.array([[0.96, -0.28, 0, 1.5], [0.28, 0.96, 0, -0.5], [0, 0, 1, 2.0], [0, 0, 0, 1]]), frame_to="lidar")
    ts.set_intrinsic_pinhole("cam", (1600, 1200), 800, 600, 500, 500)
    ts.set_extrinsic(np.eye(4), frame_to="cam")
    few = pts[:80000]
    check(ts.transform_points(few, "lidar"), ts.transform_points(few.cuda(), "lidar"), (True,))                             # fp64 [80000, 3]
    host, dev = ts.project_points_to_camera(few, "cam"), ts.project_points_to_camera(few.cuda(), "cam")
    assert len(host[1]) == 80000                                             # every point in view: uv fp64 [80000, 2], mask int64 [80000]
    check(host, dev, (True, False))
    uv, mask = ts.project_points_to_camera(cloud[:80000], "cam")
    assert isinstance(uv, np.ndarray) and np.array_equal(uv, host[0].numpy()) and np.array_equal(mask, host[1].numpy())

    feat = torch.from_numpy(rng.normal(size=(1, 4, 8, 8)).astype(np.float32))
    coord = torch.from_numpy(np.concatenate([np.zeros((70000, 1)), rng.uniform(0, 7, (70000, 2))], 1).astype(np.float32))
    check(aligned_scatter_forward(coord, feat, AlignType.LINEAR), aligned_scatter_forward(coord.cuda(), feat.cuda(), AlignType.LINEAR), (True,))


def test_ship():
    """i64, i32, f32 and u8 pieces of 0, 1, 3 and 5 elements in an order that misaligns every wider piece unless its start is padded"""
    from d3d_amd import _lib
    rng = np.random.default_rng(2)
    dtypes = (np.uint8, np.int64, np.float32, np.int32)
    pieces = []
    for length in (5, 0, 1, 3):                                             # u8[5] i64[5] f32[5] i32[5] u8[0] ... u8[3] i64[3] ...
        pieces += [(rng.integers(0, 200, size=length) - 100 * (dt != np.uint8)).astype(dt) for dt in dtypes]
    pieces.append(rng.normal(size=(3, 1, 5)).astype(np.float32))            # (a shape of its own)
    dev = torch.device("cuda", torch.cuda.current_device())
    views = _lib.ship(dev, *pieces)
    assert len(views) == len(pieces)
    for a, v in zip(pieces, views):
        assert v.device == dev and v.dtype == torch.from_numpy(a).dtype and tuple(v.shape) == a.shape
        assert np.array_equal(v.cpu().numpy(), a) and v.data_ptr() % 8 == 0
        assert bool((v + 1 == torch.from_numpy(a).to(dev) + 1).all())       # (a kernel reads the view as it lies)


def refused(exc, message, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == message


def test_refusals_that_answer_after_the_library_is_loaded():
    from d3d_amd import box
    from d3d_amd.tracking import matcher
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)      # noqa: E731
    f7 = "Input boxes should have 7 fields: x, y, z, lx, ly, lz, rz"
    refused(AssertionError, "Input should be both numpy tensor or pytorch tensor!", box.iou3d, np.zeros((3, 7)), z(3, 7))
    refused(ValueError, "Unrecognized iou type!", box.iou3d, z(3, 6), z(3, 7), "grbox")                 # the name before the width
    refused(ValueError, "Unrecognized iou type!", box.iou3d, z(3, 7), z(3, 7), "circle")
    for bad in (z(7), z(3, 6), z(3, 8)):
        refused(ValueError, f7, box.iou3d, bad, z(3, 7))
        refused(ValueError, f7, box.iou3d, z(3, 7).cuda(), bad)
    for fn in (box.crop_2dr, box.pdist2dr_forward, box.box2dr_crop):
        for p, b in ((z(4), z(3, 5)), (z(4, 3), z(3, 5)), (z(4, 2), z(5)), (z(4, 2), z(3, 4))):
            refused(ValueError, "points should be Nx2 and boxes Mx5", fn, p, b)
        refused(RuntimeError, "points and boxes must have the same dtype", fn, z(4, 2), z(3, 5).double())
        refused(RuntimeError, "boxes must be float32 or float64", fn, z(4, 2).int(), z(3, 5).int())
    refused(ValueError, "Unsupported iou type!", box.nms2d, z(3, 5), z(3), box.IouType.GRBOX, 0, 0.5, 0, 0)
    refused(ValueError, "Unsupported supression type!", box.nms2d, z(3, 5), z(3), box.IouType.BOX, 3, 0.5, 0, 0)
    refused(RuntimeError, "boxes and scores must have the same dtype", box.nms2d, z(3, 5), z(3).double(), 1, 0, 0.5, 0, 0)
    refused(ValueError, "wide32 takes fp32 boxes and scores", box.nms2d, z(3, 5).double(), z(3).double(), 1, 0, 0.5, 0, 0, wide32=True)
    refused(RuntimeError, "boxes1 and boxes2 must have the same dtype", box.iou2d_forward, z(3, 5), z(3, 5).double())
    mixed = "matrix32 takes fp64 boxes, wide32 fp32 boxes, both the box / rbox methods"
    refused(ValueError, mixed, box._iou_forward, z(3, 5), z(3, 5), box.IouType.RBOX, matrix32=True)
    refused(ValueError, mixed, box._iou_forward, z(3, 5), z(3, 5), box.IouType.GRBOX, wide32=True)
    refused(ValueError, mixed, box._iou_backward, z(3, 5).double(), z(3, 5).double(), z(3, 3), box.IouType.BOX, wide32=True)
    rows9 = "%s should be [n,9] rows of (label, score, x, y, z, lx, ly, lz, yaw)"
    refused(ValueError, rows9 % "src_boxes", matcher.prepare_boxes, z(3, 8), z(3, 9), 1)
    refused(ValueError, rows9 % "dst_boxes", matcher.prepare_boxes, z(3, 9), z(3, 8), 1)
    for fn in (matcher.hungarian_match, matcher.nearest_neighbor_match):
        d = z(3, 4)
        refused(ValueError, "src_tags should hold one tag per box (3), got 4", fn, d, [0] * 4, [0] * 4, {0: 1.0})
        refused(ValueError, "dst_tags should hold one tag per box (4), got 3", fn, d.cuda(), [0] * 3, np.zeros(3), {0: 1.0})
        refused(ValueError, "src_tags should hold one tag per box (3), got 2", fn, d, [0] * 2, [0] * 4, {}, [5], [9])     # tags before subsets
        refused(ValueError, "src_subset holds an index outside 0 .. 2", fn, d, [0] * 3, [0] * 4, {}, [0, 3], [4])           # sources first
        refused(ValueError, "src_subset holds an index outside 0 .. 2", fn, d, [0] * 3, [0] * 4, {}, torch.tensor([-1]))
        refused(ValueError, "dst_subset holds an index outside 0 .. 3", fn, d, [0] * 3, [0] * 4, {}, None, np.array([4]))
