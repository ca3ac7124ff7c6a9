"""GPU: the sparse IoU operators (box2d_iou_sparse / iou3d_sparse, boxsparse.hip).  For every scene of sparse_iou_cases.py, method,
dtype route and threshold: pairs, values and offsets are those of the library's own matrix operator through nonzero -- indices
equal, values bit for bit -- and, independently, the pair set is the oracle's wherever the oracle's value is not a rounding tie
with the threshold.  Then the paired operators on the listed pairs (the same bits), the plumbing around the call, the raw C
entries, and one 4000 x 3000 case that crosses several workgroups and LDS column chunks."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import sparse_iou_cases as sc
from d3d_amd import _lib, synth

pytestmark = pytest.mark.gpu

# (name, numpy dtype of the boxes, precise)
ROUTES_2D = (("fp32", np.float32, False), ("fp32-precise", np.float32, True), ("fp64", np.float64, True))
ROUTES_3D = (("fp32", np.float32, None),)
# The band around the threshold inside which the oracle does not decide a pair.  fp64 arithmetic: sc.TIE, on the oracle's value
# rounded to the stored type like ours.  fp32 arithmetic (fp32 boxes without `precise`, the 7-column operator): the clip sums
# cross products of coordinates up to ~100 with 2^-24 relative error each, ~1e-6 of an IoU; ten times that.
TIE_F32 = 1e-5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dense_op(dims, method, precise):
    from d3d_amd.box import box2d_iou, iou3d
    return (lambda a, b: box2d_iou(a, b, method=method, precise=precise)) if dims == 2 else (lambda a, b: iou3d(a, b, method))


def sparse_op(dims, method, precise):
    from d3d_amd.box import box2d_iou_sparse, iou3d_sparse
    if dims == 2:
        return lambda a, b, t, **kw: box2d_iou_sparse(a, b, method=method, threshold=t, precise=precise, **kw)
    return lambda a, b, t, **kw: iou3d_sparse(a, b, method=method, threshold=t, **kw)


def matrix_model(dense, threshold):
    """the issue's definition on the library's own matrix"""
    keep = dense > torch.tensor(threshold, dtype=dense.dtype)
    pairs = keep.nonzero()
    offsets = torch.zeros(dense.shape[0] + 1, dtype=torch.int64, device=dense.device)
    offsets[1:] = keep.sum(1).cumsum(0)
    return pairs, dense[pairs[:, 0], pairs[:, 1]], offsets


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def assert_is_model(got, dense, threshold, what):
    pairs, values, offsets = got
    mp, mv, mo = matrix_model(dense, threshold)
    assert pairs.dtype == torch.int64 and pairs.shape == mp.shape and torch.equal(pairs, mp), what
    assert values.dtype == dense.dtype and torch.equal(bits(values), bits(mv)), what
    assert offsets.dtype == torch.int64 and torch.equal(offsets, mo), what


@pytest.mark.parametrize("scene", sc.SCENES, ids=lambda s: s["name"])
def test_scene_is_the_matrix_through_nonzero_and_the_oracle_pair_set(scene):
    dims = scene["dims"]
    n, m = len(scene["b1"]), len(scene["b2"])
    for method in sc.METHODS:
        for route, dtype, precise in (ROUTES_2D if dims == 2 else ROUTES_3D):
            b1, b2 = scene["b1"].astype(dtype), scene["b2"].astype(dtype)
            dense = dense_op(dims, method, precise)(T(b1), T(b2))
            # the oracle on the boxes the kernels see, in fp64 (7 columns: its own fp32), rounded to the stored type
            o = oracle.box2d_iou(b1.astype(np.float64), b2.astype(np.float64), method, precise=True) if dims == 2 else oracle.iou3d(b1, b2, method)
            band = sc.TIE if precise else TIE_F32
            thresholds = list(sc.THRESHOLDS)
            if scene["stored"]:
                hits = dense[dense > 0].sort().values
                thresholds.append(hits[len(hits) // 2].item())       # one stored value: strictness must drop that pair
            for t in thresholds:
                what = (scene["name"], method, route, t)
                got = sparse_op(dims, method, precise)(T(b1), T(b2), t, return_offsets=True)
                assert all(x.is_cuda for x in got), what
                assert_is_model(got, dense, t, what)
                if scene["stored"] and t == thresholds[-1]:
                    assert (dense == t).any() and not (got[1] == t).any(), what
                # independently: the oracle's pair set outside the ties
                t_stored = float(np.asarray(t, dense.cpu().numpy().dtype))
                with np.errstate(invalid="ignore"):
                    tie = (np.abs(o.astype(np.float64) - t_stored) <= band) & ~((o == 0) & (t_stored == 0))
                    want = o.astype(dense.cpu().numpy().dtype) > t_stored
                assert tie.sum() <= sc.TIE_CAP * n * m, what + (int(tie.sum()),)
                mine = np.zeros((n, m), bool)
                p = got[0].cpu().numpy()
                mine[p[:, 0], p[:, 1]] = True
                assert np.array_equal(mine[~tie], want[~tie]), what + (np.argwhere((mine != want) & ~tie)[:5].tolist(),)


@pytest.mark.parametrize("name", ["odd_130x75", "degenerate", "odd3_130x75", "zcases3"])
def test_values_are_the_paired_operators_on_the_listed_pairs(name):
    from d3d_amd.box import box2d_iou_paired, box3d_iou_paired
    scene = next(s for s in sc.SCENES if s["name"] == name)
    dims = scene["dims"]
    for method in sc.METHODS:
        for route, dtype, precise in (ROUTES_2D if dims == 2 else ROUTES_3D):
            b1, b2 = T(scene["b1"].astype(dtype)), T(scene["b2"].astype(dtype))
            pairs, values = sparse_op(dims, method, precise)(b1, b2, 0.0)
            assert len(pairs) > 0 and not values.requires_grad
            if dims == 2:
                again = box2d_iou_paired(b1[pairs[:, 0]], b2[pairs[:, 1]], method=method, precise=precise)
            else:
                again = box3d_iou_paired(b1[pairs[:, 0]], b2[pairs[:, 1]], method=method, precise=False)
            assert torch.equal(bits(values), bits(again)), (name, method, route)


def test_plumbing_numpy_cpu_strides_and_stream():
    from d3d_amd.box import box2d_iou, box2d_iou_sparse, iou3d, iou3d_sparse
    s2 = next(s for s in sc.SCENES if s["name"] == "odd_130x75")
    s3 = next(s for s in sc.SCENES if s["name"] == "odd3_130x75")
    a, b = s2["b1"].astype(np.float32), s2["b2"].astype(np.float32)
    dense = box2d_iou(T(a), T(b), method="rbox", precise=True)
    want = [x.cpu() for x in matrix_model(dense, 0.25)]
    # numpy in, numpy out
    got = box2d_iou_sparse(a, b, method="rbox", threshold=0.25, return_offsets=True)
    assert all(isinstance(x, np.ndarray) for x in got) and got[1].dtype == np.float32
    assert all(np.array_equal(x, y.numpy()) for x, y in zip(got, want))
    assert len(box2d_iou_sparse(a, b, method="rbox", threshold=0.25)) == 2
    # CPU tensors in, CPU tensors out
    got = box2d_iou_sparse(torch.from_numpy(a), torch.from_numpy(b), method="rbox", threshold=0.25, return_offsets=True)
    assert all(x.device.type == "cpu" for x in got) and all(torch.equal(x, y) for x, y in zip(got, want))
    # any strides: a column slice of a wider tensor, every second row of a taller one
    wide1, wide2 = torch.zeros(len(a), 9), torch.zeros(2 * len(b), 5)
    wide1[:, 2:7] = torch.from_numpy(a)
    wide2[::2] = torch.from_numpy(b)
    v1, v2 = wide1.cuda()[:, 2:7], wide2.cuda()[::2]
    assert not v1.is_contiguous() and not v2.is_contiguous()
    got = box2d_iou_sparse(v1, v2, method="rbox", threshold=0.25, return_offsets=True)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(got, want))
    # a non-default current stream, 7 columns; fp64 rows are taken as fp32 like iou3d's
    a3, b3 = T(s3["b1"]), T(s3["b2"])
    dense3 = iou3d(a3, b3, "rbox")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = iou3d_sparse(a3, b3, method="rbox", threshold=0.0, return_offsets=True)
    stream.synchronize()
    assert_is_model(got, dense3, 0.0, "stream")


def test_raw_entries_capacity_and_repeat():
    lib = _lib.load()
    scene = next(s for s in sc.SCENES if s["name"] == "odd_130x75")
    b1, b2 = T(scene["b1"]), T(scene["b2"])
    n, m = len(b1), len(b2)
    ws = torch.empty(lib.d3d_iou_sparse_workspace_bytes(n, m), dtype=torch.uint8, device="cuda")
    inputs = (_lib.ptr(b1), n, _lib.ptr(b2), m, 5, 2, _lib.F64, 0.0)
    tail = (_lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    offsets = [torch.full((n + 1,), -7, dtype=torch.int64, device="cuda") for _ in range(2)]
    for off in offsets:                                            # count twice: identical offsets
        assert lib.d3d_iou_sparse_count(*inputs, _lib.ptr(off), *tail) == _lib.OK
    assert torch.equal(offsets[0], offsets[1])
    k = int(offsets[0][n])
    assert k > 1 and int(offsets[0][0]) == 0 and bool((offsets[0][1:] >= offsets[0][:-1]).all())
    extra = 5
    pairs = torch.full((k + extra, 2), -1, dtype=torch.int64, device="cuda")
    values = torch.full((k + extra,), -3.0, dtype=torch.float64, device="cuda")
    # one short: BAD_ARG, the poisoned buffers untouched
    assert lib.d3d_iou_sparse_emit(*inputs, _lib.ptr(offsets[0]), k - 1, _lib.ptr(pairs), _lib.ptr(values), *tail) == _lib.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((pairs == -1).all()) and bool((values == -3.0).all())
    # larger than K: the tail untouched
    assert lib.d3d_iou_sparse_emit(*inputs, _lib.ptr(offsets[0]), k + extra, _lib.ptr(pairs), _lib.ptr(values), *tail) == _lib.OK
    torch.cuda.synchronize()
    assert bool((pairs[k:] == -1).all()) and bool((values[k:] == -3.0).all())
    from d3d_amd.box import box2d_iou
    assert_is_model((pairs[:k], values[:k], offsets[0]), box2d_iou(b1, b2, method="rbox", precise=True), 0.0, "raw")
    # a workspace too small, a null one
    assert lib.d3d_iou_sparse_count(*inputs, _lib.ptr(offsets[1]), _lib.ptr(ws), 16, _lib.stream_ptr()) == _lib.ERR_WORKSPACE
    assert lib.d3d_iou_sparse_count(*inputs, _lib.ptr(offsets[1]), None, 0, _lib.stream_ptr()) == _lib.ERR_WORKSPACE
    # no pair at all: _count clears offsets without a launch
    assert lib.d3d_iou_sparse_count(_lib.ptr(b1), n, None, 0, 5, 2, _lib.F64, 0.0, _lib.ptr(offsets[1]), None, 0, _lib.stream_ptr()) == _lib.OK
    torch.cuda.synchronize()
    assert not bool(offsets[1].any())


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1023, 1024, 1025))
def test_rows_around_the_scan_tile(n):
    """n rows around a wavefront's 256 and a workgroup's 1024 of the offsets scan against three columns, hits in the first and in
    the last row: the raw entries on poisoned buffers, offsets, offsets[n] and the pairs against the matrix's"""
    from d3d_amd.box import box2d_iou
    lib = _lib.load()
    m = 3
    b2 = np.array([[10.0 * j, 0.0, 2.0, 2.0, 0.3] for j in range(m)])
    i = np.arange(n)
    b1 = np.stack([1000.0 + 3.0 * i, np.full(n, 500.0), np.full(n, 2.0), np.full(n, 1.5), 0.1 * (i % 7)], 1)      # far from every column
    one = (i % 5 == 0) | (i == n - 1)                               # these rows lie on column i % 3 ...
    b1[one, 0], b1[one, 1] = 10.0 * (i[one] % m) + 0.3, 0.2
    wide = i % 11 == 0                                              # ... and these across up to all three
    b1[wide, 0], b1[wide, 2] = 10.0, 30.0
    b1, b2 = T(b1), T(b2)
    dense = box2d_iou(b1, b2, method="rbox", precise=True)
    assert bool((dense[0] > 0).any()) and bool((dense[n - 1] > 0).any())
    ws = torch.empty(lib.d3d_iou_sparse_workspace_bytes(n, m), dtype=torch.uint8, device="cuda")
    inputs = (_lib.ptr(b1), n, _lib.ptr(b2), m, 5, 2, _lib.F64, 0.0)
    tail = (_lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    assert lib.d3d_iou_sparse_count(*inputs, _lib.ptr(offsets), *tail) == _lib.OK
    mp, mv, mo = matrix_model(dense, 0.0)
    assert torch.equal(offsets, mo)
    k, extra = int(offsets[n]), 5
    assert k == len(mp) and k > n // 5
    pairs = torch.full((k + extra, 2), -1, dtype=torch.int64, device="cuda")
    values = torch.full((k + extra,), -3.0, dtype=torch.float64, device="cuda")
    assert lib.d3d_iou_sparse_emit(*inputs, _lib.ptr(offsets), k + extra, _lib.ptr(pairs), _lib.ptr(values), *tail) == _lib.OK
    torch.cuda.synchronize()
    assert bool((pairs[k:] == -1).all()) and bool((values[k:] == -3.0).all())
    assert_is_model((pairs[:k], values[:k], offsets), dense, 0.0, n)


def test_4000_by_3000_at_config_3_density():
    """the only non-tiny shape: 250 workgroups of 16 rows, three LDS chunks of 1024 columns (the last one partial)"""
    from d3d_amd.box import box2d_iou, box2d_iou_sparse
    b1, _ = synth.boxes2d_sparse(4000, 5)
    b2, _ = synth.boxes2d_sparse(3000, 6)
    b2[:, :2] *= np.sqrt(4000 / 3000.0)                             # the same ground as b1
    for dtype, precise in ((np.float32, True), (np.float64, True)):
        a, b = T(b1.astype(dtype)), T(b2.astype(dtype))
        dense = box2d_iou(a, b, method="rbox", precise=precise)
        for t in (0.0, 0.3):
            got = box2d_iou_sparse(a, b, method="rbox", threshold=t, precise=precise, return_offsets=True)
            assert len(got[0]) > (1000 if t == 0 else 50)
            assert_is_model(got, dense, t, (dtype.__name__, t))
