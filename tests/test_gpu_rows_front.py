"""GPU: the one ingress and egress of the row operators (d3d_amd._rows).  Every operator takes the same rows as a numpy array, as a
host tensor and as a CUDA tensor; each result comes back as the same kind on the same side, all three hold the same bits, and so do
the gradients, which land where the input lives.  Then the refusals that need a built owner, word for word.

The shapes are the smallest that take both paths of the row kernels: C = 3 (an odd width: the scalar path) and C = 4 (16 bytes of
fp32: the vector path), over 7 points in 3 voxels for the pooling pair and over 5 voxels that are neighbours in a 3 x 3 x 3 window
for everything else."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COORDS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1], [2, 1, 1]], np.int64)              # 5 voxels
MAPPING = np.array([0, 2, 1, -1, 0, 2, 2], np.int64)                                               # 7 points in 3 voxels
POSITIONS = np.array([[0.25, 0.5, 0.0], [1.0, 0.75, 0.5], [0.5, 0.5, 0.5], [1.75, 1.0, 1.0], [-0.5, 0.0, 0.25], [9.0, 9.0, 9.0],
                      [1.5, 0.5, 0.5]], np.float32)                                                # 7 points around them, one far off
KNOWN = COORDS.astype(np.float32) * 0.5
DENSE_SHAPE = (3, 2, 2)
COUT = 5
TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
HALF = ("sparse_pool3d", "voxel_interpolate", "voxel_splat", "voxel_to_dense", "voxel_from_dense", "point_interpolate")
OPERATORS = ("voxel_pool", "voxel_unpool", "neighbor_gather", "subm_conv3d", "sparse_conv3d", "sparse_pool3d", "voxel_interpolate", "voxel_splat",
             "voxel_to_dense", "voxel_from_dense", "point_interpolate")


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def owners():
    from d3d_amd.point import PointInterp
    from d3d_amd.voxel import SparseConvMap, VoxelDenseMap, VoxelIndex, VoxelInterp, VoxelNeighbors
    return dict(index=VoxelIndex(cuda(MAPPING), 3), nbrs=VoxelNeighbors(cuda(COORDS), 3), cmap=SparseConvMap(cuda(COORDS), 2, 2),
                interp=VoxelInterp(cuda(COORDS), cuda(POSITIONS)), dmap=VoxelDenseMap(cuda(COORDS), DENSE_SHAPE),
                pinterp=PointInterp(cuda(KNOWN), cuda(POSITIONS), k=3))


def operator(name, c, dtype):
    """-> (fn(rows), the shape of its rows)"""
    from d3d_amd import point, voxel
    o = owners()
    weight = lambda k: (torch.arange(k * c * COUT, dtype=torch.float64).reshape(k, c, COUT) % 7 - 3).to(dtype).cuda()
    return {
        "voxel_pool": (lambda x: voxel.voxel_pool(x, o["index"], reduction="max"), (7, c)),
        "voxel_unpool": (lambda x: voxel.voxel_unpool(x, o["index"]), (3, c)),
        "neighbor_gather": (lambda x: voxel.neighbor_gather(x, o["nbrs"]), (5, c)),
        "subm_conv3d": (lambda x: voxel.subm_conv3d(x, o["nbrs"], weight(27), method="gather"), (5, c)),
        "sparse_conv3d": (lambda x: voxel.sparse_conv3d(x, o["cmap"], weight(8)), (5, c)),
        "sparse_pool3d": (lambda x: voxel.sparse_pool3d(x, o["cmap"], "mean"), (5, c)),
        "voxel_interpolate": (lambda x: voxel.voxel_interpolate(x, o["interp"]), (5, c)),
        "voxel_splat": (lambda x: voxel.voxel_splat(x, o["interp"]), (7, c)),
        "voxel_to_dense": (lambda x: voxel.voxel_to_dense(x, o["dmap"], -1.5), (5, c)),
        "voxel_from_dense": (lambda x: voxel.voxel_from_dense(x, o["dmap"]), (1, c) + DENSE_SHAPE),
        "point_interpolate": (lambda x: point.point_interpolate(x, o["pinterp"]), (5, c)),
    }[name]


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# bfloat16 where the operator takes it at these widths (the pooling pair and the gathers are float32 / float64, and half precision
# reaches the convolutions through the fused kernels only, which need C % 16 == 0)
CASES = [(name, c, dtype) for name in OPERATORS for c in (3, 4) for dtype in ("f32", "f64", "bf16") if dtype != "bf16" or name in HALF]


@pytest.mark.parametrize("name,c,dtype", CASES)
def test_three_ways_in_give_the_same_bits_on_the_callers_side(name, c, dtype):
    fn, shape = operator(name, c, TORCH[dtype])
    rng = np.random.default_rng(len(name) * 8 + c)
    rows = torch.from_numpy(rng.normal(size=shape)).to(TORCH[dtype])
    outs, grads = [], []
    if dtype != "bf16":                                     # numpy has no bfloat16
        out = fn(rows.numpy().copy())
        assert isinstance(out, np.ndarray)
        outs.append(torch.from_numpy(out))
    upstream = torch.from_numpy(rng.normal(size=tuple(fn(rows).shape))).to(TORCH[dtype])
    for x in (rows.clone(), rows.cuda()):
        x.requires_grad_()
        out = fn(x)
        assert isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == x.dtype
        out.backward(upstream.to(x.device))
        assert x.grad.device == x.device and x.grad.dtype == x.dtype and x.grad.shape == x.shape
        outs.append(out), grads.append(x.grad)
    assert all(same_bits(outs[0], o) for o in outs[1:])
    assert same_bits(grads[0], grads[1])
    assert bool(outs[0].float().abs().sum() > 0) and bool(grads[0].float().abs().sum() > 0)          # (something was computed)


def refused(call, message):
    with pytest.raises(ValueError) as e:
        call()
    assert type(e.value) is ValueError and str(e.value) == message


def test_owner_dependent_refusals_word_for_word():
    from d3d_amd import point, voxel
    o = owners()
    x = lambda rows: torch.zeros((rows, 4), device="cuda")
    refused(lambda: voxel.voxel_pool(x(8), o["index"]), "features has 8 rows, the mapping 7 points")
    refused(lambda: voxel.voxel_pool(x(6).cpu().numpy(), o["index"]), "features has 6 rows, the mapping 7 points")
    refused(lambda: voxel.voxel_pool(x(7), o["index"], num_voxels=4), "num_voxels = 4, the VoxelIndex was built for 3")
    refused(lambda: voxel.voxel_unpool(x(4), o["index"]), "num_voxels = 4, the VoxelIndex was built for 3")
    refused(lambda: voxel.voxel_unpool(x(4), o["index"], num_voxels=3), "voxel_features has 4 rows, the index 3 voxels")
    refused(lambda: voxel.neighbor_gather(x(6), o["nbrs"]), "features has 6 rows where the VoxelNeighbors expects 5")
    refused(lambda: voxel.subm_conv3d(x(4), o["nbrs"], torch.zeros((27, 4, COUT))), "features has 4 rows where the VoxelNeighbors expects 5")
    refused(lambda: voxel.sparse_conv3d(x(6).cpu(), o["cmap"], torch.zeros((8, 4, COUT))), "features has 6 rows where the SparseConvMap expects 5")
    vout = o["cmap"].num_out
    refused(lambda: voxel.sparse_inverse_conv3d(x(vout + 1), o["cmap"], torch.zeros((8, 4, COUT))),
            "features has %d rows where the SparseConvMap expects %d" % (vout + 1, vout))
    refused(lambda: voxel.sparse_pool3d(x(4), o["cmap"]), "features has 4 rows where the SparseConvMap expects 5")
    refused(lambda: voxel.sparse_pool3d(x(6), o["nbrs"], "sum"), "features has 6 rows where the VoxelNeighbors expects 5")
    refused(lambda: voxel.voxel_interpolate(x(6), o["interp"]), "voxel_features has 6 rows where the VoxelInterp expects 5")
    refused(lambda: voxel.voxel_splat(x(6), o["interp"]), "point_features has 6 rows where the VoxelInterp expects 7")
    refused(lambda: voxel.voxel_to_dense(x(4), o["dmap"]), "features has 4 rows where the VoxelDenseMap expects 5")
    refused(lambda: voxel.voxel_from_dense(torch.zeros((1, 4, 3, 2, 3), device="cuda"), o["dmap"]),
            "dense has the shape (1, 4, 3, 2, 3) where the VoxelDenseMap expects (1, C, 3, 2, 2)")
    refused(lambda: point.point_interpolate(x(6), o["pinterp"]), "known_features has 6 rows where the PointInterp expects 5")
    if torch.cuda.device_count() > 1:                       # rows on another GPU than the owner's
        far = torch.zeros((5, 4), device="cuda:1")
        for call, owner in ((lambda: voxel.neighbor_gather(far, o["nbrs"]), "VoxelNeighbors"), (lambda: voxel.sparse_pool3d(far, o["cmap"]), "SparseConvMap"),
                            (lambda: voxel.voxel_interpolate(far, o["interp"]), "VoxelInterp"), (lambda: voxel.voxel_to_dense(far, o["dmap"]), "VoxelDenseMap"),
                            (lambda: point.point_interpolate(far, o["pinterp"]), "PointInterp"),
                            (lambda: voxel.voxel_unpool(far[:3], o["index"]), "VoxelIndex")):
            refused(call, "features live on cuda:1, the %s on cuda:0" % owner)
