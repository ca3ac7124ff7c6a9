"""The refusals of the row operators' fronts, word for word: every front of d3d_amd.voxel and d3d_amd.point that takes feature rows
checks them through d3d_amd._rows, and what a caller reads when a check fails is part of the interface.  For each front: something
that is no tensor, a 1-D tensor, an integer dtype, a dtype the operator (or the chosen route) does not take, and a row count off by
one -- against owners that were never built (building one needs a GPU), so everything here answers before any GPU work.  Then the
rule the Python layer keeps: operator modules share through _lib, _rows and voxel/_coords, never through each other's private names.
"""
import ast
import os

import numpy as np
import pytest
import torch

DEV = torch.device("cuda", 0)
V, K, C = 6, 9, 4                   # voxels (or known rows), points, channels


def _neighbors():
    from d3d_amd.voxel.conv import TableView, VoxelNeighbors
    nb = VoxelNeighbors.__new__(VoxelNeighbors)
    nb.device, nb.num_voxels, nb.kernel_volume = DEV, V, 27
    nb._view = TableView(torch.zeros((V, 27), dtype=torch.int32), V, 27, DEV)
    return nb


def _conv_map():
    from d3d_amd.voxel.conv import TableView
    from d3d_amd.voxel.sparse_conv import SparseConvMap
    m = SparseConvMap.__new__(SparseConvMap)
    m.device, m.num_voxels, m.num_out, m.kernel_volume = DEV, V, 3, 8
    m._down = TableView(torch.zeros((3, 8), dtype=torch.int32), V, 8, DEV)
    m._up = TableView(torch.zeros((V, 8), dtype=torch.int32), 3, 8, DEV)
    return m


def _voxel_interp():
    from d3d_amd.voxel import VoxelInterp
    itp = VoxelInterp.__new__(VoxelInterp)
    itp.device, itp.num_voxels, itp.num_points, itp.num_corners, itp.num_entries = DEV, V, K, 8, 0
    return itp


def _dense_map():
    from d3d_amd.voxel import VoxelDenseMap
    m = object.__new__(VoxelDenseMap)
    m.num_voxels, m.batch_size, m.dense_shape, m.device = V, 1, (2, 3, 4), DEV
    return m


def _point_interp():
    from d3d_amd.point import PointInterp
    itp = PointInterp.__new__(PointInterp)
    itp._set(DEV, torch.zeros((K, 3), dtype=torch.int32), None, torch.zeros((K, 3)), V)
    return itp


def _fronts():
    """name -> (call(rows), the rows it expects, the argument's name, what a row is, the dtypes it takes)"""
    from d3d_amd import point, voxel
    mapping = torch.zeros(K, dtype=torch.int64)
    nb, cmap, vi, dm, pi = _neighbors(), _conv_map(), _voxel_interp(), _dense_map(), _point_interp()
    w27, w8 = torch.zeros((27, C, 16)), torch.zeros((8, C, 16))
    return {
        "voxel_pool": (lambda x: voxel.voxel_pool(x, mapping, V), K, "features", "point", 2),
        "voxel_unpool": (lambda x: voxel.voxel_unpool(x, mapping), V, "voxel_features", "voxel", 2),
        "neighbor_gather": (lambda x: voxel.neighbor_gather(x, nb), V, "features", "voxel", 2),
        "subm_conv3d": (lambda x: voxel.subm_conv3d(x, nb, w27.to(_dtype_of(x))), V, "features", "voxel", 4),
        "sparse_conv3d": (lambda x: voxel.sparse_conv3d(x, cmap, w8.to(_dtype_of(x))), V, "features", "voxel", 4),
        "sparse_inverse_conv3d": (lambda x: voxel.sparse_inverse_conv3d(x, cmap, w8.to(_dtype_of(x))), 3, "features", "voxel", 4),
        "sparse_pool3d": (lambda x: voxel.sparse_pool3d(x, cmap), V, "features", "voxel", 4),
        "voxel_interpolate": (lambda x: voxel.voxel_interpolate(x, vi), V, "voxel_features", "voxel", 4),
        "voxel_splat": (lambda x: voxel.voxel_splat(x, vi), K, "point_features", "point", 4),
        "voxel_to_dense": (lambda x: voxel.voxel_to_dense(x, dm), V, "features", "voxel", 4),
        "point_interpolate": (lambda x: point.point_interpolate(x, pi), V, "known_features", "known point", 4),
    }


def _dtype_of(x):
    return x.dtype if isinstance(x, torch.Tensor) and x.is_floating_point() else torch.float32


OWNERS = {"neighbor_gather": "VoxelNeighbors", "subm_conv3d": "VoxelNeighbors", "sparse_conv3d": "SparseConvMap",
          "sparse_inverse_conv3d": "SparseConvMap", "sparse_pool3d": "SparseConvMap", "voxel_interpolate": "VoxelInterp",
          "voxel_splat": "VoxelInterp", "voxel_to_dense": "VoxelDenseMap", "point_interpolate": "PointInterp"}
VOXEL_FEATURES = ("voxel_pool", "voxel_unpool", "neighbor_gather", "subm_conv3d", "sparse_conv3d", "sparse_inverse_conv3d", "sparse_pool3d")
FRONTS = ("voxel_pool", "voxel_unpool", "neighbor_gather", "subm_conv3d", "sparse_conv3d", "sparse_inverse_conv3d", "sparse_pool3d",
          "voxel_interpolate", "voxel_splat", "voxel_to_dense", "point_interpolate")


def _refused(call, x, exc, message):
    with pytest.raises(exc) as e:
        call(x)
    assert type(e.value) is exc and str(e.value) == message


@pytest.mark.parametrize("front", FRONTS)
def test_front_refusals_word_for_word(front):
    call, rows, name, row, ndtypes = _fronts()[front]
    subject = "voxel features" if front in VOXEL_FEATURES else name
    takes = "float32 or float64" if ndtypes == 2 else "float32, float64, float16 or bfloat16"
    _refused(call, [[0.0] * C] * rows, TypeError, "%s must be a torch.Tensor or numpy array" % name)
    _refused(call, None, TypeError, "%s must be a torch.Tensor or numpy array" % name)
    for bad in (torch.zeros(rows), torch.zeros((rows, C, 1)), np.zeros(rows, np.float32)):
        _refused(call, bad, ValueError, "%s must be a 2-D tensor of one row per %s" % (name, row))
    for bad, dtype in ((torch.zeros((rows, C), dtype=torch.int32), "torch.int32"), (np.zeros((rows, C), np.int64), "torch.int64"),
                       (torch.zeros((rows, C), dtype=torch.complex64), "torch.complex64")):
        _refused(call, bad, ValueError, "%s must be %s, not %s" % (subject, takes, dtype))
    if ndtypes == 2:                    # float32 and float64 only: the half types are refused by name
        _refused(call, torch.zeros((rows, C), dtype=torch.float16), ValueError, "%s must be %s, not torch.float16" % (subject, takes))
        _refused(call, torch.zeros((rows, C), dtype=torch.bfloat16), ValueError, "%s must be %s, not torch.bfloat16" % (subject, takes))
    for off in (rows - 1, rows + 1):
        x = torch.zeros((off, C))
        if front == "voxel_pool":
            _refused(call, x, ValueError, "features has %d rows, the mapping %d points" % (off, rows))
        elif front == "voxel_unpool":       # (the row count of voxel_features IS num_voxels with a bare mapping: a built index is the GPU file's)
            continue
        else:
            _refused(call, x, ValueError, "%s has %d rows where the %s expects %d" % (name, off, OWNERS[front], rows))


def test_the_dtypes_a_route_refuses():
    """float64 on the fp32-only fused route of the convolutions, and half precision on their gather route"""
    from d3d_amd import voxel
    nb, cmap = _neighbors(), _conv_map()
    x, w27, w8 = torch.zeros((V, 16), dtype=torch.float64), torch.zeros((27, 16, 16), dtype=torch.float64), torch.zeros((8, 16, 16), dtype=torch.float64)
    fused = "method=\"fused\" takes float32, float16 and bfloat16, not float64"
    _refused(lambda t: voxel.subm_conv3d(t, nb, w27, method="fused"), x, ValueError, fused)
    _refused(lambda t: voxel.sparse_conv3d(t, cmap, w8, method="fused"), x, ValueError, fused)
    _refused(lambda t: voxel.sparse_inverse_conv3d(t, cmap, w8, method="fused"), x[:3], ValueError, fused)
    for dtype in (torch.float16, torch.bfloat16):
        gather = "%s runs on the fused kernels only: method=\"gather\" takes float32 and float64" % dtype
        _refused(lambda t: voxel.subm_conv3d(t, nb, w27.to(dtype), method="gather"), x.to(dtype), ValueError, gather)
        _refused(lambda t: voxel.sparse_conv3d(t, cmap, w8.to(dtype), method="gather"), x.to(dtype), ValueError, gather)


def test_dense_front_refusals_word_for_word():
    """voxel_to_dense checks the dtype first, then the fill value, then the shape; voxel_from_dense takes a 5-D tensor"""
    from d3d_amd.voxel import voxel_from_dense, voxel_to_dense
    dm = _dense_map()
    dtypes = "float32, float64, float16 or bfloat16"
    _refused(lambda x: voxel_to_dense(x, dm), torch.zeros(V, dtype=torch.int32), ValueError, "features must be %s, not torch.int32" % dtypes)
    _refused(lambda x: voxel_to_dense(x, dm, "0"), torch.zeros(V), TypeError, "fill_value must be a number, not '0'")
    _refused(lambda x: voxel_to_dense(x, dm, True), torch.zeros((V, C)), TypeError, "fill_value must be a number, not True")
    _refused(lambda x: voxel_to_dense(x, object()), torch.zeros((V, C)), TypeError, "dmap must be a VoxelDenseMap")
    call = lambda x: voxel_from_dense(x, dm)
    _refused(call, [[0.0]], TypeError, "dense must be a torch.Tensor or numpy array")
    _refused(call, torch.zeros((1, C, 2, 3, 4), dtype=torch.int32), ValueError, "dense must be %s, not torch.int32" % dtypes)
    _refused(call, np.zeros((1, C, 2, 3, 4), np.int64), ValueError, "dense must be %s, not torch.int64" % dtypes)
    for bad in (torch.zeros(V), torch.zeros((V, C)), torch.zeros((1, C, 2, 3, 5)), torch.zeros((2, C, 2, 3, 4)), torch.zeros((1, C, 4, 3, 2))):
        _refused(call, bad, ValueError, "dense has the shape %r where the VoxelDenseMap expects (1, C, 2, 3, 4)" % (tuple(bad.shape),))


def test_owner_type_refusals_word_for_word():
    from d3d_amd import point, voxel
    x = torch.zeros((V, C))
    for owner in (None, "owner", torch.zeros((V, 27), dtype=torch.int32)):
        _refused(lambda t: voxel.neighbor_gather(t, owner), x, TypeError, "nbrs must be a VoxelNeighbors")
        _refused(lambda t: voxel.subm_conv3d(t, owner, torch.zeros((27, C, 16))), x, TypeError, "nbrs must be a VoxelNeighbors")
        _refused(lambda t: voxel.sparse_conv3d(t, owner, torch.zeros((8, C, 16))), x, TypeError, "cmap must be a SparseConvMap")
        _refused(lambda t: voxel.sparse_pool3d(t, owner), x, TypeError, "where must be a SparseConvMap or a VoxelNeighbors")
        _refused(lambda t: voxel.voxel_interpolate(t, owner), x, TypeError, "interp must be a VoxelInterp")
        _refused(lambda t: voxel.voxel_splat(t, owner), x, TypeError, "interp must be a VoxelInterp")
        _refused(lambda t: point.point_interpolate(t, owner), x, TypeError, "interp must be a PointInterp")
    _refused(lambda t: point.point_interpolate(t, _voxel_interp()), x, TypeError, "interp must be a PointInterp")
    _refused(lambda t: voxel.voxel_interpolate(t, _point_interp()), x, TypeError, "interp must be a VoxelInterp")


def test_operator_modules_share_through_the_three_private_modules_only():
    """no module under d3d_amd imports an underscore name from an operator module: such names come from _lib, _rows and
    voxel/_coords (box_impl's `as _name` aliases of public functions are no such import)"""
    import d3d_amd
    root = os.path.dirname(d3d_amd.__file__)
    shared = ("_lib", "_rows", "_coords")
    found = []
    for folder, _, files in os.walk(root):
        for f in (f for f in files if f.endswith(".py")):
            path = os.path.join(folder, f)
            with open(path) as fh:
                tree = ast.parse(fh.read())
            for node in (n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)):
                source = (node.module or "").split(".")[-1]
                found += ["%s: from %s import %s" % (os.path.relpath(path, root), node.module, a.name) for a in node.names
                          if a.name.startswith("_") and a.name not in shared and source not in shared]
    assert found == []


def test_what_every_row_operator_needs_is_defined_once():
    import d3d_amd
    root = os.path.dirname(d3d_amd.__file__)
    paths = [os.path.join(root, "_rows.py")]
    for sub in ("voxel", "point"):
        paths += [os.path.join(root, sub, f) for f in sorted(os.listdir(os.path.join(root, sub))) if f.endswith(".py")]
    text = "".join(open(p).read() for p in paths)
    for once in ("def as_tensor(", "2 ** 31 - 1", "def transpose(", "def weights_as(", "torch.float32: _lib.F32", "torch.float16: _lib.F16"):
        assert text.count(once) == 1, once
