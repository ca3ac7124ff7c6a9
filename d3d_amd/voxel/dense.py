"""d3d_amd.voxel.dense -- the exit of a sparse backbone: sparse voxel rows [V, C] into a dense channels-first grid [N, C, A, B, D]
(spconv's `.dense()`), the same tensor viewed as the BEV map [N, C * A, B, D] that the 2D heads of SECOND / CenterPoint / PV-RCNN's
RPN take, and the reverse: the values of a dense tensor at the active sites as [V, C], which brings a dense branch back into the
sparse one.  Each is the other's gradient.  An extension (the reference stops at the voxelizer).

    sp   = VoxelGenerator(bounds, shape, max_points=32, max_points_filter="trim")(pts)    # sparse contract, coords are (x, y, z)
    dmap = VoxelDenseMap(stage.out_coords, stage_shape, axes=(2, 1, 0))   # once per frame and stage; every forward and backward reuses it
    bev  = voxel_to_bev(backbone_features, dmap)                 # [1, C * Z, Y, X]: one launch, every element written once
    vf   = voxel_from_dense(head(bev).unflatten(1, (-1, Z)), dmap)    # [V, C']: the values at the active sites

One launch each: a workgroup owns a stretch of cells of one sample and transposes the rows of its present cells through LDS (rows are
channel-minor, the grid is channel-major); a stretch without a present cell is only filled.  No memset, no [.., C]-minor
intermediate, no float atomics: every run gives the same bits (kernels and the exact rules: csrc/vdense.hip, include/d3d_hip.h).

Out of scope: layouts other than channels-first (there is no channels-last output), and discovering the active sites of an
arbitrary dense tensor (there is no `from_dense` that finds nonzeros: voxel_from_dense reads at the sites of a map).
"""
import ctypes
from functools import partial

import numpy as np
import torch

from .. import _lib
from .._rows import FEATURE_CODES, ROW_MAX, TransposePair, as_tensor, back_to_caller, check_owner_device, device_of, dtype_code
from ._coords import _check_coords, _triple

_MAX_CELLS = 2 ** 39 - 1             # N * A * B * D: the launch numbers stretches of cells in 31 bits


def _axes(axes):
    t = tuple(axes) if isinstance(axes, (tuple, list)) else None
    if t is None or len(t) != 3 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in t) or sorted(t) != [0, 1, 2]:
        raise ValueError("axes must be a permutation of (0, 1, 2), not %r" % (axes,))
    return tuple(int(a) for a in t)


class VoxelDenseMap:
    """Where every voxel row of one frame sits in a dense grid, and which row sits at every cell.

    :param coords: [V, 3] int64 (int32 is widened) voxel coordinates; torch tensor (GPU or host) or numpy array.  (batch, coordinate)
        must be unique
    :param spatial_shape: three ints >= 1, the size of the grid per coordinate COLUMN (column 0 first: SparseConvMap's convention)
    :param batch_index: [V] int64 / int32 sample numbers in [0, batch_size), or None: one sample
    :param batch_size: N; required exactly when batch_index is given (nothing is read back to guess it)
    :param origin: an int or three ints, the coordinate that lands in dense cell 0 per column; negative coordinates are legal
    :param axes: a permutation of (0, 1, 2): the coordinate column each dense spatial axis walks.  The voxelizer's coordinates are
        (x, y, z), so axes=(2, 1, 0) gives [N, C, Z, Y, X] and voxel_to_bev of that the usual [N, C * Z, Y, X]

    Holds, on the GPU: `cell` [V] int64, the flat cell ((n * A + a) * B + b) * D + d of every row, and `index` [N * A * B * D] int32,
    the row at every cell, -1 for none; and `num_voxels`, `batch_size`, `spatial_shape`, `dense_shape` = (A, B, D) (the three permuted
    sizes), `cells_per_sample` = A * B * D, `origin`, `axes`, `device`.  Building it reads two counters back, once.  ValueError (with the count) when rows lie outside
    [origin, origin + spatial_shape) on some axis or their batch value outside [0, N), and when a (batch, coordinate) repeats;
    ValueError for V above 2^31 - 1.  Nothing here is differentiable."""

    def __init__(self, coords, spatial_shape, batch_index=None, batch_size=None, origin=0, axes=(0, 1, 2)):
        coords, batch_index, v = _check_coords(coords, batch_index)
        if isinstance(spatial_shape, (int, float)):
            raise ValueError("spatial_shape must be three ints, not %r" % (spatial_shape,))
        shape, origin, axes = _triple(spatial_shape, "spatial_shape"), _triple(origin, "origin"), _axes(axes)
        if any(s < 1 for s in shape):
            raise ValueError("spatial_shape must be >= 1 per axis, not %r" % (spatial_shape,))
        if any(abs(o) >= 2 ** 63 for o in origin):
            raise ValueError("origin must fit in int64, not %r" % (origin,))
        if (batch_index is None) != (batch_size is None):
            raise ValueError("batch_size is required exactly when batch_index is given")
        if batch_size is None:
            batch_size = 1
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError("batch_size must be an int >= 1, not %r" % (batch_size,))
        batch_size = int(batch_size)
        if v > ROW_MAX:
            raise ValueError("VoxelDenseMap takes at most 2^31 - 1 voxels")
        dense_shape = tuple(shape[a] for a in axes)
        cells = batch_size * shape[0] * shape[1] * shape[2]
        if cells > _MAX_CELLS:
            raise ValueError("VoxelDenseMap takes at most 2^39 - 1 cells (batch_size * A * B * D), not %d" % cells)
        dev = device_of(coords)
        self.device, self.num_voxels, self.batch_size = dev, v, batch_size
        self.spatial_shape, self.dense_shape, self.origin, self.axes = shape, dense_shape, origin, axes
        self.cells_per_sample = cells // batch_size
        coords = coords.to(device=dev, dtype=torch.int64).contiguous()
        batch = None if batch_index is None else batch_index.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            self.cell = torch.empty((v,), dtype=torch.int64, device=dev)
            self.index = torch.empty((cells,), dtype=torch.int32, device=dev)
            counts = torch.empty((2,), dtype=torch.int64, device=dev)
            rc = _lib.load().d3d_vdense_map(_lib.ptr(coords), _lib.ptr(batch), v, (ctypes.c_int64 * 3)(*shape), (ctypes.c_int64 * 3)(*origin),
                                            (ctypes.c_int32 * 3)(*axes), batch_size, _lib.ptr(self.cell), _lib.ptr(self.index),
                                            _lib.ptr(counts), _lib.stream_ptr())
            _lib.check(rc, "vdense_map")
            outside, dups = counts.tolist()                      # the one read-back of a frame's map
        if outside:
            raise ValueError("coords holds %d rows outside the grid: origin %r, spatial_shape %r, batch_size %d"
                             % (outside, origin, shape, batch_size))
        if dups:
            raise ValueError("coords holds %d rows whose (batch, coordinate) an earlier row already has" % dups)

    def grid_shape(self, c):
        """the shape of the dense tensor of c channels: (N, c, A, B, D)"""
        return (self.batch_size, c) + self.dense_shape


def _scatter(feat, dmap, fill=0.0):
    """feat [V, C] on dmap.device -> [N, C, A, B, D]; one launch writes every element"""
    c = feat.shape[1]
    with torch.cuda.device(dmap.device):
        out = torch.empty(dmap.grid_shape(c), dtype=feat.dtype, device=dmap.device)
        rc = _lib.load().d3d_vdense_scatter(_lib.ptr(feat), dmap.num_voxels, c, FEATURE_CODES[feat.dtype], _lib.ptr(dmap.index), dmap.batch_size,
                                            dmap.cells_per_sample, fill, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "vdense_scatter")
    return out


def _gather(dense, dmap):
    """dense [N, C, A, B, D] on dmap.device -> [V, C]; one launch, every row written once"""
    c = dense.shape[1]
    with torch.cuda.device(dmap.device):
        out = torch.empty((dmap.num_voxels, c), dtype=dense.dtype, device=dmap.device)
        rc = _lib.load().d3d_vdense_gather(_lib.ptr(dense), dmap.batch_size, c, FEATURE_CODES[dense.dtype], _lib.ptr(dmap.index),
                                           dmap.cells_per_sample, dmap.num_voxels, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "vdense_gather")
    return out


def _front(x, what, dmap, fill, scatter):
    if not isinstance(dmap, VoxelDenseMap):
        raise TypeError("dmap must be a VoxelDenseMap")
    x, was_numpy = as_tensor(x, what)
    dtype_code(x, FEATURE_CODES, what)                       # (the dtype first, then the fill, then the shape: this front's own order)
    if scatter:
        if isinstance(fill, bool) or not isinstance(fill, (int, float)):
            raise TypeError("fill_value must be a number, not %r" % (fill,))
        if x.dim() != 2:
            raise ValueError("%s must be a 2-D tensor of one row per voxel" % what)
        if x.shape[0] != dmap.num_voxels:
            raise ValueError("%s has %d rows where the VoxelDenseMap expects %d" % (what, x.shape[0], dmap.num_voxels))
        fill = float(fill)
    elif x.dim() != 5 or tuple(x.shape) != dmap.grid_shape(x.shape[1]):
        raise ValueError("%s has the shape %r where the VoxelDenseMap expects (%d, C, %d, %d, %d)"
                         % ((what, tuple(x.shape), dmap.batch_size) + dmap.dense_shape))
    check_owner_device(dmap, x)
    ops = (partial(_scatter, fill=fill), _gather) if scatter else (_gather, _scatter)      # each the other's gradient, its fill 0
    return back_to_caller(TransposePair.apply(x, dmap, *ops), was_numpy)


def voxel_to_dense(features, dmap, fill_value=0):
    """Scatter sparse voxel rows into a dense channels-first grid (spconv's `.dense()`).

    :param features: [V, C] float32, float64, float16 or bfloat16, any C >= 0; torch tensor (GPU or host) or numpy array;
        differentiable (once)
    :param dmap: the frame's VoxelDenseMap
    :param fill_value: what every cell without a voxel holds, rounded to the dtype; the default is +0.0, -inf is the useful
        alternative before a dense max-pool
    :return: a fresh contiguous [N, C, A, B, D] ((A, B, D) = dmap.dense_shape) on the side features came from.  A present cell holds
        its row's values bit for bit (NaN payloads, infinities and -0.0 are kept).  Every element is written exactly once, by ONE
        launch: no memset before it, no [.., C]-minor intermediate.  The gradient is voxel_from_dense of the incoming gradient;
        fill_value plays no part in it.  Channels-first only: there is no channels-last output
    """
    return _front(features, "features", dmap, fill_value, True)


def voxel_to_bev(features, dmap, fill_value=0):
    """voxel_to_dense(...).flatten(1, 2): the same tensor viewed [N, C * A, B, D], no copy -- with axes=(2, 1, 0) on (x, y, z)
    coordinates the usual BEV map [N, C * Z, Y, X]."""
    dense = voxel_to_dense(features, dmap, fill_value)
    if torch.is_tensor(dense):
        return dense.flatten(1, 2)
    return dense.reshape(dense.shape[0], -1, dense.shape[3], dense.shape[4])      # (numpy in, numpy out: a view as well)


def voxel_from_dense(dense, dmap):
    """The transpose of voxel_to_dense: read a dense tensor at the active sites of a map.

    :param dense: [N, C, A, B, D] float32, float64, float16 or bfloat16 in the layout voxel_to_dense returns (a BEV map: unflatten
        it first); differentiable (once).  Another shape, dtype or device than the map expects raises ValueError
    :param dmap: the frame's VoxelDenseMap
    :return: [V, C] on the side dense came from: out[v, c] = dense[n(v), c, cell(v)], every row written once.  Its gradient is
        voxel_to_dense(grad, dmap, 0).  It reads at the sites of the map only: it does NOT discover the active sites (the nonzeros)
        of an arbitrary dense tensor
    """
    return _front(dense, "dense", dmap, None, False)


__all__ = ["VoxelDenseMap", "voxel_to_dense", "voxel_to_bev", "voxel_from_dense"]
