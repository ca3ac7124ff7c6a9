"""d3d_amd.point.roi -- from a proposal box back to features: the points inside every rotated box binned into the cells of the box's own
grid and pooled per cell (Part-A2's roiaware_pool3d), or sampled to a fixed count per box (PointRCNN's roipoint_pool3d); and the same
differentiable pooling for any -1-padded table (a ball_query or knn_query table).  An extension (the reference has crop_points only).

    grid   = RoiGrid(cloud, boxes, out_size=12, max_points_per_cell=128)       # once per frame: table, counts, inside
    pooled = roiaware_pool3d(point_features, grid, "max")                       # [M, 12, 12, 12, C], differentiable in the features
    table, _ = ball_query(cloud, cloud[idx], 0.8, 16)
    grouped = group_pool(point_features, table, "max")                          # [M', C]: a set abstraction's pooling
    rois, empty = roipoint_pool3d(cloud, point_features, boxes, 512)            # [M, 512, 3 + C], [M] bool

Defined exactly (the rules: include/d3d_hip.h; kernels: csrc/roipool.hip, csrc/vtpool.hip): membership is crop_points' test on finite
points, a cell's entries are its first P members in ascending row, the pooling folds them in that order and its gradient folds, per
point, the entries that name it in ascending entry -- no [M, N] mask, no float atomics, the same bits on every run.
"""
import ctypes
import types

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._rows import FEATURE_CODES, ROW_MAX, as_tensor, back_to_caller, check_rows, device_of, host_offsets, on_owner, rows_on
from ..voxel.pool import EXTREME, REDUCTIONS, VoxelIndex
from ..voxel.interp import WeightedTable
from .knn import PointInterp, point_interpolate

_P_MAX = 1024                       # max_points_per_cell
_K_MAX = 343                        # the table pool's width limit
_PADS = {"none": 0, "cycle": 1}


def roi_grid_max_cells():
    """The largest number of cells ox * oy * oz of a RoiGrid.  Pure host."""
    return int(_lib.load().d3d_roi_grid_max_cells())


def roi_grid_plan(segment_rows, cells=1):
    """-> (tile_rows, slab_rows, round_rows): for a segment of that many points and a grid of `cells` cells, the rows one ballot of the
    table kernel judges, the contiguous rows one wavefront judges at a time, and the rows a workgroup takes between two barriers (a
    whole number of slabs).  Where the kernel's seams lie, not what it computes.  Pure host arithmetic."""
    tile, slab, rnd = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().d3d_roi_grid_plan(int(segment_rows), int(cells), ctypes.byref(tile), ctypes.byref(slab), ctypes.byref(rnd)),
               "roi_grid_plan")
    return tile.value, slab.value, rnd.value


class PoolTable(WeightedTable):
    """A -1-padded table [rows, width] int32 on `device` that names rows of a source of `src_rows` rows -- no weights: it is pooled, not
    folded -- and, through WeightedTable's transpose(), its inverted index: `order` [E] int32 and `offsets` [src_rows + 1] int64, per
    source row the table entries e = r * width + kk that hold it, in ascending e; built on the first call and kept."""

    def __init__(self, device, table, src_rows):
        self.device, self.table, self.src_rows = device, table, int(src_rows)
        self.num_voxels, self.width = table.shape[0], table.shape[1]          # (num_voxels: the rows, as the table views call them)
        self._index = None

    def _invert(self):
        """over the PRESENT entries only (the table is mostly padding): their numbers are gathered, a VoxelIndex runs over their rows,
        the two are composed"""
        flat = self.table.reshape(-1)
        present = torch.nonzero(flat >= 0).view(-1)                           # ascending entry number
        idx = VoxelIndex(flat[present], self.src_rows, keep_mapping=False)
        return types.SimpleNamespace(order=present.to(torch.int32)[idx.order.long()].contiguous(), offsets=idx.offsets)


def _pool_forward(feat, owner, red, need_arg, need_count):
    rows, c = owner.num_voxels, feat.shape[1]
    with torch.cuda.device(owner.device):
        out = torch.empty((rows, c), dtype=feat.dtype, device=owner.device)
        arg = torch.empty((rows, c), dtype=torch.int16, device=owner.device) if need_arg else None
        count = torch.empty((rows,), dtype=torch.int32, device=owner.device) if need_count else None
        if rows and c:
            rc = _lib.load().d3d_table_pool_forward(_lib.ptr(feat), owner.src_rows, c, FEATURE_CODES[feat.dtype], _lib.ptr(owner.table), rows,
                                                    owner.width, red, _lib.ptr(out), _lib.ptr(arg), _lib.ptr(count), _lib.stream_ptr())
            _lib.check(rc, "table_pool")
    return out, arg, count


def _pool_backward(grad, owner, red, arg, count):
    v, c = owner.src_rows, grad.shape[1]
    with torch.cuda.device(owner.device):
        if v == 0 or c == 0 or owner.num_voxels == 0:
            return grad.new_zeros((v, c))
        idx = owner.transpose()
        if idx.order.numel() == 0:
            return grad.new_zeros((v, c))
        out = torch.empty((v, c), dtype=grad.dtype, device=owner.device)
        rc = _lib.load().d3d_table_pool_backward_index(_lib.ptr(grad), owner.num_voxels, c, FEATURE_CODES[grad.dtype], _lib.ptr(idx.order),
                                                       _lib.ptr(idx.offsets), v, owner.width, red, _lib.ptr(arg), _lib.ptr(count),
                                                       _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "table_pool backward")
    return out


class IndexPool(torch.autograd.Function):
    """(features [owner.src_rows, C], a PoolTable, the reduction code) -> [rows, C], one launch; the gradient is one launch through the
    table's inverted index.  Saves the winners' columns (max / min) or the counts (mean).  Differentiable once, in the features."""

    @staticmethod
    def forward(ctx, features, owner, red):
        need = ctx.needs_input_grad[0]
        out, arg, count = on_owner(_pool_forward, features, owner, features.device, red, need and red in EXTREME,
                                   need and red == _lib.REDUCE_MEAN)
        if need:
            ctx.owner, ctx.red, ctx.odev = owner, red, features.device
            ctx.save_for_backward(*[t for t in (arg, count) if t is not None])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        saved = ctx.saved_tensors[0] if ctx.saved_tensors else None
        arg, count = (saved, None) if ctx.red in EXTREME else (None, saved)
        return on_owner(_pool_backward, grad, ctx.owner, ctx.odev, ctx.red, arg, count), None, None


def _check_reduction(reduction, who):
    if not isinstance(reduction, str) or reduction.lower() not in REDUCTIONS:
        raise ValueError("Unsupported reduction %r in %s: sum, mean, max or min" % (reduction, who))
    return REDUCTIONS[reduction.lower()]


def _check_int(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s must be an int in %d .. %d, not %r" % (what, lo, hi, v))
    return int(v)


class RoiGrid:
    """The cell table of one frame's RoIs: which points lie in which cell of which box.

    :param points: [N, D], D >= 3, float32; columns 0..2 are the coordinates.  torch tensor (GPU or host) or numpy array
    :param boxes: [M, 7] float32 rows (x, y, z, lx, ly, lz, rz), z the centre, as crop_points reads them
    :param out_size: an int or (ox, oy, oz): the cells per axis of every box's grid, ox * oy * oz <= roi_grid_max_cells()
    :param max_points_per_cell: P in 1 .. 1024
    :param point_offsets, box_offsets: [B + 1] segment boundaries of the two arrays, both or neither, as ball_query's; a box sees the
        points of its own segment only
    :param pad: 'none': the slots after a cell's last entry are -1; 'cycle' (PointRCNN's fill): slot j >= count repeats entry
        j % count -- an empty cell stays -1

    Holds on the GPU `table` [M, ox, oy, oz, P] int32 (global point rows, -1: none), `counts` [M, ox, oy, oz] int32 (the kept entries),
    `inside` [M] int32 (all members of the box, uncapped), and `num_points` = N, `num_boxes` = M, `out_size`, `max_points_per_cell`.
    The rule (exact, include/d3d_hip.h): a point is a member iff it is finite and crop_points' test holds; its cell comes from its
    fp32 local coordinates, clamped into the grid; a cell keeps its first P members in ascending row.  `transpose()` -> the inverted
    index (`order` [E] int32, `offsets` [N + 1] int64: per point the entries of the flattened [M * G * P] table that hold it, in
    ascending entry), built from the PRESENT entries only on the first call and kept: what the gradient of roiaware_pool3d walks.
    Nothing here is differentiable.  Every refusal raises ValueError before a GPU is needed."""

    def __init__(self, points, boxes, out_size=12, max_points_per_cell=128, point_offsets=None, box_offsets=None, pad="none"):
        points, _ = as_tensor(points, "points")
        boxes, _ = as_tensor(boxes, "boxes")
        if points.dim() != 2 or points.shape[1] < 3:
            raise ValueError("points must be [N, D] with D >= 3 (columns 0..2 are the coordinates), not %s" % (tuple(points.shape),))
        if boxes.dim() != 2 or boxes.shape[1] != 7:
            raise ValueError("boxes must be [M, 7] rows (x, y, z, lx, ly, lz, rz), not %s" % (tuple(boxes.shape),))
        if points.dtype != torch.float32 or boxes.dtype != torch.float32:
            raise ValueError("points and boxes must be float32, not %s and %s" % (points.dtype, boxes.dtype))
        if isinstance(out_size, (int, np.integer)) and not isinstance(out_size, bool):
            out_size = (out_size,) * 3
        if not isinstance(out_size, (tuple, list)) or len(out_size) != 3:
            raise ValueError("out_size must be an int or three, not %r" % (out_size,))
        out_size = tuple(_check_int(v, "out_size", 1, ROW_MAX) for v in out_size)
        g = out_size[0] * out_size[1] * out_size[2]
        if g > roi_grid_max_cells():
            raise ValueError("out_size %s has %d cells, more than %d" % (out_size, g, roi_grid_max_cells()))
        p = _check_int(max_points_per_cell, "max_points_per_cell", 1, _P_MAX)
        if not isinstance(pad, str) or pad.lower() not in _PADS:
            raise ValueError("pad must be 'none' or 'cycle', not %r" % (pad,))
        if (point_offsets is None) != (box_offsets is None):
            raise ValueError("point_offsets and box_offsets go together: give both or neither")
        n, m = points.shape[0], boxes.shape[0]
        if n > ROW_MAX or m * g * p > ROW_MAX:
            raise ValueError("a RoiGrid takes at most 2^31 - 1 points and table slots (boxes x cells x max_points_per_cell)")
        segments = 0
        if point_offsets is not None:
            poffs, boffs = host_offsets(point_offsets, n, "point_offsets"), host_offsets(box_offsets, m, "box_offsets")
            if len(poffs) != len(boffs):
                raise ValueError("point_offsets names %d segments, box_offsets %d" % (len(poffs) - 1, len(boffs) - 1))
            segments = len(poffs) - 1
        dev = device_of(points, boxes)
        self.device, self.num_points, self.num_boxes, self.out_size, self.max_points_per_cell = dev, n, m, out_size, p
        self.pad = pad.lower()
        with torch.cuda.device(dev):
            table = torch.empty((m * g, p), dtype=torch.int32, device=dev)
            counts = torch.empty((m,) + out_size, dtype=torch.int32, device=dev)
            inside = torch.empty((m,), dtype=torch.int32, device=dev)
            if m:
                pts, pstride = rows_on(points, dev)
                bxs = boxes.detach().to(dev).contiguous()
                both = torch.from_numpy(np.asarray(poffs + boffs, np.int64)).to(dev) if segments else None
                size = (ctypes.c_int32 * 3)(*out_size)
                rc = _lib.load().d3d_roi_grid_table(_lib.ptr(pts), n, pstride, _lib.ptr(bxs), m, 7, 0, _lib.F32,
                                                    _lib.ptr(both[:segments + 1]) if segments else None,
                                                    _lib.ptr(both[segments + 1:]) if segments else None, segments,
                                                    ctypes.cast(size, ctypes.c_void_p), p, _PADS[self.pad], _lib.ptr(table), _lib.ptr(counts),
                                                    _lib.ptr(inside), _lib.stream_ptr())
                _lib.check(rc, "roi_grid_table")
        self._pool = PoolTable(dev, table, n)
        self.table, self.counts, self.inside = table.view((m,) + out_size + (p,)), counts, inside
        self.transpose = self._pool.transpose


def roiaware_pool3d(features, grid, reduction="max"):
    """Pool point features per cell of every RoI (Part-A2's roiaware_pool3d).

    :param features: [N, C] float32, float64, float16 or bfloat16, one row per point of the grid; torch tensor (GPU or host) or numpy
        array; differentiable (once)
    :param grid: the frame's RoiGrid; max_points_per_cell at most 343 (the table pool's width)
    :param reduction: 'max' | 'min' | 'sum' | 'mean' (any case), by sparse_pool3d's rules over a cell's entries in ascending slot; an
        empty cell gives 0
    :return: [M, ox, oy, oz, C] on the side the features came from.  The gradient goes to the winner (max / min; ties: the lowest
        slot), to every entry (sum), divided by the count (mean), and is summed per point over the entries that name it in ascending
        entry number of the flattened table: the same bits on every run
    """
    if not isinstance(grid, RoiGrid):
        raise TypeError("grid must be a RoiGrid")
    if grid.max_points_per_cell > _K_MAX:
        raise ValueError("roiaware_pool3d pools at most %d points per cell, the grid keeps %d" % (_K_MAX, grid.max_points_per_cell))
    red = _check_reduction(reduction, "roiaware_pool3d")
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "point", "features", FEATURE_CODES, grid, grid.num_points)
    out = IndexPool.apply(features, grid._pool, red)
    return back_to_caller(out.view((grid.num_boxes,) + grid.out_size + (out.shape[1],)), was_numpy)


def group_pool(features, table, reduction="max"):
    """Pool the rows a table names: the differentiable consumer of a ball_query or knn_query table.

    :param features: [N, C] float32, float64, float16 or bfloat16; differentiable (once)
    :param table: [M, K] int32, K in 1 .. 343, rows of `features` in [0, N), -1 for "none"; torch tensor or numpy array.  Checked once
        (ValueError for an entry outside [-1, N)): one number read back when it lives on the GPU
    :param reduction: 'max' | 'min' | 'sum' | 'mean', as roiaware_pool3d's; a row without entries gives 0
    :return: [M, C] on the side the features came from
    """
    table, _ = as_tensor(table, "table")
    if table.dim() != 2 or table.dtype != torch.int32:
        raise ValueError("table must be a [M, K] int32 tensor")
    if not 1 <= table.shape[1] <= _K_MAX:
        raise ValueError("the width of the table must be in 1 .. %d, not %d" % (_K_MAX, table.shape[1]))
    red = _check_reduction(reduction, "group_pool")
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "point", "features", FEATURE_CODES)
    n = features.shape[0]
    if n > ROW_MAX or table.numel() > ROW_MAX:
        raise ValueError("group_pool takes at most 2^31 - 1 rows and table entries")
    if table.numel() and bool(((table < -1) | (table >= n)).any()):
        raise ValueError("table holds rows outside [-1, %d)" % n)
    dev = device_of(features, table)
    owner = PoolTable(dev, table.detach().to(dev).contiguous(), n)
    return back_to_caller(IndexPool.apply(features, owner, red), was_numpy)


def roipoint_pool3d(points, features, boxes, num_samples=512, point_offsets=None, box_offsets=None):
    """A fixed number of points per RoI with their features (PointRCNN's roipoint_pool3d).

    :param points: [N, D], D >= 3, float32, and
    :param boxes: [M, 7] float32, as RoiGrid's
    :param features: [N, C] float32, float64, float16 or bfloat16; differentiable (once)
    :param num_samples: S in 1 .. 1024: the first S members of a box in ascending row; a box with fewer repeats them cyclically
    :param point_offsets, box_offsets: as RoiGrid's
    :return: (pooled [M, S, 3 + C] in the dtype of the features -- xyz (rounded once to that dtype) then the features --, empty [M] bool)
        on the side the features came from.  A box without members gets zeros and empty = True.  It is RoiGrid(out_size=1,
        max_points_per_cell=S, pad='cycle') and a gather through the width-1 fold of PointInterp.from_table: bit-exact copies,
        and the gradient of a feature row is the fold of the slots that hold it in ascending slot number
    """
    grid = RoiGrid(points, boxes, 1, num_samples, point_offsets, box_offsets, pad="cycle")
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "point", "features", FEATURE_CODES, grid, grid.num_points)
    m, s = grid.num_boxes, grid.max_points_per_cell
    table = grid.table.view(m * s, 1)
    with torch.cuda.device(grid.device):
        ones = torch.ones((m * s, 1), dtype=torch.float32, device=grid.device)
    interp = PointInterp.from_table(table, ones, grid.num_points)
    points, _ = as_tensor(points, "points")
    xyz = point_interpolate(points.detach()[:, :3].to(grid.device).contiguous(), interp)
    feat = point_interpolate(features, interp)
    pooled = torch.cat([xyz.to(device=feat.device, dtype=feat.dtype), feat], dim=1).view(m, s, 3 + features.shape[1])
    empty = _lib.to_caller(grid.inside == 0, features.device, grid.device)
    if was_numpy:
        return pooled.detach().numpy(), empty.numpy()
    return pooled, empty


__all__ = ["RoiGrid", "roiaware_pool3d", "group_pool", "roipoint_pool3d", "roi_grid_plan", "roi_grid_max_cells", "IndexPool", "PoolTable"]
