"""d3d_amd.voxel.interp -- from the voxels back to ARBITRARY points: trilinear (or nearest) interpolation of sparse voxel features at
fractional positions and its transpose, the splat of point rows onto the voxels, both differentiable in the features: the devoxelize
step of SPVCNN / PVCNN, PV-RCNN's keypoint features, the point head of a sparse U-Net.  The sparse counterpart of
d3d.point.aligned_scatter(LINEAR).  An extension (the reference stops at the voxelizer).

    sp   = VoxelGenerator(bounds, shape, max_points=32, max_points_filter="trim")(pts)    # sparse contract
    pos  = voxel_positions(pts, voxel_size, voxel_offset)        # every point of the cloud, trimmed ones and keypoints alike
    itp  = VoxelInterp(sp.coords, pos)                           # once per frame; every layer and every backward reuses it
    pf   = voxel_interpolate(backbone_features, itp)             # [K, C]
    vf   = voxel_splat(point_features, itp)                      # [V, C]: the transpose

voxel_unpool copies a voxel's row onto the points the voxelizer itself put there; this reads the 8 voxels AROUND any position, with
the trilinear weights, and skips the ones that are not active.  No float atomics: the interpolation folds a point's corners in
ascending corner, the splat (and the interpolation's gradient) a voxel's entries in ascending entry number through an inverted index
built once (`VoxelInterp.transpose()`), so the results are the same bits on every run (kernels and the exact rules: csrc/vnbr.hip,
csrc/vinterp.hip, include/d3d_hip.h).  Positions and weights get NO gradient.
"""
import torch

from .. import _lib
from .._rows import FEATURE_CODES, FLOAT_CODES, ROW_MAX, TransposePair, as_tensor, back_to_caller, check_rows, device_of
from ._coords import _check_coords, _host_spans_fit
from .pool import VoxelIndex

_MODES = {"linear": 8, "nearest": 1}


class WeightedTable:
    """A table with weights, as table_fold reads it: `table` [num_points, width] int32 names rows of a source of `src_rows` feature
    rows (-1: none), `weights` [num_points, width] float32 or float64 belong to its entries, both on `device`; `num_entries` is what
    makes a fold worth a launch (0: the result is zero).  A subclass names the pair of C entries (interpolate, splat) that fold
    through it in `_entries` and calls _set_table once its table is made: VoxelInterp here, d3d_amd.point.PointInterp."""

    _entries = None

    def _set_table(self, device, table, weights, src_rows, num_entries):
        self.device, self.table, self.weights = device, table, weights
        self.src_rows, self.num_points, self.width, self.num_entries = int(src_rows), table.shape[0], table.shape[1], num_entries
        self._index = None
        self._cast = {weights.dtype: weights}

    def transpose(self):
        """The inverted table: a VoxelIndex over the flattened table [num_points * width] taken as a mapping -- per source row the
        entries that name it, in ascending entry number.  Built on the first call (VoxelIndex's one read-back) and kept: what a splat
        and the gradient of an interpolation walk.  It holds `order` and `offsets` only: its `mapping` is None (the table is the
        mapping).  (A table that is mostly padding inverts its present entries only: _invert of d3d_amd.point.roi.)"""
        if self._index is None:
            with torch.cuda.device(self.device):
                self._index = self._invert()
        return self._index

    def _invert(self):
        return VoxelIndex(self.table.view(-1), self.src_rows, keep_mapping=False)

    def weights_as(self, dtype):
        """the weights a fold in `dtype` multiplies by: float64 for float64 features, float32 otherwise.  Weights of the other width
        are cast once -- ONE more rounding when fp64 positions meet narrower features -- and kept"""
        want = torch.float64 if dtype == torch.float64 else torch.float32
        w = self._cast.get(want)
        if w is None:
            w = self._cast[want] = self.weights.to(want)
        return w


class VoxelInterp(WeightedTable):
    """The corner table of one frame: for every position the rows of the voxels around it and their weights.

    :param coords: [V, 3] int64 (int32 is widened) voxel coordinates, any values; torch tensor (GPU or host) or numpy array.
        (batch, coordinate) must be unique
    :param positions: [K, 3] float32 or float64 in VOXEL UNITS, integer n the centre of voxel n (`voxel_positions` makes them from
        metric points); any values -- a position that is not finite or not in [-2^62, 2^62) simply has no corners
    :param batch_index: [V] int64 / int32 or None
    :param position_batch: [K] int64 / int32, required exactly when batch_index is given; a point only sees voxels of its batch value
    :param mode: "linear" -- the 8 corners b + (dx, dy, dz) of b = floor(x), column j = dx * 4 + dy * 2 + dz, weight (wx * wy) * wz with
        wa = x_a - b_a for a set bit and 1 - (x_a - b_a) otherwise -- or "nearest": the one voxel floor(x + 0.5), weight 1
    :param normalize: divide a point's weights by the sum of its PRESENT corners' weights (in ascending column): a point near the
        border of the active set gets a weighted mean of the voxels that exist instead of a value damped by the missing ones

    Holds `table` [K, J] int32 (-1: no voxel there) and `weights` [K, J] in the dtype of positions (0 where absent) on the GPU,
    `num_points`, `num_voxels`, `num_corners` = J and `num_entries` (the entries >= 0).  Building it reads three numbers back, once.
    ValueError on duplicates and when the product of the coordinate (and batch) spans exceeds 2^62, as VoxelNeighbors.  Nothing here
    is differentiable: positions and weights get no gradient."""

    _entries = ("d3d_table_interp_forward", "d3d_table_interp_backward")

    def __init__(self, coords, positions, batch_index=None, position_batch=None, mode="linear", normalize=False):
        coords, batch_index, v = _check_coords(coords, batch_index)
        positions, _ = as_tensor(positions, "positions")
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError("positions must be a [K, 3] tensor in voxel units")
        if positions.dtype not in FLOAT_CODES:
            raise ValueError("positions must be float32 or float64, not %s" % positions.dtype)
        k = positions.shape[0]
        if (batch_index is None) != (position_batch is None):
            raise ValueError("position_batch is required exactly when batch_index is given")
        if position_batch is not None:
            position_batch, _ = as_tensor(position_batch, "position_batch")
            if position_batch.dim() != 1 or position_batch.shape[0] != k:
                raise ValueError("position_batch must be a [K] tensor, one value per row of positions")
            if position_batch.dtype not in (torch.int64, torch.int32):
                raise ValueError("position_batch must be int64 or int32, not %s" % position_batch.dtype)
        if not isinstance(mode, str) or mode not in _MODES:
            raise ValueError("mode must be \"linear\" or \"nearest\", not %r" % (mode,))
        j = _MODES[mode]
        if v > ROW_MAX or k * j > ROW_MAX:
            raise ValueError("VoxelInterp takes at most 2^31 - 1 voxels and table entries (points x corners)")
        overflow = "the spans of the coordinates (and batch values) multiply to more than 2^62"
        if v and not coords.is_cuda and not _host_spans_fit(coords, None if batch_index is None or batch_index.is_cuda else batch_index):
            raise ValueError(overflow)
        dev = device_of(coords, positions)
        self.num_voxels, self.num_corners, self.mode, self.normalize = v, j, mode, bool(normalize)
        coords = coords.to(device=dev, dtype=torch.int64).contiguous()
        positions = positions.detach().to(device=dev).contiguous()
        batch = None if batch_index is None else batch_index.to(device=dev, dtype=torch.int64).contiguous()
        pbatch = None if position_batch is None else position_batch.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            table = torch.empty((k, j), dtype=torch.int32, device=dev)
            weights = torch.empty((k, j), dtype=positions.dtype, device=dev)
            entries = dups = over = 0
            if v or k:
                lib = _lib.load()
                counts = torch.empty((3,), dtype=torch.int64, device=dev)
                ws = _lib.workspace(lib.d3d_voxel_corners_workspace_bytes(v), dev)
                rc = lib.d3d_voxel_corners(_lib.ptr(coords), _lib.ptr(batch), v, _lib.ptr(positions), _lib.ptr(pbatch), k,
                                           FLOAT_CODES[positions.dtype], j, int(self.normalize), _lib.ptr(table), _lib.ptr(weights),
                                           _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "voxel_corners")
                entries, dups, over = counts.tolist()            # the one read-back of a frame's table
        if over:
            raise ValueError(overflow)
        if dups:
            raise ValueError("coords holds %d rows whose (batch, coordinate) an earlier row already has" % dups)
        self._set_table(dev, table, weights, v, entries)


def _interp(feat, itp):
    """feat [src_rows, C] on itp.device -> [num_points, C]; one launch.  itp: a WeightedTable"""
    k, c = itp.num_points, feat.shape[1]
    with torch.cuda.device(itp.device):
        if k == 0 or c == 0 or itp.num_entries == 0:
            return feat.new_zeros((k, c))
        out = torch.empty((k, c), dtype=feat.dtype, device=itp.device)
        rc = getattr(_lib.load(), itp._entries[0])(_lib.ptr(feat), itp.src_rows, c, FEATURE_CODES[feat.dtype], _lib.ptr(itp.table),
                                                   _lib.ptr(itp.weights_as(feat.dtype)), k, itp.width, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "table_interp")
    return out


def _splat(rows, itp):
    """rows [num_points, C] on itp.device -> [src_rows, C] through the inverted table; one launch, every source row written once"""
    v, c = itp.src_rows, rows.shape[1]
    with torch.cuda.device(itp.device):
        if v == 0 or c == 0 or itp.num_entries == 0:
            return rows.new_zeros((v, c))
        idx = itp.transpose()
        out = torch.empty((v, c), dtype=rows.dtype, device=itp.device)
        rc = getattr(_lib.load(), itp._entries[1])(_lib.ptr(rows), itp.num_points, c, FEATURE_CODES[rows.dtype], _lib.ptr(idx.order),
                                                   _lib.ptr(idx.offsets), _lib.ptr(itp.weights_as(rows.dtype)), itp.width, v,
                                                   _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "table_interp backward")
    return out


def table_fold(rows, itp, splat=False):
    """The interpolation of source rows [src_rows, C] through a WeightedTable -> [num_points, C], or with `splat` its transpose, the
    splat of point rows; each is the other's gradient.  Rows as a tensor anywhere, already checked; differentiable once, in the rows."""
    return TransposePair.apply(rows, itp, *((_splat, _interp) if splat else (_interp, _splat)))


def _front(rows, what, itp, splat):
    if not isinstance(itp, VoxelInterp):
        raise TypeError("interp must be a VoxelInterp")
    rows, was_numpy = as_tensor(rows, what)
    check_rows(rows, what, "point" if splat else "voxel", what, FEATURE_CODES, itp, itp.num_points if splat else itp.num_voxels)
    return back_to_caller(table_fold(rows, itp, splat), was_numpy)


def voxel_interpolate(voxel_features, interp):
    """Interpolate sparse voxel features at the positions of a VoxelInterp.

    :param voxel_features: [V, C] float32, float64, float16 or bfloat16, torch tensor (GPU or host) or numpy array; differentiable
        (once)
    :param interp: the frame's VoxelInterp
    :return: [K, C] on the side voxel_features came from: row r = 0 + w[r, 0] * f[table[r, 0]] + w[r, 1] * f[table[r, 1]] + ... over the
        PRESENT corners in ascending column, product and sum rounded separately (half types: in fp32, one rounding at the end); a point
        without corners gets a zero row.  The weights are float64 for float64 features and float32 otherwise (cast once from the
        table's when the positions had the other width: one more rounding).  The gradient reaches voxel_features only -- positions and
        weights get NONE: grad[v] = the fold of w[e] * grad_out[e // J] over the entries e that name v, in ascending e
    """
    return _front(voxel_features, "voxel_features", interp, False)


def voxel_splat(point_features, interp):
    """The transpose of voxel_interpolate: spread point rows onto the voxels around them with the same weights.

    :param point_features: [K, C] float32, float64, float16 or bfloat16; differentiable (once)
    :param interp: the frame's VoxelInterp
    :return: [V, C] on the side point_features came from: voxel v = 0 + w[e] * p[e // J] over the entries e of the flattened table that
        name v, in ascending e; a voxel that no point touches gets a zero row.  With normalize=False and positions inside the active set
        the column sums are kept (the 8 weights of a point add up to 1).  Its gradient is voxel_interpolate of the incoming gradient;
        positions and weights get NONE
    """
    return _front(point_features, "point_features", interp, True)


def voxel_positions(points, voxel_size, voxel_offset=0, dtype=None):
    """Metric points -> positions in voxel units for a VoxelInterp: points[:, :3] / voxel_size - voxel_offset - 0.5, plain torch
    arithmetic.  The sparse contract numbers a voxel floor(p / size) - offset, so its centre sits at that integer + 0.5 cells; here
    centres sit on the integers.

    :param points: [K, >= 3] tensor or numpy array (x, y, z first)
    :param voxel_size: a number or three (VoxelGenerator's `_size`)
    :param voxel_offset: a number or three, in cells (VoxelGenerator's `_offset`)
    :param dtype: the dtype of the result (default: that of points); float64 keeps positions of large grids exact to more digits
    """
    points, was_numpy = as_tensor(points, "points")
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("points must be a [K, >= 3] tensor")
    dtype = points.dtype if dtype is None else dtype
    if dtype not in FLOAT_CODES:
        raise ValueError("positions are float32 or float64, not %s" % (dtype,))
    xyz = points[:, :3].to(dtype)
    size = torch.as_tensor(voxel_size, dtype=dtype, device=xyz.device)
    off = torch.as_tensor(voxel_offset, dtype=dtype, device=xyz.device)
    out = xyz / size - off - 0.5
    return back_to_caller(out, was_numpy)


__all__ = ["VoxelInterp", "voxel_interpolate", "voxel_splat", "voxel_positions"]
