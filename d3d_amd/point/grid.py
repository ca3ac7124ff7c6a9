"""d3d_amd.point.grid -- PointGrid: a uniform cell index of a cloud, built once per frame, that ball_query, knn_query and PointInterp
take in place of the points.  The grid route reads only the cells a centre can reach and returns BIT FOR BIT what the brute-force
route returns: made for a whole frame against itself (KPConv / PointNeXt / Point Transformer neighbourhoods, Voxel R-CNN's voxel
query, normals), where O(M N) is out of reach.  An extension (the reference has no point sampling).

    grid = PointGrid(cloud, 0.8)                                    # once per cloud: bounds, one read-back, the cell index
    table, counts = ball_query(grid, cloud, 0.8, 16)                # [N, 16] int32 rows (-1: none), [N] int32
    table, dist2 = knn_query(grid, cloud, 16)                       # [N, 16] int32 rows, squared distances
    interp = PointInterp(grid, queries, k=3)

The rules stand in include/d3d_hip.h, the kernels in csrc/pgrid.hip, the proofs in DESIGN.md 8j.  nsample and k stop at 64 here.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._rows import FLOAT_CODES, ROW_MAX, as_tensor, check_xyz_rows, device_of, host_offsets, rows_on

GRID_MAX = _lib.KNN_MAX              # nsample / k of the grid route: one held entry per lane


class _Segment(ctypes.Structure):    # D3DPointGridSegment
    _fields_ = [("lo", ctypes.c_double * 3), ("h", ctypes.c_double), ("inv_h", ctypes.c_double), ("base", ctypes.c_int64),
                ("dim", ctypes.c_int32 * 3), ("pad_", ctypes.c_int32)]


def _positive(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
        raise ValueError("%s must be a finite positive number, not %r" % (what, v))
    return float(v)


def grid_plan(bounds, finite_rows, cell_size, max_cells_per_point=2.0):
    """d3d_point_grid_plan, pure host arithmetic: bounds [S, 6] float64 (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), finite_rows [S] ->
    (a list of S dicts with lo, h, inv_h, dims, base; total_cells).  ValueError for what the entry refuses."""
    bounds = np.ascontiguousarray(np.asarray(bounds, np.float64).reshape(-1, 6))
    rows = np.ascontiguousarray(np.asarray(finite_rows, np.int64).reshape(-1))
    if len(bounds) != len(rows):
        raise ValueError("bounds names %d segments, finite_rows %d" % (len(bounds), len(rows)))
    plan, total = _plan(bounds, rows, _positive(cell_size, "cell_size"), _positive(max_cells_per_point, "max_cells_per_point"))
    return [dict(lo=tuple(g.lo), h=g.h, inv_h=g.inv_h, dims=tuple(g.dim), base=g.base) for g in plan[:len(rows)]], total


def _plan(bounds, rows, cell_size, max_cells_per_point):
    plan, total = (_Segment * max(len(rows), 1))(), ctypes.c_int64(-1)
    rc = _lib.load().d3d_point_grid_plan(bounds.ctypes.data, rows.ctypes.data, len(rows), cell_size, max_cells_per_point,
                                         ctypes.addressof(plan), ctypes.byref(total))
    if rc == _lib.ERR_UNSUPPORTED:
        raise ValueError("the grid would hold more than 2^31 - 1 cells (or its extent is not finite): raise cell_size or lower max_cells_per_point")
    _lib.check(rc, "point_grid_plan")
    return plan, total.value


class PointGrid:
    """The cell index of one cloud (or of every segment of a ragged batch), built once and queried many times.

    :param points: [N, D], D >= 3, float32 or float64; columns 0..2 are used, rows as they lie.  torch tensor (GPU or host) or numpy
        array; the grid keeps them (on the GPU) together with their coordinates in cell order
    :param cell_size: the edge of a cell, a finite positive float: about the radius of the balls, or the distance of the k-th
        neighbour.  Any value gives the same tables; it decides the time alone
    :param offsets: [B + 1] segment boundaries as furthest_point_sample's; None: one segment.  A grid built with offsets wants
        center_offsets from every query, one without wants none
    :param max_cells_per_point: the memory bound: a segment gets at most max(64, ceil(max_cells_per_point * its finite rows)) cells,
        cell_size is doubled until they fit (`cell_size` tells)

    Read-only: `cell_size` (per segment, after the doubling), `dims` (per segment (x, y, z) cells), `bases`, `num_cells` (all
    segments, overflow cells included), `order` (int32, the mapped rows grouped by cell, ascending row inside a cell), `offsets`
    (int64 [num_cells + 1]), `packed` ([len(order), 3], the coordinates in cell order), `mapping` (int64 [N]: the cell of a row, -1
    for a NaN row), `num_points`, `point_offsets`, `dtype`, `device`.  One host read-back (the bounds); no float atomics, the same
    bits on every run.  Raises ValueError before any GPU work for a wrong shape, dtype, cell_size, max_cells_per_point or offsets."""

    def __init__(self, points, cell_size, offsets=None, max_cells_per_point=2.0):
        points, was_numpy = as_tensor(points, "points")
        check_xyz_rows(points, "points")
        cell_size, cap = _positive(cell_size, "cell_size"), _positive(max_cells_per_point, "max_cells_per_point")
        n = points.shape[0]
        if n > ROW_MAX:
            raise ValueError("a PointGrid takes at most 2^31 - 1 points")
        offs = host_offsets(offsets, n, "offsets") if offsets is not None else None
        s = len(offs) - 1 if offs is not None else 1
        odev, dev = points.device, device_of(points)
        pts, stride = rows_on(points, dev)
        lib, code = _lib.load(), FLOAT_CODES[pts.dtype]
        with torch.cuda.device(dev):
            poffs = torch.from_numpy(np.asarray(offs, np.int64)).to(dev) if offs is not None else None
            if s == 0:                                   # a batch of no segments: nothing to index, and no centre can ask
                plan, total = (_Segment * 1)(), 0
                mapping, order, packed = (torch.empty((0,), dtype=t, device=dev) for t in (torch.int64, torch.int32, pts.dtype))
                cells, counts, plan_dev = torch.zeros((1,), dtype=torch.int64, device=dev), torch.zeros((2,), dtype=torch.int64, device=dev), None
            else:
                box = torch.empty((s * 7,), dtype=torch.int64, device=dev)      # [S, 6] doubles, then [S] int64
                rc = lib.d3d_point_grid_bounds(_lib.ptr(pts), n, stride, code, _lib.ptr(poffs), s, _lib.ptr(box), _lib.ptr(box[s * 6:]),
                                               _lib.stream_ptr())
                _lib.check(rc, "point_grid_bounds")
                host = box.cpu().numpy()                 # the one read-back
                plan, total = _plan(np.ascontiguousarray(host[:s * 6].view(np.float64)), np.ascontiguousarray(host[s * 6:]), cell_size, cap)
                plan_dev = torch.from_numpy(np.frombuffer(bytes(plan), np.uint8).copy()).to(dev)
                mapping = torch.empty((n,), dtype=torch.int64, device=dev)
                order = torch.empty((n,), dtype=torch.int32, device=dev)
                cells = torch.empty((total + 1,), dtype=torch.int64, device=dev)
                counts = torch.empty((2,), dtype=torch.int64, device=dev)
                packed = torch.empty((n * 3,), dtype=pts.dtype, device=dev)
                ws = _lib.workspace(lib.d3d_point_grid_workspace_bytes(n, total), dev)
                rc = lib.d3d_point_grid_build(_lib.ptr(pts), n, stride, code, _lib.ptr(poffs), s, _lib.ptr(plan_dev), total, _lib.ptr(mapping),
                                              _lib.ptr(order), _lib.ptr(cells), _lib.ptr(counts), _lib.ptr(packed), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr())
                _lib.check(rc, "point_grid_build")
        self._set(dev, pts, offs, [plan[i] for i in range(s)], total, plan_dev, mapping, order, cells, packed, counts, odev, was_numpy)

    def _set(self, dev, points, offs, plan, total, plan_dev, mapping, order, cells, packed, counts, odev=None, was_numpy=False):
        self.device, self.points, self.point_offsets = dev, points, offs
        self.num_points, self.dtype, self.num_cells = int(points.shape[0]), points.dtype, int(total)
        self.cell_size = tuple(float(g.h) for g in plan)
        self.dims = tuple(tuple(int(d) for d in g.dim) for g in plan)
        self.bases = tuple(int(g.base) for g in plan)
        self.lo = tuple(tuple(float(v) for v in g.lo) for g in plan)
        self.mapping, self.offsets = mapping, cells
        self._plan, self._order, self._packed, self._counts, self._mapped = plan_dev, order, packed, counts, None
        self._odev, self._was_numpy = (points.device if odev is None else odev), was_numpy

    @property
    def num_segments(self):
        return len(self.cell_size)

    @property
    def num_mapped(self):
        """the rows without a NaN coordinate: the entries of `order` (read back once)"""
        if self._mapped is None:
            self._mapped = int(self._counts[0])
        return self._mapped

    @property
    def order(self):
        return self._order[:self.num_mapped]

    @property
    def packed(self):
        return self._packed[:self.num_mapped * 3].view(-1, 3)

    # ---- what sample.py / knn.py ask of a grid: the checks of a query that only the grid can make, and the two launches ----
    def check_query(self, centers, width, what, point_offsets, center_offsets, brute):
        """refusals of a query on this grid, before any GPU work -> the centre offsets as a list (None: one segment)"""
        if point_offsets is not None:
            raise ValueError("a PointGrid carries its own segments: give %s alone" % what[1])
        if (center_offsets is None) != (self.point_offsets is None):
            raise ValueError("%s is required iff the PointGrid was built with offsets" % what[1])
        if width > GRID_MAX:
            raise ValueError("%s is at most %d on a PointGrid, not %d: pass the points themselves for the brute-force route%s"
                             % (what[0], GRID_MAX, width, brute))
        if centers.is_cuda and centers.device != self.device:
            raise ValueError("centres live on %s, the PointGrid on %s" % (centers.device, self.device))
        if center_offsets is None:
            return None
        coffs = host_offsets(center_offsets, centers.shape[0], what[1])
        if len(coffs) != len(self.point_offsets):
            raise ValueError("the PointGrid has %d segments, %s %d" % (len(self.point_offsets) - 1, what[1], len(coffs) - 1))
        return coffs

    def _centres(self, centers, coffs):
        ctr, cstride = rows_on(centers, self.device)
        dev_offs = torch.from_numpy(np.asarray(coffs, np.int64)).to(self.device) if coffs is not None else None
        return ctr, cstride, dev_offs

    def ball(self, centers, coffs, radius, nsample, pad_first):
        """-> (table [M, nsample] int32, counts [M] int32) on the grid's GPU; M > 0"""
        m = centers.shape[0]
        with torch.cuda.device(self.device):
            ctr, cstride, dev_offs = self._centres(centers, coffs)
            table = torch.empty((m, nsample), dtype=torch.int32, device=self.device)
            counts = torch.empty((m,), dtype=torch.int32, device=self.device)
            rc = _lib.load().d3d_ball_query_grid(_lib.ptr(ctr), m, cstride, FLOAT_CODES[self.dtype], _lib.ptr(dev_offs), self.num_segments,
                                                 _lib.ptr(self._plan), _lib.ptr(self._order), _lib.ptr(self.offsets), _lib.ptr(self._packed),
                                                 self.num_points, float(radius), nsample, int(pad_first), _lib.ptr(table), _lib.ptr(counts),
                                                 _lib.stream_ptr())
        _lib.check(rc, "ball_query (grid)")
        return table, counts

    def knn(self, centers, coffs, k, want_dist):
        """-> (table [M, k] int32, dist2 [M, k] or None) on the grid's GPU; M > 0"""
        m = centers.shape[0]
        with torch.cuda.device(self.device):
            ctr, cstride, dev_offs = self._centres(centers, coffs)
            table = torch.empty((m, k), dtype=torch.int32, device=self.device)
            dist2 = torch.empty((m, k), dtype=self.dtype, device=self.device) if want_dist else None
            rc = _lib.load().d3d_knn_query_grid(_lib.ptr(ctr), m, cstride, FLOAT_CODES[self.dtype], _lib.ptr(dev_offs), self.num_segments,
                                                _lib.ptr(self._plan), _lib.ptr(self._order), _lib.ptr(self.offsets), _lib.ptr(self._packed),
                                                self.num_points, k, _lib.ptr(table), _lib.ptr(dist2), _lib.stream_ptr())
        _lib.check(rc, "knn_query (grid)")
        return table, dist2


__all__ = ["PointGrid", "grid_plan"]
