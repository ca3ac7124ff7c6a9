"""d3d_amd.point.knn -- the way back up: the k nearest known rows of every query row and the inverse-distance-weighted sum of their
features, what a PointNet++ feature-propagation layer, 3DSSD, PV-RCNN's point heads do (pointnet2's three_nn / three_interpolate),
and with a wider k the neighbourhoods of DGCNN and Point Transformer.  An extension (the reference has no point sampling).

    idx    = furthest_point_sample(cloud, 2048)
    interp = PointInterp(cloud[idx], cloud, k=3)                    # once per frame and layer: table, dist2, weights
    dense  = point_interpolate(keypoint_features, interp)           # [N, C], differentiable in the features
    table, dist2 = knn_query(cloud, cloud[idx], 16)                 # [2048, 16] int32 rows (-1: none), squared distances

Defined exactly (the rules: include/d3d_hip.h; kernels: csrc/psample.hip, csrc/vinterp.hip): the neighbours of a row are its
candidates in ascending (q, row), the interpolation folds them in that order, and its gradient is a splat through the inverted table
-- no [M, N] matrix, no [M, k, C] buffer, no float atomics, the same bits on every run.  O(M N) per segment, as pointnet2's own
three_nn: made for keypoint counts.
"""
import numpy as np
import torch

from .. import _lib
from .._rows import FEATURE_CODES, FLOAT_CODES, ROW_MAX, as_tensor, back_to_caller, check_rows, device_of, host_offsets, rows_on
from ..voxel.interp import WeightedTable, table_fold
from .grid import PointGrid
from .sample import check_xyz_rows

_K_MAX = _lib.KNN_MAX


def _check_k(k, what="k"):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("%s must be an int, not %r" % (what, k))
    if not 1 <= int(k) <= _K_MAX:
        raise ValueError("%s must be in 1 .. %d, not %d" % (what, _K_MAX, int(k)))
    return int(k)


def _check_pair(points, centers, k, point_offsets, center_offsets, names=("points", "centers")):
    """every host-side refusal of a query -> (points, centers, k, poffs + coffs or None, segments, points came as numpy).  A
    PointGrid in the place of the points comes back as it is, with the centre offsets alone (None: one segment)"""
    grid = points if isinstance(points, PointGrid) else None
    if grid is not None:
        points, was_numpy = grid.points, grid._was_numpy
    else:
        points, was_numpy = as_tensor(points, names[0])
    centers, _ = as_tensor(centers, names[1])
    check_xyz_rows(points, names[0])
    check_xyz_rows(centers, names[1])
    if points.dtype != centers.dtype:
        raise ValueError("%s (%s) and %s (%s) must share a dtype" % (names[0], points.dtype, names[1], centers.dtype))
    k = _check_k(k)
    if grid is not None:
        if centers.shape[0] * k > ROW_MAX:
            raise ValueError("a kNN query takes at most 2^31 - 1 points and table entries (centres x k)")
        coffs = grid.check_query(centers, k, ("k", names[1].rstrip("s") + "_offsets"), point_offsets, center_offsets, "")
        return grid, centers, k, coffs, grid.num_segments, was_numpy
    if (point_offsets is None) != (center_offsets is None):
        raise ValueError("%s_offsets and %s_offsets go together: give both or neither" % (names[0].rstrip("s"), names[1].rstrip("s")))
    n, m = points.shape[0], centers.shape[0]
    if n > ROW_MAX or m * k > ROW_MAX:
        raise ValueError("a kNN query takes at most 2^31 - 1 points and table entries (centres x k)")
    offs, segments = None, 0
    if point_offsets is not None:
        poffs, coffs = host_offsets(point_offsets, n, "point_offsets"), host_offsets(center_offsets, m, "center_offsets")
        if len(poffs) != len(coffs):
            raise ValueError("point_offsets names %d segments, center_offsets %d" % (len(poffs) - 1, len(coffs) - 1))
        offs, segments = poffs + coffs, len(poffs) - 1
    return points, centers, k, offs, segments, was_numpy


def _query(points, centers, k, offs, segments, dev, want_dist):
    """-> (table [M, k] int32, dist2 [M, k] or None) on dev; M > 0"""
    if isinstance(points, PointGrid):
        return points.knn(centers, offs, k, want_dist)
    n, m = points.shape[0], centers.shape[0]
    pts, pstride = rows_on(points, dev)
    ctr, cstride = rows_on(centers, dev)
    with torch.cuda.device(dev):
        both = torch.from_numpy(np.asarray(offs, np.int64)).to(dev) if segments else None
        table = torch.empty((m, k), dtype=torch.int32, device=dev)
        dist2 = torch.empty((m, k), dtype=pts.dtype, device=dev) if want_dist else None
        rc = _lib.load().d3d_knn_query(_lib.ptr(pts), n, pstride, _lib.ptr(ctr), m, cstride, FLOAT_CODES[pts.dtype],
                                       _lib.ptr(both[:segments + 1]) if segments else None,
                                       _lib.ptr(both[segments + 1:]) if segments else None, segments, k, _lib.ptr(table), _lib.ptr(dist2),
                                       _lib.stream_ptr())
    _lib.check(rc, "knn_query")
    return table, dist2


def knn_query(points, centers, k, point_offsets=None, center_offsets=None, return_distances=True):
    """The `k` nearest rows of `points` to every centre, nearest first.

    :param points: [N, D], D >= 3, and
    :param centers: [M, D'], D' >= 3, of the same dtype (float32 or float64); columns 0..2 are used.  torch tensors or numpy arrays
    :param k: 1 .. 64, the width of the table
    :param point_offsets, center_offsets: [B + 1] segment boundaries of the two arrays, both or neither; a centre sees the points of
        its own segment only.  On the host; a GPU tensor is read back once for the checks
    :param return_distances: False: return the table alone
    :return: (table [M, k] int32, dist2 [M, k] in the dtype) on the side `points` came from (numpy in, numpy out).  Table values are
        GLOBAL point rows, -1 for "none" (dist2 +inf there): the table neighbor_gather and the table pooling operators read

    The rule (exact): q as in furthest_point_sample; row i is a candidate iff q is not NaN (rows and centres that are not finite by a
    NaN drop out; a q that overflows to +inf is a candidate and sorts last); a centre's entries are its candidates in ascending
    (q, i), the lower row first where q is equal; dist2 holds their q.  O(M N) per segment: made for keypoint counts.

    A PointGrid in the place of `points` takes the grid route: the same table and the same bits of dist2 from rings of cells around
    every centre -- made for N = M = 10^5.  Its segments are the point offsets (point_offsets with it is a ValueError, center_offsets
    is required iff the grid was built with offsets); the centres' dtype must be the grid's.
    """
    points, centers, k, offs, segments, was_numpy = _check_pair(points, centers, k, point_offsets, center_offsets)
    m = centers.shape[0]
    grid = points if isinstance(points, PointGrid) else None
    odev = points.device if grid is None else grid._odev
    if m == 0:
        table, dist2 = torch.empty((0, k), dtype=torch.int32, device=odev), torch.empty((0, k), dtype=points.dtype, device=odev)
    else:
        dev = device_of(points, centers) if grid is None else grid.device
        table, dist2 = _query(points, centers, k, offs, segments, dev, return_distances)
        if return_distances:
            table, dist2 = _lib.to_caller((table, dist2), odev, dev)
        else:
            table = _lib.to_caller(table, odev, dev)
    if was_numpy:
        table, dist2 = table.numpy(), (dist2.numpy() if return_distances else None)
    return (table, dist2) if return_distances else table


class PointInterp(WeightedTable):
    """The neighbour table of one frame and layer: for every unknown (query) row its k nearest known rows and their weights.

    :param known: [Nk, D], D >= 3: the rows that carry features (the keypoints of the coarser level), or a PointGrid over them (the
        grid route of knn_query: the same table, dist2 and weights; known_offsets is then the grid's), and
    :param unknown: [Mu, D'], D' >= 3: the rows that want them, of the same dtype (float32 or float64); torch tensors or numpy arrays
    :param k: 1 .. 64 neighbours (3: pointnet2's three_nn)
    :param known_offsets, unknown_offsets: [B + 1] segment boundaries, both or neither, as knn_query's
    :param power: 1: u = 1 / (sqrt(q) + eps), pointnet2's 1 / (dist + 1e-8); 2: u = 1 / (q + eps)
    :param eps: finite, >= 0 (rounded to the dtype).  w = u / s with s = 0 + u_0 + u_1 + ... over the present entries in ascending
        column; a row whose s is 0 or not finite gets all-zero weights -- with eps = 0 that is every query row that coincides with
        a known row (u = inf): keep eps > 0 where that can happen

    Holds `table` [Mu, k] int32 (-1: none), `dist2` and `weights` [Mu, k] in the dtype of the rows (weights 0 where absent) on the
    GPU, `num_known`, `num_points` = Mu and `k`.  Nothing here is differentiable: positions and weights get no gradient."""

    _entries = ("d3d_knn_interp_forward", "d3d_knn_interp_backward")

    def __init__(self, known, unknown, k=3, known_offsets=None, unknown_offsets=None, power=1, eps=1e-8):
        known, unknown, k, offs, segments, _ = _check_pair(known, unknown, k, known_offsets, unknown_offsets, ("known", "unknown"))
        if isinstance(power, bool) or power not in (1, 2):
            raise ValueError("power must be 1 or 2, not %r" % (power,))
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not np.isfinite(eps) or eps < 0:
            raise ValueError("eps must be a finite float >= 0, not %r" % (eps,))
        eps = float(eps)
        if known.dtype == torch.float32 and eps > float(np.finfo(np.float32).max):
            raise ValueError("eps = %r is not finite in float32" % (eps,))
        dev = known.device if isinstance(known, PointGrid) else device_of(known, unknown)
        m = unknown.shape[0]
        with torch.cuda.device(dev):
            if m == 0:
                table = torch.empty((0, k), dtype=torch.int32, device=dev)
                dist2 = torch.empty((0, k), dtype=known.dtype, device=dev)
                weights = torch.empty((0, k), dtype=known.dtype, device=dev)
            else:
                table, dist2 = _query(known, unknown, k, offs, segments, dev, True)
                weights = torch.empty((m, k), dtype=dist2.dtype, device=dev)
                rc = _lib.load().d3d_knn_weights(_lib.ptr(table), _lib.ptr(dist2), m, k, FLOAT_CODES[dist2.dtype], int(power), eps,
                                                 _lib.ptr(weights), _lib.stream_ptr())
                _lib.check(rc, "knn_weights")
        self._set(dev, table, dist2, weights, known.num_points if isinstance(known, PointGrid) else known.shape[0])
        self.power, self.eps = int(power), eps

    def _set(self, dev, table, dist2, weights, num_known):
        self._set_table(dev, table, weights, num_known, table.numel())       # (the slots: absent ones are skipped by the kernel)
        self.dist2, self.num_known, self.k = dist2, int(num_known), table.shape[1]

    @classmethod
    def from_table(cls, table, weights, num_known):
        """A PointInterp over a table that came from elsewhere, e.g. a ball_query table with weights of the caller's.

        :param table: [M, J] int32 rows of the known set in [0, num_known), -1 for "none"; J in 1 .. 64
        :param weights: [M, J] float32 or float64 (an absent entry's weight is not read)
        :param num_known: the rows of the feature matrix the table names
        The table is checked once (ValueError for an entry outside [-1, num_known)): one number read back when it lives on the GPU.
        `dist2` is None."""
        table, _ = as_tensor(table, "table")
        weights, _ = as_tensor(weights, "weights")
        if table.dim() != 2 or table.dtype != torch.int32:
            raise ValueError("table must be a [M, J] int32 tensor")
        if not 1 <= table.shape[1] <= _K_MAX:
            raise ValueError("the width of the table must be in 1 .. %d, not %d" % (_K_MAX, table.shape[1]))
        if weights.shape != table.shape:
            raise ValueError("weights must have the shape of the table %s, not %s" % (tuple(table.shape), tuple(weights.shape)))
        if weights.dtype not in FLOAT_CODES:
            raise ValueError("weights must be float32 or float64, not %s" % weights.dtype)
        if isinstance(num_known, bool) or not isinstance(num_known, (int, np.integer)) or not 0 <= num_known <= ROW_MAX:
            raise ValueError("num_known must be an int in 0 .. 2^31 - 1, not %r" % (num_known,))
        if table.numel() > ROW_MAX:
            raise ValueError("a table takes at most 2^31 - 1 entries")
        if table.numel() and bool(((table < -1) | (table >= int(num_known))).any()):
            raise ValueError("table holds rows outside [-1, %d)" % int(num_known))
        dev = device_of(table, weights)
        self = cls.__new__(cls)
        self._set(dev, table.detach().to(dev).contiguous(), None, weights.detach().to(dev).contiguous(), num_known)
        self.power = self.eps = None
        return self


def point_interpolate(known_features, interp):
    """Propagate the features of the known rows to the query rows of a PointInterp (pointnet2's three_interpolate for k = 3).

    :param known_features: [Nk, C] float32, float64, float16 or bfloat16, any C; torch tensor (GPU or host) or numpy array;
        differentiable (once)
    :param interp: the PointInterp
    :return: [Mu, C] on the side known_features came from: row r = 0 + w[r, 0] * f[table[r, 0]] + w[r, 1] * f[table[r, 1]] + ... over
        the PRESENT entries in ascending column, product and sum rounded separately (half types: in fp32, one rounding at the end); a
        row without entries is 0.  The weights are float64 for float64 features and float32 otherwise (cast once).  The gradient
        reaches known_features only: grad[v] = the fold of w[e] * grad_out[e // k] over the entries e that name v, in ascending e --
        a splat through the inverted table, no float atomics, the same bits on every run
    """
    if not isinstance(interp, PointInterp):
        raise TypeError("interp must be a PointInterp")
    rows, was_numpy = as_tensor(known_features, "known_features")
    check_rows(rows, "known_features", "known point", "known_features", FEATURE_CODES, interp, interp.num_known)
    return back_to_caller(table_fold(rows, interp), was_numpy)


__all__ = ["knn_query", "PointInterp", "point_interpolate"]
