"""d3d_amd.point.sample -- furthest point sampling and ball query: choose M well-spread rows of a cloud, then group the rows inside
a radius of each.  The first two steps of a PointNet++ set abstraction, PV-RCNN's keypoints, 3DSSD, Voxel R-CNN.  An extension (the
reference has no point sampling).

    idx = furthest_point_sample(cloud, 2048)                        # [2048] int64 rows of cloud [N, 4]
    table, counts = ball_query(cloud, cloud[idx], 0.8, 16)          # [2048, 16] int32 rows (-1: none), [2048] int32

Both return indices only and are defined exactly (the rules: include/d3d_hip.h; kernels: csrc/psample.hip): the same bits on every
run.  Ragged batches go in as offsets, one workgroup per segment in ONE launch -- which is also how a huge cloud is sampled fast:
split it into sectors (PV-RCNN++'s sectorised FPS) and pass their offsets.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._rows import FLOAT_CODES, ROW_MAX, as_tensor, check_xyz_rows, device_of, host_offsets, rows_on
from .grid import PointGrid

_NSAMPLE_MAX = 1024


def fps_plan(segment_rows, dtype=torch.float32):
    """-> (route, capacity): the route a segment of that many rows takes (0 .. 2 registers, _lib.FPS_ROUTE_LDS, _lib.FPS_ROUTE_STREAM)
    and the rows that route holds.  Pure host arithmetic."""
    if dtype not in FLOAT_CODES:
        raise ValueError("dtype must be float32 or float64, not %s" % dtype)
    route, cap = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().d3d_fps_plan(int(segment_rows), FLOAT_CODES[dtype], ctypes.byref(route), ctypes.byref(cap)), "fps_plan")
    return route.value, cap.value


def furthest_point_sample(points, num_samples, offsets=None, return_distances=False):
    """Furthest point sampling of every segment of a ragged batch, one launch.

    :param points: [N, D], D >= 3, float32 or float64; columns 0..2 are used (a LiDAR [N, 4] cloud goes in as it is).  torch tensor
        (GPU or host) or numpy array
    :param num_samples: M, one int for every segment, or B ints.  M above a segment's rows is legal (the lowest row repeats once
        every distance is 0); M = 0 is legal
    :param offsets: [B + 1] segment boundaries, nondecreasing from 0 to N (list, numpy or CPU tensor; a GPU tensor is read back once,
        a blocking copy, for the host checks); None: one segment.  B = 0 is legal
    :param return_distances: also return the distance of every sample to the set before it, squared: +inf at a segment's first
        sample, then non-increasing (the coverage radius squared)
    :return: indices [sum M_b] int64, segment after segment, GLOBAL row numbers; with return_distances (indices, distances) with
        distances in the dtype of the points.  On the caller's side: host in, host out; numpy in, numpy out

    The rule (exact; every operation one rounding in the dtype): a row with a coordinate that is not finite is excluded, the others
    start at d = +inf; each step takes the non-excluded row with the largest d (the lowest row on a tie), then lowers every d to
    q = ((dx * dx) + (dy * dy)) + (dz * dz) against the new sample where that is smaller.  A segment of excluded rows only returns its
    first row M times with NaN distances.  Raises ValueError before any GPU work for malformed offsets, a segment of 0 rows with
    M > 0, a segment above 2^31 - 1 rows, a wrong dtype or shape, a negative num_samples.
    """
    points, was_numpy = as_tensor(points, "points")
    check_xyz_rows(points, "points")
    n = points.shape[0]
    offs = host_offsets(offsets, n, "offsets")
    b = len(offs) - 1
    if isinstance(num_samples, (torch.Tensor, np.ndarray)):
        num_samples = num_samples.tolist()
    if isinstance(num_samples, (list, tuple)):
        ms = [int(v) for v in num_samples]
        if len(ms) != b:
            raise ValueError("num_samples has %d entries for %d segments" % (len(ms), b))
    else:
        ms = [int(num_samples)] * b
    if any(m < 0 for m in ms):
        raise ValueError("num_samples must not be negative")
    for i, m in enumerate(ms):
        if m > 0 and offs[i + 1] == offs[i]:
            raise ValueError("segment %d has no rows but %d samples are asked of it" % (i, m))
    total = sum(ms)
    odev = points.device
    if total == 0:                                       # nothing to launch
        idx, dist = torch.empty((0,), dtype=torch.int64, device=odev), torch.empty((0,), dtype=points.dtype, device=odev)
    else:
        dev = device_of(points)
        pts, stride = rows_on(points, dev)
        lib = _lib.load()
        code = FLOAT_CODES[pts.dtype]
        with torch.cuda.device(dev):
            soffs = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
            both = torch.from_numpy(np.concatenate([np.asarray(offs, np.int64), soffs])).to(dev)
            idx = torch.empty((total,), dtype=torch.int64, device=dev)
            dist = torch.empty((total,), dtype=pts.dtype, device=dev) if return_distances else None
            ws = _lib.workspace(lib.d3d_fps_workspace_bytes(n, b, code), dev)
            rc = lib.d3d_furthest_point_sample(_lib.ptr(pts), n, stride, code, _lib.ptr(both[:b + 1]), _lib.ptr(both[b + 1:]), b, _lib.ptr(idx),
                                               _lib.ptr(dist), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "furthest_point_sample")
        if return_distances:
            idx, dist = _lib.to_caller((idx, dist), odev, dev)
        else:
            idx = _lib.to_caller(idx, odev, dev)
    if was_numpy:
        idx, dist = idx.numpy(), (dist.numpy() if return_distances else None)
    return (idx, dist) if return_distances else idx


def ball_query(points, centers, radius, nsample, point_offsets=None, center_offsets=None, pad="none"):
    """The first `nsample` rows of `points` inside the ball of `radius` around every centre, in ascending row order.

    :param points: [N, D], D >= 3, and
    :param centers: [M, D'], D' >= 3, of the same dtype (float32 or float64); columns 0..2 are used.  torch tensors or numpy arrays
    :param radius: a finite positive float
    :param nsample: 1 .. 1024, the width of the table
    :param point_offsets, center_offsets: [B + 1] segment boundaries of the two arrays, both or neither; a centre sees the points of
        its own segment only.  On the host; a GPU tensor is read back once for the checks
    A PointGrid in the place of `points` takes the grid route: the same table and counts, bit for bit, from the cells around every
    centre alone -- made for N = M = 10^5.  Its segments are the point offsets (point_offsets with it is a ValueError, center_offsets
    is required iff the grid was built with offsets), the centres' dtype must be the grid's, and nsample stops at 64 there
    :param pad: 'none': the slots after the last entry are -1; 'first' (pointnet2's convention): they repeat the first entry -- an
        empty ball stays all -1 with count 0
    :return: (table [M, nsample] int32, counts [M] int32) on the side `points` came from (numpy in, numpy out).  Table values are
        GLOBAL point rows; with -1 for "none" it is the table neighbor_gather and the table pooling operators read

    The rule (exact): r2 = r * r with r rounded to the dtype; row i is inside iff q < r2 (strict; false for NaN, so rows and centres
    that are not finite match nothing), q as in furthest_point_sample.  O(M N) per segment: made for keypoint counts.
    """
    grid = points if isinstance(points, PointGrid) else None
    if grid is not None:
        points, was_numpy = grid.points, grid._was_numpy
    else:
        points, was_numpy = as_tensor(points, "points")
    centers, _ = as_tensor(centers, "centers")
    check_xyz_rows(points, "points")
    check_xyz_rows(centers, "centers")
    if points.dtype != centers.dtype:
        raise ValueError("points (%s) and centers (%s) must share a dtype" % (points.dtype, centers.dtype))
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not np.isfinite(radius) or not radius > 0:
        raise ValueError("radius must be a finite positive float, not %r" % (radius,))
    nsample = int(nsample)
    if not 1 <= nsample <= _NSAMPLE_MAX:
        raise ValueError("nsample must be in 1 .. %d, not %d" % (_NSAMPLE_MAX, nsample))
    if not isinstance(pad, str) or pad.lower() not in ("none", "first"):
        raise ValueError("pad must be 'none' or 'first', not %r" % (pad,))
    if grid is None and (point_offsets is None) != (center_offsets is None):
        raise ValueError("point_offsets and center_offsets go together: give both or neither")
    n, m = points.shape[0], centers.shape[0]
    if n > ROW_MAX or m > ROW_MAX:
        raise ValueError("ball_query takes at most 2^31 - 1 points and centres")
    segments = 0
    if grid is not None:
        coffs = grid.check_query(centers, nsample, ("nsample", "center_offsets"), point_offsets, center_offsets, " (nsample up to 1024)")
    elif point_offsets is not None:
        poffs, coffs = host_offsets(point_offsets, n, "point_offsets"), host_offsets(center_offsets, m, "center_offsets")
        if len(poffs) != len(coffs):
            raise ValueError("point_offsets names %d segments, center_offsets %d" % (len(poffs) - 1, len(coffs) - 1))
        segments = len(poffs) - 1
    odev = points.device if grid is None else grid._odev
    if m == 0:
        table, counts = (torch.empty((0, nsample), dtype=torch.int32, device=odev), torch.empty((0,), dtype=torch.int32, device=odev))
    elif grid is not None:
        table, counts = _lib.to_caller(grid.ball(centers, coffs, radius, nsample, pad.lower() == "first"), odev, grid.device)
    else:
        dev = device_of(points, centers)
        pts, pstride = rows_on(points, dev)
        ctr, cstride = rows_on(centers, dev)
        with torch.cuda.device(dev):
            both = torch.from_numpy(np.asarray(poffs + coffs, np.int64)).to(dev) if segments else None
            table = torch.empty((m, nsample), dtype=torch.int32, device=dev)
            counts = torch.empty((m,), dtype=torch.int32, device=dev)
            rc = _lib.load().d3d_ball_query(_lib.ptr(pts), n, pstride, _lib.ptr(ctr), m, cstride, FLOAT_CODES[pts.dtype],
                                            _lib.ptr(both[:segments + 1]) if segments else None,
                                            _lib.ptr(both[segments + 1:]) if segments else None, segments, float(radius), nsample,
                                            int(pad.lower() == "first"), _lib.ptr(table), _lib.ptr(counts), _lib.stream_ptr())
        _lib.check(rc, "ball_query")
        table, counts = _lib.to_caller((table, counts), odev, dev)
    if was_numpy:
        table, counts = table.numpy(), counts.numpy()
    return table, counts


__all__ = ["furthest_point_sample", "ball_query", "fps_plan"]
