"""The numpy model of d3d_roi_grid_table and d3d_table_pool_backward_index (csrc/roipool.hip, csrc/vtpool.hip; d3d_amd.point.roi),
written from the rules of include/d3d_hip.h: membership is the oracle's crop_points on the finite rows, the cell the stated fp32
expressions with the sine and cosine of the library's host routine, a cell's entries its first P members in ascending row; the
backward is a literal loop over the present entries in ascending entry number, in the fold type of the dtype.  The forward fold is
the table pool's own model, sparse_pool_reference.forward."""
import ctypes

import numpy as np

import oracle
import sparse_pool_reference as pref
from d3d_amd import _lib

F = np.float32
MAX_ANGLE = 119.0               # the range d3d_internal_host_sincosf covers with its restated path: keep every test angle inside


def host_sincos(angles):
    """(sin, cos) float32 of float32 angles by the library's host build of the routine the kernels run"""
    a = np.ascontiguousarray(angles, F)
    fn = _lib.load().d3d_internal_host_sincosf
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int64
    s, c = np.empty_like(a), np.empty_like(a)
    fn(a.ctypes.data, a.size, s.ctypes.data, c.ctypes.data)
    return s, c


def segments(offsets, total):
    offs = [0, total] if offsets is None else [int(v) for v in offsets]
    return list(zip(offs[:-1], offs[1:]))


def triple(out_size):
    return (int(out_size),) * 3 if np.isscalar(out_size) else tuple(int(v) for v in out_size)


def members(points, boxes):
    """bool[M, N]: crop_points on the rows whose x, y, z are all finite (a NaN z, inside for crop_points, is no member)"""
    xyz = np.ascontiguousarray(np.asarray(points, F)[:, :3])
    boxes = np.ascontiguousarray(boxes, F)
    if len(boxes) == 0 or len(xyz) == 0:
        return np.zeros((len(boxes), len(xyz)), bool)
    return oracle.crop_points(boxes, xyz) & np.isfinite(xyz).all(1)[None, :]


def _axis(t, o):
    """0 where !(t >= 0), NaN included; else min(trunc(t), o - 1), saturated before the conversion"""
    with np.errstate(invalid="ignore"):
        ok = t >= 0
        return np.where(ok, np.minimum(np.trunc(np.where(ok, t, F(0))), F(o - 1)), F(0)).astype(np.int64)


def cells(xyz, box, out_size):
    """the cell of every row of xyz [K, 3] float32 in one box row (7 float32): every operation one fp32 rounding"""
    ox, oy, oz = triple(out_size)
    xyz, b = np.asarray(xyz, F), np.asarray(box, F)
    s, c = host_sincos(b[6:7])
    s, c = s[0], c[0]
    with np.errstate(all="ignore"):
        dx, dy, dz = xyz[:, 0] - b[0], xyz[:, 1] - b[1], xyz[:, 2] - b[2]
        u = dx * c + dy * s
        v = dy * c - dx * s
        tx = (u / b[3] + F(0.5)) * F(ox)
        ty = (v / b[4] + F(0.5)) * F(oy)
        tz = (dz / b[5] + F(0.5)) * F(oz)
    assert tx.dtype == ty.dtype == tz.dtype == F
    return (_axis(tx, ox) * oy + _axis(ty, oy)) * oz + _axis(tz, oz)


def grid_model(points, boxes, out_size=12, max_points=128, point_offsets=None, box_offsets=None, pad="none"):
    """-> (table [M, G, P] int32, counts [M, G] int32, inside [M] int32)"""
    points, boxes = np.asarray(points, F), np.asarray(boxes, F)
    ox, oy, oz = triple(out_size)
    g, p, m = ox * oy * oz, int(max_points), len(boxes)
    table, counts, inside = np.full((m, g, p), -1, np.int32), np.zeros((m, g), np.int32), np.zeros(m, np.int32)
    for (a, b), (ba, bb) in zip(segments(point_offsets, len(points)), segments(box_offsets, m)):
        mask = members(points[a:b], boxes[ba:bb])
        for i in range(ba, bb):
            rows = np.flatnonzero(mask[i - ba])                     # ascending
            inside[i] = len(rows)
            if not len(rows):
                continue
            cell = cells(points[a:b][rows, :3], boxes[i], (ox, oy, oz))
            order = np.argsort(cell, kind="stable")
            cs, rs = cell[order], rows[order] + a
            start = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
            rank = np.arange(len(cs)) - np.repeat(start, np.diff(np.r_[start, len(cs)]))
            keep = rank < p
            table[i, cs[keep], rank[keep]] = rs[keep]
            counts[i] = np.minimum(np.bincount(cell, minlength=g), p)
            if pad == "cycle":
                for cc in np.flatnonzero((counts[i] > 0) & (counts[i] < p)):
                    k = counts[i, cc]
                    table[i, cc, k:] = table[i, cc, np.arange(k, p) % k]
    return table, counts, inside


def pool_forward(feat, table, reduction, kind):
    """feat [N, C] in the fold type, table [R, K] -> (out [R, C] before the final rounding, arg [R, C] int16, count [R] int32): the
    table pool's rules"""
    return pref.forward(feat, np.asarray(table).reshape(-1, table.shape[-1]), reduction, kind)


def pool_backward(grad, table, num_src, reduction, kind, arg=None, count=None):
    """grad [R, C] in the fold type, the forward's table [R, K] -> grad_feat [num_src, C] in the fold type, before the final rounding.
    A literal loop: every present entry e = r * K + kk in ascending e adds to row table[e] what it owes it -- grad[r] (sum),
    grad[r] / (T)count[r] (mean), grad[r, ch] where arg[r, ch] == kk (max / min) -- one rounding per addition"""
    d = pref.fold_type(kind)
    grad = np.asarray(grad)
    assert grad.dtype == d
    table = np.asarray(table).reshape(-1, table.shape[-1])
    k = table.shape[1]
    flat = table.reshape(-1)
    acc = np.zeros((num_src, grad.shape[1]), d)
    with np.errstate(all="ignore"):
        for e in np.flatnonzero(flat >= 0):
            r, kk, v = e // k, e % k, flat[e]
            if reduction == pref.SUM:
                acc[v] = acc[v] + grad[r]
            elif reduction == pref.MEAN:
                acc[v] = acc[v] + grad[r] / d(count[r])
            else:
                acc[v] = np.where(arg[r] == kk, acc[v] + grad[r], acc[v])
    assert acc.dtype == d
    return acc


def roipoint_model(points, feat, boxes, num_samples, point_offsets=None, box_offsets=None):
    """-> (pooled [M, S, 3 + C] in feat's dtype -- bit copies of xyz and of the feature rows, zeros for an empty box --, empty [M] bool,
    the table [M, S])"""
    table, _, inside = grid_model(points, boxes, 1, num_samples, point_offsets, box_offsets, "cycle")
    table = table[:, 0, :]
    rows = np.maximum(table, 0)
    xyz, feat = np.asarray(points, F)[:, :3], np.asarray(feat)
    if len(xyz) == 0:
        xyz, feat = np.zeros((1, 3), F), np.zeros((1, feat.shape[1]), feat.dtype)
    out = np.concatenate([xyz[rows].astype(feat.dtype), feat[rows]], 2)
    out[table < 0] = 0
    return out, inside == 0, table
