"""The numpy models of furthest_point_sample and ball_query (the rules of include/d3d_hip.h), in the stated operation order and in
the dtype of the points; and an independent implementation of both in Python integers for scenes with integer coordinates."""
import numpy as np


def _q(x, c):
    """((dx * dx) + (dy * dy)) + (dz * dz) of every row of x [n, 3] against c [3]; numpy keeps the dtype, one rounding per operation"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def _segments(offsets, total):
    offs = [0, total] if offsets is None else [int(v) for v in offsets]
    return list(zip(offs[:-1], offs[1:]))


def _per_segment(num_samples, b):
    return [int(num_samples)] * b if np.isscalar(num_samples) else [int(m) for m in num_samples]


def fps_model(points, num_samples, offsets=None, trace=None):
    """-> (indices int64 [sum M], distances [sum M] in points.dtype).  trace (a list): gets, per step, (segment start, d before the
    pick with excluded rows at -1) for the property tests."""
    points = np.asarray(points)
    dtype = points.dtype
    segs = _segments(offsets, points.shape[0])
    idx, dist = [], []
    for (a, b), m in zip(segs, _per_segment(num_samples, len(segs))):
        x = points[a:b, :3]
        ok = np.isfinite(x).all(axis=1) if b > a else np.zeros(0, bool)
        d = np.where(ok, dtype.type(np.inf), dtype.type(-1)).astype(dtype)
        for _ in range(m):
            if trace is not None:
                trace.append((a, d.copy()))
            if not ok.any():
                idx.append(a)
                dist.append(dtype.type(np.nan))
                continue
            c = int(np.argmax(d))                        # the first maximum: the lowest row
            idx.append(a + c)
            dist.append(d[c])
            q = _q(x, x[c])
            lower = ok & (q < d)
            d[lower] = q[lower]
    return np.asarray(idx, np.int64), np.asarray(dist, dtype)


def ball_model(points, centers, radius, nsample, point_offsets=None, center_offsets=None, pad="none"):
    """-> (table int32 [M, nsample], counts int32 [M])"""
    points, centers = np.asarray(points), np.asarray(centers)
    dtype = points.dtype
    r = dtype.type(radius)
    r2 = r * r
    m = centers.shape[0]
    table, counts = np.full((m, nsample), -1, np.int32), np.zeros(m, np.int32)
    psegs, csegs = _segments(point_offsets, points.shape[0]), _segments(center_offsets, m)
    for (a, b), (ca, cb) in zip(psegs, csegs):
        x = points[a:b, :3]
        for c in range(ca, cb):
            with np.errstate(invalid="ignore"):
                inside = np.nonzero(_q(x, centers[c, :3]) < r2)[0][:nsample] + a
            counts[c] = len(inside)
            table[c, :len(inside)] = inside
            if pad == "first" and len(inside):
                table[c, len(inside):] = inside[0]
    return table, counts


# ---- Python integers: no rounding anywhere.  Coordinates must be integers; distances are ints, None stands for +inf ----
def fps_exact(points, num_samples, offsets=None):
    """-> (indices list, distances list of int or None).  Rows are all finite here."""
    pts = [[int(v) for v in row[:3]] for row in np.asarray(points).tolist()]
    segs = _segments(offsets, len(pts))
    idx, dist = [], []
    for (a, b), m in zip(segs, _per_segment(num_samples, len(segs))):
        d = [None] * (b - a)
        for _ in range(m):
            best = 0
            for i in range(1, b - a):                    # the largest d, the lowest row on a tie (None = +inf is the largest)
                if d[best] is not None and (d[i] is None or d[i] > d[best]):
                    best = i
            idx.append(a + best)
            dist.append(d[best])
            cx, cy, cz = pts[a + best]
            for i in range(b - a):
                x, y, z = pts[a + i]
                q = (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2
                if d[i] is None or q < d[i]:
                    d[i] = q
    return idx, dist


def ball_exact(points, centers, radius, nsample, point_offsets=None, center_offsets=None, pad="none"):
    """-> (table as lists, counts list); radius an integer"""
    pts = [[int(v) for v in row[:3]] for row in np.asarray(points).tolist()]
    ctr = [[int(v) for v in row[:3]] for row in np.asarray(centers).tolist()]
    r2 = int(radius) ** 2
    table, counts = [], []
    ordered = []
    for (a, b), (ca, cb) in zip(_segments(point_offsets, len(pts)), _segments(center_offsets, len(ctr))):
        for c in range(ca, cb):
            cx, cy, cz = ctr[c]
            inside = [i for i in range(a, b) if (pts[i][0] - cx) ** 2 + (pts[i][1] - cy) ** 2 + (pts[i][2] - cz) ** 2 < r2][:nsample]
            fill = inside[0] if (pad == "first" and inside) else -1
            ordered.append((c, inside + [fill] * (nsample - len(inside)), len(inside)))
    for _, row, count in sorted(ordered):
        table.append(row)
        counts.append(count)
    return table, counts
