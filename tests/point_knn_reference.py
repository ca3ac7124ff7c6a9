"""The numpy models of knn_query, the kNN weights and the weighted fold with its transpose (the rules of include/d3d_hip.h), in the
stated operation order and in the dtype of the data; and an independent brute force of the query in exact rational arithmetic for
scenes whose coordinates are integers or multiples of 1/64."""
from fractions import Fraction

import numpy as np


def _q(x, c):
    """((dx * dx) + (dy * dy)) + (dz * dz) of every row of x [n, 3] against c [3]; numpy keeps the dtype, one rounding per operation"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def _segments(offsets, total):
    offs = [0, total] if offsets is None else [int(v) for v in offsets]
    return list(zip(offs[:-1], offs[1:]))


def knn_model(points, centers, k, point_offsets=None, center_offsets=None):
    """-> (table int32 [M, k], dist2 [M, k] in points.dtype): per centre its candidates (q not NaN) by a stable lexsort on (q, i)"""
    points, centers = np.asarray(points), np.asarray(centers)
    dtype = points.dtype
    m = centers.shape[0]
    table, dist2 = np.full((m, k), -1, np.int32), np.full((m, k), np.inf, dtype)
    for (a, b), (ca, cb) in zip(_segments(point_offsets, points.shape[0]), _segments(center_offsets, m)):
        x = points[a:b, :3]
        for c in range(ca, cb):
            q = _q(x, centers[c, :3])
            rows = np.nonzero(~np.isnan(q))[0]
            order = rows[np.lexsort((rows, q[rows]))][:k]          # (the last key is the primary one)
            table[c, :len(order)] = order + a
            dist2[c, :len(order)] = q[order]
    return table, dist2


def knn_weights_model(table, dist2, power=1, eps=1e-8):
    """-> weights [M, k] in dist2.dtype: u = 1 / (sqrt(q) + eps) or 1 / (q + eps), s = 0 + u_0 + u_1 + ... over the present entries in
    ascending column, w = u / s; absent entries 0; the whole row 0 where s == 0 or s is not finite"""
    dtype = dist2.dtype.type
    eps, one = dtype(eps), dtype(1)
    out = np.zeros(dist2.shape, dist2.dtype)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for r in range(table.shape[0]):
            cols = [j for j in range(table.shape[1]) if table[r, j] >= 0]
            u = {j: one / ((np.sqrt(dist2[r, j]) if power == 1 else dist2[r, j]) + eps) for j in cols}
            s = dtype(0)
            for j in cols:
                s = s + u[j]
            if s > 0 and np.isfinite(s):
                for j in cols:
                    out[r, j] = u[j] / s
    return out


def wfold_model(feat, table, weights):
    """feat [V, C], weights [R, J] in the ACCUMULATION dtype (float32 for the half types: widen first, round the result once),
    table [R, J] -> [R, C]: row r = 0, then + (w * x) per present entry in ascending column, product and sum rounded separately"""
    acc = np.zeros((table.shape[0], feat.shape[1]), feat.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(table.shape[1]):
            present = table[:, j] >= 0
            prod = weights[present, j][:, None] * feat[table[present, j]]
            acc[present] = acc[present] + prod
    return acc


def wfold_transpose_model(grad, table, weights, v):
    """grad [R, C] and weights [R, J] in the accumulation dtype -> [v, C]: row u = 0, then + (w[e] * grad[e // J]) over the entries e
    of the flattened table that name u, in ascending e"""
    out = np.zeros((v, grad.shape[1]), grad.dtype)
    j = table.shape[1]
    flat, w = table.reshape(-1), weights.reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        for e in np.nonzero(flat >= 0)[0]:
            out[flat[e]] = out[flat[e]] + w[e] * grad[e // j]
    return out


# ---- exact rationals: no rounding anywhere.  Coordinates must be finite; returns q as Fractions ----
def knn_exact(points, centers, k, point_offsets=None, center_offsets=None):
    """-> (table as lists, dist2 as lists of Fraction, None where absent)"""
    pts = [[Fraction(v) for v in row[:3]] for row in np.asarray(points, np.float64).tolist()]
    ctr = [[Fraction(v) for v in row[:3]] for row in np.asarray(centers, np.float64).tolist()]
    table, dist2 = [None] * len(ctr), [None] * len(ctr)
    for (a, b), (ca, cb) in zip(_segments(point_offsets, len(pts)), _segments(center_offsets, len(ctr))):
        for c in range(ca, cb):
            cx, cy, cz = ctr[c]
            best = sorted(((pts[i][0] - cx) ** 2 + (pts[i][1] - cy) ** 2 + (pts[i][2] - cz) ** 2, i) for i in range(a, b))[:k]
            table[c] = [i for _, i in best] + [-1] * (k - len(best))
            dist2[c] = [q for q, _ in best] + [None] * (k - len(best))
    return table, dist2
