"""The numpy model of d3d_frustum_map_count / _emit and of the three lift-splat folds (csrc/vlift.hip; d3d_amd.voxel.lift), written from
the rules of include/d3d_hip.h and from nothing else.

The geometry is np.float32 operation by operation (one ufunc per operation, so nothing contracts).  The folds keep features in
np.float64 for "f64" and in np.float32 otherwise -- the half types multiply and add in np.float32 (their values are fp32 values) and
are rounded once by sparse_pool_reference.to_tensor.  Features and gradients come and go as numpy arrays in the FOLD type."""
from fractions import Fraction

import numpy as np

import sparse_pool_reference as pref

KINDS = pref.KINDS
CODES = pref.CODES
fold_type, of_kind, to_tensor, equal_bits = pref.fold_type, pref.of_kind, pref.to_tensor, pref.equal_bits
F = np.float32


def grid(bounds, shape):
    """(xmin, xmax, ymin, ymax, zmin, zmax), (n0, n1, n2) -> lo [3], size [3] float32: the minima and (max - min) / shape from fp64,
    each rounded once"""
    b = np.asarray(bounds, np.float64)
    return b[0::2].astype(F), ((b[1::2] - b[0::2]) / np.asarray(shape, np.float64)).astype(F)


def positions(us, vs, ds, pre, post):
    """-> x [3][S, D, H, W] float32, every operation one rounding:
    a = (us[w], vs[h], ds[d]); q_i = ((pre[i,0] a0 + pre[i,1] a1) + pre[i,2] a2) + pre[i,3]; e = (q0 q2, q1 q2, q2); x_i likewise by post"""
    us, vs, ds, pre, post = (np.asarray(a, F) for a in (us, vs, ds, pre, post))
    a = (us[None, None, None, :], vs[None, None, :, None], ds[None, :, None, None])

    def affine(m, p):
        col = [[m[:, i, j][:, None, None, None] for j in range(4)] for i in range(3)]
        return [((col[i][0] * p[0] + col[i][1] * p[1]) + col[i][2] * p[2]) + col[i][3] for i in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        q = affine(pre, a)
        e = (q[0] * q[2], q[1] * q[2], q[2])
        x = affine(post, e)
    full = (len(pre), len(ds), len(vs), len(us))
    x = [np.broadcast_to(xi, full) for xi in x]
    assert all(xi.dtype == F for xi in x)
    return x


def cells(us, vs, ds, pre, post, lo, size, shape, cams_per_sample):
    """-> (t [K, 3] float32, member [K] bool, cell [K, 4] int64 = (b, c0, c1, c2), zero where not a member), K = S D H W,
    p = ((s D + d) H + h) W + w.  t_i = (x_i - lo_i) / size_i; member iff t_i >= 0 and t_i < shape_i on all axes (NaN fails);
    c_i = trunc(t_i); b = s // cams_per_sample"""
    lo, size = np.asarray(lo, F), np.asarray(size, F)
    x = positions(us, vs, ds, pre, post)
    s = len(np.asarray(pre))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = np.stack([((x[i] - lo[i]) / size[i]).reshape(-1) for i in range(3)], 1)
    assert t.dtype == F
    with np.errstate(invalid="ignore"):
        member = np.all((t >= 0) & (t.astype(np.float64) < np.asarray(shape, np.float64)), 1)
    c = np.where(member[:, None], np.where(member[:, None], t, 0).astype(np.int64), 0)
    per_cam = len(t) // s if s else 0
    b = np.where(member, (np.arange(len(t)) // max(per_cam, 1)) // cams_per_sample, 0)
    return t, member, np.concatenate([b[:, None], c], 1)


def number(member, cell, shape):
    """-> (mapping [K] int64, coords [V, 3] int64, batch_index [V] int64): the present cells numbered by ascending key
    ((b n0 + c0) n1 + c1) n2 + c2"""
    key = ((cell[:, 0] * shape[0] + cell[:, 1]) * shape[1] + cell[:, 2]) * shape[2] + cell[:, 3]
    present = np.unique(key[member])
    mapping = np.where(member, np.searchsorted(present, key), -1).astype(np.int64)
    k = present.copy()
    c2, k = k % shape[2], k // shape[2]
    c1, k = k % shape[1], k // shape[1]
    c0, b = k % shape[0], k // shape[0]
    return mapping, np.stack([c0, c1, c2], 1).astype(np.int64).reshape(-1, 3), b.astype(np.int64)


def frustum_map(us, vs, ds, pre, post, lo, size, shape, cams_per_sample):
    _, member, cell = cells(us, vs, ds, pre, post, lo, size, shape, cams_per_sample)
    return number(member, cell, shape)


def cells_exact(us, vs, ds, pre, post, lo, size, shape, cams_per_sample):
    """the same in Python Fractions, point by point, for finite inputs: -> (member [K] bool, cell [K, 4] int64)"""
    fr = lambda a: [Fraction(float(v)) for v in np.asarray(a).reshape(-1)]      # noqa: E731
    us, vs, ds, lo, size = fr(us), fr(vs), fr(ds), fr(lo), fr(size)
    member, cell = [], []
    for s in range(len(pre)):
        m, n = fr(pre[s]), fr(post[s])
        for d in ds:
            for v in vs:
                for u in us:
                    a = (u, v, d, 1)
                    q = [sum(m[4 * i + j] * a[j] for j in range(4)) for i in range(3)]
                    e = (q[0] * q[2], q[1] * q[2], q[2], 1)
                    x = [sum(n[4 * i + j] * e[j] for j in range(4)) for i in range(3)]
                    t = [(x[i] - lo[i]) / size[i] for i in range(3)]
                    ok = all(0 <= t[i] < shape[i] for i in range(3))
                    member.append(ok)
                    cell.append([s // cams_per_sample] + [int(ti) for ti in t] if ok else [0, 0, 0, 0])      # (t >= 0: int() is floor)
    return np.array(member, bool).reshape(-1), np.array(cell, np.int64).reshape(-1, 4)


def pixel_of(p, frustum):
    d, h, w = frustum
    return (p // (d * h * w)) * (h * w) + p % (h * w)


def forward(depth, feat, mapping, num_voxels, frustum, kind):
    """depth [K], feat [S H W, C] in the fold type -> out [V, C] in the fold type, before the final rounding: row r is 0, then
    + (depth[p] * feat[pix(p)]) over the points p with mapping[p] == r in ascending p, a rounding after the product and one after the
    sum.  One pass per rank of a point inside its cell"""
    d = fold_type(kind)
    depth, feat = np.asarray(depth).reshape(-1), np.asarray(feat)
    assert depth.dtype == d and feat.dtype == d and feat.ndim == 2
    acc = np.zeros((num_voxels, feat.shape[1]), d)
    p = np.nonzero(mapping >= 0)[0]
    p = p[np.argsort(mapping[p], kind="stable")]
    row = mapping[p]
    rank = np.arange(len(p)) - np.searchsorted(row, row, side="left")
    with np.errstate(invalid="ignore", over="ignore"):
        for rk in range(int(rank.max()) + 1 if len(p) else 0):
            sel = p[rank == rk]
            prod = depth[sel, None] * feat[pixel_of(sel, frustum)]
            acc[mapping[sel]] = acc[mapping[sel]] + prod
    assert acc.dtype == d
    return acc


def backward_feat(grad, depth, mapping, cameras, frustum, kind):
    """grad [V, C], depth [K] in the fold type -> grad_feat [S H W, C]: pixel row is 0, then + (depth[p] * grad[mapping[p]]) over
    d ascending for its points with a row"""
    t = fold_type(kind)
    grad, depth = np.asarray(grad), np.asarray(depth).reshape(-1)
    assert grad.dtype == t and depth.dtype == t
    dn, h, w = frustum
    acc = np.zeros((cameras * h * w, grad.shape[1]), t)
    pix = np.arange(cameras * h * w)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(dn):
            p = (pix // (h * w)) * (dn * h * w) + d * (h * w) + pix % (h * w)
            m = mapping[p]
            if len(grad):
                prod = depth[p, None] * grad[np.maximum(m, 0)]
                acc = np.where((m >= 0)[:, None], acc + prod, acc)
    assert acc.dtype == t
    return acc


EXACT = np.longdouble                 # 64 bits of significand on x86: a unit roundoff 2^-11 of fp64's, so "exact" beside every kind here
assert np.finfo(EXACT).eps <= 2.0 ** -63


def backward_depth_exact(grad, feat, mapping, frustum):
    """-> (exact [K], scale [K]) as float64 / long double: sum_c g f and sum_c |g f| for the points with a row, 0 elsewhere.  Inputs of
    any fold type; products and sums in long double (the inputs are fp32, half or fp64 values: against fp64's unit roundoff the
    error of this sum is 2^-11 of the bound it is used in)"""
    g, f = np.asarray(grad).astype(EXACT), np.asarray(feat).astype(EXACT)
    p = np.arange(len(mapping))
    has = mapping >= 0
    if not len(g):
        return np.zeros(len(mapping), EXACT), np.zeros(len(mapping), EXACT)
    prod = g[np.maximum(mapping, 0)] * f[pixel_of(p, frustum)]
    return np.where(has, prod.sum(1), 0), np.where(has, np.abs(prod).sum(1), 0)


def forward_brute(depth, feat, cell, member, frustum):
    """the forward from the cells alone, with a dictionary and Python scalars of the arrays' dtype: -> {(b, c0, c1, c2): row [C]}"""
    out = {}
    for p in range(len(member)):
        if not member[p]:
            continue
        key = tuple(int(a) for a in cell[p])
        acc = out.get(key)
        if acc is None:
            acc = out[key] = [feat.dtype.type(0)] * feat.shape[1]
        w = depth[p]
        row = feat[pixel_of(p, frustum)]
        for ch in range(feat.shape[1]):
            acc[ch] = acc[ch] + w * row[ch]
    return out
