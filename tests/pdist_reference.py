"""A plain fp64 model of the signed point-to-box distance (d3d_pdist2dr_forward / _backward, box2dr_pdist / box3dr_pdist) for
tests: no GPU, no compiled code.  numpy for values and features, torch (CPU) for the gradients.

Conventions (include/d3d_hip.h, oracle.pdist2dr): points[n,2], boxes[m,5] = (x, y, w, h, r); dist[m,n] positive inside;
feature k = edge k (corner k -> k + 1), 4 + k = corner k; corners in the box frame (-a,-b), (a,-b), (a,b), (-a,b) with
a = w / 2, b = h / 2, so edge 0 = bottom, 1 = right, 2 = top, 3 = left.

`signed_distance` and the torch form behind `grad_reference` are the closed form in the box frame and hold for w, h > 0.
`features` walks the four edges (any w, h) and says where the answer is beyond doubt: near a tie between two features no
finite-precision routine can be held to one of them, so those pairs only have to name a feature that is as near as the best."""
import numpy as np
import torch

MARGIN = 1e-3


# ---------------------------------------------------------------- inputs
def scene(n, m, seed, offset=0.0, dtype=np.float64):
    """(points[n,2], boxes[m,5]) rounded to `dtype`: the boxes of test_gpu_boxloss._rand_boxes (centres +-4, sizes 0.1 .. 5.1,
    angles +-5 rad), points uniform in +-6 with a third of them planted in randomly chosen boxes (reaching 10 % beyond their
    sides, as test_crop_points._scene does: random points alone are inside for 5 % of the pairs); everything moved by
    (offset, offset)"""
    from test_gpu_boxloss import _rand_boxes
    boxes = _rand_boxes(m, seed, 8.0)
    rng = np.random.default_rng(seed + 7919)
    pts = (rng.random((n, 2)) - 0.5) * 12
    k = n // 3
    which = rng.integers(0, m, k)
    c, s = np.cos(boxes[which, 4]), np.sin(boxes[which, 4])
    u, v = (rng.random(k) - 0.5) * boxes[which, 2] * 1.1, (rng.random(k) - 0.5) * boxes[which, 3] * 1.1
    pts[:k, 0] = boxes[which, 0] + c * u - s * v
    pts[:k, 1] = boxes[which, 1] + s * u + c * v
    pts = pts[rng.permutation(n)]                                # planted points in every column block
    boxes[:, :2] += offset
    pts += offset
    return np.ascontiguousarray(pts.astype(dtype)), np.ascontiguousarray(boxes.astype(dtype))


FORWARD_SHAPES = [(1, 1), (3, 1), (4, 65), (255, 64), (257, 63), (1023, 2), (1024, 1), (1025, 129), (1031, 131)]       # (n, m)
BACKWARD_SHAPES = [(1, 1), (257, 65), (700, 90), (1031, 131)]
OFFSETS = (0.0, 50.0)
WEIGHT_KINDS = ("dense", "sparse", "zero_row_col", "zero")


def seed_of(n, m):
    # With 100 * n + m the case (1024, 1) has 1.27 % of its pairs undecided (the next: (1023, 2) 0.78 %, all others under
    # 0.4 %; the backward exclusions 0.17 % at most): a third of ALL points is planted in its one box, and that draw is a
    # slender one.  + 6 draws boxes at which every case is under the 1 % cap, so the cap holds by this choice of inputs.
    return 100 * n + m + 6


def weights(kind, n, m, seed):
    """g[m,n] (fp64): dense and signed; 1 % of that; that with box row m // 2 and point column n // 3 zero; all zero"""
    rng = np.random.default_rng(seed + 31)
    w = rng.random((m, n)) - 0.3
    if kind == "sparse":
        w = w * (rng.random((m, n)) < 0.01)
    elif kind == "zero_row_col":
        w[m // 2, :] = 0
        w[:, n // 3] = 0
    elif kind == "zero":
        w = np.zeros((m, n))
    else:
        assert kind == "dense"
    return w


def backward_case(n, m, offset, kind, dtype):
    """(points, boxes, g, excluded share) in `dtype`: the scene of the shape with the weights of the kind, zero at the kinks
    (found in fp64 on the rounded inputs)"""
    pts, boxes = scene(n, m, seed_of(n, m), offset, dtype)
    kink = kink_mask(pts, boxes)
    g = np.where(kink, 0.0, weights(kind, n, m, seed_of(n, m))).astype(dtype)
    return pts, boxes, np.ascontiguousarray(g), float(kink.mean())


def scale(points, boxes):
    """|px| + |py| + |cx| + |cy| + |w| + |h| per pair [m,n]: what a rounding error of the distance is proportional to"""
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    return (np.abs(p).sum(1))[None, :] + (np.abs(b[:, :4]).sum(1))[:, None]


# ---------------------------------------------------------------- values
def _local(points, boxes):
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    c, s = np.cos(b[:, 4])[:, None], np.sin(b[:, 4])[:, None]
    rx, ry = p[None, :, 0] - b[:, 0, None], p[None, :, 1] - b[:, 1, None]
    return rx * c + ry * s, ry * c - rx * s, b[:, 2, None] / 2, b[:, 3, None] / 2


def signed_distance(points, boxes):
    """dist[m,n] for boxes with w, h > 0: inside the smallest of the four gaps, outside -hypot(max(dx, 0), max(dy, 0))"""
    assert np.all(np.asarray(boxes)[:, 2:4] > 0)
    lx, ly, a, b = _local(points, boxes)
    dx, dy = np.abs(lx) - a, np.abs(ly) - b
    inside = (dx < 0) & (dy < 0)
    gaps = np.minimum(np.minimum(ly + b, a - lx), np.minimum(b - ly, lx + a))
    return np.where(inside, gaps, -np.hypot(np.maximum(dx, 0), np.maximum(dy, 0)))


# ---------------------------------------------------------------- features
def _edge_candidates(points, boxes):
    """the four edges' nearest points, any w and h: (t[4,m,n] unclamped, d[4,m,n] distance to the segment, f[4,m,n] feature)"""
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    ux, uy, vx, vy = b[:, 2] * c / 2, b[:, 2] * s / 2, -b[:, 3] * s / 2, b[:, 3] * c / 2
    qx = np.stack([b[:, 0] - ux - vx, b[:, 0] + ux - vx, b[:, 0] + ux + vx, b[:, 0] - ux + vx])          # [4,m]
    qy = np.stack([b[:, 1] - uy - vy, b[:, 1] + uy - vy, b[:, 1] + uy + vy, b[:, 1] - uy + vy])
    m, n = len(b), len(p)
    t, d, f = np.empty((4, m, n)), np.empty((4, m, n)), np.empty((4, m, n), np.int64)
    for e in range(4):
        ex, ey = (qx[(e + 1) & 3] - qx[e])[:, None], (qy[(e + 1) & 3] - qy[e])[:, None]
        rx, ry = p[None, :, 0] - qx[e][:, None], p[None, :, 1] - qy[e][:, None]
        len2 = ex * ex + ey * ey
        with np.errstate(divide="ignore", invalid="ignore"):
            t[e] = np.where(len2 > 0, (rx * ex + ry * ey) / np.where(len2 > 0, len2, 1.0), 0.0)
        tc = np.clip(t[e], 0.0, 1.0)
        d[e] = np.hypot(rx - tc * ex, ry - tc * ey)
        f[e] = np.where(t[e] <= 0, 4 + e, np.where(t[e] >= 1, 4 + ((e + 1) & 3), e))
    return t, d, f


def features(points, boxes, margin=MARGIN, loop=False):
    """(feat[m,n], decided[m,n], accept[m,n]).  feat = the nearest feature (the first minimum over the edges, as the
    reference's loop keeps it).  decided: every candidate of ANOTHER feature is farther than the best by more than
    tol = margin * (|w| + |h|), no edge's projection parameter t is within `margin` of 0 or 1, and the point is farther than
    tol from the boundary.  A feature is a candidate where the point's nearest point ON it is the feature itself: an edge
    while the foot of the perpendicular lies within it (0 < t < 1), a corner while the point lies beyond the ends of both
    edges that meet there.  Inside a box those are the four edges (the medial axis is where two of them tie); outside it
    is one feature, the regions being told apart by t alone -- a point far out beside an edge, 4 % of its length from the
    corner, is hardly nearer to the edge than to the corner, yet nothing is in doubt about it.
    loop=True counts all four edges' nearest points as candidates wherever they lie, as the reference's loop compares them:
    the yardstick for what walks the edges the same way (boxes without positive size), where a corner and the edge beside
    it can tie in fp32 although t is clear of the margin.
    accept = bit mask of the features whose nearest point is within tol of the best (an edge whose t is within `margin` of
    an end stands for that end's corner too, and the reverse): what an undecided pair may answer."""
    t, d, f = _edge_candidates(points, boxes)
    b = np.asarray(boxes, np.float64)
    tol = (margin * (np.abs(b[:, 2]) + np.abs(b[:, 3])))[:, None]
    best = d.min(0)
    first = d.argmin(0)
    feat = np.take_along_axis(f, first[None], 0)[0]
    valid = np.empty(f.shape, bool)
    for e in range(4):
        valid[e] = loop | np.where(t[e] <= 0, t[(e - 1) & 3] >= 1, np.where(t[e] >= 1, t[(e + 1) & 3] <= 0, True))
    other = np.where(valid & (f != feat[None]), d, np.inf).min(0)
    near_end = ((np.abs(t) <= margin) | (np.abs(t - 1) <= margin)).any(0)
    decided = (other > best + tol) & ~near_end & (best > tol)
    accept = np.zeros(feat.shape, np.int64)
    for e in range(4):
        ok = d[e] <= best + tol
        accept |= np.where(ok, 1 << f[e], 0)
        accept |= np.where(ok & (np.abs(t[e]) <= margin), (1 << e) | (1 << (4 + e)), 0)
        accept |= np.where(ok & (np.abs(t[e] - 1) <= margin), (1 << e) | (1 << (4 + ((e + 1) & 3))), 0)
    return feat, decided, accept


def feature_ok(got, feat, decided, accept):
    """bool[m,n]: the feature `got` is the expected one where that is decided, an accepted one elsewhere"""
    got = np.asarray(got).astype(np.int64)
    return np.where(decided, got == feat, (got < 8) & (((accept >> np.minimum(got, 7)) & 1) == 1))


def kink_mask(points, boxes, margin=MARGIN):
    """bool[m,n]: pairs at which the distance's gradient jumps, w, h > 0 -- inside within tol of the medial axis (two gaps
    within tol of each other) or, inside or outside, within tol of the boundary (the reference decides the sign and the
    feature there by rounding).  Outside the box the distance is C1, so every other outside pair has one gradient."""
    lx, ly, a, b = _local(points, boxes)
    tol = 2 * margin * (a + b)
    gaps = np.sort(np.stack([ly + b, a - lx, b - ly, lx + a]), 0)
    inside = gaps[0] > 0
    return (np.abs(signed_distance(points, boxes)) <= tol) | (inside & (gaps[1] - gaps[0] <= tol))


# ---------------------------------------------------------------- gradients
def dist_torch(P, B):
    """the closed form on torch tensors, pair by pair: P[..., 2], B[..., 5] of one shape up to the last axis"""
    rx, ry = P[..., 0] - B[..., 0], P[..., 1] - B[..., 1]
    c, s = torch.cos(B[..., 4]), torch.sin(B[..., 4])
    lx, ly = rx * c + ry * s, ry * c - rx * s
    dx, dy = lx.abs() - B[..., 2] / 2, ly.abs() - B[..., 3] / 2
    inside = (dx < 0) & (dy < 0)
    ox, oy = dx.clamp_min(0), dy.clamp_min(0)
    sq = ox * ox + oy * oy
    flat = inside | (sq == 0)                                    # (the square root's slope at 0 must not meet a zero weight)
    outside = -torch.sqrt(torch.where(flat, torch.ones_like(sq), sq))
    return torch.where(inside, torch.minimum(-dx, -dy), torch.where(flat, torch.zeros_like(sq), outside))


def _pairwise_leaves(points, boxes, dtype):
    p, b = torch.as_tensor(np.asarray(points), dtype=dtype), torch.as_tensor(np.asarray(boxes), dtype=dtype)
    m, n = b.shape[0], p.shape[0]
    P = p[None].expand(m, n, p.shape[1]).clone().requires_grad_(True)
    B = b[:, None].expand(m, n, b.shape[1]).clone().requires_grad_(True)
    return P, B


def _sums(P, B, centre, dims):
    """S_p[n,1] and S_b[m,5] from the per-pair terms: the sum of |g_ij| times the size of what the pair's derivative is
    made of.  For a point, the centre and the two sizes that is the LENGTH of d dist_ij / d p_j (a unit vector: a rounding
    error turns it, which moves its small component by as much as its large one, and leaves a residue of that size where a
    component is 0 by construction, as d / dh beside the right edge); for the angle it is that length times the lever the
    kernel's terms have, |p - c| + half the diagonal."""
    gl = P.grad.double().norm(dim=-1)                                               # |g_ij| * 1
    with torch.no_grad():
        lever = (P[..., centre] - B[..., centre]).double().norm(dim=-1) + B[..., dims].double().norm(dim=-1) / 2
    sp = gl.sum(0)[:, None]
    sb = torch.stack([gl.sum(1)] * (B.shape[-1] - 1) + [(gl * lever).sum(1)], 1)
    return sp.numpy(), sb.numpy()


def grad_reference(points, boxes, weight, dtype=torch.float64):
    """(grad_points[n,2], grad_boxes[m,5], S_p[n,1], S_b[m,5]) of sum(weight * dist) by autograd on the CPU; every pair gets
    leaves of its own, so the per-pair terms g_ij * d dist_ij / d(.) are at hand for the sums S (_sums)"""
    P, B = _pairwise_leaves(points, boxes, dtype)
    dist_torch(P, B).backward(torch.as_tensor(np.asarray(weight), dtype=dtype))
    return (P.grad.sum(0).double().numpy(), B.grad.sum(1).double().numpy()) + _sums(P, B, [0, 1], [2, 3])


# ---------------------------------------------------------------- 3-D (box3dr_pdist)
_AXES = {0: ([1, 2], [1, 2, 4, 5, 6]), 1: ([0, 2], [0, 2, 3, 5, 6]), 2: ([0, 1], [0, 1, 3, 4, 6])}


def scene3(n, m, axis, seed):
    """(points[n,3], boxes[m,7]) in fp64 for box3dr_pdist along `axis`: boxes with centres +-4, sizes 0.1 .. 5.1, angles +-5;
    points uniform in +-6, but a quarter inside a box, an eighth above or below one within its footprint and an eighth
    beside one within its extent along the axis"""
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([(rng.random((m, 3)) - 0.5) * 8, rng.random((m, 3)) * 5 + 0.1, (rng.random((m, 1)) - 0.5) * 10], 1)
    pts = (rng.random((n, 3)) - 0.5) * 12
    pc, bc = _AXES[axis]
    k = n // 2 + 2
    which = rng.integers(0, m, k)
    bx = boxes[which]
    kind = np.arange(k) % 4                                      # 0, 1: inside; 2: above / below; 3: beside
    u = (rng.random(k) - 0.5) * 0.9
    v = (rng.random(k) - 0.5) * 0.9
    z = (rng.random(k) - 0.5) * 0.9
    far = np.where(rng.random(k) < 0.5, -1.0, 1.0) * (0.55 + rng.random(k))
    z = np.where(kind == 2, far, z)
    u = np.where(kind == 3, far, u)
    u, v, z = u * bx[:, bc[2]], v * bx[:, bc[3]], z * bx[:, 3 + axis]
    c, s = np.cos(bx[:, 6]), np.sin(bx[:, 6])
    pts[:k, pc[0]] = bx[:, bc[0]] + c * u - s * v
    pts[:k, pc[1]] = bx[:, bc[1]] + s * u + c * v
    pts[:k, axis] = bx[:, axis] + z
    return np.ascontiguousarray(pts[rng.permutation(n)]), boxes


def scale3(points, boxes):
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    return (np.abs(p).sum(1))[None, :] + (np.abs(b[:, :6]).sum(1))[:, None]


def dist3_torch(P, B, axis):
    """box3dr_pdist's composition pair by pair: the planar distance with the 1-D gap along `axis`.  P[..., 3], B[..., 7]"""
    pc, bc = _AXES[axis]
    d2 = dist_torch(P[..., pc], B[..., bc])
    z, zc, half = P[..., axis], B[..., axis], B[..., 3 + axis] / 2
    dp = torch.where(z > zc, zc + half - z, z - (zc - half))
    return torch.where(dp > 0, torch.where(d2 > 0, torch.minimum(dp, d2), d2),
                       torch.where(d2 > 0, dp, -torch.sqrt(d2.square() + dp.square())))


def signed_distance3(points, boxes, axis):
    P, B = _pairwise_leaves(points, boxes, torch.float64)
    with torch.no_grad():
        return dist3_torch(P, B, axis).numpy()


def kink_mask3(points, boxes, axis, margin=MARGIN):
    """bool[m,n]: the planar kinks, or one of the composition's conditions within tol of switching (the gap along the axis
    near 0 or near its ridge at the centre, the planar distance near 0, the two near each other where the smaller counts)"""
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    pc, bc = _AXES[axis]
    p2, b2 = p[:, pc], b[:, bc]
    d2 = signed_distance(p2, b2)
    dz = p[None, :, axis] - b[:, axis, None]
    dp = b[:, 3 + axis, None] / 2 - np.abs(dz)
    tol = margin * (np.abs(b[:, 3:6]).sum(1))[:, None]
    return (kink_mask(p2, b2, margin) | (np.abs(dp) <= tol) | (np.abs(dz) <= tol) | (np.abs(d2) <= tol)
            | ((dp > 0) & (d2 > 0) & (np.abs(dp - d2) <= tol)))


def grad_reference3(points, boxes, weight, axis):
    P, B = _pairwise_leaves(points, boxes, torch.float64)
    dist3_torch(P, B, axis).backward(torch.as_tensor(np.asarray(weight), dtype=torch.float64))
    return (P.grad.sum(0).numpy(), B.grad.sum(1).numpy()) + _sums(P, B, [0, 1, 2], [3, 4, 5])
