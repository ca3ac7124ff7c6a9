"""An fp64 model of TransformSet.project_points_to_camera / transform_points, written from the formulas of the operator's
specification with explicit per-component sums (left to right), for the sizes where no golden file fits; and the comparison
rule every camera test uses.  No GPU, no library.

    cam = rt[0:3, 0:3] . p + rt[0:3, 3];  h = P . cam;  d = h[2];  u = h[0] / d;  v = h[1] / d
    dmask = d > 0;  mask = 0 < u < W and 0 < v < H and dmask
    with distortion (k1, k2, p1, p2, k3) and intri_matrix (fx, fy, cx, cy):
        pre = -20 < u < W + 20 and -20 < v < H + 20
        u, v = (u - cx) / fx, (v - cy) / fy;  r2 = u u + v v;  cd = 1 + k1 r2 + k2 r2^2 + k3 r2^3
        ud = u cd + p1 (2 u v) + p2 (r2 + 2 u u);  vd = v cd + p1 (r2 + 2 v v) + p2 (2 u v)
        u, v = ud fx + cx, vd fy + cy;  mask = pre and 0 < u < W and 0 < v < H and dmask
"""
import json

import numpy as np

PRE_MASK = 20            # pixels around the image a point may lie in before the distortion
NEAR = 1e-6              # a point this close to a bound it is compared with (or with |d| below it) may fall either way
MAX_NEAR = 10            # ... and a case may hold at most this many of them
UV_ATOL = 1e-9           # px, points in view
UV_RTOL = 1e-9           # points out of view
XYZ_TOL = 1e-12          # transform_points, rtol and atol


def _rows(m, x, y, z, w=None):
    """m[r, 0] x + m[r, 1] y + m[r, 2] z (+ m[r, 3]) for r = 0, 1, 2"""
    out = []
    for r in range(3):
        s = m[r, 0] * x + m[r, 1] * y + m[r, 2] * z
        out.append(s if w is None else s + m[r, 3])
    return out


def project(points, rt, P, width, height, dist=None, intri=None):
    """-> dict: u0, v0 (before the distortion), d, u, v (final), pre, mask, dmask (bool [N])"""
    pts = np.asarray(points)
    rt, P = np.asarray(rt, np.float64), np.asarray(P, np.float64)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        cam = _rows(rt, x, y, z, True)
        h = _rows(P, cam[0], cam[1], cam[2])
        d = h[2]
        u0, v0 = h[0] / d, h[1] / d
        dmask = d > 0
        u, v = u0, v0
        pre = np.ones(len(pts), bool)
        if dist is not None and len(dist):
            k1, k2, p1, p2, k3 = (float(c) for c in dist)
            fx, fy, cx, cy = intri[0, 0], intri[1, 1], intri[0, 2], intri[1, 2]
            pre = (-PRE_MASK < u0) & (u0 < width + PRE_MASK) & (-PRE_MASK < v0) & (v0 < height + PRE_MASK)
            a, b = (u0 - cx) / fx, (v0 - cy) / fy
            r2 = a * a + b * b
            cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            ud = a * cd + p1 * (2 * a * b) + p2 * (r2 + 2 * a * a)
            vd = b * cd + p1 * (r2 + 2 * b * b) + p2 * (2 * a * b)
            u, v = ud * fx + cx, vd * fy + cy
        mask = pre & (0 < u) & (u < width) & (0 < v) & (v < height) & dmask
    return dict(u0=u0, v0=v0, d=d, u=u, v=v, pre=pre, mask=mask, dmask=dmask, width=width, height=height,
                distorted=dist is not None and len(dist) > 0)


def near_points(model):
    """bool [N]: the points the comparison rule may leave out"""
    w, h = model["width"], model["height"]
    with np.errstate(all="ignore"):
        def close(a, bounds):
            return np.any([np.abs(a - b) < NEAR for b in bounds], axis=0)
        near = close(model["u"], (0, w)) | close(model["v"], (0, h)) | (np.abs(model["d"]) < NEAR)
        if model["distorted"]:
            near |= close(model["u0"], (-PRE_MASK, w + PRE_MASK)) | close(model["v0"], (-PRE_MASK, h + PRE_MASK))
    return near


def expected(model):
    """the operator's outputs in full form: uv_all [N,2], uv_kept [K,2], mask [K], dmask [Kd]"""
    uv = np.stack([model["u"], model["v"]], 1)
    return dict(uv_all=uv, uv_kept=uv[model["mask"]], mask=np.nonzero(model["mask"])[0], dmask=np.nonzero(model["dmask"])[0])


def full_form(n, call):
    """call(remove_outlier, return_dmask) -> the operator's tuple; runs the four combinations, checks that they agree with each
    other where they overlap, and returns the full form"""
    uv_all, mask, dmask = [np.asarray(a) for a in call(False, True)]
    uv_kept, mask2, dmask2 = [np.asarray(a) for a in call(True, True)]
    r3, r4 = call(False, False), call(True, False)
    assert len(r3) == 2 and len(r4) == 2
    assert uv_all.shape == (n, 2) and uv_all.dtype == np.float64 and mask.dtype == np.int64 and dmask.dtype == np.int64
    assert uv_kept.shape == (len(mask), 2) and uv_kept.dtype == np.float64
    assert np.array_equal(mask, mask2) and np.array_equal(dmask, dmask2)
    assert np.array_equal(np.asarray(r3[1]), mask) and np.array_equal(np.asarray(r4[1]), mask)
    assert np.array_equal(np.asarray(r3[0]), uv_all, equal_nan=True) and np.array_equal(np.asarray(r4[0]), uv_kept)
    assert np.array_equal(uv_all[mask], uv_kept)
    return dict(uv_all=uv_all, uv_kept=uv_kept, mask=mask, dmask=dmask)


def check_projection(exp, got, near, what=""):
    """The comparison rule.  dmask, mask, K and Kd equal; only the points of `near` (at most MAX_NEAR, asserted) stay out of
    it.  uv of the compared points in view within UV_ATOL px; out of view rtol UV_RTOL, NaN equal to NaN, infinities equal in
    sign."""
    n = len(near)
    n_near = int(near.sum())
    assert n_near <= MAX_NEAR, "%s: %d points near a bound" % (what, n_near)
    keep = ~near
    for key in ("mask", "dmask"):
        e, g = np.zeros(n, bool), np.zeros(n, bool)
        e[exp[key]] = True
        g[got[key]] = True
        assert np.all(np.diff(got[key]) > 0), "%s: %s is not ascending" % (what, key)
        bad = np.nonzero((e != g) & keep)[0]
        assert bad.size == 0, "%s: %s differs at points %s" % (what, key, bad[:10])
        if n_near == 0:
            assert np.array_equal(exp[key], got[key]), "%s: %s" % (what, key)
    assert got["uv_all"].shape == (n, 2) and got["uv_kept"].shape == (len(got["mask"]), 2), what
    e, g = np.zeros(n, bool), np.zeros(n, bool)
    e[exp["mask"]] = True
    g[got["mask"]] = True
    inview = e & g & keep
    if inview.any():
        delta = np.abs(got["uv_all"][inview] - exp["uv_all"][inview]).max()
        assert delta <= UV_ATOL, "%s: uv in view off by %.3g px" % (what, delta)
        # the compacted rows are the rows of the kept points, in point order
        ge = np.full(n, -1)
        ge[got["mask"]] = np.arange(len(got["mask"]))
        ee = np.full(n, -1)
        ee[exp["mask"]] = np.arange(len(exp["mask"]))
        idx = np.nonzero(inview)[0]
        delta = np.abs(got["uv_kept"][ge[idx]] - exp["uv_kept"][ee[idx]]).max()
        assert delta <= UV_ATOL, "%s: compacted uv off by %.3g px" % (what, delta)
    outview = ~e & ~g & keep
    with np.errstate(all="ignore"):
        ok = np.isclose(got["uv_all"][outview], exp["uv_all"][outview], rtol=UV_RTOL, atol=0, equal_nan=True)
    assert ok.all(), "%s: uv out of view differs at points %s" % (what, np.nonzero(outview)[0][~ok.all(1)][:10])
    return n_near


# ---------------------------------------------------------------- rigs as data
# A rig is {"base": name, "calls": [[method, args, kwargs], ...]}: the calls that build a TransformSet, replayed on whichever class
# is under test.  Arrays travel as {"nd": nested list}.

def encode(x):
    if isinstance(x, np.ndarray):
        return {"nd": x.tolist()}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, dict):
        return {k: encode(v) for k, v in x.items()}
    if isinstance(x, (np.floating, np.integer)):
        return x.item()
    return x


def decode(x):
    if isinstance(x, dict):
        if set(x) == {"nd"}:
            return np.array(x["nd"], dtype=np.float64)
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def replay(cls, rig):
    """-> cls(base) after the rig's calls"""
    rig = json.loads(rig) if isinstance(rig, (str, bytes)) else rig
    ts = cls(rig["base"])
    for method, args, kwargs in rig["calls"]:
        getattr(ts, method)(*decode(args), **decode(kwargs))
    return ts


def transform(points, rt):
    """transform_points: fp64 [N, cols]"""
    pts = np.asarray(points)
    rt = np.asarray(rt, np.float64)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    out = pts.astype(np.float64)
    for r, col in enumerate(_rows(rt, x, y, z, True)):
        out[:, r] = col
    return out
