"""Scenes for the point-in-box operators (crop_points, paint_label, crop_2dr, box3dp_crop): box sets that drive the per-workgroup
box grid of crop.hip to each of its levels, and clouds with points planted where a grid or a tile loop goes wrong.  Data only:
tests/test_crop_cases.py holds the scenes against the oracle without a GPU, tests/test_gpu_crop_routes.py runs the kernels on
them.  Everything is fp32 in a 100 m x 100 m scene; every generator is seeded and takes (name, n) or (m, n)."""
import ctypes
import ctypes.util
import functools
import types

import numpy as np

SCENES = ("g32", "g16_list", "g16_box", "g8_box", "g8_single", "all_list", "all_nan", "all_inf_w", "all_inf_yaw", "zero_extent",
          "huge_extent")
CLASSES = 3
SPOILED_ROW = 57            # the non-finite row of all_nan / all_inf_w / all_inf_yaw
BIG_ROW = 100               # where g16_box / g8_box insert their large box
F = np.float32


def _host_sincos(r):
    """sinf / cosf of the host's libm, angle by angle: the numbers the oracle builds its corners from (numpy's own float32
    sine may differ from it in the last bit, and a corner copied with another sine is no longer ON the box)"""
    r = np.asarray(r, F)
    try:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.sinf.restype = libm.cosf.restype = ctypes.c_float
        libm.sinf.argtypes = libm.cosf.argtypes = [ctypes.c_float]
        s = np.array([libm.sinf(float(a)) for a in r], F)
        c = np.array([libm.cosf(float(a)) for a in r], F)
    except OSError:
        with np.errstate(all="ignore"):
            s, c = np.sin(r).astype(F), np.cos(r).astype(F)
    return s, c


def corners(boxes):
    """corners of [M,7] boxes in fp32, in the oracle's own expressions (quad_from_xywhr): qx[M,4], qy[M,4]"""
    b = np.asarray(boxes, F)
    x, y, w, h = b[:, 0], b[:, 1], b[:, 3], b[:, 4]
    s, c = _host_sincos(b[:, 6])
    with np.errstate(all="ignore"):
        dxs, dxc, dys, dyc = w * s / F(2), w * c / F(2), h * s / F(2), h * c / F(2)
        qx = np.stack([x - dxc + dys, x + dxc + dys, x + dxc - dys, x - dxc - dys], 1)
        qy = np.stack([y - dxs - dyc, y + dxs - dyc, y + dxs + dyc, y - dxs + dyc], 1)
    return qx.astype(F), qy.astype(F)


def _boxes(rng, m, lo=1.5, hi=5.5):
    return np.stack([rng.random(m) * 100 - 50, rng.random(m) * 100 - 50, rng.random(m) * 2 - 1.5,
                     rng.random(m) * (hi - lo) + lo, rng.random(m) * (hi - lo) + lo, rng.random(m) * 1.5 + 1.0,
                     rng.random(m) * 6.28 - 3.14], 1).astype(F)


def _duplicates(m, skip=()):
    """(lo, hi) rows that share one geometry: two pairs of DIFFERENT classes (a point of hi's class lies in lo first), two of
    the SAME class (the lower index wins).  hi lies far behind lo: in another tile of 64 wherever m allows it."""
    if m < 5:
        return [], []
    want = [(3, m - 1), (min(10, m // 2 - 1), m // 2 + 1), (min(5, m // 2 - 2), m - 2), (min(20, m // 2), m // 2 + 7 if m > 20 else m - 3)]
    taken, pairs = set(skip), []
    for lo, hi in want:
        while lo in taken:
            lo += 1
        taken.add(lo)
        while hi in taken:
            hi -= 1
        taken.add(hi)
        assert 0 <= lo < hi < m
        pairs.append((lo, hi))
    return pairs[:2], pairs[2:]


def _label_boxes(rng, boxes, skip=()):
    m = len(boxes)
    labels = rng.integers(1, CLASSES + 1, m).astype(np.uint8)
    wrong, tie = _duplicates(m, skip)
    for k, (lo, hi) in enumerate(wrong + tie):
        boxes[lo, 2], boxes[lo, 5] = 6 + 3 * k, 2            # a z layer of the pair's own: among 1000 overlapping boxes of 25 m
        boxes[hi] = boxes[lo]                               # another box would take every point first
        labels[hi] = labels[lo] % CLASSES + 1 if k < len(wrong) else labels[lo]
    return labels, wrong, tie


@functools.lru_cache(maxsize=None)
def _scene_boxes(name):
    """-> (boxes[M,7], labels[M], wrong-class pairs, same-class pairs); the boxes of a scene do not depend on n"""
    if name not in SCENES:
        raise KeyError(name)
    base = np.random.default_rng(4201)                      # g32's boxes are shared by every scene that is "g32 plus ..."
    rng = np.random.default_rng(4300 + SCENES.index(name))
    skip = ()
    if name in ("g32", "g16_box", "g8_box", "all_nan", "all_inf_w", "all_inf_yaw"):
        boxes = _boxes(base, 200)
        if name == "g16_box":
            boxes = np.insert(boxes, BIG_ROW, np.array([0.5, -1.0, -0.5, 30, 30, 4, 0.3], F), 0)
        if name == "g8_box":
            boxes = np.insert(boxes, BIG_ROW, np.array([1.0, 0.5, -0.5, 60, 60, 4, 0.1], F), 0)
        if name in ("g16_box", "g8_box"):
            skip = (BIG_ROW,)
        if name.startswith("all_"):
            skip = (SPOILED_ROW,)
    elif name == "g16_list":
        boxes = _boxes(rng, 2000)
    elif name == "g8_single":
        boxes = np.array([[3, -4, -0.5, 4.5, 2, 1.6, 0.7]], F)
    elif name == "all_list":
        boxes = _boxes(rng, 1000, 25, 30)
    elif name == "zero_extent":
        boxes = np.array([[12.5, -7.25, z, 0, 0, lz, r] for z, lz, r in
                          [(-0.5, 2, 0.0), (-0.25, 2.5, 0.4), (-0.5, 2, 0.4), (0, 3, -1.0), (-0.75, 1.5, 2.0)]], F)
    else:                                                   # huge_extent: hi - lo of the common range is inf in fp32
        boxes = np.array([[-2.5e38, 0, 0, 1e37, 1, 2, 0], [2.5e38, 0.25, 0, 1e37, 1, 2, 0]], F)
    if name == "zero_extent":                               # one place: box 0 is of another class than 1 and 2, which tie
        labels, wrong, tie = np.array([1, 2, 2, 3, 1], np.uint8), [(0, 1)], [(1, 2)]
    else:
        labels, wrong, tie = _label_boxes(rng, boxes, skip)
    if name == "all_nan":
        boxes[SPOILED_ROW, 0] = np.nan
    if name == "all_inf_w":
        boxes[SPOILED_ROW, 3] = np.inf
    if name == "all_inf_yaw":
        boxes[SPOILED_ROW, 6] = np.inf
    boxes.setflags(write=False)
    labels.setflags(write=False)
    return boxes, labels, tuple(wrong), tuple(tie)


def _inside(rng, boxes, which, spread=1.1):
    """a point per entry of `which`, uniform in that box scaled by `spread` (1.1: a tenth of them just outside)"""
    k = len(which)
    b = boxes[which]
    s, c = _host_sincos(b[:, 6])
    u = ((rng.random(k) - 0.5) * spread).astype(F) * b[:, 3]
    v = ((rng.random(k) - 0.5) * spread).astype(F) * b[:, 4]
    return np.stack([b[:, 0] + c * u - s * v, b[:, 1] + s * u + c * v, b[:, 2] + ((rng.random(k) - 0.5) * spread).astype(F) * b[:, 5]],
                    1).astype(F)


def _assemble(rng, boxes, labels, wrong, tie, n, planted, sem_planted, special, sem_special, pairs, lo_xy, hi_xy):
    """planted + special + random filler -> shuffled cloud[n,6], semantics[n], pairs with shuffled indices"""
    nfill = n - len(planted) - len(special)
    assert nfill >= 0, "n too small for the planted points of this scene"
    fill = np.stack([rng.random(nfill) * (hi_xy[0] - lo_xy[0]) + lo_xy[0], rng.random(nfill) * (hi_xy[1] - lo_xy[1]) + lo_xy[1],
                     rng.random(nfill) * 4 - 2.5], 1).astype(F)
    xyz = np.concatenate([planted, special, fill], 0).astype(F)
    sem = np.concatenate([sem_planted, sem_special, rng.integers(0, CLASSES + 1, nfill).astype(np.uint8)])
    perm = rng.permutation(n)                               # new position p holds old point perm[p]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    pts = np.concatenate([xyz[perm], rng.random((n, 3)).astype(F)], 1)
    m = len(boxes)
    scores = np.sort(rng.random(m))[::-1]
    rows9 = np.concatenate([labels[:, None].astype(F), scores[:, None].astype(F), boxes], 1).astype(F)
    pairs = np.array([(b, inv[len(planted) + i], inv[len(planted) + o]) for b, i, o in pairs], np.int64).reshape(-1, 3)
    return types.SimpleNamespace(boxes=np.array(boxes), rows9=rows9, labels=np.array(labels), pts=pts, sem=sem[perm], pairs=pairs,
                                 wrong=wrong, tie=tie, m=m, n=n)


def _plant(rng, boxes, labels, wrong, tie, k, finite):
    """k points inside boxes; the first quarter inside the duplicated geometries with the semantics that make the pair matter"""
    which = finite[rng.integers(0, len(finite), k)]
    sem = rng.integers(0, CLASSES + 1, k).astype(np.uint8)
    dup = list(wrong) + list(tie)
    for t in range(k // 4 if dup else 0):
        lo, hi = dup[t % len(dup)]
        which[t] = lo
        sem[t] = labels[hi]                                 # (different classes: lo holds the point, hi is painted; same: lo is)
    return _inside(rng, boxes, which), sem


def rows11(boxes):
    """the [M,7] rows inside [M,11] rows at column 3 (box_stride 11, box_offset 3 of the raw entries); NaN around them"""
    out = np.full((len(boxes), 11), np.nan, F)
    out[:, 3:10] = boxes
    return out


@functools.lru_cache(maxsize=8)
def scene(name, n):
    """-> namespace: boxes[M,7], rows9[M,9], labels[M] u8, pts[n,6], sem[n] u8, pairs[K,3] = (box, a point ON that box's
    boundary, its twin one fp32 step outside), wrong / tie = the duplicated rows"""
    boxes, labels, wrong, tie = _scene_boxes(name)
    m = len(boxes)
    rng = np.random.default_rng(977 * (SCENES.index(name) + 1) + n)
    with np.errstate(all="ignore"):
        qx, qy = corners(boxes)
        finite = np.flatnonzero(np.isfinite(qx).all(1) & np.isfinite(qy).all(1))
        planted, sem_planted = _plant(rng, boxes, labels, wrong, tie, n // 3, finite)
        special, sem_special, pairs = [], [], []

        def add(x, y, z, sem):
            special.append((x, y, z))
            sem_special.append(sem)
            return len(special) - 1

        # corners, edge midpoints, top and bottom faces of up to 40 boxes (the duplicated and the large ones among them)
        chosen = [i for p in list(wrong) + list(tie) for i in p]
        if name in ("g16_box", "g8_box"):
            chosen.append(BIG_ROW)
        chosen += [int(i) for i in finite[:: max(1, len(finite) // 24)]]
        for i in dict.fromkeys(chosen):
            b, cls = boxes[i], labels[i]
            for e in range(4):
                add(qx[i, e], qy[i, e], b[2], cls)
                add((qx[i, e] + qx[i, (e + 1) & 3]) / F(2), (qy[i, e] + qy[i, (e + 1) & 3]) / F(2), b[2], cls)
            top, bot = b[2] + b[5] / F(2), b[2] - b[5] / F(2)            # dgal_wrap.h:12, fp32
            pairs.append((i, add(b[0], b[1], top, cls), add(b[0], b[1], np.nextafter(top, F(np.inf)), cls)))
            pairs.append((i, add(b[0], b[1], bot, cls), add(b[0], b[1], np.nextafter(bot, F(-np.inf)), cls)))
        # the common range of the (finite) boxes: the extreme corner itself, one step outside it, and points well outside
        fx, fy = qx[finite], qy[finite]
        ext = []
        for q, other, pick, away in ((fx, fy, np.argmin, -np.inf), (fx, fy, np.argmax, np.inf), (fy, fx, np.argmin, -np.inf),
                                     (fy, fx, np.argmax, np.inf)):
            r, e = np.unravel_index(pick(q), q.shape)
            i = int(finite[r])
            on, off = q[r, e], np.nextafter(q[r, e], F(away))
            ext.append(on)
            if q is fx:
                pairs.append((i, add(on, other[r, e], boxes[i, 2], labels[i]), add(off, other[r, e], boxes[i, 2], labels[i])))
            else:
                pairs.append((i, add(other[r, e], on, boxes[i, 2], labels[i]), add(other[r, e], off, boxes[i, 2], labels[i])))
        xmin, xmax, ymin, ymax = ext
        dx, dy = max(F(1), F(0.01) * max(abs(xmin), abs(xmax))), max(F(1), F(0.01) * max(abs(ymin), abs(ymax)))
        xm, ym, z0 = (xmin / F(2) + xmax / F(2)), (ymin / F(2) + ymax / F(2)), boxes[finite[0], 2]
        for x, y in ((xmin - dx, ym), (xmin - 50 * dx, ymin), (xmax + dx, ym), (xmax + 50 * dx, ymax), (xm, ymin - dy), (xmin, ymin - 50 * dy),
                     (xm, ymax + dy), (xmax, ymax + 50 * dy), (xmin - dx, ymin - dy), (xmax + dx, ymax + dy), (xmin - dx, ymax + dy),
                     (xmax + dx, ymin - dy)):
            add(x, y, z0, labels[finite[0]])
        # non-finite points, at the centre of a box where a coordinate is left to decide (NaN z is INSIDE there: closed tests)
        b0, c0 = boxes[finite[0]], labels[finite[0]]
        for x, y, z in ((np.nan, b0[1], b0[2]), (b0[0], np.nan, b0[2]), (b0[0], b0[1], np.nan), (np.inf, b0[1], b0[2]),
                        (-np.inf, b0[1], b0[2]), (b0[0], b0[1], np.inf), (b0[0], b0[1], -np.inf)):
            add(x, y, z, c0)
        if name == "huge_extent":
            lo_xy, hi_xy = (-3.0e38, -2.0), (3.0e38, 2.0)
        elif name == "g8_box":                              # the large box holds most of the filler
            lo_xy, hi_xy = (-36.0, -36.0), (36.0, 36.0)
        else:
            lo_xy, hi_xy = (-55.0, -55.0), (55.0, 55.0)
        return _assemble(rng, boxes, labels, wrong, tie, n, planted, sem_planted, np.array(special, F).reshape(-1, 3),
                         np.array(sem_special, np.uint8), pairs, lo_xy, hi_xy)


@functools.lru_cache(maxsize=8)
def pairs_scene(m, n):
    """m boxes of 1.5 - 5.5 m with the duplicated rows of _duplicates and n points for the all-pairs kernels at ANY n >= 1: even
    points inside boxes (every 7th of them exactly on the top face, the first ones in the duplicated rows), odd ones anywhere"""
    rng = np.random.default_rng(100003 * m + n)
    boxes = _boxes(rng, m)
    labels, wrong, tie = _label_boxes(rng, boxes)
    k = (n + 1) // 2
    planted, sem_planted = _plant(rng, boxes, labels, wrong, tie, k, np.arange(m))
    which = rng.integers(0, m, k)
    top = np.arange(0, k, 7)
    planted[top, :2] = boxes[which[top], :2]
    planted[top, 2] = boxes[which[top], 2] + boxes[which[top], 5] / F(2)
    sem_planted[top] = labels[which[top]]
    sc = _assemble(rng, boxes, labels, wrong, tie, n, planted, sem_planted, np.zeros((0, 3), F), np.zeros((0,), np.uint8), [],
                   (-55.0, -55.0), (55.0, 55.0))
    return sc


def paint_early_exit(m=129, n=1025):
    """box 0 of class 1 holds every point and the first 1024 points (one workgroup of k_paint_label) are of class 1: that
    workgroup is done after the first tile; the last point is of another class and walks on"""
    sc = pairs_scene(m, n)
    boxes, labels, sem = sc.boxes.copy(), sc.labels.copy(), sc.sem.copy()
    boxes[0] = [0, 0, 0, 400, 400, 40, 0.2]
    labels[0] = 1
    sem[:1024] = 1
    sem[1024:] = 2
    return types.SimpleNamespace(boxes=boxes, labels=labels, pts=sc.pts, sem=sem, m=m, n=n)


def paint_last_tile(m=129, n=1025):
    """every box but the last is of class 1, the last one (alone in its tile of 64) is of class 2 and holds every point, and
    every point is of class 2: the only match is in the last tile"""
    sc = pairs_scene(m, n)
    boxes, labels = sc.boxes.copy(), np.ones(m, np.uint8)
    boxes[m - 1] = [0, 0, 0, 400, 400, 40, -0.3]
    labels[m - 1] = 2
    return types.SimpleNamespace(boxes=boxes, labels=labels, pts=sc.pts, sem=np.full(n, 2, np.uint8), m=m, n=n)


def wrap_scene(m=65600, n=200):
    """more boxes than uint16 ids: rows below 65535 are of classes 1 and 2; row 65535 (class 3) and row 65540 (class 4) hold
    every point.  A point of class 3 is painted 65536 = 0 in uint16, a point of class 4 is painted 65541 = 5."""
    sc = pairs_scene(m, n)
    boxes, labels = sc.boxes.copy(), (np.arange(m) % 2 + 1).astype(np.uint8)
    boxes[65535] = [0, 0, 0, 400, 400, 40, 0.2]
    boxes[65540] = [0, 0, 0, 400, 400, 40, -0.2]
    labels[65535], labels[65540] = 3, 4
    return types.SimpleNamespace(boxes=boxes, labels=labels, pts=sc.pts, sem=(np.arange(n) % 4 + 1).astype(np.uint8), m=m, n=n)


def axes_scene(n, dtype, m=60):
    """points[n,3] and boxes[m,7] for box3dp_crop along every axis: a quarter of the points planted for each axis a -- inside
    the rectangle the other two coordinates form with the box's angle, and within the strict interval along a"""
    rng = np.random.default_rng(5150 + n)
    boxes = _boxes(rng, m).astype(np.float64)
    boxes[:, 2] = rng.random(m) * 100 - 50                  # the scene is a cube here: every projection sees spread boxes
    boxes[:, 5] = rng.random(m) * 4 + 1.5
    pts = rng.random((n, 3)) * 110 - 55
    k = n // 4
    for a, (i0, i1) in enumerate(((1, 2), (0, 2), (0, 1))):
        which = rng.integers(0, m, k)
        b = boxes[which]
        u, v = (rng.random(k) - 0.5) * b[:, 3 + i0] * 1.1, (rng.random(k) - 0.5) * b[:, 3 + i1] * 1.1
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        sl = slice(a * k, (a + 1) * k)
        pts[sl, i0] = b[:, i0] + c * u - s * v
        pts[sl, i1] = b[:, i1] + s * u + c * v
        pts[sl, a] = b[:, a] + (rng.random(k) - 0.5) * b[:, 3 + a] * 1.1
    pts = pts[rng.permutation(n)]
    return pts.astype(dtype), boxes.astype(dtype)
