"""The scenes of the lift-splat tests (test_lift.py, test_gpu_lift.py): small frustums, S in 1 .. 6 cameras over B in 1 .. 2 samples,
D in {1, 5, 7}, H x W in {1 x 1, 3 x 5, 4 x 16}.  A scene is a dict of read-only numpy arrays (us, vs, ds, pre, post), `bounds`, `shape`,
`cams` (cameras per sample) and what the model makes of it, computed once and shared.  The conditions at the end of this file are
asserted when it is imported, on the CPU."""
import functools

import numpy as np

import lift_reference as ref

F = np.float32
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def _affine(rows=None, shift=(0, 0, 0)):
    m = EYE.copy() if rows is None else np.array(rows, np.float64)
    m[:, 3] += shift
    return m


def _scene(us, vs, ds, pre, post, bounds, shape, cams, integer=False, degenerate=False):
    pre, post = np.array(pre, F).reshape(-1, 3, 4), np.array(post, F).reshape(-1, 3, 4)
    assert len(pre) == len(post) and len(pre) % cams == 0
    sc = dict(us=np.array(us, F), vs=np.array(vs, F), ds=np.array(ds, F), pre=pre, post=post, bounds=tuple(bounds), shape=tuple(shape),
              cams=cams, integer=integer, degenerate=degenerate)
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def _camera(rng, yaw, scale=1.0):
    """a pinhole looking along +x turned by yaw about z: (pre, post) in fp64, LSS's formula with a mild image augmentation"""
    c, s = np.cos(yaw), np.sin(yaw)
    cam2ego = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[0, 0, 1.0], [-1, 0, 0], [0, -1, 0]])
    intr = np.array([[12.0 * scale, 0, 8], [0, 12.0 * scale, 2], [0, 0, 1]])
    post_rot = np.diag([1.1, 0.9, 1.0])
    post_tr = np.array([0.5, -0.25, 0])
    inv = np.linalg.inv(post_rot)
    pre = np.concatenate([inv, -(inv @ post_tr)[:, None]], 1)
    post = np.concatenate([cam2ego @ np.linalg.inv(intr), rng.uniform(-0.5, 0.5, (3, 1))], 1)
    return pre, post


# a signed permutation: (e0, e1, e2) -> (e2, -e0, e1)
_TURN = [[0, 0, 1, 0], [-1, 0, 0, 0], [0, 1, 0, 0]]


def _int_3x5():
    """2 cameras of one sample, D 5, 3 x 5, integers throughout: x = (d - 2, -(u - 2) d - 1, (v - 1) d) and the same half a cell (1 m)
    further in y -- the two cameras feed the same cells.  Cells of 2 m from lo = (0, -7, -2), 1 x 6 x 2 of them: on every axis t hits
    0, the shape and (-1, 0) while the other two axes are inside"""
    pre = [_affine(shift=(-2, -1, 0))] * 2
    post = [_affine(_TURN, (-2, -1, 0)), _affine(_TURN, (-2, -2, 0))]
    return _scene(range(5), range(3), range(1, 6), pre, post, (0, 2, -7, 5, -2, 2), (1, 6, 2), 2, integer=True)


def _int_4x16():
    """6 cameras over 2 samples, D 7, 4 x 16 (D H W = 448 = 7 x 64), integers; camera 4 lies entirely outside the grid, camera 5 repeats
    camera 3 (same sample, same cells); half-metre cells on z"""
    pre = [_affine(shift=(-8 + s, -2, 0)) for s in range(6)]
    post = [_affine(_TURN, (0, s, 0)) for s in range(6)]
    post[4] = _affine(_TURN, (1000, 0, 0))
    pre[5], post[5] = pre[3], post[3]
    return _scene(range(16), range(4), range(1, 8), pre, post, (1, 7, -20, 20, -4, 4), (6, 10, 16), 3, integer=True)


def _pixel():
    return _scene([3], [2], [4], [EYE], [EYE], (0, 16, 0, 16, 0, 8), (4, 4, 2), 1, integer=True, degenerate=True)


def _one_bin():
    """D = 1: a single depth plane, 2 samples of one camera"""
    return _scene(range(5), range(3), [2], [EYE, _affine(shift=(1, 0, 0))], [EYE, EYE], (0, 8, 0, 4, 0, 4), (4, 2, 1), 1,
                  integer=True, degenerate=True)


def _cameras(seed, yaws, us, vs, ds, bounds, shape, cams, spoil=()):
    rng = np.random.default_rng(seed)
    mats = [_camera(rng, y) for y in yaws]
    pre, post = [m[0] for m in mats], [m[1] for m in mats]
    for s, which, i, j, value in spoil:
        (pre if which == "pre" else post)[s][i, j] = value
    return _scene(us, vs, ds, pre, post, bounds, shape, cams)


def _ring_3x5():
    """4 cameras over 2 samples looking four ways, D 5, 3 x 5, real calibrations (nothing exact)"""
    return _cameras(1, (0.0, 1.5, 3.1, 4.6), np.linspace(0, 16, 5), np.linspace(0, 4, 3), np.linspace(1, 9, 5),
                    (-6, 6, -6, 6, -3, 3), (8, 8, 2), 2)


def _spoiled_4x16():
    """6 cameras of one sample, D 7, 4 x 16; NaN in camera 1's pre and +inf in camera 3's post (an entry that multiplies a nonzero value)
    take their points out, -inf in a column of camera 5 that multiplies e1 takes all but none back in"""
    return _cameras(2, np.arange(6) * 1.05, np.linspace(0, 16, 16), np.linspace(0, 4, 4), np.linspace(1, 10, 7),
                    (-10, 10, -10, 10, -3, 3), (10, 10, 3), 6,
                    spoil=((1, "pre", 0, 0, np.nan), (3, "post", 1, 2, np.inf), (5, "post", 2, 3, -np.inf)))


def _empty():
    """every camera looks at a grid that is elsewhere: V = 0"""
    return _cameras(3, (0.0, 2.0), np.linspace(0, 16, 5), np.linspace(0, 4, 3), np.linspace(1, 9, 5),
                    (100, 110, 100, 110, 0, 3), (5, 5, 1), 1)


def _crowded():
    """6 cameras of one sample, D 7, 4 x 16, x = (u d, v d, d) in cells of 128 x 32 x 8 from (-256, 0, 0): cameras 0 .. 3 land in
    cell 2 whole, camera 4 (u d + 23, v d - 1) loses its v = 0 row to t in (-1, 0) and three points to cell 3, camera 5 (u d - 233,
    v d - 21) puts ONE point in cell 1 and 15 in cell 0; cell 4 stays empty"""
    post = [EYE] * 4 + [_affine(shift=(23, -1, 0)), _affine(shift=(-233, -21, 0))]
    return _scene(range(16), range(4), range(1, 8), [EYE] * 6, post, (-256, 384, 0, 32, 0, 8), (5, 1, 1), 6, integer=True)


_BUILD = {"int_3x5": _int_3x5, "int_4x16": _int_4x16, "pixel": _pixel, "one_bin": _one_bin, "ring_3x5": _ring_3x5,
          "spoiled_4x16": _spoiled_4x16, "empty": _empty, "crowded": _crowded}
SCENES = tuple(_BUILD)
INTEGER = tuple(n for n in SCENES if _BUILD[n]()["integer"])
WINDOWS = (4, 8)                              # the rows a fold keeps in flight (csrc/vlift.hip: kLiftBins, kLiftAhead)


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILD[name]()


def frustum(name):
    sc = scene(name)
    return len(sc["ds"]), len(sc["vs"]), len(sc["us"])


def sizes(name):
    """-> (S, B, K)"""
    sc = scene(name)
    s = len(sc["pre"])
    d, h, w = frustum(name)
    return s, s // sc["cams"], s * d * h * w


@functools.lru_cache(maxsize=None)
def model(name):
    """-> dict(t, member, cell, mapping, coords, batch_index, V) of the numpy model, read-only"""
    sc = scene(name)
    lo, size = ref.grid(sc["bounds"], sc["shape"])
    t, member, cell = ref.cells(sc["us"], sc["vs"], sc["ds"], sc["pre"], sc["post"], lo, size, sc["shape"], sc["cams"])
    mapping, coords, batch = ref.number(member, cell, sc["shape"])
    out = dict(lo=lo, size=size, t=t, member=member, cell=cell, mapping=mapping, coords=coords, batch_index=batch)
    for a in out.values():
        a.setflags(write=False)
    out["V"] = len(coords)
    return out


def randoms(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape)


def integers(shape, seed, lo=-4, hi=5):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.float64)


def dyadic(shape, seed):
    """multiples of 1/8 in [-2, 2]: products are multiples of 1/64 below 4, sums of thousands of them stay exact in fp32"""
    return np.random.default_rng(seed).integers(-16, 17, shape) / 8.0


# ---------------------------------------------------------------- what the scenes must contain (asserted on import)
def _conditions():
    for name in SCENES:
        sc, m = scene(name), model(name)
        s, b, k = sizes(name)
        d, h, w = frustum(name)
        assert 1 <= s <= 6 and 1 <= b <= 2 and d in (1, 5, 7) and (h, w) in ((1, 1), (3, 5), (4, 16)), name
        if sc["degenerate"] or name == "empty":
            continue
        which_d = (np.arange(k) // (h * w)) % d
        assert len(np.unique(which_d[m["member"]])) >= 2, name                       # members from at least two depth bins
        assert np.count_nonzero(~m["member"]) <= 0.9 * k, name                        # at most 90 % outside
    assert sum((frustum(n)[0] * frustum(n)[1] * frustum(n)[2]) % 64 != 0 for n in SCENES) > len(SCENES) // 2
    # the borders: t exactly 0, t exactly the shape (out), t inside (-1, 0) (out) -- each with the other two axes inside, so that
    # the point's fate hangs on that axis alone; truncation toward zero would keep the last kind in cell 0
    for name in ("int_3x5", "crowded"):
        sc, m = scene(name), model(name)
        t, shape = m["t"].astype(np.float64), np.array(sc["shape"], np.float64)
        inside = (t >= 0) & (t < shape)
        for axis in range(3):
            others = np.all(np.delete(inside, axis, 1), 1)
            if name == "int_3x5" or axis == 1:
                assert np.any(others & (t[:, axis] > -1) & (t[:, axis] < 0)), (name, axis)
            if name == "int_3x5":
                assert np.any(others & (t[:, axis] == 0) & m["member"]), (name, axis)
                assert np.any(others & (t[:, axis] == shape[axis]) & ~m["member"]), (name, axis)
    # NaN / inf calibrations take whole cameras out, and a camera can be outside on its own
    per_cam = lambda name: model(name)["member"].reshape(len(scene(name)["pre"]), -1).sum(1)      # noqa: E731
    assert not np.all(np.isfinite(scene("spoiled_4x16")["pre"])) and not np.all(np.isfinite(scene("spoiled_4x16")["post"]))
    sp = per_cam("spoiled_4x16")
    assert sp[1] == 0 and sp[3] == 0 and sp[5] == 0 and sp[0] > 0 and sp[2] > 0 and sp[4] > 0
    assert per_cam("int_4x16")[4] == 0 and np.all(np.delete(per_cam("int_4x16"), 4) > 0)
    assert model("empty")["V"] == 0 and sizes("empty")[2] > 0
    # two cameras feed the same cells
    for name, a, c in (("int_3x5", 0, 1), ("int_4x16", 3, 5)):
        rows = model(name)["mapping"].reshape(len(scene(name)["pre"]), -1)
        assert len(np.intersect1d(rows[a][rows[a] >= 0], rows[c][rows[c] >= 0])) >= 2, name
    # the crowded scene: one cell with at least 2000 points and a tail beside the window, cells with one entry and with none
    per_row = np.bincount(model("crowded")["mapping"][model("crowded")["member"]])
    assert per_row.max() >= 2000 and all(per_row.max() % n != 0 for n in WINDOWS) and per_row.min() == 1
    assert model("crowded")["V"] < int(np.prod(scene("crowded")["shape"]))
    # the integer scenes: every intermediate is exact in fp32 -- the fp32 model's positions equal the fp64 evaluation of the same
    # expressions, for EVERY point (nothing is left out of the comparison with exact arithmetic)
    for name in INTEGER:
        sc, m = scene(name), model(name)
        x32 = ref.positions(sc["us"], sc["vs"], sc["ds"], sc["pre"], sc["post"])
        a = np.meshgrid(sc["ds"].astype(np.float64), sc["vs"].astype(np.float64), sc["us"].astype(np.float64), indexing="ij")
        a = (a[2], a[1], a[0])
        pre, post = sc["pre"].astype(np.float64), sc["post"].astype(np.float64)
        for s in range(len(pre)):
            q = [sum(pre[s, i, j] * a[j] for j in range(3)) + pre[s, i, 3] for i in range(3)]
            e = (q[0] * q[2], q[1] * q[2], q[2])
            for i in range(3):
                x = sum(post[s, i, j] * e[j] for j in range(3)) + post[s, i, 3]
                assert np.all(np.abs(x) < 2 ** 24) and np.array_equal(x, x32[i][s].astype(np.float64)), (name, s, i)
                t = (x - float(m["lo"][i])) / float(m["size"][i])
                assert np.array_equal(t.reshape(-1), m["t"].reshape(len(pre), -1, 3)[s, :, i].astype(np.float64)), (name, s, i)


_conditions()
