"""Seeded scenes for furthest_point_sample and ball_query.  Every scene is float64 numpy here; a test casts it to the dtype it runs.
Integer-valued scenes keep |x| <= 1000, where every q is exact in fp32 (3 * 2000^2 < 2^24)."""
import ctypes

import numpy as np


def _lidar(rng, n, d=4):
    pts = rng.uniform(-1.0, 1.0, (n, d)) * np.array([50.0, 50.0, 2.0] + [1.0] * (d - 3))
    return np.round(pts * 64) / 64                       # coordinates on a 1/64 grid: no squared distance gets near the subnormals


def _lattice(rng, nx, ny, nz, scale=1):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return rng.permutation(g * scale - np.array([nx // 2, ny // 2, nz // 2]) * scale)


def _with_nonfinite(rng, pts):
    """NaN, +inf and -inf in each of the three columns, at the first row among others"""
    pts = pts.copy()
    rows = [0] + sorted(rng.choice(np.arange(1, len(pts)), 8, replace=False).tolist())
    bad = [np.nan, np.inf, -np.inf]
    for k, r in enumerate(rows):
        pts[r, k % 3] = bad[(k // 3) % 3]
    return pts


def integer_fps_scenes():
    """-> [(name, points, num_samples, offsets)] with integer coordinates, all rows finite: for the exact implementation"""
    rng = np.random.default_rng(11)
    out = [("lattice", _lattice(rng, 7, 6, 4), 40, None),
           ("lattice_scaled", _lattice(rng, 5, 5, 3, 250), 80, None),
           ("random_int", rng.integers(-1000, 1001, (150, 3)).astype(np.float64), 30, None),
           ("identical", np.tile(np.array([[3.0, -7.0, 11.0]]), (60, 1)), 8, None),
           ("duplicates", np.repeat(rng.integers(-20, 21, (70, 4)).astype(np.float64), 2, axis=0), 50, None)]
    rag = rng.integers(-30, 31, (1 + 0 + 90 + 40, 3)).astype(np.float64)
    out.append(("ragged_int", rag, [3, 0, 25, 45], [0, 1, 1, 91, 131]))           # (M above the rows in the first and last segment)
    return out


def fps_scenes(big_rows):
    """-> [(name, points, num_samples, offsets)].  big_rows: a segment size just past the on-chip capacity of the dtype under test
    (d3d_fps_plan tells), for the mixed-route batch."""
    rng = np.random.default_rng(12)
    out = integer_fps_scenes()
    out.append(("lidar", _lidar(rng, 3000), 64, None))
    out.append(("lidar_d3", _lidar(rng, 700, 3), 33, None))
    out.append(("lidar_d5", _lidar(rng, 700, 5), 33, None))
    out.append(("nonfinite", _with_nonfinite(rng, _lidar(rng, 150)), 20, None))
    pts = _lidar(rng, 22, 3)
    pts[10:15] = np.nan                                   # the middle segment: every row excluded
    pts[15, 1] = np.inf                                   # the last one starts with an excluded row
    out.append(("all_excluded", pts, [4, 3, 9], [0, 10, 15, 22]))
    out.append(("huge", rng.uniform(-2e19, 2e19, (200, 3)), 20, None))             # fp32: q overflows to +inf
    n = [1, 0, 500, big_rows]
    offs = np.concatenate([[0], np.cumsum(n)])
    mixed = _lidar(rng, int(offs[-1]))
    mixed[offs[3]] = np.nan                               # the big segment starts with an excluded row
    out.append(("mixed_routes", mixed, [2, 0, 40, 24], offs.tolist()))
    return out


def integer_ball_scenes():
    """-> [(name, points, centers, radius, point_offsets, center_offsets)]: integer coordinates, integer radius -- lattice rows lie
    at exactly r from lattice centres (and are outside)"""
    rng = np.random.default_rng(13)
    lat = _lattice(rng, 9, 8, 4)
    out = [("lattice_r2", lat, lat[rng.choice(len(lat), 40, replace=False)], 2, None, None),
           ("lattice_r3", lat, np.concatenate([lat[:20], [[100.0, 100.0, 100.0]]]), 3, None, None),   # (one empty ball)
           ("identical", np.tile(np.array([[1.0, 2.0, 3.0]]), (70, 1)), np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [1.0, 2.0, 5.0]]), 2,
            None, None)]
    rag = rng.integers(-6, 7, (130 + 0 + 65, 3)).astype(np.float64)
    ctr = rng.integers(-6, 7, (12 + 5 + 0 + 9, 3)).astype(np.float64)
    out.append(("ragged_int", rag, ctr, 4, [0, 130, 130, 130, 195], [0, 12, 17, 17, 26]))   # (an empty point segment WITH centres)
    return out


def ball_scenes():
    rng = np.random.default_rng(14)
    out = integer_ball_scenes()
    pts = _lidar(rng, 1500)
    out.append(("lidar", pts, pts[rng.choice(1500, 60, replace=False), :3] + 0.25, 6.0, None, None))
    bad = _with_nonfinite(rng, _lidar(rng, 300))
    ctr = np.concatenate([bad[:3, :3], _lidar(rng, 20, 3), [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]])
    out.append(("nonfinite", bad, ctr, 20.0, None, None))
    return out


def fps_plan_of(rows, code):
    """d3d_fps_plan(rows, dtype code) -> (route, capacity); pure host arithmetic"""
    from d3d_amd import _lib
    route, cap = ctypes.c_int32(-7), ctypes.c_int32(-7)
    assert _lib.load().d3d_fps_plan(rows, code, ctypes.byref(route), ctypes.byref(cap)) == _lib.OK
    return route.value, cap.value


def fps_boundaries(code):
    """-> [(route, capacity)] of every route below streaming, read from d3d_fps_plan alone"""
    from d3d_amd import _lib
    out, n = [], 1
    while True:
        route, cap = fps_plan_of(n, code)
        if route == _lib.FPS_ROUTE_STREAM:
            return out
        out.append((route, cap))
        n = cap + 1
