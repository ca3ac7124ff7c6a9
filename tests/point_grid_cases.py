"""Seeded scenes for PointGrid and the grid routes of ball_query / knn_query.  Every scene is float64 numpy here; a test casts it to
the dtype it runs.  All of them hold at most 4096 rows."""
import numpy as np

import point_knn_cases
import point_sample_cases

CLUSTERS = (63, 64, 65, 255, 256, 257)        # candidate counts around the tile (64) and the round of four tiles (256)


def _scene(name, points, centers, radius, cell_sizes, poffs=None, coffs=None, cap=2.0):
    return dict(name=name, points=np.asarray(points, np.float64), centers=np.asarray(centers, np.float64), radius=float(radius),
                cell_sizes=tuple(float(c) for c in cell_sizes), poffs=poffs, coffs=coffs, cap=cap)


def _outside(lo, hi, by):
    """six centres outside the box lo .. hi, one beyond each face"""
    mid = (lo + hi) / 2
    out = []
    for a in range(3):
        for side in (lo[a] - by, hi[a] + by):
            c = mid.copy()
            c[a] = side
            out.append(c)
    return np.array(out)


def scenes():
    """-> [dict(name, points, centers, radius, cell_sizes, poffs, coffs, cap)]"""
    rng = np.random.default_rng(41)
    out = []
    # a lattice on steps of 1/4, r = 1/2: rows at exactly r (outside), and with cell_size = r, r / 2 and 6 r rows exactly on cell
    # faces (lo is a lattice point); 0.4 r puts the faces between the rows
    lat = point_sample_cases._lattice(rng, 9, 8, 5) * 0.25
    r = 0.5
    ctr = np.concatenate([lat[rng.choice(len(lat), 30, replace=False)], lat[:6] + 0.125, _outside(lat.min(0), lat.max(0), 0.25),
                          _outside(lat.min(0), lat.max(0), 3.0)])
    out.append(_scene("lattice", lat, ctr, r, (r, r / 2, 0.4 * r, 6 * r)))
    out.append(_scene("one_point", [[1.0, 2.0, 3.0, 9.0]], [[1.0, 2.0, 3.0], [1.25, 2.0, 3.0], [1.5, 2.0, 3.0], [-4.0, 0.0, 0.0]], 0.5, (0.5, 4.0)))
    same = np.tile(np.array([[3.0, -7.0, 11.0]]), (70, 1))
    out.append(_scene("identical", same, [[3.0, -7.0, 11.0], [3.0, -7.0, 11.25], [3.0, -7.0, 12.0], [40.0, 0.0, 0.0]], 0.5, (0.5, 0.125)))
    # 50 rows over 200 units with cells of 1/2: the cap (100 cells) forces h up
    out.append(_scene("capped", np.round(rng.uniform(-100, 100, (50, 3)) * 4) / 4, np.round(rng.uniform(-110, 110, (24, 3)) * 4) / 4, 30.0, (0.5,)))
    bad = point_sample_cases._with_nonfinite(rng, point_sample_cases._lidar(rng, 300))
    ctr = np.concatenate([bad[:3, :3], point_sample_cases._lidar(rng, 20, 3), [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.inf, 0, 1]]])
    out.append(_scene("nonfinite", bad, ctr, 20.0, (20.0, 7.0)))
    huge = [s for s in point_knn_cases.scenes() if s[0] == "huge"][0]
    out.append(_scene("huge", huge[1], huge[2], 3.0, (1.0,)))                      # fp32: q overflows, the cap doubles h sixty times
    far = 1e6 + rng.uniform(0, 1e-3, (400, 3))
    out.append(_scene("far", far, np.concatenate([far[:20], far[20:30] + 1e-4, [[1e6, 1e6, 1e6 - 1.0]]]), 2e-4, (2e-4, 1e-4)))
    # a ragged batch: an empty segment, one of rows that are not finite only, and segments of different extent (different h)
    sizes, counts = [120, 0, 9, 300, 40], [7, 3, 4, 9, 5]
    parts = [point_sample_cases._lidar(rng, 120), np.zeros((0, 4)), np.full((9, 4), np.nan), point_sample_cases._lidar(rng, 300) * 8,
             point_sample_cases._lidar(rng, 40) / 16]
    parts[2][::2] = [np.inf, 0.0, 1.0, 0.0]
    parts[2][1::2, 1:] = 0.0
    cparts = [parts[0][:7, :3] + 0.5, point_sample_cases._lidar(rng, 3, 3), point_sample_cases._lidar(rng, 4, 3), parts[3][:9, :3] - 1.0,
              parts[4][:5, :3]]
    poffs, coffs = np.concatenate([[0], np.cumsum(sizes)]).tolist(), np.concatenate([[0], np.cumsum(counts)]).tolist()
    out.append(_scene("ragged", np.concatenate(parts), np.concatenate(cparts), 9.0, (9.0, 3.0), poffs, coffs))
    # clusters of 63 .. 257 rows, each inside one ball and (with cells of 4, counted from the lone row at -6: a cluster at 16 i lies at 16 i + 6 +- 1/4, in the middle of cell 4 i + 1) inside one cell
    pts, ctr = [np.array([[-6.0, -6.0, -6.0]])], []
    for i, size in enumerate(CLUSTERS):
        at = np.array([16.0 * i, 4.0 * (i % 2), 0.0])
        pts.append(at + np.round(rng.uniform(-0.25, 0.25, (size, 3)) * 64) / 64)
        ctr.append(at)
    out.append(_scene("clusters", rng.permutation(np.concatenate(pts)), ctr, 0.5, (4.0, 0.5)))
    return out


def borrowed_ball_scenes():
    """the ball scenes of point_sample_cases as grid scenes: cells of r and of r / 3"""
    return [_scene("ball_" + name, pts, ctr, r, (float(r), float(r) / 3), poffs, coffs) for name, pts, ctr, r, poffs, coffs
            in point_sample_cases.ball_scenes()]


def borrowed_knn_scenes():
    """the kNN scenes of point_knn_cases (tie lattices, ascending / descending distance, fewer rows than k, ragged) as grid scenes"""
    return [_scene("knn_" + name, pts, ctr, 1.0, (1.0, 0.37), poffs, coffs) for name, pts, ctr, poffs, coffs in point_knn_cases.scenes()]
