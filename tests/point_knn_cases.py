"""Seeded scenes for knn_query and point_interpolate.  Every scene is float64 numpy here; a test casts it to the dtype it runs.
Where ties matter the coordinates are integers with |x| <= 1000 (3 * 2000^2 < 2^24) or multiples of 1/64 with |x| <= 8
(3 * (16 * 64)^2 < 2^24 in units of 1/4096): every q is exact in fp32, so equal distances are equal bits."""
import numpy as np

TILE, ROUND = 64, 256                # rows per tile of a wavefront's walk, rows per round of four tiles


def _lattice(rng, nx, ny, nz, scale=1):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return rng.permutation(g * scale - np.array([nx // 2, ny // 2, nz // 2]) * scale)


def _fine(rng, n, d=3):
    """multiples of 1/64 in [-8, 8]"""
    return rng.integers(-512, 513, (n, d)).astype(np.float64) / 64


def _by_distance(pts, centre, descending):
    d = ((pts[:, :3] - centre) ** 2).sum(1)
    order = np.argsort(d, kind="stable")
    return pts[order[::-1] if descending else order]


def exact_scenes():
    """-> [(name, points, centers, point_offsets, center_offsets)]: finite coordinates, every q exact in fp32 -- for the brute force"""
    rng = np.random.default_rng(21)
    lat = _lattice(rng, 7, 6, 5)
    out = [("lattice", lat, lat[rng.choice(len(lat), 23, replace=False)], None, None),                 # many equal q
           ("lattice_off_centre", _lattice(rng, 5, 5, 4, 250), rng.integers(-1000, 1001, (9, 3)).astype(np.float64), None, None),
           ("duplicates", np.repeat(rng.integers(-20, 21, (90, 4)).astype(np.float64), 3, axis=0), rng.integers(-20, 21, (11, 3)).astype(np.float64),
            None, None),
           ("identical", np.tile(np.array([[3.0, -7.0, 11.0]]), (150, 1)), np.array([[3.0, -7.0, 11.0], [3.0, -7.0, 12.0]]), None, None)]
    cloud = _fine(rng, 700)
    centre = np.array([0.25, -0.5, 1.0])
    out.append(("descending", _by_distance(cloud, centre, True), centre[None], None, None))            # every row inserts
    out.append(("ascending", _by_distance(cloud, centre, False), centre[None], None, None))            # none after the first k
    out.append(("fewer_than_k", _fine(rng, 2), _fine(rng, 5), None, None))
    # a ragged batch of 5 segments whose sizes straddle the tile and the round; one has no rows but has centres
    sizes = [TILE - 1, 0, TILE + 1, ROUND, ROUND + TILE + 1]
    counts = [5, 3, 1, 6, 7]
    out.append(("ragged", _fine(rng, sum(sizes), 4), _fine(rng, sum(counts)), np.concatenate([[0], np.cumsum(sizes)]).tolist(),
                np.concatenate([[0], np.cumsum(counts)]).tolist()))
    out.append(("empty_segment", _fine(rng, 40), _fine(rng, 6), [0, 0, 40], [0, 4, 6]))
    return out


def scenes():
    """exact_scenes and the ones with values that are not finite"""
    rng = np.random.default_rng(22)
    out = exact_scenes()
    bad = _fine(rng, 300, 4)
    rows = [0] + sorted(rng.choice(np.arange(1, 300), 8, replace=False).tolist())
    for i, r in enumerate(rows):                         # NaN, +inf and -inf in each of the three columns, the first row among them
        bad[r, i % 3] = [np.nan, np.inf, -np.inf][(i // 3) % 3]
    ctr = np.concatenate([_fine(rng, 12), [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]])          # (inf - inf: NaN, no candidate)
    out.append(("nonfinite", bad, ctr, None, None))
    out.append(("nan_centre", _fine(rng, 70), np.array([[0.0, np.nan, 0.0], [np.nan] * 3, [1.0, 2.0, 3.0]]), None, None))
    huge = rng.uniform(1.5e19, 2e19, (200, 3)) * rng.choice([-1.0, 1.0], (200, 3))      # fp32: q overflows to +inf against a small centre: a candidate that sorts last (by row)
    huge[::3] = _fine(rng, 67)
    out.append(("huge", huge, np.concatenate([_fine(rng, 4), [[1e19, -1e19, 1e19]]]), None, None))
    return out
