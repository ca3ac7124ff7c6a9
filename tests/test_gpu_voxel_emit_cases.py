"""GPU: the dense contract's one-launch output kernels (k_emit on the pooled and resident routes, k_emit_split on the fresh-tensor
route) at the smallest sizes where each of their paths can go wrong, bit-exact against the oracle.  A wavefront of the output launch
owns 64 consecutive point indices and the voxels whose first point lies among them, so every case is a point ORDER: which of 64
indices start a voxel, how many rows those voxels keep, which of them carry a record (255 points and more).  Grid [15, 9, 5] on
bounds whose cell sizes in x and y (7/15, 0.6) are no powers of two; a few hundred to a few thousand points per case."""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_voxel import _np, check_dense

pytestmark = pytest.mark.gpu

BOUNDS = [0, 7, -3, 2.4, -1, 1.5]
SHAPE = [15, 9, 5]
NCELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
_cache = {}


def _points(cells, seed):
    """one point per entry of `cells` (linear cell numbers, x-major as the kernels' keys), well inside its cell, random intensity"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, dtype=np.int64)
    idx = np.stack([cells // (SHAPE[1] * SHAPE[2]), (cells // SHAPE[2]) % SHAPE[1], cells % SHAPE[2]], 1).astype(np.float64)
    lo = np.array(BOUNDS[0::2], dtype=np.float64)
    size = (np.array(BOUNDS[1::2], dtype=np.float64) - lo) / np.array(SHAPE, dtype=np.float64)
    xyz = lo + (idx + rng.uniform(0.2, 0.8, idx.shape)) * size
    return np.ascontiguousarray(np.concatenate([xyz, rng.uniform(-1, 1, (len(cells), 1))], 1), dtype=np.float32)


def _distinct(n, seed):
    return np.random.default_rng(seed).permutation(NCELLS)[:n]


def mixed_cloud(seed, n=3000):
    """40 % of the points uniform over the cells, 50 % in 20 cells (more than 48 points each), 300 in one cell (a record, and more
    than 256 points), in random order"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(NCELLS)
    hot, hottest = cells[:20], cells[20]
    c = np.concatenate([rng.integers(0, NCELLS, int(0.4 * n)), rng.choice(hot, n - int(0.4 * n) - 300), np.full(300, hottest)])
    return _points(rng.permutation(c), seed + 1000)


def record_among_singles():
    """wavefront 0: 64 first points, index 31 starts the cell of 300 points; its other 299 points come behind, then more singles"""
    c = _distinct(130, 11)
    return _points(np.concatenate([c[:64], np.full(299, c[31]), c[64:]]), 12)


def every_voxel_a_record():
    """wavefront 0: the first points of three cells of 300 points each, the rest of its indices and 14 wavefronts more their repeats"""
    c = _distinct(3, 13)
    return _points(np.tile(c, 300), 14)


def rows_in_one_wavefront(rows):
    """indices 0 .. 63 start 64 distinct cells; rows - 64 further points visit the same cells in the same order: the first wavefront's
    voxels keep exactly `rows` rows (max_points 32 and rows <= 2048)"""
    c = _distinct(64, 15)
    return _points(np.concatenate([c, np.resize(c, rows - 64)]), 16 + rows)


def edge_cloud():
    """points on the lower bounds, in the last cell of each axis, just below the upper bounds, -0.0, outside the range, and NaN / inf
    rows between valid ones"""
    f = np.float32
    lo, hi = np.array(BOUNDS[0::2], f), np.array(BOUNDS[1::2], f)
    below = np.nextafter(hi, -np.inf, dtype=f)
    size = (hi - lo) / np.array(SHAPE, f)
    rows = [lo, below, hi, np.array([-0.0, lo[1], lo[2]], f), np.array([-0.0, 0.0, -0.0], f), hi - size * f(0.5), lo - f(1e-3),
            np.nextafter(lo, -np.inf, dtype=f), np.array([lo[0], below[1], lo[2]], f), np.array([below[0], lo[1], below[2]], f),
            np.array([3.0, 0.0, 0.0], f), np.array([100.0, 0.0, 0.0], f), np.array([3.0, -50.0, 0.0], f), np.array([3.0, 0.0, 9.0], f)]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            r = np.array([3.0, 0.0, 0.0], f)
            r[axis] = bad
            rows.append(r)
    special = np.concatenate([np.stack(rows), np.arange(len(rows), dtype=f)[:, None] / f(8)], 1).astype(f)
    valid = _points(np.random.default_rng(17).integers(0, NCELLS, 400), 18)
    out = np.empty((len(valid) + 4 * len(special), 4), f)             # every special row four times, every fifth row
    out[:] = np.nan
    k = np.arange(4 * len(special)) * 5 + 2
    k = k[k < len(out)]
    keep = np.ones(len(out), bool)
    keep[k] = False
    out[k] = np.resize(special, (len(k), 4))
    out[keep] = np.resize(valid, (int(keep.sum()), 4))
    return out


CASES = {}
for P in (16, 32, 256):
    CASES["record among singles, P=%d" % P] = (record_among_singles, dict(max_points=P, max_voxels=5000, reduction="mean"))
CASES["no record in the cloud"] = (lambda: _points(np.random.default_rng(19).integers(0, NCELLS, 1500), 20),
                                   dict(max_points=32, max_voxels=5000, reduction="mean"))
CASES["every voxel of a wavefront has a record"] = (every_voxel_a_record, dict(max_points=32, max_voxels=5000, reduction="mean"))
# 64 / 65 and 256 / 257 rows: one and two trips of the row loops, the buffer full and one row over; 64 first rows + 0, 1, 64, 65
# rows of rank 1 and more (64, 65, 128, 129); 2048: 64 voxels of 32 rows, eight batches
for rows in (64, 65, 128, 129, 256, 257, 2048):
    CASES["%d rows in one wavefront" % rows] = (lambda rows=rows: rows_in_one_wavefront(rows),
                                                dict(max_points=32, max_voxels=5000, reduction="mean"))
for mv in (10, 37, 64, 65):
    CASES["max_voxels=%d" % mv] = (lambda: mixed_cloud(21, 1200), dict(max_points=32, max_voxels=mv, reduction="mean"))
CASES["edge coordinates"] = (edge_cloud, dict(max_points=32, max_voxels=5000, reduction="mean"))
for red in (None, "mean", "max", "min"):
    for P in (16, 32, 48, 256):
        CASES["reduction=%s, P=%d" % (red, P)] = (lambda: mixed_cloud(23), dict(max_points=P, max_voxels=5000, reduction=red))


def cloud(name):
    if ("cloud", name) not in _cache:
        _cache[("cloud", name)] = CASES[name][0]()
    return _cache[("cloud", name)]


def other_cloud():
    """the frame between two frames of a case: other cells, other counts, so voxel ids change hands and rows go stale"""
    if "other" not in _cache:
        _cache["other"] = mixed_cloud(29, 2000)
    return _cache["other"]


def expected(name, which):
    """the oracle's result, computed once per (case, cloud)"""
    kw = CASES[name][1]
    key = ("exp", which if which == "case" else "other", name if which == "case" else tuple(sorted(kw.items(), key=str)))
    if key not in _cache:
        _cache[key] = oracle.VoxelGenerator(BOUNDS, SHAPE, dense=True, **kw)(cloud(name) if which == "case" else other_cloud())
    return _cache[key]


@pytest.mark.parametrize("resident", [None, True, False], ids=["pooled", "resident", "fresh"])
@pytest.mark.parametrize("name", list(CASES))
def test_emit_case(name, resident):
    from d3d_amd.voxel import VoxelGenerator
    kw = CASES[name][1]
    gen = VoxelGenerator(BOUNDS, SHAPE, dense=True, resident=resident, **kw)
    frames = {"case": torch.from_numpy(cloud(name)).cuda(), "other": torch.from_numpy(other_cloud()).cuda()}
    for which in ("case", "other", "case", "other"):
        got = gen(frames[which], poison=False)
        check_dense(_np(got), expected(name, which), kw["max_points"])
        del got                                           # (the pooled route reuses its buffer only when the result is gone)
    if resident is None:
        assert gen._pool_stats == dict(pooled=4, second=0, fresh=0)


def test_the_cases_are_what_they_claim():
    """the constructions above, checked on the oracle's own numbers (no GPU result involved)"""
    exp = expected("record among singles, P=32", "case")
    assert exp["voxel_npoints"][31] == 300 and np.all(np.delete(exp["voxel_npoints"], 31) == 1) and len(exp["coords"]) == 130
    exp = expected("every voxel of a wavefront has a record", "case")
    assert exp["voxel_npoints"].tolist() == [300, 300, 300]
    for rows in (64, 65, 128, 129, 256, 257, 2048):
        exp = expected("%d rows in one wavefront" % rows, "case")
        assert len(exp["coords"]) == 64 and int(np.minimum(exp["voxel_npoints"], 32).sum()) == rows
    for mv in (10, 37, 64, 65):
        assert len(expected("max_voxels=%d" % mv, "case")["coords"]) == mv
    exp = expected("edge coordinates", "case")
    top = np.array(SHAPE) - 1
    assert (exp["coords"] == 0).all(1).any() and (exp["coords"] == top).all(1).any()
    n = exp["voxel_npoints"].sum()
    c = cloud("edge coordinates")
    assert n < len(c) and not np.isfinite(c).all()
    counts = expected("reduction=mean, P=256", "case")["voxel_npoints"]
    assert counts.max() >= 300 and (counts > 48).sum() >= 20 and (counts == 1).sum() > 50
