"""Scenes for the RoI pooling operators (RoiGrid, roiaware_pool3d, roipoint_pool3d): clouds and boxes planted where the table kernel of
csrc/roipool.hip can go wrong -- the seams of its plan (tile, slab, round), the cap, cells that fill from several slabs, faces and
corners, rows and boxes that are not finite.  Data only: tests/test_roi_pool.py holds every scene against the property it exists
for without a GPU, tests/test_gpu_roi_pool.py runs the kernels on them.  Everything is fp32; every generator is seeded.

A scene is a namespace: points [N, D], boxes [M, 7], out_size, max_points (P), point_offsets / box_offsets (lists or None)."""
import types

import numpy as np

import crop_cases
from d3d_amd.point import roi_grid_plan

F = np.float32
CAR = np.array([4.2, 1.8, 1.6])


def scene(points, boxes, out_size, max_points, point_offsets=None, box_offsets=None):
    return types.SimpleNamespace(points=np.ascontiguousarray(points, F), boxes=np.ascontiguousarray(boxes, F).reshape(-1, 7),
                                 out_size=out_size, max_points=max_points, point_offsets=point_offsets, box_offsets=box_offsets)


def car_boxes(rng, m, rz=None, spread=10.0):
    """m boxes of about a car's size inside a square of 2 * spread; rz: one angle for all, None: any angle in +-3.1"""
    ang = rng.uniform(-3.1, 3.1, m) if rz is None else np.full(m, rz)
    return np.concatenate([rng.uniform(-spread, spread, (m, 2)), rng.uniform(-1.0, 0.0, (m, 1)), CAR * rng.uniform(0.9, 1.1, (m, 3)),
                           ang[:, None]], 1).astype(F)


def plant(rng, boxes, k, spread=1.1):
    """k points, each uniform in one of the boxes scaled by `spread` (1.1: a tenth of them just outside)"""
    b = np.asarray(boxes, np.float64)[rng.integers(0, len(boxes), k)]
    loc = (rng.random((k, 3)) - 0.5) * spread * b[:, 3:6]
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    return np.stack([b[:, 0] + c * loc[:, 0] - s * loc[:, 1], b[:, 1] + s * loc[:, 0] + c * loc[:, 1], b[:, 2] + loc[:, 2]], 1).astype(F)


def random_scene(n, m, seed, rz=None, d=3, out_size=12, max_points=128, spread=10.0):
    """half of the points planted in the boxes, half anywhere in the square, shuffled; d - 3 further columns of noise"""
    rng = np.random.default_rng(seed)
    boxes = car_boxes(rng, m, rz, spread)
    k = n // 2 if m else 0
    fill = np.concatenate([rng.uniform(-spread - 3, spread + 3, (n - k, 2)), rng.uniform(-2.5, 1.5, (n - k, 1))], 1).astype(F)
    xyz = np.concatenate([plant(rng, boxes, k) if k else np.zeros((0, 3), F), fill], 0)[rng.permutation(n)]
    return scene(np.concatenate([xyz, rng.random((n, d - 3)).astype(F)], 1), boxes, out_size, max_points)


RANDOM_SCENES = {"r_small": (300, 5, 11), "r_mid": (1500, 16, 12), "r_big": (4096, 32, 13)}


def lattice_scene(n=600, seed=5):
    """rz = 0, box centres and extents such that every expression of the rule is exact: points on a 1/4 lattice (faces, edges and
    corners of the boxes among them, and duplicates), two overlapping boxes of 4 x 2 x 2 cells"""
    rng = np.random.default_rng(seed)
    boxes = np.array([[1, -2, 0.5, 8, 4, 2, 0], [3, -1, 0, 4, 8, 4, 0]], F)
    pts = np.stack([rng.integers(-16, 28, n), rng.integers(-24, 16, n), rng.integers(-10, 10, n)], 1) / 4.0
    pts[:8] = [[-3, -4, -0.5], [5, 0, 1.5], [5, -4, 1.5], [1, -2, 0.5], [1, 3, 2], [5, 3, -2], [-3, 0, 0.5], [5.25, 0, 0.5]]
    return scene(pts, boxes, (4, 2, 2), 4)


def cap_scene(p=5, seed=6):
    """one box of 2 x 2 x 2 cells: cell 0 holds exactly P members, cell 7 holds P + 1, the others a few; far points between them"""
    rng = np.random.default_rng(seed)
    box = np.array([[0, 0, 0, 4, 4, 4, 0]], F)
    lo = rng.uniform(-1.9, -0.1, (p, 3))
    hi = rng.uniform(0.1, 1.9, (p + 1, 3))
    other = rng.uniform(-1.9, 1.9, (30, 3))
    other = other[~((other < 0).all(1) | (other > 0).all(1))]                     # neither cell 0 nor cell 7
    pts = np.concatenate([lo, hi, other, rng.uniform(5, 9, (20, 3))])
    return scene(pts[rng.permutation(len(pts))], box, 2, p)


def overlap_scene(n=400, seed=7):
    """three boxes around one centre at different angles (the points near the centre lie in all three), a fourth far away, empty"""
    rng = np.random.default_rng(seed)
    boxes = np.array([[0, 0, 0, 4.2, 1.8, 1.6, 0.0], [0.1, 0.05, 0, 4.0, 1.9, 1.5, 0.7], [-0.1, 0, 0.1, 4.4, 1.7, 1.7, -1.2],
                      [100, 100, 0, 4, 2, 1.5, 0.3]], F)
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (n // 2, 3)), rng.uniform(-3, 3, (n - n // 2, 3))])[rng.permutation(n)]
    return scene(pts, boxes, 3, 64)


def _one_box():
    return np.array([[2, -1, 0, 4, 2, 2, 0.4]], F)


def _far(rng, n):
    return rng.uniform(20, 40, (n, 3))


def seam_scene(n=4096, seed=8):
    """one box; the only members are copies of ONE point (one cell) in the last row of slab k and the first row of slab k + 1, for
    every slab seam of the plan inside the segment, the seam between the two rounds among them: the cell's members straddle every seam"""
    rng = np.random.default_rng(seed)
    _, slab, _ = roi_grid_plan(n, 8)
    pts = _far(rng, n)
    for s in range(slab, n, slab):
        pts[s - 1] = pts[s] = [2.5, -0.75, 0.25]
    return scene(pts, _one_box(), 2, 16)


def one_cell_tile_scene(seed=9):
    """256 rows: the 64 rows of the second tile are copies of one point -- all lanes of that tile fall into one cell; members of
    other cells before and after"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([plant(rng, _one_box(), 64, 0.9), np.tile(F([2.5, -0.75, 0.25]), (64, 1)), plant(rng, _one_box(), 128, 0.9)])
    return scene(pts, _one_box(), 2, 128)


def two_cells_scene(seed=10):
    """192 rows that alternate between two points of two different cells, then 64 rows anywhere in the box"""
    rng = np.random.default_rng(seed)
    a, b = F([2.5, -0.75, 0.25]), F([1.2, -1.3, -0.5])
    pts = np.concatenate([np.stack([a, b] * 96), plant(rng, _one_box(), 64, 0.9)])
    return scene(pts, _one_box(), 2, 40)


def early_cap_scene(seed=14):
    """4096 rows (two rounds), P = 2, 2 x 1 x 1 cells: cell 0 gets three members inside the FIRST slab and more in later slabs and in
    the second round (its cap is reached before the first seam); cell 1 gets one member in the first slab, its second in the third,
    more in the fourth and in the second round"""
    rng = np.random.default_rng(seed)
    _, slab, rnd = roi_grid_plan(4096, 2)
    pts = _far(rng, 4096)
    left, right = [1.0, -1.2, 0.0], [3.0, -0.8, 0.0]
    for r in (5, 9, slab - 1, slab + 2, 2 * slab + 7, 1023, rnd + 3, 4095):
        pts[r] = left
    for r in (70, 2 * slab + 1, 3 * slab, rnd + slab):
        pts[r] = right
    return scene(pts, _one_box(), (2, 1, 1), 2)


def overflow_scene(seed=15):
    """4096 rows, all inside one large box: every row of every slab is a member -- the slabs' queues are full to the last entry in
    both rounds -- and 27 cells of 128 slots cannot hold them"""
    rng = np.random.default_rng(seed)
    box = np.array([[0, 0, 0, 40, 40, 8, 0.3]], F)
    return scene(plant(rng, box, 4096, 0.95), box, 3, 128)


def copies_scene(seed=16):
    """32 copies of one box over a cloud of 1000 rows"""
    sc = random_scene(1000, 1, seed, out_size=4, max_points=16, spread=3.0)
    return scene(sc.points, np.tile(sc.boxes, (32, 1)), 4, 16)


def duplicates_scene(seed=17):
    """every point four times, in a row"""
    sc = random_scene(200, 6, seed, out_size=3, max_points=8, spread=5.0)
    return scene(np.repeat(sc.points, 4, 0), sc.boxes, 3, 8)


def nonfinite_points_scene(seed=18):
    """a random scene with rows spoiled at the centre of box 0: NaN in x, y, z (the NaN z row is INSIDE for crop_points), +-inf"""
    sc = random_scene(500, 6, seed, out_size=3, max_points=32, spread=5.0)
    pts, b0 = sc.points.copy(), sc.boxes[0]
    bad = [(np.nan, b0[1], b0[2]), (b0[0], np.nan, b0[2]), (b0[0], b0[1], np.nan), (np.inf, b0[1], b0[2]), (-np.inf, b0[1], b0[2]),
           (b0[0], np.inf, b0[2]), (b0[0], b0[1], np.inf), (b0[0], b0[1], -np.inf), (np.nan, np.nan, np.nan)]
    rows = np.arange(3, 3 + 7 * len(bad), 7)
    pts[rows] = np.array(bad, F)
    sc.points, sc.nan_z_row = pts, int(rows[2])
    return sc


def bad_boxes_scene(seed=19):
    """a random scene whose boxes are followed by rows with a NaN field, with zero, negative and infinite extents, and by the
    zero-extent rows of crop_cases with points at their centre"""
    sc = random_scene(600, 4, seed, out_size=2, max_points=16, spread=5.0)
    good = sc.boxes[0]
    rows = [good.copy() for _ in range(8)]
    rows[0][0] = np.nan
    rows[1][2] = np.nan
    rows[2][3] = np.nan
    rows[3][5] = np.nan
    rows[4][3] = 0
    rows[5][4] = -1.5
    rows[6][5] = 0
    rows[7][3] = np.inf
    zero = crop_cases._scene_boxes("zero_extent")[0]
    pts = sc.points.copy()
    pts[:4] = [12.5, -7.25, -0.5]
    pts[4:8, :3] = good[:3]
    sc.boxes = np.concatenate([sc.boxes, np.array(rows, F), zero]).astype(F)
    sc.points = pts
    return sc


def faces_scene(seed=20):
    """corners, edge midpoints and the centres of the top and bottom faces of every box, and each of them one fp32 step outward"""
    sc = random_scene(256, 8, seed, out_size=4, max_points=16, spread=6.0)
    sc.boxes[0, 6], sc.boxes[1, 6], sc.boxes[2, 6] = 0, np.pi / 2, np.pi
    qx, qy = crop_cases.corners(sc.boxes)
    extra = []
    for i, b in enumerate(sc.boxes):
        top, bot = b[2] + b[5] / F(2), b[2] - b[5] / F(2)
        for e in range(4):
            mx, my = (qx[i, e] + qx[i, (e + 1) & 3]) / F(2), (qy[i, e] + qy[i, (e + 1) & 3]) / F(2)
            extra += [(qx[i, e], qy[i, e], b[2]), (qx[i, e], qy[i, e], top), (qx[i, e], qy[i, e], bot), (mx, my, b[2]), (mx, my, top)]
        extra += [(b[0], b[1], top), (b[0], b[1], bot), (b[0], b[1], np.nextafter(top, F(np.inf))), (b[0], b[1], np.nextafter(bot, F(-np.inf)))]
    sc.points = np.concatenate([sc.points, np.array(extra, F)]).astype(F)
    return sc


def ragged_scene(seed=21):
    """three segments, the middle one without points (its boxes stay empty); boxes of a segment see its own points only"""
    parts = [random_scene(300, 3, seed, out_size=3, max_points=8, spread=4.0), random_scene(0, 2, seed + 1, spread=4.0),
             random_scene(500, 4, seed + 2, spread=4.0)]
    poffs = np.cumsum([0] + [len(p.points) for p in parts]).tolist()
    boffs = np.cumsum([0] + [len(p.boxes) for p in parts]).tolist()
    return scene(np.concatenate([p.points for p in parts]), np.concatenate([p.boxes for p in parts]), 3, 8, poffs, boffs)


def angle_scenes():
    """-> [(name, scene)]: all boxes at rz = 0, +-pi / 2, pi, and at any angle"""
    out = []
    for k, (name, rz) in enumerate((("rz0", 0.0), ("rz+90", np.pi / 2), ("rz-90", -np.pi / 2), ("rz180", np.pi), ("generic", None))):
        out.append((name, random_scene(700, 8, 30 + k, rz=rz, out_size=(3, 2, 2), max_points=16, spread=5.0)))
    return out


def special_scenes():
    """-> [(name, scene)]: every scene that exists for one property"""
    return [("lattice", lattice_scene()), ("cap", cap_scene()), ("overlap", overlap_scene()), ("seam", seam_scene()),
            ("one_cell_tile", one_cell_tile_scene()), ("two_cells", two_cells_scene()), ("early_cap", early_cap_scene()),
            ("overflow", overflow_scene()), ("copies", copies_scene()), ("duplicates", duplicates_scene()),
            ("nonfinite_points", nonfinite_points_scene()), ("bad_boxes", bad_boxes_scene()), ("faces", faces_scene()),
            ("ragged", ragged_scene())]
