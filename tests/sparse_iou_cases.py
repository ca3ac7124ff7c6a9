"""Seeded scenes for the sparse IoU operators (box2d_iou_sparse / iou3d_sparse), each small (N, M <= 320) and each built to hit one
way the kernels can go wrong; shared by test_sparse_iou_cases.py (the claims, on the oracle alone) and test_gpu_sparse_iou.py.

A scene: name, dims (2: rows (x,y,w,h,r); 3: rows (x,y,z,lx,ly,lz,rz)), b1 [N,cols], b2 [M,cols] as float64 with values that
float32 holds exactly where exactness matters, `stored` (whether the threshold 'one stored value of the scene' is run: not
where all values are equal), and `claims`, what the scene promises -- checked against the oracle without a GPU."""
import numpy as np

THRESHOLDS = (0.0, 0.25, 0.5)
TIE = 1e-9            # an oracle value this close to the threshold (and not 0 == 0) does not decide a pair: a rounding tie
TIE_CAP = 0.01        # of a scene's N * M pairs


def rand2d(n, seed, span, lo=(2.0, 1.0), hi=(6.0, 4.0)):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) * span, rng.random(n) * span, lo[0] + rng.random(n) * (hi[0] - lo[0]),
                     lo[1] + rng.random(n) * (hi[1] - lo[1]), rng.random(n) * 2 * np.pi - np.pi], 1)


def with_z(b, seed, z=None, lz=None):
    rng = np.random.default_rng(seed)
    n = len(b)
    z = rng.random(n) * 2 - 1 if z is None else np.broadcast_to(np.asarray(z, np.float64), (n,))
    lz = rng.random(n) * 2 + 1 if lz is None else np.broadcast_to(np.asarray(lz, np.float64), (n,))
    return np.stack([b[:, 0], b[:, 1], z, b[:, 2], b[:, 3], lz, b[:, 4]], 1)


def _scene(name, dims, b1, b2, stored=True, **claims):
    return dict(name=name, dims=dims, b1=np.ascontiguousarray(b1, np.float64), b2=np.ascontiguousarray(b2, np.float64),
                stored=stored, claims=claims)


def _touching():
    """axis-aligned 2 x 2 squares on even centres; against each: itself moved by one side along x (a shared edge), along x and y (a
    shared corner) and by half a side (a real overlap) -- then ordinary boxes, far from the squares, so that ties stay rare"""
    cx, cy = np.meshgrid(np.arange(4) * 8.0, np.arange(3) * 8.0)
    sq = np.stack([cx.ravel(), cy.ravel(), np.full(12, 2.0), np.full(12, 2.0), np.zeros(12)], 1)
    edge, corner, over = sq.copy(), sq.copy(), sq.copy()
    edge[:, 0] += 2.0
    corner[:, 0] += 2.0
    corner[:, 1] -= 2.0
    over[:, 1] += 1.0
    fill1, fill2 = rand2d(90, 61, 40.0), rand2d(70, 62, 40.0)
    fill1[:, :2] += 100.0
    fill2[:, :2] += 100.0
    return np.concatenate([fill1[:45], sq, fill1[45:]]), np.concatenate([edge, fill2[:35], corner, over, fill2[35:]])


def _degenerate(seed):
    b1, b2 = rand2d(60, seed, 25.0), rand2d(50, seed + 1, 25.0)
    b1[5, 2] = 0.0
    b1[17, 3] = 0.0
    b1[30, 2:4] = 0.0
    b2[3, 3] = 0.0
    b2[44, 2] = 0.0
    b1[41] = np.nan
    b2[20] = np.nan
    return b1, b2


def _gaps():
    """every fifth row sits on a box of b2, the others (the first and the last among them) far away"""
    b2 = rand2d(30, 51, 40.0)
    b1 = rand2d(41, 52, 40.0)
    b1[:, :2] += 500.0
    hit = np.arange(2, 40, 5)
    b1[hit] = b2[hit % 30]
    b1[hit, 0] += 0.25
    return b1, b2, hit


def _dense_row():
    """row 3: one 60 x 60 box over 100 small ones (more than 64 hits inside the first 64-column chunk); the other rows ordinary"""
    b2 = rand2d(100, 41, 30.0, lo=(1.0, 1.0), hi=(3.0, 3.0))
    b2[:, :2] += 15.0
    b1 = rand2d(21, 42, 60.0)
    b1[3] = (30.0, 30.0, 60.0, 60.0, 0.0)
    return b1, b2


def _zcases():
    """BEV footprints that overlap (each b2 row is a b1 row moved a little), z ranges by row group: overlapping, apart, touching"""
    a = rand2d(48, 71, 300.0)
    b = a.copy()
    b[:, 0] += 0.5
    z1 = np.zeros(48)
    z2 = np.where(np.arange(48) % 3 == 0, 0.5, np.where(np.arange(48) % 3 == 1, 7.0, 2.0))      # lz = 2 both: 2.0 apart = touching
    return with_z(a, 0, z1, 2.0), with_z(b, 0, z2, 2.0)


def scenes():
    out = []
    out.append(_scene("odd_130x75", 2, rand2d(130, 11, 40.0), rand2d(75, 12, 40.0), hits=True))
    out.append(_scene("m_below_64", 2, rand2d(70, 13, 30.0), rand2d(37, 14, 30.0), hits=True))
    one = np.array([[15.0, 15.0, 20.0, 18.0, 0.3]])
    # (fewer than 100 pairs: the one pair a stored-value threshold ties with is more than TIE_CAP of them)
    out.append(_scene("m_one", 2, rand2d(50, 15, 30.0), one, stored=False, hits=True))
    out.append(_scene("n_one", 2, one, rand2d(90, 16, 30.0), stored=False, hits=True))
    b1, b2 = _dense_row()
    out.append(_scene("dense_row", 2, b1, b2, hits=True, row_over_64=3))
    box = np.array([[3.0, -2.0, 4.0, 2.5, 0.4]])
    out.append(_scene("all_hit_96x70", 2, np.repeat(box, 96, 0), np.repeat(box, 70, 0), stored=False, all_hit=True))
    far = rand2d(75, 22, 40.0)
    far[:, 0] += 1000.0
    out.append(_scene("apart", 2, rand2d(130, 21, 40.0), far, stored=False, no_hits=True))
    b1, b2, hit = _gaps()
    out.append(_scene("gaps", 2, b1, b2, hits=True, hit_rows=hit))
    b1, b2 = _touching()
    out.append(_scene("touching", 2, b1, b2, hits=True, zero_candidates=24))
    b1, b2 = _degenerate(31)
    out.append(_scene("degenerate", 2, b1, b2, hits=True, dead_rows=(5, 17, 30, 41), dead_cols=(3, 44, 20)))
    # 7 columns
    out.append(_scene("odd3_130x75", 3, with_z(rand2d(130, 11, 40.0), 81), with_z(rand2d(75, 12, 40.0), 82), hits=True))
    out.append(_scene("m_one3", 3, with_z(rand2d(50, 15, 30.0), 83), with_z(one, 84, 0.0, 3.0), stored=False, hits=True))
    b1, b2 = _zcases()
    out.append(_scene("zcases3", 3, b1, b2, hits=True, z_groups=True))
    out.append(_scene("all_hit3_96x70", 3, with_z(np.repeat(box, 96, 0), 0, 0.5, 2.0), with_z(np.repeat(box, 70, 0), 0, 0.75, 1.5),
                      stored=False, all_hit=True))
    out.append(_scene("apart3", 3, with_z(rand2d(130, 21, 40.0), 85), with_z(far, 86), stored=False, no_hits=True))
    b1, b2 = _degenerate(33)
    out.append(_scene("degenerate3", 3, with_z(b1, 87), with_z(b2, 88), hits=True))
    return out


SCENES = scenes()
METHODS = ("box", "rbox")


def model(dense, threshold):
    """the definition on a dense matrix (numpy): pairs [K,2] by row then column, values [K], offsets [N+1]"""
    keep = dense > np.asarray(threshold, dense.dtype)
    pairs = np.argwhere(keep).astype(np.int64)
    offsets = np.zeros(dense.shape[0] + 1, np.int64)
    offsets[1:] = np.cumsum(keep.sum(1))
    return pairs, dense[keep], offsets


def ties(oracle_dense, threshold):
    """bool [N,M]: the oracle's value is within TIE of the threshold and the case is not the exact 0 against threshold 0 (a pair
    whose value is exactly 0 must be absent: no tie)"""
    o = oracle_dense.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(o - threshold) <= TIE) & ~((o == 0) & (threshold == 0))
