"""Scenes of the centre-head tests, shared by test_center.py (the numpy models against independent formulations, no GPU) and
test_gpu_center.py (the kernels against the models).  Everything is generated from fixed seeds."""
import numpy as np

PEAK_SHAPES = ((1, 1, 1, 1), (1, 2, 1, 70), (1, 2, 70, 1), (2, 3, 37, 53), (2, 4, 128, 160))
PEAK_KS = (1, 7, 64, 65, 500, 4096)
KERNELS = (1, 3, 5, 7)


def _f32_from_bits(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def peak_scenes(shape, seed=0):
    """name -> float32 [B, C, H, W].  `tie_free` says which scenes have no two equal values among their finite cells."""
    rng = np.random.default_rng(1000 + seed + sum(shape))
    n = int(np.prod(shape))
    b, c, h, w = shape
    out = {}
    # distinct values in random positions: logits in (-6, 6)
    out["random"] = (rng.permutation(n).astype(np.float64) / n * 12 - 6).astype(np.float32).reshape(shape)
    # eight levels: ties everywhere, plateaus of equal neighbours
    out["plateaus"] = (rng.integers(0, 8, shape) / 8).astype(np.float32)
    # every cell a tie: the k-th rank is decided by the flat index alone
    out["constant"] = np.full(shape, 0.5, np.float32)
    out["three_values"] = rng.choice(np.array([-1.0, 0.25, 3.0], np.float32), shape)
    # 1 + j * 2^-23, j < 2048: every key shares its top 12 bits; j < 256: its top 24 bits
    out["top12_shared"] = _f32_from_bits(0x3f800000 + rng.integers(0, 2048, shape)).copy()
    out["top24_shared"] = _f32_from_bits(0x3f800000 + rng.integers(0, 256, shape)).copy()
    # NaN poisons its window; +inf and -inf are values; -0.0 beside +0.0 are equal
    special = out["random"].copy().reshape(-1)
    pick = rng.permutation(n)
    m = max(n // 50, 1)
    special[pick[:m]] = np.nan
    special[pick[m:2 * m]] = np.inf
    special[pick[2 * m:3 * m]] = -np.inf
    special[pick[3 * m:5 * m]] = -0.0
    special[pick[5 * m:7 * m]] = 0.0
    out["special"] = special.reshape(shape)
    zeros = np.where(rng.integers(0, 2, shape) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    out["signed_zeros"] = zeros
    # a peak in every corner and on every border of every plane, nothing inside
    borders = np.full(shape, -2.0, np.float32)
    for y in sorted({0, h // 2, h - 1}):
        for x in sorted({0, w // 2, w - 1}):
            if y in (0, h - 1) or x in (0, w - 1):
                borders[:, :, y, x] = 1.0 + (y * w + x) / 4096.0 + np.arange(c, dtype=np.float32)[None, :] / 8
    out["borders"] = borders
    return out


TIE_FREE = ("random",)


# ---------------------------------------------------------------- circle NMS
def circle_lattice(n, dtype, seed=0, side=None, levels=None):
    """n centres on an integer lattice of side x side cells (every d2 is exact; duplicates and rows exactly at the threshold 4.0 are
    common) in [n, 4] rows, and scores: distinct (levels None) or on `levels` values (ties)"""
    rng = np.random.default_rng(2000 + seed + n)
    side = side or max(4, int(np.sqrt(n)) + 1)
    rows = rng.integers(0, side, (n, 4)).astype(dtype)
    if levels:
        scores = (rng.integers(0, levels, n) / levels).astype(dtype)
    else:
        scores = (rng.permutation(n).astype(np.float64) / max(n, 1)).astype(dtype)
    return rows, scores


def circle_chain(dtype, first_rank):
    """ranks first_rank, +1, +2 lie 1.5 apart on a line: A suppresses B, B alone would suppress C, so C is kept (t = 2.25).  130 rows,
    all others 100 apart; scores descending by row, so rank == row.  -> (centers [130, 2], scores, t, the expected keep)"""
    n = 130
    centers = np.stack([np.arange(n) * 100.0, np.full(n, 1000.0)], 1)
    a = first_rank
    centers[a], centers[a + 1], centers[a + 2] = (0.0, 0.0), (1.5, 0.0), (3.0, 0.0)
    scores = (n - np.arange(n)).astype(dtype)
    keep = np.ones((n,), bool)
    keep[a + 1] = False
    return centers.astype(dtype), scores, 2.25, keep


# ---------------------------------------------------------------- drawing
DRAW_SHAPE = (3, 3, 37, 53)


def draw_scenes():
    """name -> (centers [M, 2] int64 (x, y), radii [M], classes [M], offsets [B + 1]) on DRAW_SHAPE"""
    b, c, h, w = DRAW_SHAPE
    rng = np.random.default_rng(3000)

    def scene(rows, offsets):
        rows = np.asarray(rows, np.int64).reshape(-1, 4)
        return rows[:, :2].copy(), rows[:, 2].copy(), rows[:, 3].copy(), list(offsets)

    out = {}
    out["no_boxes"] = scene([], [0, 0, 0, 0])
    # sample 1 is empty, class 1 is unused; r = 0; one centre with two radii; overlaps inside one class and across two
    out["basics"] = scene([(10, 10, 0, 0), (20, 12, 3, 0), (20, 12, 6, 0), (24, 14, 4, 0), (24, 14, 4, 2), (26, 15, 5, 2),
                           (30, 30, 2, 2), (5, 30, 7, 0)], [0, 7, 7, 8])
    # windows clipped at every border and corner; centres outside the map whose windows reach in, and some that do not
    out["clipped"] = scene([(0, 0, 4, 0), (w - 1, 0, 4, 1), (0, h - 1, 4, 2), (w - 1, h - 1, 4, 0), (w // 2, 0, 5, 1), (w // 2, h - 1, 5, 1),
                            (0, h // 2, 5, 2), (w - 1, h // 2, 5, 2), (-3, 10, 5, 0), (w + 2, 20, 4, 1), (25, -2, 3, 2), (25, h + 4, 6, 0),
                            (-6, -6, 8, 1), (-10, 10, 5, 0), (w + 9, 9, 9, 2), (-2 ** 31, 5, 4095, 0), (2 ** 31 - 1, 2 ** 31 - 1, 4095, 1),
                            (2 ** 40, -2 ** 40, 7, 2)], [0, 8, 14, 18])
    out["whole_map"] = scene([(w // 2, h // 2, 60, 1), (3, 3, 4095, 2), (40, 20, 2, 1)], [0, 1, 3, 3])
    many = np.concatenate([rng.integers(-4, w + 4, (300, 1)), rng.integers(-4, h + 4, (300, 1)), rng.integers(0, 9, (300, 1)),
                           rng.integers(0, c, (300, 1))], 1)
    few = np.concatenate([rng.integers(0, w, (5, 1)), rng.integers(0, h, (5, 1)), rng.integers(0, 4, (5, 1)), rng.integers(0, c, (5, 1))], 1)
    out["many"] = scene(np.concatenate([few, many]), [0, 5, 305, 305])
    return out
