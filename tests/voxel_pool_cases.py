"""Scenes for the voxel_pool tests: mappings (voxel id per point, -1 = none) and feature rows, all seeded."""
import numpy as np


def features(k, c, dtype, seed=0):
    """normal rows; every third row on a grid of halves, so that equal values, +0.0 and -0.0 meet inside a voxel"""
    f = np.random.default_rng(1000 + seed).standard_normal((k, c)) * 3
    f[::3] = np.round(f[::3] * 2) / 2
    return f.astype(dtype)


def from_counts(counts, seed=0, unmapped=0):
    """a mapping whose voxel j holds counts[j] points, the points shuffled, `unmapped` ids of -1 among them"""
    m = np.concatenate([np.repeat(np.arange(len(counts), dtype=np.int64), counts), np.full(unmapped, -1, np.int64)])
    np.random.default_rng(seed).shuffle(m)
    return m, len(counts)


def random_mapping(k, v, seed=0, unmapped=0.0):
    r = np.random.default_rng(seed)
    m = r.integers(0, v, k).astype(np.int64)
    if unmapped:
        m[r.random(k) < unmapped] = -1
    return m, v


FAN_IN = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def fan_in_scenes():
    s = {
        "identity": (np.arange(300, dtype=np.int64), 300),
        "reversed": (np.arange(300, dtype=np.int64)[::-1].copy(), 300),
        "crowded": from_counts(FAN_IN, 1),
        "one_voxel_3000": (np.zeros(3000, np.int64), 1),
        "one_of_five_3000": (np.full(3000, 3, np.int64), 5),
        # voxels 0-9, 20-29 and 35-39 without a point
        "empty_runs": from_counts([0] * 10 + [7, 1, 30, 2, 5, 1, 1, 9, 3, 4] + [0] * 10 + [6, 2, 2, 11, 1] + [0] * 5, 2),
        "minus_one_sprinkled": random_mapping(3000, 97, 3, unmapped=0.3),
        "minus_one_only": (np.full(500, -1, np.int64), 13),
    }
    return s


# K: the launch tiles (256 lanes) and the argsort's routes (one workgroup up to 2048 keys, the sample sort up to 131072, radix above)
SIZES_K = (1, 255, 256, 257, 2048, 2049, 4097, 65537, 131072, 131073)
# V: the launch tiles and the offsets scan's (V + 1 items in tiles of 1024, block sums in steps of 4096)
SIZES_V = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537)


def mixed(seed=5):
    """the scene of the channel-count tests: crowded and single voxels, empty ones, unmapped points; K = 2500"""
    return from_counts([300, 0, 1, 64, 65, 0, 0, 2, 1000, 17] + [3] * 300 + [0] * 4, seed, unmapped=151)


def special_values(dtype):
    """-> (f [K, 2], mapping, V): column 0 holds the cases below, column 1 their negation; voxel by voxel
    0: NaN first   1: NaN last   2: NaN alone   3: two NaNs around a number   4: +0.0 then -0.0   5: -0.0 then +0.0
    6: +inf and -inf among numbers   7: equal values   8: only -inf   9: empty"""
    nan, inf = np.nan, np.inf
    rows = [(0, nan), (0, 1.0), (0, -2.0), (1, 3.0), (1, -1.0), (1, nan), (2, nan), (3, nan), (3, 5.0), (3, nan), (4, 0.0), (4, -0.0),
            (5, -0.0), (5, 0.0), (6, 1.0), (6, inf), (6, -inf), (6, 2.0), (7, 4.0), (7, 4.0), (7, 4.0), (8, -inf), (8, -inf)]
    # the voxels interleaved (first points of all voxels, then the second ones, ...): inside a voxel the order above stays
    seen, rank = {}, []
    for vox, _ in rows:
        rank.append(seen.get(vox, 0))
        seen[vox] = rank[-1] + 1
    perm = np.argsort(np.array(rank), kind="stable")
    m = np.array([rows[i][0] for i in perm], np.int64)
    x = np.array([rows[i][1] for i in perm], dtype)
    return np.stack([x, -x], 1), m, 10
