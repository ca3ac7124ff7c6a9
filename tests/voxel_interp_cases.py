"""Seeded scenes for the tests of d3d_amd.voxel.interp: name -> (coords [V, 3] int64, batch [V] int64 or None, positions [K, 3] float64,
position_batch [K] int64 or None), about 65 voxels and 130 points each, the voxels in a shuffled row order.  The positions are made in
fp64 from values that fp32 holds exactly where a scene is about exact values (integers, quarters); `positions(name, dtype)` casts."""
import functools

import numpy as np

import voxel_conv_cases as ccases
import voxel_interp_reference as ref

BOX = (5, 6, 7)
CHANNELS = (1, 3, 4, 12, 16, 20, 64, 260)
CROWD = 300


def _uniform(seed, k, lo, hi):
    return np.random.default_rng(seed).uniform(np.array(lo, np.float64), np.array(hi, np.float64), (k, 3))


def random(seed=1):
    return ccases.fill(BOX, 65, seed), None, _uniform(seed + 100, 130, (-0.5,) * 3, [b - 0.5 for b in BOX]), None


def negative(seed=2):
    """negative and offset coordinates: the box moved by (-40, 1000, -7)"""
    shift = np.array((-40, 1000, -7), np.int64)
    c, _, p, _ = random(seed)
    return c + shift, None, p + shift, None


def batches(seed=3):
    """one cloud under the batch values 0 and 2; the points carry 0, 2, 1 (inside the span of the batch values, but no voxel has it),
    5 and -3 (outside it)"""
    a = ccases.fill(BOX, 32, seed)
    c = np.concatenate([a, a])
    ids = np.concatenate([np.zeros(32), np.full(32, 2)]).astype(np.int64)
    perm = np.random.default_rng(seed + 1).permutation(64)
    pb = np.random.default_rng(seed + 2).choice(np.array([0, 2, 0, 2, 1, 5, -3], np.int64), 130)
    return c[perm], ids[perm], _uniform(seed + 3, 130, (-0.5,) * 3, [b - 0.5 for b in BOX]), pb


def integers(seed=4):
    """positions on integers: f = 0 on every axis, corner 0 carries weight 1"""
    c = ccases.fill(BOX, 65, seed)
    return c, None, np.floor(_uniform(seed + 1, 130, (0,) * 3, BOX)), None


def quarters(seed=5):
    """positions at multiples of 1 / 4: every weight is a multiple of 1 / 64, exact in every type"""
    c = ccases.fill(BOX, 65, seed)
    return c, None, np.floor(_uniform(seed + 1, 130, (-1,) * 3, [b for b in BOX]) * 4) / 4, None


def tiny_negative(seed=6):
    """positions a tiny step below an integer on some axes, the voxels at -1 and 0 present: floor gives n - 1 and f = x - (n - 1) rounds
    to exactly 1 in both types"""
    c = ccases.fill((4, 4, 4), 60, seed, shift=(-2, -2, -2))
    p = np.floor(_uniform(seed + 1, 130, (-2,) * 3, (2,) * 3))
    r = np.random.default_rng(seed + 2)
    tiny = r.choice(np.array([0.0, -1e-30, -1.5e-38, -1e-10]), (130, 3))
    p = np.where((p == 0) | (tiny == -1e-10), p + tiny, p)               # (n - 1e-30 is n again for n != 0: only -1e-10 survives there)
    return c, None, p, None


def outside(seed=7):
    """positions up to three cells outside the box of the coordinates on every side, and inside it"""
    c = ccases.fill(BOX, 65, seed)
    return c, None, _uniform(seed + 1, 130, (-3.5,) * 3, [b + 2.5 for b in BOX]), None


def nonfinite(seed=8):
    """NaN, +-inf, 1e30 and the ends of [-2^62, 2^62) on one axis or all of them, among ordinary positions"""
    c, _, p, _ = random(seed)
    odd = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 62, -2.0 ** 62, 4e18, -4e18, 2.0 ** 62 - 2.0 ** 40, 2.0 ** 31, -2.0 ** 31 - 1]
    r = np.random.default_rng(seed + 1)
    for i, value in enumerate(odd * 3):
        p[i, r.integers(3) if i < 2 * len(odd) else slice(None)] = value
    return c, None, p, None


def crowded(seed=9):
    """CROWD points inside one cell of a full 3 x 3 x 3 block and one in the cell next to it: the voxels at the first cell's corners
    get CROWD or CROWD + 1 entries each -- long folds on the way back, whole steps of four and a remainder"""
    c = ccases.block((3, 3, 3), seed)
    p = np.concatenate([_uniform(seed + 1, CROWD, (1, 1, 1), (2, 2, 2)), np.array([[1.5, 1.25, 0.5]])])
    return c, None, p, None


def untouched(seed=10):
    """the points stay in the low corner of the box: most voxels are named by no entry"""
    c = ccases.fill(BOX, 65, seed)
    return c, None, _uniform(seed + 1, 130, (-0.5,) * 3, (1.5, 1.5, 2.5)), None


def no_points(seed=11):
    return ccases.fill(BOX, 65, seed), None, np.zeros((0, 3)), None


def no_voxels(seed=12):
    return np.zeros((0, 3), np.int64), None, _uniform(seed, 130, (-1,) * 3, BOX), None


def wrap(seed=13):
    """the probe-chain scene of voxel_conv_cases (a chain of look-ups that crosses the end of the hash table): points along its line,
    around voxels of the chain and around the coordinate whose look-up misses only after the whole run"""
    c, absent = ccases.wrap()
    r = np.random.default_rng(seed)
    x = np.concatenate([r.choice(c[:, 0], 110), np.full(20, absent)]).astype(np.float64)
    p = np.stack([x + r.uniform(-1.0, 1.0, 130), 7 + r.uniform(-1.0, 0.5, 130), -2 + r.uniform(-0.5, 1.0, 130)], 1)
    return c, None, p, None


MAKERS = dict(random=random, negative=negative, batches=batches, integers=integers, quarters=quarters, tiny_negative=tiny_negative,
              outside=outside, nonfinite=nonfinite, crowded=crowded, untouched=untouched, no_points=no_points, no_voxels=no_voxels, wrap=wrap)
SCENES = tuple(MAKERS)
DTYPES = {"f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def scene(name):
    out = MAKERS[name]()
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def positions(name, dtype):
    return scene(name)[2].astype(DTYPES[dtype])


@functools.lru_cache(maxsize=None)
def table(name, dtype, mode="linear", normalize=False):
    """the model's (table, weights) of a scene, computed once and read-only"""
    c, b, _, pb = scene(name)
    t, w = ref.corners(c, positions(name, dtype), b, pb, mode, normalize)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def randoms(rows, c, seed):
    return np.random.default_rng(seed).standard_normal((rows, c))


def small_integers(rows, c, seed):
    """integers in -8 .. 8: with weights that are multiples of 1 / 64 every product and every partial sum of a fold is exact in every
    type (bf16's 8 bits hold the rounded result only at the end)"""
    return np.random.default_rng(seed).integers(-8, 9, (rows, c)).astype(np.float64)
