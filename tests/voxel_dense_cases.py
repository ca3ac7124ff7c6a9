"""Seeded scenes for the tests of d3d_amd.voxel.dense, built around the tile T of the two kernels (the cells of one sample a workgroup
owns): P = A * B * D in {1, T - 1, T, T + 1, 3 T + 5}, N in {1, 3}, eight occupancies (the
eighth puts the stretches on both sides of the kernels' sparse threshold).  `scene(name)` -> a Scene; SCENES lists the
names.  The axes, a negative origin and int32 coordinates rotate through the scenes, so every scene differs from its neighbours in
more than one way; N = 1 alternates between no batch_index and a batch_index of zeros."""
import collections
import functools
import itertools

import numpy as np

TILE_MIRROR = 256                    # kVdTile of csrc/vdense.hip, for a checkout without the built library
SPARSE_MIRROR = 16                   # kVdSparse: at most this many present cells and a stretch goes element by element


def library_tile():
    """d3d_vdense_tile_cells() where the library loads, else None"""
    try:
        from d3d_amd import _lib
        return int(_lib.load().d3d_vdense_tile_cells())
    except (ImportError, OSError, AttributeError):
        return None


def library_sparse():
    """d3d_vdense_sparse_cells() where the library loads, else None"""
    try:
        from d3d_amd import _lib
        return int(_lib.load().d3d_vdense_sparse_cells())
    except (ImportError, OSError, AttributeError):
        return None


TILE = library_tile() or TILE_MIRROR
SPARSE = library_sparse() or SPARSE_MIRROR

Scene = collections.namedtuple("Scene", "coords batch batch_size spatial_shape origin axes")

PERMUTATIONS = tuple(itertools.permutations((0, 1, 2)))
ORIGINS = ((0, 0, 0), (-3, 1000, -7), (-40, -1, 5))
OCCUPANCIES = ("empty", "last", "full", "checker", "first_lane", "last_lane", "random", "threshold")
CHANNELS = (1, 3, 8, 31, 32, 33, 64, 130, 260)
FILLS = (0, float("-inf"), 1.5)


def factor3(p, turn):
    """p as three factors >= 1 (prime factors dealt out smallest first, the rest multiplied into the last), rotated by `turn`: unit
    axes where p has fewer than three prime factors"""
    primes, q, f = [], p, 2
    while q > 1:
        while q % f == 0:
            primes.append(f)
            q //= f
        f += 1
    three = primes[:2] + [int(np.prod(primes[2:], dtype=np.int64))] if len(primes) > 2 else primes + [1] * (3 - len(primes))
    return tuple(three[(k + turn) % 3] for k in range(3))


def sizes():
    t = TILE
    return {"one": 1, "tm1": t - 1, "t": t, "tp1": t + 1, "3tp5": 3 * t + 5}


def occupied(kind, n, p, seed):
    """the flat cells (over n samples of p cells) that hold a voxel, in row order"""
    t, cells = TILE, n * p
    stretch_starts = [s * p + k for s in range(n) for k in range(0, p, t)]
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "last":
        return np.array([cells - 1], np.int64)
    if kind == "full":
        return np.arange(cells, dtype=np.int64)
    if kind == "checker":
        return np.arange(cells, dtype=np.int64)[::2][::-1].copy()
    if kind == "first_lane":            # the first and the last stretch of every sample: only their first cell
        return np.array(sorted({s for s in stretch_starts if s % p == 0 or s % p + t >= p}), np.int64)
    if kind == "last_lane":             # the same stretches: only their last (live) cell
        return np.array(sorted({min(s - s % p + p, s + t) - 1 for s in stretch_starts if s % p == 0 or s % p + t >= p}), np.int64)
    r = np.random.default_rng(seed)
    if kind == "threshold":             # stretch number j holds SPARSE - 1, SPARSE, SPARSE + 1, SPARSE - 1, .. cells (as far as it has them)
        picks = [s + r.permutation(min(t, p - s % p))[:SPARSE - 1 + j % 3] for j, s in enumerate(stretch_starts)]
        return r.permutation(np.concatenate(picks)).astype(np.int64)
    return r.permutation(cells)[:max(1, int(round(0.3 * cells)))].astype(np.int64)


def make(pname, n, kind, number):
    p = sizes()[pname]
    axes, origin = PERMUTATIONS[number % 6], ORIGINS[number % 3]
    dshape = factor3(p, number)
    flat = occupied(kind, n, p, seed=number)
    a, b, d = np.unravel_index(flat % p, dshape) if len(flat) else (np.zeros(0, np.int64),) * 3
    coords = np.zeros((len(flat), 3), np.int64)
    shape = [0, 0, 0]
    for k, x in enumerate((a, b, d)):
        coords[:, axes[k]] = x + origin[axes[k]]
        shape[axes[k]] = dshape[k]
    batch = flat // p
    if number % 4 == 3:
        coords, batch = coords.astype(np.int32), batch.astype(np.int32)
    if n == 1 and number % 2 == 0:
        return Scene(coords, None, None, tuple(shape), origin, axes)
    return Scene(coords, batch, n, tuple(shape), origin, axes)


_NAMES = ["%s-n%d-%s" % (p, n, k) for p in ("one", "tm1", "t", "tp1", "3tp5") for n in (1, 3) for k in OCCUPANCIES]
SCENES = tuple(_NAMES)


@functools.lru_cache(maxsize=None)
def scene(name):
    pname, n, kind = name.split("-")
    s = make(pname, int(n[1:]), kind, _NAMES.index(name))
    for a in (s.coords, s.batch):
        if a is not None:
            a.setflags(write=False)
    return s


def kwargs(s):
    """the keyword arguments of VoxelDenseMap for a scene (without coords and batch_index)"""
    return dict(spatial_shape=s.spatial_shape, batch_size=s.batch_size, origin=s.origin, axes=s.axes)


def batch_size(s):
    return 1 if s.batch_size is None else s.batch_size


def features(v, c, dtype, seed, special=False):
    """[v, c] torch tensor of `dtype`: normal values; special: NaN (with a payload), +-inf and -0.0 sprinkled in"""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((v, c), generator=g, dtype=torch.float64).to(dtype)
    if special and x.numel():
        flat = x.view(-1)
        pick = torch.randperm(flat.numel(), generator=g)
        for k, val in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
            flat[pick[k::7][:max(1, flat.numel() // 9)]] = val
        payload = {torch.float32: (torch.int32, 0x7fc00001), torch.float64: (torch.int64, 0x7ff8000000000001),
                   torch.float16: (torch.int16, 0x7e01), torch.bfloat16: (torch.int16, 0x7fc1)}[dtype]
        flat.view(payload[0])[pick[0]] = payload[1]
    return x
