"""Seeded scenes for the tests of d3d_amd.voxel.conv: name -> (coords [V, 3] int64, batch [V] int64 or None), every one of at most
about 10 000 voxels, in a shuffled row order (a table that is right only for sorted rows must fail)."""
import numpy as np

import voxel_conv_reference as ref

KERNELS = ((3, 3, 3), (1, 1, 1), (3, 1, 1), (1, 3, 5), (5, 5, 5), (7, 7, 7))
DILATIONS = (1, 2, (1, 2, 3))


def fill(shape, count, seed, shift=(0, 0, 0)):
    """`count` distinct cells of a grid of `shape`, in random order, moved by `shift`"""
    r = np.random.default_rng(seed)
    cells = r.choice(int(np.prod(shape)), size=count, replace=False)
    return np.stack(np.unravel_index(cells, shape), -1).astype(np.int64) + np.array(shift, np.int64)


def block(shape, seed=0):
    return fill(shape, int(np.prod(shape)), seed)


def voxelizer_range(seed=5):
    """The voxelizer's own range: a 704 x 800 x 40 grid moved by (0, -400, -30).  A 5 % fill of all of it is 1.1 M voxels; this is
    a 5 % fill of its far 64 x 80 x 40 corner (10 240 voxels, the same neighbour density) plus the grid's two extreme cells, so the
    measured spans are the whole grid's and most coordinates are negative in y and z."""
    far = fill((64, 80, 40), 10240, seed, shift=(640, 320, -30))
    ends = np.array([[0, -400, -30], [703, 399, 9]], np.int64)
    far = far[~np.any(np.all(far[:, None, :] == ends[None], -1), 1)]
    c = np.concatenate([far, ends])
    return c[np.random.default_rng(seed + 1).permutation(len(c))]


def batches(seed=6):
    """one cloud under batch ids 0 and 1 and another under batch id 5, rows interleaved: neighbours must not cross batches"""
    a, b = fill((14, 14, 14), 1500, seed), fill((14, 14, 14), 900, seed + 1)
    c = np.concatenate([a, a, b])
    ids = np.concatenate([np.zeros(len(a)), np.ones(len(a)), np.full(len(b), 5)]).astype(np.int64)
    p = np.random.default_rng(seed + 2).permutation(len(c))
    return c[p], ids[p]


def far_away(seed=7):
    """coordinates near +-2^40, a span of 10 per axis"""
    return fill((10, 10, 10), 400, seed) + np.array([2 ** 40, -2 ** 40, 2 ** 40 + 7], np.int64)


def comb():
    """4096 voxels in pairs (x, x + 1) at a stride of 2^50 along x: the keys share their low 50 bits up to the pair bit, whatever
    the spans, and every voxel has exactly one x neighbour; every other look-up is a miss inside the measured box.  (A hash that
    takes the TOP bits of key * odd constant spreads such keys evenly: the longest probe here is 1.  The chains are `wrap`'s.)"""
    x = np.arange(2048, dtype=np.int64) * 2 ** 50
    c = np.zeros((4096, 3), np.int64)
    c[:, 0] = np.concatenate([x, x + 1])
    c[:, 1:] = (-3, 11)
    return c[np.random.default_rng(8).permutation(4096)]


WRAP_LINE, WRAP_WINDOW, WRAP_CHAIN, WRAP_FED = 1 << 15, 8, 190, 20


def wrap():
    """A chain that must cross the end of the hash table, built against the hash vnbr.hip uses (ref.hash_home): voxels on the line
    0 <= x < 2^15 (y, z constant, so the key is x itself) with both ends present.  WRAP_CHAIN of them start their probe in the LAST
    8 slots of the 512-slot table: whatever the order of insertion at most 8 stay there and the others step from slot 511 to slot 0,
    a run of about 190 occupied slots.  WRAP_FED of the chain's voxels have their x - 1 neighbour present (look-ups that HIT after
    the wrap: at least WRAP_FED - 8 of them in any order), and one voxel sits at x - 1 of a coordinate that starts in the last slots
    but is absent (a look-up that MISSES only after walking the whole run across the end).  test_voxel_conv.py asserts all of this
    with a replay, so the property cannot vanish silently if the hash changes."""
    total = WRAP_CHAIN + WRAP_FED + 3
    log2cap = ref.hash_log2cap(total)
    cap = 1 << log2cap
    late = [x for x in range(2, WRAP_LINE - 1) if ref.hash_home(x, log2cap) >= cap - WRAP_WINDOW]
    assert len(late) > WRAP_CHAIN + 1, "the line is too short for this hash"
    chain, spare = late[:WRAP_CHAIN], late[WRAP_CHAIN:]
    taken = set(chain) | {0, WRAP_LINE - 1}
    fed = [x - 1 for x in chain if x - 1 not in taken and ref.hash_home(x - 1, log2cap) < cap - WRAP_WINDOW][:WRAP_FED]
    taken |= set(fed)
    absent = next(x for x in spare if x - 1 not in taken and x + 1 not in taken and ref.hash_home(x - 1, log2cap) < cap - WRAP_WINDOW)
    xs = sorted(taken | {absent - 1})
    assert len(xs) == total and len(fed) == WRAP_FED
    c = np.zeros((total, 3), np.int64)
    c[:, 0] = xs
    c[:, 1:] = (7, -2)
    return c[np.random.default_rng(10).permutation(total)], absent


def scenes():
    s = {"v%d" % v: (fill((6, 6, 6), v, v), None) for v in (1, 63, 64, 65)}
    s["block12"] = (block((12, 12, 12), 1), None)
    s["line_x"], s["line_y"], s["line_z"] = (block((40, 1, 1), 2), None), (block((1, 40, 1), 3), None), (block((1, 1, 40), 4), None)
    s["fill32"] = (fill((32, 32, 32), 9830, 9), None)
    s["voxelizer_range"] = (voxelizer_range(), None)
    s["batches"] = batches()
    s["far_away"] = (far_away(), None)
    for v in (4095, 4096, 4097):                                  # the hash table's capacity steps between 4096 and 4097
        s["v%d" % v] = (fill((24, 24, 24), v, v), None)
    s["comb"] = (comb(), None)
    s["wrap"] = (wrap()[0], None)
    return s


SCENES = scenes()
SMALL = tuple(n for n in sorted(SCENES) if len(SCENES[n][0]) <= 600)


def features(v, c, dtype, seed=0):
    return np.random.default_rng(seed).standard_normal((v, c)).astype(dtype)


def dense(name):
    """a scene as a dense grid: (index [V, 4] of every row as (n, x, y, z) into a grid of `shape` = (N, X, Y, Z))"""
    c, b = SCENES[name]
    ids = np.zeros(len(c), np.int64) if b is None else np.unique(b, return_inverse=True)[1]
    local = c - c.min(0)
    return np.concatenate([ids[:, None], local], 1), (int(ids.max()) + 1,) + tuple(int(a) for a in local.max(0) + 1)
