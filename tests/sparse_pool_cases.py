"""What the tests of d3d_amd.voxel.sparse_pool pool through: the scenes and configurations of sparse_conv_cases.py under the tables of
both owners, computed once by the numpy models and shared (do not modify), and the scene of the largest kernel."""
import functools

import numpy as np

import sparse_conv_cases as scases
import voxel_conv_cases as vcases
import voxel_conv_reference as vref

SCENES = ("v1", "v63", "v64", "v65", "batches", "negative_odd")
CONFIGS = ("k3s2p1", "k2s2p0", "k1s1p0", "k312s213d211")      # through a SparseConvMap
KERNELS = ((3, 3, 3), (1, 3, 5))                              # through a VoxelNeighbors
WHERES = tuple(("map", c) for c in CONFIGS) + tuple(("nbrs", k) for k in KERNELS)
CHANNELS = (1, 3, 4, 8, 20, 64, 260)          # scalar path, vector path, a lane group that is no power of two, two passes per row


@functools.lru_cache(maxsize=None)
def tables(scene, kind, what):
    """-> (forward table [rows, K], backward table [V, K], whether the backward one is read mirrored) of the numpy models"""
    if kind == "map":
        _, _, t_out, t_in = scases.model(scene, what)
        return t_out, t_in, False
    c, b = scases.SCENES[scene]
    tab = vref.table(c, what, 1, b)
    tab.setflags(write=False)
    return tab, tab, True


def owner(scene, kind, what, to_gpu):
    """the library's owner of the same tables, built on the GPU"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors
    c, b = scases.SCENES[scene]
    if kind == "map":
        return SparseConvMap(to_gpu(c), *scases.CONFIGS[what], batch_index=to_gpu(b))
    return VoxelNeighbors(to_gpu(c), what, batch_index=to_gpu(b))


def randoms(rows, c, seed):
    return np.random.default_rng(seed).standard_normal((rows, c))


@functools.lru_cache(maxsize=None)
def large_kernel(channels=4):
    """the full 8 x 8 x 8 block in shuffled row order under kernel size 7 (K = 343) -> (coords, features [512, channels], table).
    Channel 0 grows with the position (x slowest), channel 1 falls with it, the others are distinct random integers: the voxel at the
    origin finds its maximum of channel 0 at offset (+3, +3, +3), column 342, and every voxel with x <= 5 beyond column 255"""
    c = vcases.block((8, 8, 8), 12)
    pos = ((c[:, 0] * 8 + c[:, 1]) * 8 + c[:, 2]).astype(np.float64) / 8          # (eighths: a sum of 343 of them fits fp16)
    cols = [pos, -pos] + [np.random.default_rng(20 + i).permutation(512).astype(np.float64) / 8 for i in range(channels - 2)]
    tab = vref.table(c, 7)
    tab.setflags(write=False)
    return c, np.stack(cols[:channels], 1), tab
