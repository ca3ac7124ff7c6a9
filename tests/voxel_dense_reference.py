"""The numpy model of d3d_amd.voxel.dense: plain indexing, no arithmetic.  It moves elements of ANY numpy dtype, so the half types go
through it as the integers of their bits (`bits` / `unbits`), and a comparison of its results is a comparison of bits.

A scene is what VoxelDenseMap takes: coords [V, 3], batch [V] or None, batch_size N, spatial_shape and origin per coordinate COLUMN,
axes = the column each dense axis walks."""
import numpy as np
import torch

INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}


def dense_shape(spatial_shape, axes):
    return tuple(int(spatial_shape[a]) for a in axes)


def sites(coords, batch, origin, axes):
    """-> (n [V], a [V], b [V], d [V]): the sample and the three dense coordinates of every row, int64"""
    coords = np.asarray(coords).astype(np.int64).reshape(-1, 3)
    n = np.zeros(len(coords), np.int64) if batch is None else np.asarray(batch).astype(np.int64)
    return (n,) + tuple(coords[:, axes[k]] - int(origin[axes[k]]) for k in range(3))


def inside(coords, batch, batch_size, spatial_shape, origin, axes):
    """[V] bool: the precondition -- every dense coordinate in [0, size), the sample in [0, N)"""
    n, *abd = sites(coords, batch, origin, axes)
    ok = (n >= 0) & (n < batch_size)
    for x, s in zip(abd, dense_shape(spatial_shape, axes)):
        ok &= (x >= 0) & (x < s)
    return ok


def cell(coords, batch, spatial_shape, origin, axes):
    """[V] int64: ((n * A + a) * B + b) * D + d"""
    n, a, b, d = sites(coords, batch, origin, axes)
    A, B, D = dense_shape(spatial_shape, axes)
    return ((n * A + a) * B + b) * D + d


def index(coords, batch, batch_size, spatial_shape, origin, axes):
    """[N * A * B * D] int32: the row at every cell, -1 for none (rows must be unique)"""
    A, B, D = dense_shape(spatial_shape, axes)
    out = np.full(batch_size * A * B * D, -1, np.int32)
    out[cell(coords, batch, spatial_shape, origin, axes)] = np.arange(len(np.asarray(coords).reshape(-1, 3)), dtype=np.int32)
    return out


def to_dense(feat, coords, batch, batch_size, spatial_shape, origin, axes, fill=0):
    """feat [V, C] -> [N, C, A, B, D]: `fill` (an element of feat's dtype) everywhere, then the rows at their sites"""
    n, a, b, d = sites(coords, batch, origin, axes)
    out = np.full((batch_size, feat.shape[1]) + dense_shape(spatial_shape, axes), fill, feat.dtype)
    out[n, :, a, b, d] = feat
    return out


def from_dense(dense, coords, batch, origin, axes):
    """dense [N, C, A, B, D] -> [V, C]: the values at the sites"""
    n, a, b, d = sites(coords, batch, origin, axes)
    return np.ascontiguousarray(dense[n, :, a, b, d])


def bev(dense):
    """[N, C, A, B, D] -> [N, C * A, B, D]"""
    return dense.reshape(dense.shape[0], dense.shape[1] * dense.shape[2], dense.shape[3], dense.shape[4])


def bits(t):
    """a torch tensor of a float dtype -> the numpy integers of its bits (a copy on the host)"""
    return t.detach().cpu().contiguous().view(INT_OF[t.dtype]).numpy().copy()


def unbits(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).view(dtype)


def fill_bits(fill, dtype):
    """`fill` rounded to the dtype by torch, as the integer of its bits"""
    return bits(torch.full((1,), fill, dtype=dtype))[0]
