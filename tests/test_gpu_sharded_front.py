"""The Python front of the sharded voxelizer on the real kernels: ShardedVoxelGenerator through HipOps against the same generator
through the NumPy twins of the kernels (sharded_helpers.NumpyOps) on the CPU copy of the frame -- every exchange, one rank through
LocalComm and two ragged virtual ranks on one GPU -- then the resident dense output over two frames and the lock-step repeat after
a status overflow that only one rank saw."""
import threading
import traceback

import numpy as np
import pytest
import torch

from d3d_amd import _lib
from d3d_amd.utils import Dict
from d3d_amd.voxel.sharded import HipOps, LocalComm, ShardedVoxelGenerator
from sharded_helpers import LockedOps, NumpyOps, ThreadWorld
from test_sharded import BOUNDS, SHAPE, _check_owned, _cloud
from test_sharded_front import CASES, Recorder, _raise_status_once

pytestmark = pytest.mark.gpu


def _frame(n, seed):
    """every fifth point in a handful of cells: candidate rows of both ranks compete for a voxel's slots"""
    cloud = _cloud(n, seed)
    cloud[::5, :3] = cloud[::5, :3] * 0.02 + np.array([30, 0, -1], np.float32)
    return cloud


FRAME = _frame(3000, 5)


def _cuts(world, n):
    return [0, n] if world == 1 else [0, 1100, n]


def _run(world, gpu, frames, wrap=None, each=None, **kw):
    """every frame through one generator per rank (HipOps on the GPU, or NumpyOps on the host) -> out[frame][rank]"""
    tw, lock = ThreadWorld(world), threading.Lock()
    out, errs = [[None] * world for _ in frames], []

    def run(rank):
        try:
            if gpu:
                torch.cuda.set_device(0)
            ops = LockedOps(HipOps(), lock) if gpu else NumpyOps()
            gen = ShardedVoxelGenerator(BOUNDS, SHAPE, comm=LocalComm() if world == 1 else tw.comm(rank),
                                        ops=wrap(rank, ops) if wrap else ops, **kw)
            for f, cloud in enumerate(frames):
                cuts = _cuts(world, len(cloud))
                points = torch.from_numpy(cloud[cuts[rank]:cuts[rank + 1]])
                res = gen(points.cuda() if gpu else points)
                if each:
                    each(gen, res)
                out[f][rank] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}      # before the next frame
        except Exception:  # pragma: no cover
            errs.append(traceback.format_exc())
            tw.barrier.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs, errs[0]
    return out


def _same(got, ref, reduction):
    assert list(got) == list(ref)
    for k, want in ref.items():
        if not torch.is_tensor(want):
            assert got[k] == want, k
        elif k == "aggregates" and reduction == "mean":
            np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
        else:
            assert got[k].dtype == want.dtype and torch.equal(got[k], want), k


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("case,reduction", [(c, r) for c in CASES for r in ("mean", "max")] + [("owner, owned voxels, dense", "min"),
                                                                                              ("bitmap", "min")])
def test_hip_ops_against_numpy_ops(case, reduction, world):
    kw = dict(CASES[case]["kw"], reduction=reduction)
    got, ref = _run(world, True, [FRAME], **kw)[0], _run(world, False, [FRAME], **kw)[0]
    for rank in range(world):
        _same(got[rank], ref[rank], reduction)


@pytest.mark.parametrize("world", [1, 2])
def test_resident_dense_output_over_two_frames(world):
    frames = [FRAME, _frame(1700, 6)]
    kw = dict(exchange="owner", replicate=False, max_points=3)

    def is_view(gen, res):
        assert res.voxels.untyped_storage().data_ptr() == gen._resident_buf.voxels.untyped_storage().data_ptr()
    got, ref = _run(world, True, frames, each=is_view, resident=True, **kw), _run(world, False, frames, **kw)
    for f in range(len(frames)):
        for rank in range(world):
            _same(got[f][rank], ref[f][rank], "mean")


@pytest.mark.parametrize("max_points", [0, 4])
def test_overflow_seen_by_one_rank_repeats_both(max_points):
    logs = [[], []]

    def wrap(rank, ops):
        hooks = {"owner_pack": _raise_status_once(_lib.STATUS_PACK_OVERFLOW, 2)} if rank == 0 else None
        return Recorder("ops", ops, logs[rank], hooks)
    out = _run(2, True, [FRAME], wrap=wrap, exchange="owner", replicate=False, max_points=max_points or None)[0]
    cuts = _cuts(2, len(FRAME))
    for rank in range(2):
        local = [entry for entry in logs[rank] if entry.startswith("ops.voxelize_reduce/")]
        assert local == ["ops.voxelize_reduce/5/max_points,want_coords", "ops.voxelize_reduce/5/max_points,plain,want_coords"]
        assert logs[rank].count("ops.owner_pack/11/points_in_shard") == 2 and logs[rank].count("ops.owner_map/3/") == 1
        res = Dict(out[rank])
        _check_owned(res, FRAME, slice(cuts[rank], cuts[rank + 1]), "mean", max_points=max_points)
