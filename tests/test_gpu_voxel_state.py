"""GPU: what a VoxelGenerator keeps from call to call lives beside it, per host thread (d3d_amd.voxel._CallState) -- settings
changed after first use are honoured, a pickled twin of a used generator computes the same, and one generator serves two host
threads at once.  Grid [44, 50, 4] on the KITTI bounds, frames of 4 000 and 2 500 points; everything bit for bit."""
import pickle
import threading

import numpy as np
import pytest
import torch

import oracle
from test_gpu_voxel import _np, check_sparse

pytestmark = pytest.mark.gpu

SHAPE = [44, 50, 4]
TRIM = dict(max_points=4, max_points_filter="trim")
_cache = {}


def frame(name):
    """A = lidar_like(4000, 1), B = lidar_like(2500, 2): on the host and on the device, made once"""
    if name not in _cache:
        from d3d_amd import synth
        cloud = {"A": synth.lidar_like(4000, 1), "B": synth.lidar_like(2500, 2)}[name]
        _cache[name] = (cloud, torch.from_numpy(cloud).cuda())
    return _cache[name]


def expected(name, **kw):
    """the oracle's sparse result for a frame, computed once per setting"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        from d3d_amd import synth
        _cache[key] = oracle.VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, **kw)(frame(name)[0])
    return _cache[key]


def generator(**kw):
    from d3d_amd import synth
    from d3d_amd.voxel import VoxelGenerator
    return VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, **kw)


def assert_identical(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k


def test_settings_changed_after_first_use_are_honoured_on_the_sparse_route():
    gen = generator(**TRIM)
    pts = frame("A")[1]
    rows = []
    for change, kw in ((dict(), TRIM), (dict(_max_points=2), dict(TRIM, max_points=2)),
                       (dict(_max_points=4, _min_points=2), dict(TRIM, min_points=2))):
        for name, value in change.items():
            setattr(gen, name, value)
        got, exp = gen(pts), expected("A", **kw)
        print(sorted(kw.items()), "points", tuple(got.points.shape), "voxels", tuple(got.coords.shape), "oracle", exp["points"].shape)
        check_sparse(_np(got), exp)
        assert_identical(dict(got), dict(generator(**kw)(pts)))
        assert got.points.shape[0] == exp["points"].shape[0]
        rows.append(got.points.shape[0])
    assert len(set(rows)) == 3, rows            # every changed setting shows at this size: no vacuous pass


@pytest.mark.parametrize("kw", [TRIM, dict(dense=True), dict(dense=True, resident=True)], ids=["sparse-trim", "dense-pooled", "dense-resident"])
def test_a_pickled_twin_of_a_used_generator_computes_the_same(kw):
    gen = generator(**kw)
    first = gen(frame("A")[1])
    twin = pickle.loads(pickle.dumps(gen))
    del first
    pts = frame("B")[1]
    got, want = twin(pts), gen(pts)
    assert_identical(dict(got), dict(want))
    if kw.get("resident"):
        assert got.voxels.untyped_storage().data_ptr() != want.voxels.untyped_storage().data_ptr()
        assert twin._resident_buf is not gen._resident_buf


@pytest.mark.parametrize("kw", [TRIM, dict(dense=True)], ids=["sparse-trim", "dense-pooled"])
def test_one_generator_called_from_two_host_threads_on_their_own_streams(kw):
    gen = generator(**kw)
    want = {name: {k: v.clone() for k, v in gen(frame(name)[1]).items()} for name in ("A", "B")}
    torch.cuda.synchronize()                    # the frames and the expected results are complete before a side stream reads them
    results, errors = {"A": [], "B": []}, []

    def work(name):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(8):
                    results[name].append(dict(gen(frame(name)[1])))
            stream.synchronize()
        except BaseException as e:              # (reported by the main thread)
            errors.append((name, e))

    threads = [threading.Thread(target=work, args=(name,)) for name in ("A", "B")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
        assert not t.is_alive()
    assert not errors, errors
    for name in ("A", "B"):
        assert len(results[name]) == 8
        for got in results[name]:
            assert_identical(got, want[name])
