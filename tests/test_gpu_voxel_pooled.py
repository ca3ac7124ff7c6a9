"""GPU: the dense VoxelGenerator's pooled default output (`voxels` as a view of a generator-owned DenseOutputBuffer whenever the
caller cannot tell) and the early size notification of the dense contract, bit-exact against the oracle.  Grid [352, 400, 20] on
the KITTI bounds, frames of 6 000 to 60 000 points: the smallest the binned routes take."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from call_opts import set_opts
from test_gpu_voxel import _np, check_dense

pytestmark = pytest.mark.gpu

SHAPE = [352, 400, 20]
_cache = {}


def frames(C=4):
    """lidar 20 k, lidar 60 k, lidar 6 k, empty, uniform 40 k, lidar 40 k with another seed: counts grow, shrink, vanish and
    return, ids change hands"""
    if ("frames", C) not in _cache:
        from d3d_amd import synth
        fs = [synth.lidar_like(20000, 1), synth.lidar_like(60000, 2), synth.lidar_like(6000, 3), np.zeros((0, 4), np.float32),
              synth.uniform_cloud(40000, 4), synth.lidar_like(40000, 5)]
        rng = np.random.default_rng(C)
        fs = [f[:, :C] if C <= 4 else np.concatenate([f, rng.random((len(f), C - 4), dtype=np.float32)], 1) for f in fs]
        _cache[("frames", C)] = [np.ascontiguousarray(f, dtype=np.float32) for f in fs]
    return _cache[("frames", C)]


def expected(k, C=4, **kw):
    """the oracle's result for frame k, computed once per configuration"""
    key = ("exp", k, C, tuple(sorted(kw.items())))
    if key not in _cache:
        from d3d_amd import synth
        _cache[key] = oracle.VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, dense=True, **kw)(frames(C)[k])
    return _cache[key]


def generator(**kw):
    from d3d_amd import synth
    from d3d_amd.voxel import VoxelGenerator
    return VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, dense=True, **kw)


def shares_pool_memory(gen, voxels):
    ptr = voxels.untyped_storage().data_ptr()
    return any(slot.buf.voxels.untyped_storage().data_ptr() == ptr for pool in gen._pool_map.values() for slot in pool.slots)


@pytest.mark.parametrize("kw,C", [(dict(max_points=32, max_voxels=60000, reduction="mean"), 4),
                                  (dict(max_points=32, max_voxels=9000, reduction="mean"), 4),          # the count is clamped
                                  (dict(max_points=1, max_voxels=60000, reduction="max"), 4),
                                  (dict(max_points=5, max_voxels=60000, reduction="mean"), 4),
                                  (dict(max_points=70, max_voxels=60000), 4),       # more rows than a wavefront has lanes
                                  (dict(max_points=8, max_voxels=60000, reduction="mean"), 3),
                                  (dict(max_points=4, max_voxels=60000, reduction="min"), 5)])
def test_one_default_generator_over_a_sequence_of_frames_results_dropped(kw, C):
    gen = generator(**kw)
    nonempty = 0
    for k, f in enumerate(frames(C)):
        before = dict(gen._pool_stats)
        got = gen(torch.from_numpy(f).cuda(), poison=False)
        check_dense(_np(got), expected(k, C, **kw), kw["max_points"])
        after = gen._pool_stats
        if len(f):
            nonempty += 1
            assert shares_pool_memory(gen, got.voxels), k
            # every non-empty frame goes through ONE pooled buffer: the previous result was dropped
            assert after["pooled"] == before["pooled"] + 1 and after["second"] == 0 and after["fresh"] == before["fresh"], (k, after)
        del got
    pools = list(gen._pool_map.values())
    assert nonempty == 5 and gen._pool_stats["pooled"] == 5 and len(pools) == 1 and len(pools[0].slots) == 1
    assert pools[0].rezeroed == 0
    # the buffer's invariant after the sequence: rows at and beyond a voxel id's state are zero, everywhere
    buf = pools[0].slots[0].buf
    state = buf.row_state.cpu().numpy().astype(np.int64) & 0xffff
    nz = (buf.voxels != 0).any(dim=2).cpu().numpy()
    assert not (nz & (np.arange(kw["max_points"])[None, :] >= state[:, None])).any()
    assert buf.capacity <= kw["max_voxels"]


def test_results_kept_alive_share_no_memory_and_stay_what_they_were():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    gen = generator(**kw)
    fs = frames()
    r1 = gen(torch.from_numpy(fs[0]).cuda(), poison=False)
    r2 = gen(torch.from_numpy(fs[1]).cuda(), poison=False)
    r3 = gen(torch.from_numpy(fs[5]).cuda(), poison=False)
    for r, k in ((r1, 0), (r2, 1), (r3, 5)):
        check_dense(_np(r), expected(k, **kw), 32)
    ptrs = {r.voxels.untyped_storage().data_ptr() for r in (r1, r2, r3)}
    assert len(ptrs) == 3
    assert gen._pool_stats == dict(pooled=1, second=1, fresh=1)
    pools = list(gen._pool_map.values())
    assert len(pools) == 1 and len(pools[0].slots) == 2
    assert shares_pool_memory(gen, r1.voxels) and shares_pool_memory(gen, r2.voxels) and not shares_pool_memory(gen, r3.voxels)
    # dropping the first frees its buffer for the next call; the second's is left alone
    del r1
    r4 = gen(torch.from_numpy(fs[2]).cuda(), poison=False)
    check_dense(_np(r4), expected(2, **kw), 32)
    check_dense(_np(r2), expected(1, **kw), 32)
    assert gen._pool_stats == dict(pooled=1, second=2, fresh=1) and len(pools[0].slots) == 2


def test_a_caller_that_writes_its_result_gets_clean_padding_next_time():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    gen = generator(**kw)
    fs = frames()
    r = gen(torch.from_numpy(fs[1]).cuda(), poison=False)
    r.voxels.add_(1.0)                                  # (its own tensor, as far as the caller knows)
    del r
    got = gen(torch.from_numpy(fs[0]).cuda(), poison=False)
    check_dense(_np(got), expected(0, **kw), 32)         # padding included: check_dense compares whole tensors
    pool = list(gen._pool_map.values())[0]
    assert pool.rezeroed == 1 and gen._pool_stats["pooled"] == 2 and len(pool.slots) == 1
    del got
    got = gen(torch.from_numpy(fs[5]).cuda(), poison=False)
    check_dense(_np(got), expected(5, **kw), 32)
    assert pool.rezeroed == 1


def test_constructor_switches():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    fs = frames()
    gen = generator(resident=False, **kw)
    kept = []                   # every result stays alive: the allocator cannot hand an earlier one's memory out again
    for k in (0, 1, 2):
        got = gen(torch.from_numpy(fs[k]).cuda(), poison=False)
        check_dense(_np(got), expected(k, **kw), 32)
        assert all(got.voxels.untyped_storage().data_ptr() != r.voxels.untyped_storage().data_ptr() for r in kept)   # a fresh tensor each
        kept.append(got)
    for k, r in enumerate(kept):                                        # ... and none was written by a later call
        check_dense(_np(r), expected(k, **kw), 32)
    del kept
    assert gen._pool_stats == dict(pooled=0, second=0, fresh=0) and not gen._pool_map
    gen = generator(resident=True, **kw)                                # as before: ONE buffer, valid until the next call
    for k in (0, 1, 2):
        got = gen(torch.from_numpy(fs[k]).cuda(), poison=False)
        check_dense(_np(got), expected(k, **kw), 32)
        assert got.voxels.untyped_storage().data_ptr() == gen._resident_buf.voxels.untyped_storage().data_ptr()
    assert gen._pool_stats == dict(pooled=0, second=0, fresh=0)
    # release_cached_buffers drops the pools, a result that is still alive keeps its memory
    from d3d_amd.voxel import release_cached_buffers
    gen = generator(**kw)
    got = gen(torch.from_numpy(fs[0]).cuda(), poison=False)
    release_cached_buffers()
    assert not gen._pool_map
    check_dense(_np(got), expected(0, **kw), 32)
    check_dense(_np(gen(torch.from_numpy(fs[1]).cuda(), poison=False)), expected(1, **kw), 32)


def test_a_default_generator_inside_and_then_outside_inference_mode():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    gen = generator(**kw)
    fs = frames()
    with torch.inference_mode():
        for k in (0, 1):
            got = gen(torch.from_numpy(fs[k]).cuda(), poison=False)
            check_dense(_np(got), expected(k, **kw), 32)
            assert shares_pool_memory(gen, got.voxels)
            del got
        got = gen(torch.from_numpy(fs[2]).cuda(), poison=False)
        got.voxels.add_(1.0)                            # a caller's write under inference mode
        del got
    for k in (5, 4, 0):
        got = gen(torch.from_numpy(fs[k]).cuda(), poison=False)
        check_dense(_np(got), expected(k, **kw), 32)
        del got
    pool = list(gen._pool_map.values())[0]
    assert gen._pool_stats == dict(pooled=6, second=0, fresh=0) and len(pool.slots) == 1 and pool.rezeroed == 1


def test_frames_the_resident_route_does_not_take_build_no_buffer():
    from d3d_amd import _lib
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    gen = generator(**kw)
    fs = frames()
    for flag in (_lib.VOXEL_PATH_HASH, _lib.VOXEL_SPLIT_FILL):
        got = gen(torch.from_numpy(fs[0]).cuda(), poison=False, flags=flag)
        check_dense(_np(got), expected(0, **kw), 32)
        del got
    misaligned = torch.from_numpy(np.concatenate([np.zeros((1, 4), np.float32), fs[2]])).cuda().reshape(-1)[2:-2].reshape(-1, 4)
    assert misaligned.data_ptr() % 16 == 8
    exp = oracle.VoxelGenerator(*_grid(), dense=True, **kw)(misaligned.cpu().numpy())
    check_dense(_np(gen(misaligned, poison=False)), exp, 32)
    set_opts(voxel_flags=_lib.VOXEL_PATH_HASH)              # ... also when the calling context sets the path
    check_dense(_np(gen(torch.from_numpy(fs[1]).cuda(), poison=False)), expected(1, **kw), 32)
    assert gen._pool_stats == dict(pooled=0, second=0, fresh=4) and not gen._pool_map


def _grid():
    from d3d_amd import synth
    return synth.KITTI_BOUNDS, SHAPE


def test_under_the_poison_hook_the_call_takes_the_fresh_tensor_path():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    set_opts(poison=True)
    gen = generator(**kw)
    for k in (0, 1):
        got = gen(torch.from_numpy(frames()[k]).cuda())
        check_dense(_np(got), expected(k, **kw), 32)
        del got
    assert gen._pool_stats == dict(pooled=0, second=0, fresh=2) and not gen._pool_map


def test_host_frames_come_back_as_host_tensors_through_the_pool():
    kw = dict(max_points=32, max_voxels=60000, reduction="mean")
    gen = generator(**kw)
    for k in (0, 2):
        got = gen(torch.from_numpy(frames()[k]), poison=False)
        assert not got.voxels.is_cuda
        check_dense(_np(got), expected(k, **kw), 32)
    assert gen._pool_stats == dict(pooled=2, second=0, fresh=0)


# ---- early size notification: the C ABI, as test_dense_notify_publishes_the_counts_to_pinned_host_memory calls it

def _dense_call(entry, pts, P, max_voxels, note, resident):
    """one call on a frame already on the device -> (voxel count as the host learnt it, outputs)"""
    from d3d_amd import _lib, synth
    lib = _lib.load()
    n = int(pts.shape[0])
    cap = max(min(n, max_voxels), 1)
    shape = (ctypes.c_int32 * 3)(*SHAPE)
    bound = (ctypes.c_float * 6)(*synth.KITTI_BOUNDS)
    ws = _lib.workspace(lib.d3d_voxelize_workspace_bytes(n, 0), torch.device("cuda", 0))
    voxels = torch.zeros((cap, P, 4), device="cuda")
    state = torch.zeros((cap,), dtype=torch.int16, device="cuda")
    coords = torch.zeros((cap, 3), dtype=torch.int64, device="cuda")
    pmask = torch.zeros((cap, P), dtype=torch.uint8, device="cuda")
    npts = torch.zeros((cap,), dtype=torch.int32, device="cuda")
    agg = torch.zeros((cap, 4), device="cuda")
    counts = torch.full((_lib.NUM_COUNTS,), -1, dtype=torch.int64, device="cuda")
    head = [_lib.ptr(pts), n, 4, ctypes.cast(shape, ctypes.c_void_p), ctypes.cast(bound, ctypes.c_void_p), P, max_voxels, 1, _lib.ptr(voxels)]
    tail = [_lib.ptr(coords), _lib.ptr(pmask), _lib.ptr(npts), _lib.ptr(agg), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()]
    note.arm()
    fn = getattr(lib, entry)
    rc = fn(*head, _lib.ptr(state), *tail, note.ptr, 0) if resident else fn(*head, *tail, note.ptr, 0)
    assert rc == 0
    host = note.wait(counts, spin_s=5.0)
    assert note.arr[_lib.NUM_COUNTS] == 1                           # the flag itself, not the fallback read
    # exactly ONE notification per call: the host re-arms at once, as it does for its next frame, while this call's output
    # launch is still to run -- a second notification from there would raise the flag again
    note.arm()
    torch.cuda.synchronize()
    assert note.arr[_lib.NUM_COUNTS] == 0
    assert host == counts.cpu().tolist()                            # the pinned words equal the device counts[]
    nv = int(host[_lib.COUNT_VOXELS])
    return nv, dict(voxels=voxels[:nv], coords=coords[:nv], voxel_pmask=pmask[:nv].view(torch.bool), voxel_npoints=npts[:nv],
                    aggregates=agg[:nv])


def _notify_cases():
    from d3d_amd import synth
    cases = [("n=%d" % n, synth.lidar_like(max(n, 1), 51)[:n], n) for n in (0, 500, 511, 512, 513, 60000, 65536, 65537)]
    cases.append(("V above max_voxels", synth.lidar_like(30000, 52), 3000))
    outside = synth.lidar_like(6000, 53)
    outside[:, 0] += 500.0
    cases.append(("no point inside the grid", outside, 6000))
    return cases


@pytest.mark.parametrize("entry,resident", [("d3d_voxelize_3d_dense_notify", False), ("d3d_voxelize_3d_dense_resident", True),
                                            ("d3d_voxelize_3d_dense_pooled", True)])
def test_early_notification_publishes_the_device_counts(entry, resident):
    from d3d_amd import _lib, synth
    note = _lib.NotifyBuffer()
    for name, cloud, max_voxels in _notify_cases():
        if ("case", name) not in _cache:
            _cache[("case", name)] = oracle.VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, dense=True, max_points=8, reduction="mean",
                                                           max_voxels=max(max_voxels, 1))(cloud)
        exp = _cache[("case", name)]
        nv, got = _dense_call(entry, torch.from_numpy(cloud).cuda(), 8, max(max_voxels, 1), note, resident)
        assert nv == len(exp["coords"]), name
        if name == "V above max_voxels":
            assert nv == 3000
        if name in ("n=0", "no point inside the grid"):
            assert nv == 0
        check_dense(_np(got), exp, 8)


@pytest.mark.parametrize("entry,resident", [("d3d_voxelize_3d_dense_notify", False), ("d3d_voxelize_3d_dense_resident", True)])
def test_two_calls_back_to_back_through_one_notify_buffer_each_return_their_own_count(entry, resident):
    """a second notification of the first call would land after the host re-armed the buffer and hand the second call a stale count"""
    from d3d_amd import _lib, synth
    note = _lib.NotifyBuffer()
    big, small = synth.lidar_like(60000, 54), synth.lidar_like(6000, 55)
    want = {}
    for name, cloud in (("big", big), ("small", small)):
        want[name] = len(oracle.VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, dense=True, max_points=8, reduction="mean",
                                               max_voxels=60000)(cloud)["coords"])
    assert want["big"] != want["small"]
    big, small = torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()
    for _ in range(3):
        assert _dense_call(entry, big, 8, 60000, note, resident)[0] == want["big"]
        assert _dense_call(entry, small, 8, 60000, note, resident)[0] == want["small"]
