"""CPU: the ownership logic of the dense VoxelGenerator's output pool (d3d_amd.voxel._OutputPool) on host tensors -- when a
buffer may serve again without the caller being able to tell that its `voxels` was not a tensor of its own.  No kernel runs."""
import pytest
import torch

from d3d_amd.voxel import DenseOutputBuffer, _OutputPool, _spare_cap


def make_pool():
    built = []

    def make(cap):
        built.append(DenseOutputBuffer(cap, 4, "cpu", columns=3, pooled=True))
        return built[-1]
    return _OutputPool(make), built


def test_a_buffer_is_free_only_when_no_tensor_slice_or_view_of_it_is_alive():
    pool, built = make_pool()
    buf, how = pool.take(100, 128)
    assert how == "pooled" and buf.capacity == 128 and buf.voxels.shape == (128, 4, 3) and len(built) == 1
    for hold in (lambda b: b.voxels[:50],                           # the slice a call hands out
                 lambda b: b.voxels[:50].reshape(-1, 3),            # a reshaped view of it
                 lambda b: b.voxels[:50][3:7, 1],                   # a slice of the slice
                 lambda b: dict(voxels=b.voxels[:10]),              # inside a result dict
                 lambda b: b.voxels[:50].numpy()):                  # the memory through numpy
        kept = hold(buf)
        other, how = pool.take(100, 128)
        assert other is not buf and how == "second", "a live view must keep the buffer out of the pool"
        del kept
        again, how = pool.take(100, 128)
        assert again is buf and how == "pooled"
        del other, again
    assert len(built) == 2 and pool.rezeroed == 0
    # a copy is the caller's own memory: it pins nothing
    copy = buf.voxels[:50].clone()
    assert pool.take(100, 128)[0] is buf
    del copy


def test_an_in_place_op_on_a_view_marks_the_buffer_written():
    pool, built = make_pool()
    buf, _ = pool.take(10, 16)
    view = buf.voxels[:10]
    view.add_(1.0)                                                  # the caller treats the result as its own tensor
    buf.row_state.fill_(3)                                          # (what a call would have left)
    del view
    again, how = pool.take(10, 16)
    assert again is buf and how == "pooled" and pool.rezeroed == 1
    assert not buf.voxels.any() and not buf.row_state.any()
    # the re-zeroing is not itself a caller's write, reading is not one either
    total = float(buf.voxels[:10].sum())
    assert total == 0.0 and pool.take(10, 16)[0] is buf and pool.rezeroed == 1
    for write in (lambda v: v.__setitem__((0, 0, 0), 5.0), lambda v: v.reshape(-1).mul_(2.0), lambda v: v[2:4].zero_(),
                  lambda v: v.copy_(torch.ones_like(v))):
        view = buf.voxels[:10]
        write(view)
        del view
        before = pool.rezeroed
        assert pool.take(10, 16)[0] is buf and pool.rezeroed == before + 1 and not buf.voxels.any()


def test_the_third_concurrent_request_gets_none():
    pool, built = make_pool()
    a, how_a = pool.take(10, 16)
    ra = a.voxels[:10]
    b, how_b = pool.take(10, 16)
    rb = b.voxels[:10]
    c, how_c = pool.take(10, 16)
    assert (how_a, how_b, how_c) == ("pooled", "second", "fresh") and c is None and a is not b and len(built) == 2
    assert ra.untyped_storage().data_ptr() != rb.untyped_storage().data_ptr()
    del ra
    assert pool.take(10, 16) == (a, "second")                       # (b is still held outside)
    del rb
    assert pool.take(10, 16) == (a, "pooled") and len(built) == 2


def test_capacity_an_idle_buffer_that_is_too_small_is_replaced_and_a_busy_one_is_left_alone():
    pool, built = make_pool()
    a, _ = pool.take(10, 16)
    assert pool.take(16, 16)[0] is a                                # a few more voxels: the same buffer
    bigger, how = pool.take(17, 32)
    assert bigger is not a and bigger.capacity == 32 and how == "pooled" and len(pool.slots) == 1
    held = bigger.voxels[:17]
    second, how = pool.take(40, 48)
    assert second.capacity == 48 and how == "second" and len(pool.slots) == 2
    assert pool.take(5, 16)[0] is second and held.shape[0] == 17
    # capacities step as the sparse call's spare outputs do: at most 12.5 % above the frame, never a rebuild for a few more points
    assert _spare_cap(585000) >= 585000 and _spare_cap(585000) <= 585000 * 1.125 and _spare_cap(585000) == _spare_cap(585900)


def test_a_torch_without_the_storage_use_count_disables_pooling(monkeypatch):
    pool, built = make_pool()
    monkeypatch.delattr(torch._C, "_storage_Use_Count")
    assert pool.take(10, 16) == (None, "fresh") and not built and not pool.slots


def test_generator_switches_and_counters_without_a_device():
    from d3d_amd.voxel import VoxelGenerator
    gen = VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], max_points=4, dense=True)
    assert gen._resident is None and gen._pool_stats == dict(pooled=0, second=0, fresh=0)
    assert VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], dense=True, resident=False)._resident is False
    assert VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], dense=True, resident=True)._resident is True
    assert VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10])._resident is None       # (sparse: the switch means nothing)
    # host frames and poisoned calls never take a pooled buffer
    assert gen._pooled_buffer(torch.zeros(8, 4), False) == (None, "fresh", None)


def test_a_buffer_built_inside_inference_mode_serves_inside_and_outside_it():
    """the usual way to run a detector: the first call comes under torch.inference_mode().  The buffer must be an ordinary
    tensor all the same -- an inference tensor has no version counter -- and writes made in either mode are seen"""
    pool, built = make_pool()
    with torch.inference_mode():
        buf, how = pool.take(10, 16)
        assert how == "pooled" and not buf.voxels.is_inference() and not buf.row_state.is_inference()
        view = buf.voxels[:10]
        del view
        assert pool.take(10, 16) == (buf, "pooled") and pool.rezeroed == 0
        view = buf.voxels[:10]
        view.add_(1.0)
        del view
        assert pool.take(10, 16) == (buf, "pooled") and pool.rezeroed == 1 and not buf.voxels.any()
    assert pool.take(10, 16) == (buf, "pooled") and pool.rezeroed == 1
    view = buf.voxels[:4]
    view.mul_(3.0)
    del view
    with torch.inference_mode():
        assert pool.take(10, 16) == (buf, "pooled") and pool.rezeroed == 2
    assert len(built) == 1


def test_a_pool_whose_buffer_the_native_route_refused_keeps_nothing():
    pool, built = make_pool()
    buf, _ = pool.take(10, 16)
    pool.refuse(buf)
    assert not pool.slots and pool.take(10, 16) == (None, "fresh") and len(built) == 1


# ---- what a generator keeps from call to call lives beside it, per host thread (d3d_amd.voxel._CallState); no kernel runs

GENERATOR_KW = (dict(), dict(max_points=4, max_points_filter="trim", max_voxels=50, max_voxels_filter="descending"),
                dict(dense=True), dict(dense=True, resident=True))


def generators(more=()):
    from d3d_amd.voxel import VoxelGenerator
    return [VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], **kw) for kw in GENERATOR_KW + tuple(more)]


def twins(gen):
    import copy
    import pickle
    return [pickle.loads(pickle.dumps(gen)), copy.deepcopy(gen), copy.copy(gen)]


def assert_plain(gen):
    from d3d_amd.voxel import MaxPointsFilterType, MaxVoxelsFilterType, ReductionType
    for name, value in vars(gen).items():
        assert type(value) in (torch.Tensor, int, float, bool, type(None), ReductionType, MaxPointsFilterType,
                               MaxVoxelsFilterType), (name, type(value))


def assert_same_vars(twin, gen):
    assert twin is not gen and type(twin) is type(gen) and set(vars(twin)) == set(vars(gen))
    for name, value in vars(gen).items():
        other = vars(twin)[name]
        assert type(other) is type(value), name
        if isinstance(value, torch.Tensor):
            assert other.dtype == value.dtype and torch.equal(other, value), name
        else:
            assert other == value, name


def test_generators_stay_plain_copyable_objects_with_pools_of_their_own():
    from d3d_amd.voxel import release_cached_buffers
    for gen in generators(more=(dict(dense=True, max_points=4),)):
        assert_plain(gen)
        for twin in twins(gen):                                     # a fresh generator: pickle, deepcopy, copy
            assert_same_vars(twin, gen)
            assert_plain(twin)
            assert twin._resident is gen._resident and twin._pool_stats is not gen._pool_stats
            assert twin._pool_map is not gen._pool_map
        assert_plain(gen)                                           # (the pools looked at above are not kept on it)
    gen._pool_map["key"] = "pool"
    release_cached_buffers()                                        # (the calling thread's pools, of every generator)
    assert not gen._pool_map


def test_a_used_generator_is_as_plain_and_its_copies_start_with_state_of_their_own():
    import ctypes
    from d3d_amd.voxel import _call_state
    for gen in generators():
        before = dict(vars(gen))
        st = _call_state(gen)                                       # what __call__ fetches: arrays marshalled, block filled
        assert _call_state(gen) is st and gen._size_h is st.size_h
        assert list(st.shape_h) == [10, 10, 10] and list(st.bounds_h) == [0, 1, 0, 1, 0, 1] and list(st.size_h) == gen._size.tolist()
        assert list(st.args.coords_bound) == [0, 10, 0, 10, 0, 10] and list(st.args.coord_offset) == [0, 0, 0]
        assert set(vars(gen)) == set(before) and all(vars(gen)[k] is v for k, v in before.items())
        assert_plain(gen)
        states = [st]
        for twin in twins(gen):
            assert_same_vars(twin, gen)
            states.append(_call_state(twin))
            assert_plain(twin)
        assert len({id(s) for s in states}) == 4 and len({ctypes.addressof(s.args) for s in states}) == 4
        assert len({id(s.pools) for s in states}) == 4 and all(s.resident_buf is None and s.stats == states[0].stats for s in states)


def test_each_host_thread_has_state_of_its_own_that_goes_with_the_thread():
    import ctypes
    import gc
    import threading
    import weakref
    from d3d_amd.voxel import _call_state
    for gen in generators():
        mine = _call_state(gen)
        seen = {}

        def work():
            st = _call_state(gen)
            seen.update(ref=weakref.ref(st), again=_call_state(gen) is st, other=st is not mine, block=ctypes.addressof(st.args),
                        pools=id(st.pools))

        thread = threading.Thread(target=work)
        thread.start()
        thread.join()
        assert seen["again"] and seen["other"] and seen["block"] != ctypes.addressof(mine.args) and seen["pools"] != id(mine.pools)
        assert _call_state(gen) is mine
        gc.collect()
        assert seen["ref"]() is None, "a thread's state must end with the thread"
    ref = weakref.ref(mine)
    del mine, gen
    gc.collect()
    assert ref() is None, "a generator's state must end with the generator"


def test_the_sparse_argument_block_follows_the_settings_it_was_filled_from():
    from d3d_amd.voxel import MaxPointsFilterType, MaxVoxelsFilterType, VoxelGenerator, _call_state
    gen = VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], max_points=4, max_points_filter="trim", min_points=1, max_voxels=50,
                         max_voxels_filter="trim")

    def block():
        a = _call_state(gen).args
        return a.min_points, a.max_points, a.max_voxels, a.max_points_filter, a.max_voxels_filter

    st = _call_state(gen)
    assert block() == (1, 4, 50, 1, 1)
    gen._max_points = 2
    assert block() == (1, 2, 50, 1, 1) and _call_state(gen) is st
    gen._min_points, gen._max_voxels_filter = 3, MaxVoxelsFilterType.DESCENDING
    assert block() == (3, 2, 50, 1, 2)
    # the reference's checks (voxelize.cpp:359-362, :470) run again for a setting changed after first use, and keep failing
    gen._max_points_filter = MaxPointsFilterType.FARTHEST_SAMPLING
    for _ in range(2):
        with pytest.raises(ValueError, match="Farthest Sampling not implemented!"):
            _call_state(gen)
    gen._max_points_filter, gen._max_voxels = MaxPointsFilterType.TRIM, None
    with pytest.raises(ValueError, match="Must specify maximum voxel count to filter voxels!"):
        _call_state(gen)
    gen._max_voxels, gen._max_points = 50, None
    with pytest.raises(ValueError, match="Must specify maximum points per voxel to filter points!"):
        _call_state(gen)
    gen._max_points, gen._max_voxels_filter, gen._max_voxels = 7, MaxVoxelsFilterType.NONE, None
    assert block() == (3, 7, 0, 1, 0) and _call_state(gen) is st


def test_release_cached_buffers_drops_every_generators_pools_and_resident_buffer():
    from d3d_amd.voxel import _call_state, release_cached_buffers
    gens = generators()
    for gen in gens:
        gen._pool_map["key"] = "pool"
        _call_state(gen).resident_buf = DenseOutputBuffer(4, 4, "cpu")
        assert gen._pool_map and gen._resident_buf is not None
    release_cached_buffers()
    for gen in gens:
        assert not gen._pool_map and gen._resident_buf is None
