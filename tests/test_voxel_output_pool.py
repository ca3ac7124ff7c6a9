"""CPU: the ownership logic of the dense VoxelGenerator's output pool (d3d_amd.voxel._OutputPool) on host tensors -- when a
buffer may serve again without the caller being able to tell that its `voxels` was not a tensor of its own.  No kernel runs."""
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


def test_generators_stay_plain_copyable_objects_with_pools_of_their_own():
    import copy
    from d3d_amd.voxel import VoxelGenerator, release_cached_buffers
    for kw in (dict(dense=True, max_points=4), dict()):
        gen = VoxelGenerator([0, 1, 0, 1, 0, 1], [10, 10, 10], **kw)
        twin = copy.deepcopy(gen)
        assert twin is not gen and twin._resident is None and twin._pool_stats is not gen._pool_stats
        assert twin._pool_map is not gen._pool_map
    gen._pool_map["key"] = "pool"
    release_cached_buffers()                                        # (the calling thread's pools, of every generator)
    assert not gen._pool_map
