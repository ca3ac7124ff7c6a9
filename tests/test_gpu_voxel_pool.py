"""GPU: VoxelIndex / voxel_pool / voxel_unpool (vpool.hip) -- unless a test says otherwise every comparison is BIT FOR BIT against
the numpy model (voxel_pool_reference.py: the strict left folds, the comparators, the backward rules): the four reductions, both
dtypes, `out`, `arg` and the backward pass, over the channel counts (vector and scalar rows, lane groups below, at and beyond a
wavefront), the fan-in per voxel, empty voxels, the -1 id, the launch / scan / sort boundaries and the special values."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_pool_cases as cases
import voxel_pool_reference as ref

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
CODE = {"mean": 1, "max": 2, "min": 3, "sum": 4}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def check_scene(m, v, c, dtypes=DTYPES, reductions=ref.REDUCTIONS, seed=0, index=None):
    """forward (`out`; `arg` as the operator writes it when a gradient is wanted) and backward of every reduction, and unpool, on
    one mapping: the model's bits"""
    from d3d_amd.voxel import VoxelIndex, voxel_pool, voxel_unpool
    from d3d_amd.voxel.pool import _forward
    idx = index if index is not None else VoxelIndex(T(m), v)
    for dtype in dtypes:
        f = cases.features(len(m), c, dtype, seed)
        g = np.random.default_rng(seed + 77).standard_normal((v, c)).astype(dtype)
        for red in reductions:
            want, want_arg = ref.pool(f, m, v, red)
            plain = voxel_pool(T(f), idx, reduction=red)                          # no gradient wanted: the kernel without `arg`
            assert plain.shape == (v, c) and plain.is_cuda and ref.same_bits(N(plain), want), (red, dtype, c)
            ft = T(f).requires_grad_()
            out = voxel_pool(ft, idx, reduction=red.upper())
            assert ref.same_bits(N(out), want), (red, dtype, c)
            if want_arg is not None:
                _, arg = _forward(T(f), idx, CODE[red], True)
                assert arg.dtype == torch.int32 and np.array_equal(N(arg), want_arg), (red, dtype, c)
            out.backward(T(g))
            assert ref.same_bits(N(ft.grad), ref.backward(g, m, v, red, want_arg)), (red, dtype, c)
        vf = T(g).requires_grad_()
        up = voxel_unpool(vf, idx)
        assert up.shape == (len(m), c) and ref.same_bits(N(up), ref.unpool(g, m))
        up.backward(T(f))
        assert ref.same_bits(N(vf.grad), ref.pool(f, m, v, "sum")[0])             # its backward is the sum forward


@pytest.mark.parametrize("c", [1, 3, 4, 5, 16, 63, 64, 65, 128])
def test_channel_counts(c):
    """vector rows (4, 16, 64, 128: groups of 1, 4, 16, 32 lanes in fp32 -- 2, 8, 32, 64 in fp64) and scalar rows (1, 3, 5, 63: a
    wavefront less one lane; 65: more than one pass of a whole wavefront)"""
    m, v = cases.mixed()
    check_scene(m, v, c, seed=c)


SCENES = cases.fan_in_scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_fan_in_empty_voxels_and_unmapped_points(name):
    m, v = SCENES[name]
    for c in (4, 5):
        check_scene(m, v, c, seed=len(name))


@pytest.mark.parametrize("k", cases.SIZES_K)
def test_point_counts(k):
    m, v = cases.random_mapping(k, max(1, k // 9), k, unmapped=0.05)
    check_scene(m, v, 4, dtypes=(np.float32,), seed=k)
    if k <= 4097:
        check_scene(m, v, 3, dtypes=(np.float64,), reductions=("mean", "min"), seed=k)


@pytest.mark.parametrize("v", cases.SIZES_V)
def test_voxel_counts(v):
    m, _ = cases.random_mapping(3001, v, v, unmapped=0.05)
    m[-1] = v - 1                                                                 # the last voxel is never empty
    check_scene(m, v, 4, dtypes=(np.float32,), seed=v)
    check_scene(m, v, 1, dtypes=(np.float64,), reductions=("sum", "max"), seed=v)


def test_nothing_to_do():
    from d3d_amd.voxel import VoxelIndex, voxel_pool, voxel_unpool
    none = np.zeros(0, np.int64)
    for red in ref.REDUCTIONS:
        f = torch.zeros((0, 3), device="cuda", requires_grad=True)
        out = voxel_pool(f, T(none), 5, reduction=red)                            # K = 0
        assert out.shape == (5, 3) and not out.any()
        out.sum().backward()
        assert f.grad.shape == (0, 3)
        assert voxel_pool(torch.zeros((0, 3), device="cuda"), T(none), 0, reduction=red).shape == (0, 3)      # K = 0 and V = 0
    unmapped = T(np.full(4, -1, np.int64))
    assert voxel_pool(torch.ones((4, 2), device="cuda"), unmapped, 0).shape == (0, 2)                         # V = 0
    up = voxel_unpool(torch.zeros((0, 2), device="cuda"), unmapped)
    assert up.shape == (4, 2) and not up.any()
    idx = VoxelIndex(none, 3)
    assert idx.num_mapped == 0 and N(idx.offsets).tolist() == [0, 0, 0, 0] and voxel_unpool(torch.ones((3, 2), device="cuda"), idx).shape == (0, 2)
    with pytest.raises(ValueError):
        VoxelIndex(T(np.array([0], np.int64)), 0)


def test_special_values():
    """NaN first, last and alone in a voxel, +0.0 against -0.0, +-inf, equal values (cases.special_values)"""
    for dtype in DTYPES:
        f, m, v = cases.special_values(dtype)
        from d3d_amd.voxel import VoxelIndex, voxel_pool
        from d3d_amd.voxel.pool import _forward
        idx = VoxelIndex(T(m), v)
        for red in ref.REDUCTIONS:
            want, want_arg = ref.pool(f, m, v, red)
            got, arg = _forward(T(f), idx, CODE[red], True)
            assert ref.same_bits(N(got), want), (red, dtype)
            if want_arg is not None:
                assert np.array_equal(N(arg), want_arg), (red, dtype)
                ft = T(f).requires_grad_()
                voxel_pool(ft, idx, reduction=red).backward(torch.ones((v, 2), dtype=ft.dtype, device="cuda"))
                assert ref.same_bits(N(ft.grad), ref.backward(np.ones((v, 2), dtype), m, v, red, want_arg))


def test_index_is_the_stable_argsort():
    from d3d_amd.voxel import VoxelIndex, voxel_pool
    for m, v in [cases.mixed(), SCENES["minus_one_sprinkled"], SCENES["crowded"], cases.random_mapping(131073, 40000, 3, unmapped=0.2),
                 cases.random_mapping(30000, 7, 4), cases.random_mapping(5000, 4097, 5)]:
        order, offsets = ref.index(m, v)
        for mt in (T(m), T(m.astype(np.int32)), torch.from_numpy(m)):
            idx = VoxelIndex(mt, v)
            assert idx.order.dtype == torch.int32 and idx.offsets.dtype == torch.int64 and idx.mapping.dtype == torch.int64
            assert idx.num_mapped == len(order) and np.array_equal(N(idx.order), order) and np.array_equal(N(idx.offsets), offsets)
    m, v = cases.mixed()
    f = T(cases.features(len(m), 8, np.float32))
    idx = VoxelIndex(T(m), v)
    for red in ref.REDUCTIONS:                                                    # a bare mapping builds the same index
        assert ref.same_bits(N(voxel_pool(f, idx, reduction=red)), N(voxel_pool(f, T(m), v, reduction=red)))
        assert ref.same_bits(N(voxel_pool(f, idx, v, reduction=red)), N(voxel_pool(f, T(m), num_voxels=v, reduction=red)))
    with pytest.raises(ValueError):
        voxel_pool(f, idx, v + 1)


@pytest.mark.parametrize("bad", ["V", "V+5", "-2"])
def test_ids_out_of_range_are_refused_and_touch_nothing(bad):
    from d3d_amd.voxel import VoxelIndex, voxel_pool
    m, v = cases.mixed()
    wrong = m.copy()
    wrong[[3, 1200, len(m) - 1]] = {"V": v, "V+5": v + 5, "-2": -2}[bad]
    with pytest.raises(ValueError, match="3 voxel ids outside"):
        VoxelIndex(T(wrong), v)
    with pytest.raises(ValueError):
        voxel_pool(T(cases.features(len(m), 4, np.float32)), T(wrong), v)
    check_scene(m, v, 4, dtypes=(np.float32,))                                    # the next call on the stream is as good as ever


def test_real_mapping_of_the_sparse_voxelizer():
    from d3d_amd import synth
    from d3d_amd.voxel import VoxelGenerator
    pts = torch.from_numpy(synth.lidar_like(20_000, 0)).cuda()
    sp = VoxelGenerator(synth.KITTI_BOUNDS, synth.KITTI_SHAPE, max_points=32, max_points_filter="trim")(pts)
    m, v = N(sp.points_mapping), int(sp.coords.shape[0])
    assert len(m) == sp.points.shape[0] and m.min() >= -1 and m.max() < v and v > 1000
    check_scene(m, v, 16, dtypes=(np.float32,), seed=1)
    check_scene(m, v, 3, dtypes=(np.float64,), reductions=("mean", "max"), seed=2)


def test_fp32_sums_against_exact_arithmetic():
    """|got - exact| <= (count - 1) u sum|x| for the left fold of `count` fp32 numbers, u = 2^-24 (each of the count - 1 additions
    rounds a partial sum that is at most sum|x| in magnitude, to first order; the first addition, to 0, is exact); the mean's one
    division adds u |mean|.  `exact` is the fp64 sum of the fp32 inputs (exact to 2^-53 sum|x|: nothing beside 2^-24).  Every element.
    Measured on an MI355X: the worst element at 0.93 of the bound for sum, 0.70 for mean (voxels of two points, where one rounding
    of a sum near sum|x| is all there is; the voxel of 2000 points stays far below)."""
    from d3d_amd.voxel import voxel_pool
    m, v = cases.from_counts([2000, 1, 0, 2, 500] + [3] * 799 + [100], 21)
    assert len(m) == 5000
    f = cases.features(len(m), 16, np.float32, 21) * np.float32(37.0)
    f64, kept = f.astype(np.float64), m >= 0
    exact, mag = np.zeros((v, 16)), np.zeros((v, 16))
    np.add.at(exact, m[kept], f64[kept])
    np.add.at(mag, m[kept], np.abs(f64[kept]))
    cnt = np.bincount(m[kept], minlength=v).astype(np.float64)[:, None]
    u = 2.0 ** -24
    bound = np.maximum(cnt - 1, 0) * u * mag
    got = N(voxel_pool(T(f), T(m), v, reduction="sum")).astype(np.float64)
    err = np.abs(got - exact)
    print("sum: worst |err| / bound = %.4f" % np.max(err[bound > 0] / bound[bound > 0]))
    assert np.all(err <= bound)
    gotm = N(voxel_pool(T(f), T(m), v, reduction="mean")).astype(np.float64)
    exactm = exact / np.maximum(cnt, 1)
    boundm = bound / np.maximum(cnt, 1) + u * np.abs(exactm)
    errm = np.abs(gotm - exactm)
    print("mean: worst |err| / bound = %.4f" % np.max(errm[boundm > 0] / boundm[boundm > 0]))
    assert np.all(errm <= boundm)


def test_gradcheck_fp64():
    from d3d_amd.voxel import VoxelIndex, voxel_pool, voxel_unpool
    k, v, c = 40, 7, 3
    r = np.random.default_rng(8)
    m = r.integers(-1, v - 1, k).astype(np.int64)                                 # some -1; voxel 6 stays empty
    idx = VoxelIndex(T(m), v)
    f = T(r.permutation(k * c).reshape(k, c) * 1e-2 + r.uniform(0, 5e-3, (k, c))).requires_grad_()     # all values >= 5e-3 apart
    vals = np.sort(N(f).ravel())
    assert np.min(np.diff(vals)) >= 1e-3
    for red in ref.REDUCTIONS:
        assert torch.autograd.gradcheck(lambda x: voxel_pool(x, idx, reduction=red), (f,))
    vf = torch.randn(v, c, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: voxel_unpool(x, idx), (vf,))
    assert torch.autograd.gradcheck(lambda x: voxel_pool(x, T(m), v, reduction="mean"), (f,))


def test_offsets_past_2_31():
    """K = 2^25 + 1 rows of 64 floats: the last row starts at element 2^31.  All ids -1 but those of the last 100 points (7 voxels),
    so the model needs those rows only; forward max and sum, and the backward's last rows"""
    if torch.cuda.mem_get_info()[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    from d3d_amd.voxel import VoxelIndex, voxel_pool
    k, c, v, n = 2 ** 25 + 1, 64, 7, 100
    tail_m = np.random.default_rng(9).integers(0, v, n).astype(np.int64)
    tail_f = cases.features(n, c, np.float32, 9)
    g = np.random.default_rng(10).standard_normal((v, c)).astype(np.float32)
    m = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    m[-n:] = T(tail_m)
    idx = VoxelIndex(m, v)
    assert idx.num_mapped == n and np.array_equal(N(idx.order) - (k - n), ref.index(tail_m, v)[0])
    f = torch.zeros((k, c), device="cuda")
    f[-n:] = T(tail_f)
    want, _ = ref.pool(tail_f, tail_m, v, "sum")
    assert ref.same_bits(N(voxel_pool(f, idx, reduction="sum")), want)
    f.requires_grad_()
    want, arg = ref.pool(tail_f, tail_m, v, "max")
    out = voxel_pool(f, idx, reduction="max")
    assert ref.same_bits(N(out), want)
    out.backward(T(g))
    assert ref.same_bits(N(f.grad[-n:]), ref.backward(g, tail_m, v, "max", arg))
    assert not f.grad[:4096].any() and not f.grad[2 ** 24:2 ** 24 + 4096].any() and not f.grad[-n - 4096:-n].any()


def _raw(lib, m, v, f, red):
    """the three C entries by hand on device tensors -> (rc list, out, arg, grad_feat of a ones gradient, counts)"""
    k, c = f.shape
    code = 0 if f.dtype == torch.float32 else 1
    order = torch.empty(k, dtype=torch.int32, device="cuda")
    offsets = torch.empty(v + 1, dtype=torch.int64, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.d3d_voxel_index_workspace_bytes(k, v), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rcs = [lib.d3d_voxel_index(p(m), k, v, p(order), p(offsets), p(counts), p(ws), ws.numel(), st)]
    out = torch.empty((v, c), dtype=f.dtype, device="cuda")
    arg = torch.empty((v, c), dtype=torch.int32, device="cuda")
    rcs.append(lib.d3d_voxel_pool_forward(p(f), k, c, code, p(order), p(offsets), v, red, p(out), p(arg), st))
    grad = torch.empty((k, c), dtype=f.dtype, device="cuda")
    rcs.append(lib.d3d_voxel_pool_backward(p(torch.ones_like(out)), v, c, code, p(m), k, p(offsets), red, p(arg), p(grad), st))
    return rcs, out, arg, grad, counts


def test_raw_entries_and_a_misaligned_feature_base():
    """a feature tensor whose base is one element past a 16-byte boundary takes the element-wise route and gives the same bits"""
    from d3d_amd import _lib
    lib = _lib.load()
    m, v = cases.mixed()
    for dtype, c in ((np.float32, 4), (np.float32, 64), (np.float64, 2)):
        f = cases.features(len(m), c, dtype, 3)
        slab = torch.zeros(f.size + 1, dtype=T(f).dtype, device="cuda")
        shifted = slab[1:].view(len(m), c)
        shifted.copy_(T(f))
        assert shifted.data_ptr() % 16 == f.itemsize
        for red in ref.REDUCTIONS:
            want, want_arg = ref.pool(f, m, v, red)
            for ft in (T(f), shifted):
                rcs, out, arg, grad, counts = _raw(lib, T(m), v, ft, CODE[red])
                assert rcs == [0, 0, 0] and N(counts).tolist() == [int((m >= 0).sum()), 0]
                assert ref.same_bits(N(out), want)
                if want_arg is not None:
                    assert np.array_equal(N(arg), want_arg)
                assert ref.same_bits(N(grad), ref.backward(np.ones((v, c), dtype), m, v, red, want_arg))


def test_raw_entries_refuse_without_launching():
    from d3d_amd import _lib
    lib = _lib.load()
    m, v = cases.mixed()
    k, c = len(m), 4
    mt, f = T(m), T(cases.features(k, c, np.float32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    order = torch.full((k,), -7, dtype=torch.int32, device="cuda")
    offsets = torch.full((v + 1,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    need = lib.d3d_voxel_index_workspace_bytes(k, v)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    assert lib.d3d_voxel_index(None, k, v, p(order), p(offsets), p(counts), p(ws), need, st) == _lib.ERR_BAD_ARG
    assert lib.d3d_voxel_index(p(mt), k, v, p(order), None, p(counts), p(ws), need, st) == _lib.ERR_BAD_ARG
    assert lib.d3d_voxel_index(p(mt), -1, v, p(order), p(offsets), p(counts), p(ws), need, st) == _lib.ERR_BAD_ARG
    assert lib.d3d_voxel_index(p(mt), k, v, p(order), p(offsets), p(counts), p(ws), need - 1, st) == _lib.ERR_WORKSPACE
    assert lib.d3d_voxel_index(p(mt), k, v, p(order), p(offsets), p(counts), None, need, st) == _lib.ERR_WORKSPACE
    assert lib.d3d_voxel_index(p(mt), 2 ** 31, v, p(order), p(offsets), p(counts), p(ws), need, st) == _lib.ERR_UNSUPPORTED
    out = torch.full((v, c), -7.0, device="cuda")
    arg = torch.full((v, c), -7, dtype=torch.int32, device="cuda")
    grad = torch.full((k, c), -7.0, device="cuda")
    fwd = lambda feat, red, dtype=0, o=p(out): lib.d3d_voxel_pool_forward(feat, k, c, dtype, p(order), p(offsets), v, red, o, p(arg), st)
    assert fwd(None, 2) == _lib.ERR_BAD_ARG and fwd(p(f), 2, o=None) == _lib.ERR_BAD_ARG
    assert fwd(p(f), 7) == _lib.ERR_UNSUPPORTED and fwd(p(f), 0) == _lib.ERR_UNSUPPORTED and fwd(p(f), 2, dtype=3) == _lib.ERR_UNSUPPORTED
    bwd = lambda g, red, a=p(arg), o=p(grad): lib.d3d_voxel_pool_backward(g, v, c, 0, p(mt), k, p(offsets), red, a, o, st)
    assert bwd(None, 4) == _lib.ERR_BAD_ARG and bwd(p(out), 2, a=None) == _lib.ERR_BAD_ARG and bwd(p(out), 4, o=None) == _lib.ERR_BAD_ARG
    assert bwd(p(out), 7) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (order, offsets, counts, arg):
        assert bool((t == -7).all())
    assert bool((out == -7).all()) and bool((grad == -7).all()) and not ws.any()


def test_host_tensors_and_numpy_arrays():
    from d3d_amd.voxel import voxel_pool, voxel_unpool
    m, v = cases.mixed()
    f = cases.features(len(m), 5, np.float32, 4)
    for red in ref.REDUCTIONS:
        want = N(voxel_pool(T(f), T(m), v, reduction=red))
        a = voxel_pool(f, m, v, reduction=red)
        assert isinstance(a, np.ndarray) and ref.same_bits(a, want)
        b = voxel_pool(torch.from_numpy(f), torch.from_numpy(m), v, reduction=red)
        assert torch.is_tensor(b) and b.device.type == "cpu" and ref.same_bits(b.numpy(), want)
    ft = torch.from_numpy(f).requires_grad_()
    voxel_pool(ft.t().contiguous().t(), torch.from_numpy(m), v, reduction="max").sum().backward()          # a non-contiguous view
    assert ft.grad.device.type == "cpu" and ref.same_bits(ft.grad.numpy(), ref.backward(np.ones((v, 5), np.float32), m, v, "max", ref.pool(f, m, v, "max")[1]))
    vf = np.random.default_rng(2).standard_normal((v, 5))
    up = voxel_unpool(vf, m)
    assert isinstance(up, np.ndarray) and up.dtype == np.float64 and ref.same_bits(up, ref.unpool(vf, m))
    assert voxel_unpool(torch.from_numpy(vf), torch.from_numpy(m)).device.type == "cpu"
