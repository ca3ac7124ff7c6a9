"""CPU: the numpy model of d3d_amd.voxel.dense (voxel_dense_reference.py) against torch on the host, the scenes of
voxel_dense_cases.py against the model's preconditions, and every refusal of the Python layer that is raised before a GPU is needed."""
import numpy as np
import pytest
import torch

import voxel_dense_cases as cases
import voxel_dense_reference as ref


def _torch_dense(feat, coords, batch, n, shape, origin, axes):
    """spconv's route on the host: zeros in coordinate-column order with the channels last, advanced-index assignment, permute"""
    c = torch.from_numpy(np.asarray(coords).astype(np.int64)) - torch.tensor(origin)
    b = torch.zeros(len(c), dtype=torch.int64) if batch is None else torch.from_numpy(np.asarray(batch).astype(np.int64))
    grid = torch.zeros((n,) + tuple(shape) + (feat.shape[1],), dtype=feat.dtype)
    grid = grid.index_put((b, c[:, 0], c[:, 1], c[:, 2]), feat)
    return grid.permute(0, 4, 1 + axes[0], 1 + axes[1], 1 + axes[2]).contiguous()


def _grid_scene(seed, n=2, shape=(3, 4, 5), origin=(-2, 7, 0), count=40):
    r = np.random.default_rng(seed)
    flat = r.permutation(n * shape[0] * shape[1] * shape[2])[:count]
    b, x, y, z = np.unravel_index(flat, (n,) + shape)
    return np.stack([x, y, z], 1) + np.array(origin), b, n, shape, origin


@pytest.mark.parametrize("axes", cases.PERMUTATIONS)
def test_model_is_torchs_index_assignment_and_permute(axes):
    """all six axes orders on a non-cubic grid: a wrong permutation cannot hide"""
    coords, batch, n, shape, origin = _grid_scene(1)
    feat = torch.randn((len(coords), 5), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    want = _torch_dense(feat, coords, batch, n, shape, origin, axes)
    got = ref.to_dense(feat.numpy(), coords, batch, n, shape, origin, axes)
    assert got.shape == (n, 5) + tuple(shape[a] for a in axes) == tuple(want.shape)
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(ref.bev(got), want.reshape(n, -1, want.shape[3], want.shape[4]).numpy())
    assert np.array_equal(ref.from_dense(got, coords, batch, origin, axes), feat.numpy())
    # the flat cell and the index say the same as the 5-D indexing
    cell = ref.cell(coords, batch, shape, origin, axes)
    assert np.array_equal(got.transpose(0, 2, 3, 4, 1).reshape(-1, 5)[cell], feat.numpy())
    idx = ref.index(coords, batch, n, shape, origin, axes)
    assert np.array_equal(idx[cell], np.arange(len(coords))) and (idx >= 0).sum() == len(coords)
    assert ref.inside(coords, batch, n, shape, origin, axes).all()


def test_model_fill_and_bits():
    coords, batch, n, shape, origin = _grid_scene(3)
    x = cases.features(len(coords), 3, torch.bfloat16, 4, special=True)
    minus_inf = ref.fill_bits(float("-inf"), torch.bfloat16)
    assert minus_inf == np.int16(-128) and ref.fill_bits(0, torch.float64) == 0 and ref.fill_bits(1.5, torch.float16) == 0x3e00
    d = ref.to_dense(ref.bits(x), coords, batch, n, shape, origin, (2, 0, 1), minus_inf)
    assert (d == minus_inf).sum() >= 3 * (n * 60 - len(coords))
    assert np.array_equal(ref.from_dense(d, coords, batch, origin, (2, 0, 1)), ref.bits(x))
    assert torch.equal(ref.unbits(ref.bits(x), torch.bfloat16).view(torch.int16), x.view(torch.int16))


def test_model_gradient_is_torchs_autograd_of_index_put():
    """to_dense's gradient is from_dense of the incoming gradient (and the reverse), against autograd through index_put in fp64"""
    coords, batch, n, shape, origin = _grid_scene(5)
    axes = (2, 0, 1)
    g = torch.Generator().manual_seed(6)
    feat = torch.randn((len(coords), 4), dtype=torch.float64, generator=g, requires_grad=True)
    dense = _torch_dense(feat, coords, batch, n, shape, origin, axes)
    gout = torch.randn(dense.shape, dtype=torch.float64, generator=g)
    dense.backward(gout)
    assert np.array_equal(ref.from_dense(gout.numpy(), coords, batch, origin, axes), feat.grad.numpy())
    # the reverse: reading the sites of a dense leaf sends the gradient rows to the sites and zeros elsewhere
    leaf = torch.randn(dense.shape, dtype=torch.float64, generator=g, requires_grad=True)
    nn, a, b, d = (torch.from_numpy(x) for x in ref.sites(coords, batch, origin, axes))
    rows = leaf[nn, :, a, b, d]
    grow = torch.randn(rows.shape, dtype=torch.float64, generator=g)
    rows.backward(grow)
    assert np.array_equal(ref.to_dense(grow.numpy(), coords, batch, n, shape, origin, axes, 0), leaf.grad.numpy())


def test_tile_mirror_agrees_with_the_library():
    got = cases.library_tile()
    if got is not None:
        assert got == cases.TILE_MIRROR == cases.TILE
    assert cases.TILE >= 8 and cases.TILE % 8 == 0
    got = cases.library_sparse()
    if got is not None:
        assert got == cases.SPARSE_MIRROR == cases.SPARSE
    assert 1 <= cases.SPARSE and cases.SPARSE + 1 < cases.TILE


def test_scenes_cover_what_they_promise():
    t = cases.TILE
    assert sorted(cases.sizes().values()) == [1, t - 1, t, t + 1, 3 * t + 5]
    assert len(cases.SCENES) == 5 * 2 * len(cases.OCCUPANCIES)
    seen = {"axes": set(), "origin": set(), "int32": 0, "nobatch": 0, "unit": 0}
    for name in cases.SCENES:
        s = cases.scene(name)
        pname, n, kind = name.split("-")
        n, p = int(n[1:]), cases.sizes()[pname]
        v = len(s.coords)
        assert int(np.prod(s.spatial_shape)) == p and cases.batch_size(s) == n, name
        assert (s.batch is None) == (s.batch_size is None), name
        # the model's preconditions: all inside, unique
        assert ref.inside(s.coords, s.batch, n, s.spatial_shape, s.origin, s.axes).all(), name
        cell = ref.cell(s.coords, s.batch, s.spatial_shape, s.origin, s.axes)
        assert len(np.unique(cell)) == v and (v == 0 or (cell.min() >= 0 and cell.max() < n * p)), name
        per_stretch = collections_count(cell, n, p, t)
        if kind == "empty":
            assert v == 0
        elif kind == "last":
            assert cell.tolist() == [n * p - 1]
        elif kind == "full":
            assert v == n * p
        elif kind == "checker":
            assert sorted(cell.tolist()) == list(range(0, n * p, 2))
        elif kind == "first_lane":
            assert v >= n and all(k == 1 for k in per_stretch.values()) and all(c % p % t == 0 for c in cell), name
        elif kind == "last_lane":
            assert v >= n and all(k == 1 for k in per_stretch.values()), name
            assert all(c % p % t == t - 1 or c % p == p - 1 for c in cell), name
        elif kind == "threshold":
            want = [min(cases.SPARSE - 1 + j % 3, min(t, p - k)) for j, (s_, k) in enumerate((s_, k) for s_ in range(n) for k in range(0, p, t))]
            assert [per_stretch.get((s_, k // t), 0) for s_ in range(n) for k in range(0, p, t)] == want, name
        else:
            assert abs(v - 0.3 * n * p) <= 1 and (v < 3 or not np.array_equal(cell, np.sort(cell))), name
        seen["axes"].add(s.axes)
        seen["origin"].add(s.origin)
        seen["int32"] += s.coords.dtype == np.int32
        seen["nobatch"] += s.batch is None
        seen["unit"] += 1 in s.spatial_shape
    assert len(seen["axes"]) == 6 and min(min(o) for o in seen["origin"]) < 0
    assert seen["int32"] > 5 and seen["nobatch"] > 5 and seen["unit"] > 5


def collections_count(cell, n, p, t):
    """{(sample, stretch): present cells}"""
    out = {}
    for c in cell.tolist():
        key = (c // p, c % p // t)
        out[key] = out.get(key, 0) + 1
    return out


# ---- refusals of the Python layer: raised before a GPU is needed ----

def _coords(v=4):
    return np.stack([np.arange(v), np.zeros(v, np.int64), np.zeros(v, np.int64)], 1)


@pytest.mark.parametrize("wrong", [
    dict(axes=(0, 1, 1)), dict(axes=(0, 1)), dict(axes=(1, 2, 3)), dict(axes=0), dict(axes=(0.0, 1, 2)), dict(axes=(True, 0, 2)),
    dict(spatial_shape=(8, 0, 1)), dict(spatial_shape=(8, -1, 1)), dict(spatial_shape=(8, 1)), dict(spatial_shape=8),
    dict(spatial_shape=(8.0, 1, 1)), dict(origin=(0, 0)), dict(origin=0.5), dict(origin=(2 ** 63, 0, 0)),
    dict(batch_size=1), dict(batch_index=np.zeros(4, np.int64)), dict(batch_index=np.zeros(4, np.int64), batch_size=0),
    dict(batch_index=np.zeros(4, np.int64), batch_size=2.0), dict(batch_index=np.zeros(4, np.int64), batch_size=True),
    dict(batch_index=np.zeros(3, np.int64), batch_size=1), dict(batch_index=np.zeros(4, np.float32), batch_size=1),
    dict(coords=np.zeros((4, 2), np.int64)), dict(coords=np.zeros((4, 3), np.float32)), dict(coords=np.zeros((12,), np.int64)),
    dict(spatial_shape=(2 ** 20, 2 ** 20, 1)),
])
def test_map_refuses_bad_arguments_before_any_gpu(wrong, monkeypatch):
    from d3d_amd import _lib
    from d3d_amd.voxel import VoxelDenseMap

    def no_gpu():
        raise AssertionError("a GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    args = dict(coords=_coords(), spatial_shape=(8, 1, 1))
    args.update(wrong)
    with pytest.raises(ValueError):
        VoxelDenseMap(**args)


def test_map_refuses_wrong_types_and_too_many_voxels(monkeypatch):
    from d3d_amd import _lib
    from d3d_amd.voxel import VoxelDenseMap
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("a GPU was asked for")))
    with pytest.raises(TypeError):
        VoxelDenseMap([[0, 0, 0]], (1, 1, 1))
    with pytest.raises(TypeError):
        VoxelDenseMap(_coords(), (8, 1, 1), batch_index=[0, 0, 0, 0], batch_size=1)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        VoxelDenseMap(torch.empty((2 ** 31, 3), dtype=torch.int64, device="meta"), (8, 1, 1))


def test_without_a_gpu_the_map_raises_instead_of_computing_elsewhere():
    from d3d_amd.voxel import VoxelDenseMap
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            VoxelDenseMap(_coords(), (8, 1, 1))


def _paper_map(v=4, n=2, dense_shape=(2, 3, 4)):
    """a VoxelDenseMap that was never built: what the operators check before they touch its tensors"""
    from d3d_amd.voxel import VoxelDenseMap
    m = object.__new__(VoxelDenseMap)
    m.num_voxels, m.batch_size, m.dense_shape, m.device = v, n, dense_shape, torch.device("cuda", 0)
    return m


def test_operators_refuse_bad_arguments_before_any_gpu():
    from d3d_amd.voxel import voxel_from_dense, voxel_to_bev, voxel_to_dense
    m = _paper_map()
    for fn in (voxel_to_dense, voxel_to_bev, voxel_from_dense):
        with pytest.raises(TypeError):
            fn(torch.zeros(4, 3), "not a map")
        with pytest.raises(TypeError):
            fn([[0.0]], m)
        with pytest.raises(ValueError, match="int64"):
            fn(torch.zeros((4, 3), dtype=torch.int64), m)
    for fn in (voxel_to_dense, voxel_to_bev):
        with pytest.raises(ValueError, match="5 rows"):
            fn(torch.zeros(5, 3), m)
        with pytest.raises(ValueError):
            fn(torch.zeros(4), m)
        with pytest.raises(ValueError):
            fn(np.zeros((4, 3, 1), np.float32), m)
        for fill in ("0", None, True, torch.zeros(())):
            with pytest.raises(TypeError):
                fn(torch.zeros(4, 3), m, fill_value=fill)
    for shape in ((2, 3, 2, 3), (2, 3, 2, 3, 5), (1, 3, 2, 3, 4), (2, 3, 3, 2, 4), (2, 6, 3, 4), (4, 3)):
        with pytest.raises(ValueError, match="expects"):
            voxel_from_dense(torch.zeros(shape), m)


def test_exports():
    import d3d_amd.voxel as v
    from d3d_amd.voxel import dense
    for name in ("VoxelDenseMap", "voxel_to_dense", "voxel_to_bev", "voxel_from_dense"):
        assert name in v.__all__ and getattr(v, name) is getattr(dense, name)
    doc = dense.__doc__ + dense.voxel_to_dense.__doc__ + dense.voxel_from_dense.__doc__
    assert "channels-last" in doc and "nonzeros" in doc


def test_c_entries_refuse_bad_arguments_without_launching():
    """the checks of the three entries run before the first HIP call: no device needed.  One 64 KiB host buffer stands in for every
    device pointer"""
    import ctypes
    from d3d_amd import _lib
    lib = _lib.load()
    arena = (ctypes.c_char * (64 << 10))()
    dev = ctypes.addressof(arena)
    bad, unsupported, f32 = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.F32
    assert lib.d3d_vdense_tile_cells() == cases.TILE and lib.d3d_vdense_sparse_cells() == cases.SPARSE
    i64x3, i32x3 = ctypes.c_int64 * 3, ctypes.c_int32 * 3
    shape, origin, axes = i64x3(3, 4, 5), i64x3(0, 0, 0), i32x3(2, 0, 1)

    def vmap(v=4, shape=shape, origin=origin, axes=axes, n=1, coords=dev, cell=dev, index=dev, counts=dev):
        return lib.d3d_vdense_map(coords, None, v, shape, origin, axes, n, cell, index, counts, None)
    assert vmap(v=-1) == bad and vmap(n=0) == bad and vmap(shape=None) == bad and vmap(origin=None) == bad and vmap(axes=None) == bad
    assert vmap(axes=i32x3(0, 1, 1)) == bad and vmap(axes=i32x3(0, 1, 3)) == bad and vmap(axes=i32x3(-1, 1, 2)) == bad
    assert vmap(shape=i64x3(3, 0, 5)) == bad and vmap(counts=None) == bad and vmap(index=None) == bad
    assert vmap(coords=None) == bad and vmap(cell=None) == bad
    assert vmap(v=2 ** 31) == unsupported and vmap(shape=i64x3(2 ** 20, 2 ** 20, 1)) == unsupported

    def scatter(v=4, c=3, dtype=f32, n=1, p=60, feat=dev, index=dev, out=dev):
        return lib.d3d_vdense_scatter(feat, v, c, dtype, index, n, p, 0.0, out, None)

    def gather(v=4, c=3, dtype=f32, n=1, p=60, dense=dev, index=dev, out=dev):
        return lib.d3d_vdense_gather(dense, n, c, dtype, index, p, v, out, None)
    for fn in (scatter, gather):
        assert fn(v=-1) == bad and fn(c=-1) == bad and fn(n=-1) == bad and fn(p=-1) == bad
        assert fn(dtype=2) == unsupported and fn(dtype=3) == unsupported and fn(dtype=6) == unsupported and fn(v=2 ** 31) == unsupported
        assert fn(index=None) == bad and fn(out=None) == bad
        assert fn(c=0) == _lib.OK and fn(n=0) == _lib.OK and fn(p=0) == _lib.OK          # nothing to write: no launch
        assert fn(n=2 ** 20, p=2 ** 20) == unsupported
    assert scatter(feat=None) == bad and gather(dense=None) == bad and gather(v=0, dense=None, out=None) == _lib.OK
