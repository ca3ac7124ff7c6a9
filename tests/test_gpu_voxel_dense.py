"""GPU: VoxelDenseMap, voxel_to_dense, voxel_to_bev, voxel_from_dense and the entries behind them (csrc/vdense.hip) against the numpy
model of voxel_dense_reference.py.  Every comparison is bit for bit: the operators move values, they compute none."""
import functools

import numpy as np
import pytest
import torch

import sparse_conv_reference as sref
import voxel_dense_cases as cases
import voxel_dense_reference as ref

pytestmark = pytest.mark.gpu

RICH = "3tp5-n3-random"              # three samples of 3 T + 5 cells, 30 % present, rows shuffled


def T(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared scenes are read-only)


def build(s, perm=None):
    from d3d_amd.voxel import VoxelDenseMap
    c, b = s.coords, s.batch
    if perm is not None:
        c, b = c[perm], (None if b is None else b[perm])
    return VoxelDenseMap(T(c), batch_index=T(b), **cases.kwargs(s))


@functools.lru_cache(maxsize=None)
def owner(name):
    return build(cases.scene(name))


def same_bits(t, a):
    """a tensor of a float dtype against the numpy integers of the expected bits: shape and every bit"""
    got = ref.bits(t)
    return got.shape == a.shape and got.dtype == a.dtype and np.array_equal(got, a)


def model(s):
    """the scene's arguments in the model's order"""
    return dict(coords=s.coords, batch=s.batch, origin=s.origin, axes=s.axes), dict(batch_size=cases.batch_size(s), spatial_shape=s.spatial_shape)


def run(fn, x, g, *args):
    x = x.detach().requires_grad_()           # (no clone: a misaligned view stays one)
    out = fn(x, *args)
    out.backward(g)
    return out.detach(), x.grad


def check(name, dtype, c, fill, seed=0, special=True, wrap=lambda t: t.cuda()):
    """both operators, forward and gradient, on scene `name` against the model; `wrap` puts a host tensor where the test wants it"""
    from d3d_amd.voxel import voxel_from_dense, voxel_to_dense
    s, dmap = cases.scene(name), owner(name)
    site, grid = model(s)
    v = len(s.coords)
    shape = (cases.batch_size(s), c) + ref.dense_shape(s.spatial_shape, s.axes)
    feat = cases.features(v, c, dtype, seed, special)
    dense = cases.features(int(np.prod(shape[:2])), int(np.prod(shape[2:])), dtype, seed + 1, special).reshape(shape)
    want_dense = ref.to_dense(ref.bits(feat), fill=ref.fill_bits(fill, dtype), **site, **grid)
    want_rows = ref.from_dense(ref.bits(dense), **site)
    out, gf = run(voxel_to_dense, wrap(feat), wrap(dense), dmap, fill)
    assert out.is_cuda and gf.is_cuda and out.is_contiguous() and out.dtype == dtype
    assert same_bits(out, want_dense), "to_dense"
    assert same_bits(gf, want_rows), "to_dense: gradient"
    rows, gd = run(voxel_from_dense, wrap(dense), wrap(feat), dmap)
    assert rows.is_cuda and gd.is_cuda and rows.is_contiguous() and rows.dtype == dtype
    assert same_bits(rows, want_rows), "from_dense"
    assert same_bits(gd, ref.to_dense(ref.bits(feat), fill=ref.fill_bits(0, dtype), **site, **grid)), "from_dense: gradient (fill 0)"
    return feat, out


# ---------------------------------------------------------------- the map

@pytest.mark.parametrize("name", cases.SCENES)
def test_map_is_the_model(name):
    s, dmap = cases.scene(name), owner(name)
    site, grid = model(s)
    assert dmap.cell.is_cuda and dmap.cell.dtype == torch.int64 and dmap.index.dtype == torch.int32
    assert (dmap.num_voxels, dmap.batch_size, dmap.spatial_shape) == (len(s.coords), cases.batch_size(s), tuple(s.spatial_shape))
    assert (dmap.dense_shape, dmap.origin, dmap.axes) == (ref.dense_shape(s.spatial_shape, s.axes), tuple(s.origin), tuple(s.axes))
    assert np.array_equal(dmap.cell.cpu().numpy(), ref.cell(s.coords, s.batch, s.spatial_shape, s.origin, s.axes))
    assert np.array_equal(dmap.index.cpu().numpy(), ref.index(s.coords, s.batch, grid["batch_size"], s.spatial_shape, s.origin, s.axes))


def test_map_refuses_outside_rows_bad_batch_values_and_duplicates():
    from d3d_amd.voxel import VoxelDenseMap
    shape, origin, n = (3, 4, 5), (-2, 7, 0), 2
    base = np.array([[-2, 7, 0], [0, 10, 4], [-1, 8, 2], [0, 7, 1]], np.int64)
    batch = np.array([0, 1, 1, 0], np.int64)
    kw = dict(spatial_shape=shape, origin=origin, axes=(1, 2, 0))
    assert VoxelDenseMap(T(base), batch_index=T(batch), batch_size=n, **kw).num_voxels == 4
    for axis in range(3):
        for value in (origin[axis] - 1, origin[axis] + shape[axis], -2 ** 63, 2 ** 63 - 1):
            c = base.copy()
            c[2, axis] = value
            with pytest.raises(ValueError, match="holds 1 rows outside"):
                VoxelDenseMap(T(c), batch_index=T(batch), batch_size=n, **kw)
            with pytest.raises(ValueError, match="holds 1 rows outside"):
                VoxelDenseMap(T(c[2:3]), **kw)
    c = base.copy()
    c[0, 0], c[3, 2] = 1, -1
    with pytest.raises(ValueError, match="holds 2 rows outside"):
        VoxelDenseMap(T(c), batch_index=T(batch), batch_size=n, **kw)
    for value in (-1, n, 2 ** 40):
        b = batch.copy()
        b[1] = value
        with pytest.raises(ValueError, match="holds 1 rows outside"):
            VoxelDenseMap(T(base), batch_index=T(b), batch_size=n, **kw)
    dup = np.concatenate([base, base[1:2]])
    with pytest.raises(ValueError, match="holds 1 rows whose"):
        VoxelDenseMap(T(dup), batch_index=T(np.append(batch, 1)), batch_size=n, **kw)
    assert VoxelDenseMap(T(dup), batch_index=T(np.append(batch, 0)), batch_size=n, **kw).num_voxels == 5       # another sample: no repeat
    with pytest.raises(ValueError, match="holds 3 rows whose"):
        VoxelDenseMap(T(np.concatenate([base, base[1:2], base[1:3]])), **kw)


# ---------------------------------------------------------------- the operators

@pytest.mark.parametrize("dtype", sorted(ref.DTYPES))
@pytest.mark.parametrize("name", cases.SCENES)
def test_operators_are_the_model_on_every_scene(name, dtype):
    """two channel counts and two fills per scene and dtype, walking through CHANNELS and FILLS with the scene's number; the features
    hold NaN (one with a payload), +-inf and -0.0"""
    k = cases.SCENES.index(name) + sorted(ref.DTYPES).index(dtype)
    for j in (0, 4):
        check(name, ref.DTYPES[dtype], cases.CHANNELS[(k + j) % len(cases.CHANNELS)], cases.FILLS[(k + j // 4) % len(cases.FILLS)], seed=k)


@pytest.mark.parametrize("dtype", sorted(ref.DTYPES))
@pytest.mark.parametrize("c", cases.CHANNELS)
def test_every_channel_count_and_fill(c, dtype):
    for k, fill in enumerate(cases.FILLS):
        feat, out = check(RICH, ref.DTYPES[dtype], c, fill, seed=10 + k)
    _, out = check("tp1-n1-checker", ref.DTYPES[dtype], c, 0, seed=20)
    # absent cells are +0.0 bits under the default fill: the odd cells of the checkerboard
    assert not ref.bits(out).reshape(1, c, -1)[:, :, 1::2].any()


def test_zero_channels_and_defaults():
    from d3d_amd.voxel import voxel_from_dense, voxel_to_bev, voxel_to_dense
    s, dmap = cases.scene(RICH), owner(RICH)
    out = voxel_to_dense(torch.zeros((dmap.num_voxels, 0), device="cuda"), dmap)
    assert tuple(out.shape) == (3, 0) + dmap.dense_shape
    assert tuple(voxel_from_dense(out, dmap).shape) == (dmap.num_voxels, 0)
    feat = cases.features(dmap.num_voxels, 5, torch.float32, 3).cuda()
    assert torch.equal(voxel_to_dense(feat, dmap), voxel_to_dense(feat, dmap, fill_value=0.0))
    assert tuple(voxel_to_bev(feat, dmap).shape) == (3, 5 * dmap.dense_shape[0]) + dmap.dense_shape[1:]


@pytest.mark.parametrize("dtype", sorted(ref.DTYPES))
@pytest.mark.parametrize("name", ("t-n3-random", "tp1-n3-random"))
def test_misaligned_views(name, dtype):
    """features and dense as contiguous views at an odd element offset of a larger buffer -- no 16-byte base on either side -- on a P that
    is a multiple of 16 / itemsize (T) and on one that is not (T + 1); C = 8 and 64 would take the 16-byte paths from an aligned base"""
    def odd(t):
        buf = torch.empty(t.numel() + 3, dtype=t.dtype, device="cuda")
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view
    for c in (8, 64):
        check(name, ref.DTYPES[dtype], c, 1.5, seed=c, wrap=odd)


# ---------------------------------------------------------------- consistency

def test_bev_is_a_view_in_torchs_layout():
    from d3d_amd.voxel import voxel_to_bev, voxel_to_dense
    s, dmap = cases.scene(RICH), owner(RICH)
    feat = cases.features(dmap.num_voxels, 6, torch.float32, 1).cuda().requires_grad_()
    bev = voxel_to_bev(feat, dmap, -1.0)
    dense = voxel_to_dense(feat, dmap, -1.0)
    a, b, d = dmap.dense_shape
    assert tuple(bev.shape) == (3, 6 * a, b, d) and bev.is_contiguous() and bev._base is not None      # a view of the dense result
    assert torch.equal(bev, dense.reshape(3, 6 * a, b, d))
    # torch's route: channels-last index_put, permute, reshape
    site, grid = model(s)
    n_, a_, b_, d_ = (T(x) for x in ref.sites(**site))
    want = torch.full((3, a, b, d, 6), -1.0, device="cuda").index_put((n_, a_, b_, d_), feat.detach()).permute(0, 4, 1, 2, 3).reshape(3, 6 * a, b, d)
    assert torch.equal(bev, want)
    g = torch.randn_like(bev)
    bev.backward(g)
    assert torch.equal(feat.grad, g.reshape(3, 6, a, b, d)[n_, :, a_, b_, d_])
    # numpy in, numpy out
    out = voxel_to_bev(feat.detach().cpu().numpy(), dmap, -1.0)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want.cpu().numpy())


@pytest.mark.parametrize("dtype", sorted(ref.DTYPES))
def test_row_order_does_not_matter_and_runs_repeat(dtype):
    from d3d_amd.voxel import voxel_from_dense, voxel_to_dense
    s, dmap = cases.scene(RICH), owner(RICH)
    feat = cases.features(dmap.num_voxels, 33, ref.DTYPES[dtype], 5, special=True).cuda()
    perm = np.random.default_rng(6).permutation(dmap.num_voxels)
    other = build(s, perm)
    first = voxel_to_dense(feat, dmap, 1.5)
    assert same_bits(voxel_to_dense(feat[T(perm)], other, 1.5), ref.bits(first))
    assert same_bits(voxel_to_dense(feat, dmap, 1.5), ref.bits(first))
    rows = voxel_from_dense(first, dmap)
    assert same_bits(rows, ref.bits(feat)) and same_bits(voxel_from_dense(first, dmap), ref.bits(rows))
    assert same_bits(voxel_from_dense(first, other), ref.bits(feat[T(perm)]))


def test_host_tensors_and_numpy_come_back_on_the_callers_side():
    from d3d_amd.voxel import VoxelDenseMap, voxel_from_dense, voxel_to_dense
    s = cases.scene(RICH)
    site, grid = model(s)
    dmap = VoxelDenseMap(np.array(s.coords), batch_index=torch.from_numpy(np.array(s.batch)), **cases.kwargs(s))       # numpy and host tensors
    assert dmap.index.is_cuda and torch.equal(dmap.index, owner(RICH).index)
    feat = cases.features(dmap.num_voxels, 7, torch.float32, 8)
    want = ref.to_dense(ref.bits(feat), fill=ref.fill_bits(0, torch.float32), **site, **grid)
    x = feat.clone().requires_grad_()
    out = voxel_to_dense(x, dmap)
    assert not out.is_cuda and same_bits(out, want)
    out.backward(out.detach())
    assert not x.grad.is_cuda and same_bits(x.grad, ref.bits(feat))
    back = voxel_from_dense(out.detach(), dmap)
    assert not back.is_cuda and same_bits(back, ref.bits(feat))
    got = voxel_to_dense(feat.numpy(), dmap)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got.view(np.int32), want)
    rows = voxel_from_dense(got, dmap)
    assert isinstance(rows, np.ndarray) and np.array_equal(rows, feat.numpy())
    with pytest.raises(ValueError, match="expects"):
        voxel_from_dense(out.detach()[:, :, :0], dmap)
    with pytest.raises(ValueError):
        voxel_from_dense(out.detach().long(), dmap)


@pytest.mark.parametrize("fn", ("voxel_to_dense", "voxel_from_dense"))
def test_gradcheck(fn):
    from d3d_amd import voxel
    name = "one-n3-full" if fn == "voxel_to_dense" else "tp1-n1-last_lane"
    s, dmap = cases.scene(name), owner(name)
    shape = (dmap.num_voxels, 3) if fn == "voxel_to_dense" else (dmap.batch_size, 2) + dmap.dense_shape
    x = torch.randn(shape, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(1)).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: getattr(voxel, fn)(t, dmap), (x,), eps=1e-6, atol=1e-7, rtol=1e-7, nondet_tol=0.0)


# ---------------------------------------------------------------- offsets past 2^31

def test_output_past_two_to_the_31_elements():
    """bf16, C = 130 on a 257^3 grid: 2.2e9 elements, 4.4 GB; a thousand voxels, the last cells among them"""
    from d3d_amd.voxel import VoxelDenseMap, voxel_from_dense, voxel_to_dense
    side, c, v = 257, 130, 1000
    assert c * side ** 3 > 2 ** 31
    r = np.random.default_rng(9)
    flat = np.unique(np.concatenate([r.integers(0, side ** 3, v - 3), side ** 3 - 1 - np.array([0, 1, 300])]))
    flat = flat[r.permutation(len(flat))]
    coords = np.stack(np.unravel_index(flat, (side,) * 3), 1)
    dmap = VoxelDenseMap(T(coords), (side,) * 3)
    feat = cases.features(len(flat), c, torch.bfloat16, 11).cuda()
    out = voxel_to_dense(feat, dmap)
    assert tuple(out.shape) == (1, c, side, side, side) and out.numel() > 2 ** 31
    assert int(torch.count_nonzero(out)) == int(torch.count_nonzero(feat)) > 0.99 * feat.numel()
    assert torch.equal(voxel_from_dense(out, dmap), feat)
    # direct reads at the highest offsets
    last = int(np.nonzero(flat == side ** 3 - 1)[0][0])
    assert torch.equal(out[0, :, side - 1, side - 1, side - 1], feat[last])
    assert out.view(-1)[out.numel() - 1] == feat[last, c - 1] and out.view(-1)[out.numel() - 3] == 0
    near = int(np.nonzero(flat == side ** 3 - 2)[0][0])
    assert torch.equal(out.view(c, -1)[:, side ** 3 - 2], feat[near])
    del out


# ---------------------------------------------------------------- a chain: sparse_conv3d -> voxel_to_dense against conv3d

def test_strided_conv_then_dense_is_conv3d_of_the_dense_input():
    """fp32: sparse voxels -> sparse_conv3d (k3 s2 p1, spatial_shape given, no bias) -> voxel_to_dense, against conv3d on the CPU in
    fp64 of the voxel_to_dense of the input.  EVERY cell is compared: the inactive ones are exact zeros on both sides (their bound is
    0).  The bound is sparse_conv_reference's dot-product bound (K Cin + 2) eps32 sum|x||w|, scattered to the cells by the model"""
    from d3d_amd.voxel import SparseConvMap, VoxelDenseMap, sparse_conv3d, voxel_to_dense
    shape, n, cin, cout = (9, 12, 7), 2, 5, 6
    ks, st, pad = (3, 3, 3), (2, 2, 2), (1, 1, 1)
    r = np.random.default_rng(12)
    flat = r.permutation(n * shape[0] * shape[1] * shape[2])[:150]
    batch, x_, y_, z_ = np.unravel_index(flat, (n,) + shape)
    coords = np.stack([x_, y_, z_], 1)
    x = r.standard_normal((len(flat), cin)).astype(np.float32)
    w = r.standard_normal((27, cin, cout)).astype(np.float32)
    cmap = SparseConvMap(T(coords), ks, st, pad, batch_index=T(batch), spatial_shape=shape)
    oshape = sref.out_shape(shape, ks, st, pad, 1)
    y = sparse_conv3d(T(x), cmap, T(w))
    got = voxel_to_dense(y, VoxelDenseMap(cmap.out_coords, oshape, batch_index=cmap.out_batch, batch_size=n)).cpu().numpy()
    dense_in = voxel_to_dense(T(x), VoxelDenseMap(T(coords), shape, batch_index=T(batch), batch_size=n)).cpu().double()
    wt = torch.from_numpy(w).double().reshape(ks + (cin, cout)).permute(4, 3, 0, 1, 2)
    want = torch.nn.functional.conv3d(dense_in, wt, None, stride=st, padding=pad).numpy()
    assert got.shape == want.shape == (n, cout) + tuple(oshape)
    oc, ob, t_out, _ = sref.build(coords, ks, st, pad, 1, batch, spatial_shape=shape)
    rows = (27 * cin + 2) * 2.0 ** -23 * sref.conv(np.abs(x), t_out, np.abs(w))
    bound = ref.to_dense(rows, oc, ob, n, oshape, (0, 0, 0), (0, 1, 2), 0.0)
    inactive = ref.to_dense(np.zeros((len(oc), cout)), oc, ob, n, oshape, (0, 0, 0), (0, 1, 2), 1.0) == 1.0
    assert inactive.any() and not want[inactive].any() and not got[inactive].any()
    assert np.all(np.abs(got - want) <= bound)
