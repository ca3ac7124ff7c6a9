"""CPU: the numpy model of the table pooling (sparse_pool_reference.py) against a brute force over the coordinates, against torch's
dense max_pool3d / ones-weight conv3d and their autograd on the densified scenes, the identity between the sum's two directions,
and the argument checks of d3d_amd.voxel.sparse_pool and of the two C entries that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_cases as cases
import sparse_conv_reference as sref
import sparse_pool_reference as ref
import voxel_conv_reference as vref

SCENES = ("v1", "v63", "v65", "negative_odd", "batches")
DENSE_CONFIGS = ("k3s2p1", "k2s2p0")


def _batch(c, b):
    return np.zeros(len(c), np.int64) if b is None else b


def _some(rows):
    """the outputs the brute force visits: all of a small scene, every 9th of a large one"""
    return np.arange(rows) if rows <= 600 else np.arange(0, rows, 9)


def _features(v, c, seed):
    """distinct values: a max or min has one winner, np.max and the first-winner rule agree"""
    return np.random.default_rng(seed).permutation(v * c).reshape(v, c).astype(np.float64) / 7 - v * c / 15


@pytest.mark.parametrize("config", ("k3s2p1", "k2s2p0", "k1s1p0", "k312s213d211"))
@pytest.mark.parametrize("name", SCENES)
def test_model_is_the_brute_force_over_coordinates(name, config):
    c, b = cases.SCENES[name]
    oc, ob, t_out, _ = cases.model(name, config)
    ks, st, pad, dil = (sref.triple(x) for x in cases.CONFIGS[config])
    x = _features(len(c), 3, 1)
    some = _some(len(oc))
    for red in ref.REDUCTIONS:
        want, n = ref.brute(x, c, _batch(c, b), oc[some], ob[some], ks, st, pad, dil, red)
        got, arg, count = ref.forward(x, t_out, red, "f64")
        assert np.array_equal(count[some], n) and np.array_equal(count, (t_out >= 0).sum(1))
        if red in (ref.MAX, ref.MIN):
            assert np.array_equal(got[some], want)
            src = t_out[np.arange(len(oc))[:, None], arg.astype(np.int64)]            # the row the winning column names
            assert np.all(arg >= 0) and np.array_equal(x[src, np.arange(3)[None, :]], got)
        else:
            assert np.allclose(got[some], want, rtol=1e-12, atol=1e-12) and np.all(arg == -1)


@pytest.mark.parametrize("ks,dil", [(3, 1), ((1, 3, 5), (1, 2, 1))])
@pytest.mark.parametrize("name", ("v63", "v65", "batches"))
def test_model_through_a_neighbour_table_is_stride_one_pooling(name, ks, dil):
    c, b = cases.SCENES[name]
    tab = vref.table(c, ks, dil, b)
    ks3, dil3 = vref.triple(ks), vref.triple(dil)
    pad = tuple((k - 1) // 2 * d for k, d in zip(ks3, dil3))
    x = _features(len(c), 2, 2)
    some = _some(len(c))
    for red in ref.REDUCTIONS:
        want, n = ref.brute(x, c, _batch(c, b), c[some], _batch(c, b)[some], ks3, (1, 1, 1), pad, dil3, red)
        got, _, count = ref.forward(x, tab, red, "f64")
        assert np.array_equal(count[some], n) and np.allclose(got[some], want, rtol=1e-12, atol=1e-12)


def _dense(name, config):
    """the scene moved to the origin inside a box with a dense output -> (index tuples of the inputs and of the outputs into the
    dense grids, the grid's shape (N, X, Y, Z), the two tables)"""
    c, b = cases.SCENES[name]
    ids = np.zeros(len(c), np.int64) if b is None else np.unique(b, return_inverse=True)[1]
    local = c - c.min(0)
    ks, st, pad, dil = (sref.triple(x) for x in cases.CONFIGS[config])
    shape = (int(ids.max()) + 1,) + tuple(max(int(a) + 1, k) for a, k in zip(local.max(0), ks))
    oc, ob, t_out, t_in = sref.build(local, ks, st, pad, dil, ids, spatial_shape=shape[1:])
    at = tuple(torch.from_numpy(a) for a in (ids, local[:, 0], local[:, 1], local[:, 2]))
    at_out = tuple(torch.from_numpy(a) for a in (ob, oc[:, 0], oc[:, 1], oc[:, 2]))
    return at, at_out, shape, t_out, t_in


@pytest.mark.parametrize("config", DENSE_CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_model_is_dense_max_pool3d_and_its_autograd(name, config):
    """the grid holds -inf at the inactive sites, so they never win: max_pool3d read at the active outputs is the sparse max, and
    its autograd (distinct values: one winner) the model's backward through table_in, up to the order of an input's sum"""
    at, at_out, shape, t_out, t_in = _dense(name, config)
    ks, st, pad, _ = (sref.triple(x) for x in cases.CONFIGS[config])
    v, ch = len(at[0]), 3
    x = _features(v, ch, 3)
    g = np.random.default_rng(4).standard_normal((len(t_out), ch))
    for red, sign in ((ref.MAX, 1.0), (ref.MIN, -1.0)):
        xt = torch.from_numpy(x).requires_grad_()
        grid = torch.full(shape + (ch,), -np.inf, dtype=torch.float64).index_put(at, sign * xt).permute(0, 4, 1, 2, 3)
        y = sign * torch.nn.functional.max_pool3d(grid, ks, st, pad).permute(0, 2, 3, 4, 1)[at_out]
        y.backward(torch.from_numpy(g))
        out, arg, count = ref.forward(x, t_out, red, "f64")
        assert np.array_equal(out, y.detach().numpy())
        gf = ref.backward(g, t_in, False, red, "f64", arg, count)          # (autograd adds an input's shares in its own order)
        assert np.array_equal(gf != 0, xt.grad.numpy() != 0) and np.allclose(gf, xt.grad.numpy(), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("config", DENSE_CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_model_sum_is_a_ones_weight_conv3d_and_its_autograd(name, config):
    """zeros at the inactive sites add nothing: the depthwise all-ones conv3d at the active outputs is the sparse sum, the mean is that
    over the count; bound: n + 2 roundings of fp64 on the sum of magnitudes, n the kernel volume"""
    at, at_out, shape, t_out, t_in = _dense(name, config)
    ks, st, pad, dil = (sref.triple(x) for x in cases.CONFIGS[config])
    v, ch, kk = len(at[0]), 3, t_out.shape[1]
    x = _features(v, ch, 5)
    g = np.random.default_rng(6).standard_normal((len(t_out), ch))
    xt = torch.from_numpy(x).requires_grad_()
    grid = torch.zeros(shape + (ch,), dtype=torch.float64).index_put(at, xt).permute(0, 4, 1, 2, 3)
    y = torch.nn.functional.conv3d(grid, torch.ones((ch, 1) + ks, dtype=torch.float64), stride=st, padding=pad, dilation=dil, groups=ch)
    y = y.permute(0, 2, 3, 4, 1)[at_out]
    y.backward(torch.from_numpy(g))
    out, _, count = ref.forward(x, t_out, ref.SUM, "f64")
    eps = (kk + 2) * 2.0 ** -52
    assert np.all(np.abs(out - y.detach().numpy()) <= eps * ref.forward(np.abs(x), t_out, ref.SUM, "f64")[0])
    gf = ref.backward(g, t_in, False, ref.SUM, "f64")
    assert np.all(np.abs(gf - xt.grad.numpy()) <= eps * ref.backward(np.abs(g), t_in, False, ref.SUM, "f64"))
    mean, _, _ = ref.forward(x, t_out, ref.MEAN, "f64")
    assert np.array_equal(mean, out / count[:, None].astype(np.float64))
    # the mean's backward against autograd of the same indexing
    xt = torch.from_numpy(x).requires_grad_()
    padded = torch.cat([xt, xt.new_zeros((1, ch))])
    ym = padded[torch.from_numpy(np.where(t_out < 0, v, t_out).astype(np.int64))].sum(1) / torch.from_numpy(count.astype(np.float64))[:, None]
    ym.backward(torch.from_numpy(g))
    gm = ref.backward(g, t_in, False, ref.MEAN, "f64", count=count)
    assert np.allclose(gm, xt.grad.numpy(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_sum_backward_is_the_sum_forward_through_the_other_table(kind):
    _, _, t_out, t_in = cases.model("negative_odd", "k3s2p1")
    _, g = ref.of_kind(np.random.default_rng(7).standard_normal((len(t_out), 5)), kind)
    assert vref_same(ref.backward(g, t_in, False, ref.SUM, kind), ref.forward(g, t_in, ref.SUM, kind)[0])
    c, b = cases.SCENES["v65"]
    tab = vref.table(c, (1, 3, 5), 1, b)
    _, g = ref.of_kind(np.random.default_rng(8).standard_normal((65, 4)), kind)
    assert vref_same(ref.backward(g, tab, False, ref.SUM, kind), ref.forward(g, tab, ref.SUM, kind)[0])
    # mirrored, a neighbour table is its own transposed map: the max's gradient lands on the rows the forward named
    x = _features(65, 4, 9).astype(ref.fold_type(kind))
    out, arg, count = ref.forward(x, tab, ref.MAX, kind)
    gf = ref.backward(np.ones_like(g), tab, True, ref.MAX, kind, arg, count)
    wins = np.zeros_like(gf)
    np.add.at(wins, (tab[np.arange(65)[:, None], arg.astype(np.int64)], np.arange(4)[None, :]), 1)
    assert np.array_equal(gf, wins) and gf.sum() == 65 * 4


def vref_same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_first_winner_nan_and_signed_zero_rules():
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, -0.0, nan, -inf, 5.0], [1.0, 0.0, 2.0, inf, nan], [2.0, -0.0, nan, inf, 7.0]], np.float32)
    tab = np.array([[0, 1, 2], [2, -1, 0], [-1, -1, -1], [-1, 1, -1]], np.int32)
    out, arg, n = ref.forward(x, tab, ref.MAX, "f32")
    assert n.tolist() == [3, 2, 0, 1]
    assert arg.tolist() == [[2, 0, 0, 1, 1], [0, 0, 0, 0, 0], [-1] * 5, [1] * 5]
    assert np.signbit(out[0, 1]) and np.isnan(out[0, 2]) and np.isnan(out[0, 4]) and out[0, 3] == inf and out[0, 0] == 2
    assert not out[2].any() and not np.signbit(out[2]).any()
    out, arg, _ = ref.forward(x, tab, ref.MIN, "f32")
    assert arg.tolist() == [[0, 0, 0, 0, 1], [2, 0, 0, 2, 2], [-1] * 5, [1] * 5]
    out, _, _ = ref.forward(x, tab, ref.SUM, "f32")
    assert out[0, 0] == 4 and not np.signbit(out[0, 1]) and np.isnan(out[0, 2]) and np.isnan(out[0, 3])
    t = ref.to_tensor(out, "bf16")
    assert t.dtype == torch.bfloat16 and bool(torch.isnan(t[0, 2])) and float(t[0, 0]) == 4


def test_large_kernel_scene_has_a_winner_beyond_column_255():
    """what tests/test_gpu_sparse_pool.py relies on: on the full 8 x 8 x 8 block under kernel size 7 with features that grow with the
    row's position, some row's argmax sits in a column above 255 -- where a byte would have wrapped"""
    import sparse_pool_cases as pcases
    c, x, tab = pcases.large_kernel()
    assert tab.shape == (512, 343)
    _, arg, count = ref.forward(x.astype(np.float32), tab, ref.MAX, "f32")
    assert arg.max() > 255 and count.max() == 343 and count.min() == 64


# ---------------------------------------------------------------- the library's host side

def _fake_neighbors(v=6, k=27):
    """a VoxelNeighbors that was never built (building one needs a GPU): what the argument checks read of it"""
    from d3d_amd.voxel.conv import TableView as _TableView, VoxelNeighbors
    nb = VoxelNeighbors.__new__(VoxelNeighbors)
    nb.device, nb.num_voxels, nb.kernel_volume = torch.device("cuda", 0), v, k
    nb._view = _TableView(torch.zeros((v, k), dtype=torch.int32), v, k, nb.device)
    return nb


def test_host_side_validation_without_gpu():
    from d3d_amd.voxel import sparse_avg_pool3d, sparse_max_pool3d, sparse_pool3d
    x = torch.zeros((6, 4))
    for fn in (sparse_pool3d, sparse_max_pool3d, sparse_avg_pool3d):
        for owner in (torch.zeros((6, 27), dtype=torch.int32), None, "neighbors"):
            with pytest.raises(TypeError):
                fn(x, owner)
    nb = _fake_neighbors()
    for red in ("median", "", None, 2):
        with pytest.raises(ValueError, match="reduction"):
            sparse_pool3d(x, nb, red)
    with pytest.raises(TypeError):
        sparse_pool3d([[0.0] * 4] * 6, nb)
    for bad in (torch.zeros((6, 4), dtype=torch.int32), np.zeros((6, 4), np.int64), torch.zeros((6, 4), dtype=torch.complex64)):
        with pytest.raises(ValueError, match="float32, float64, float16 or bfloat16"):
            sparse_pool3d(bad, nb)
    for bad in (torch.zeros(6), torch.zeros((6, 4, 1)), torch.zeros(())):
        with pytest.raises(ValueError, match="2-D"):
            sparse_pool3d(bad, nb)
    for bad in (torch.zeros((5, 4)), torch.zeros((7, 4), dtype=torch.bfloat16), np.zeros((0, 4), np.float16)):
        with pytest.raises(ValueError, match="rows"):
            sparse_max_pool3d(bad, nb)


def test_refusals_without_launching():
    """every refusal of the two entries returns before any HIP call: they answer on a machine without a GPU, with pointers that are
    never followed"""
    from d3d_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    fwd = lambda feat=p, src=10, c=4, dtype=0, tab=p, rows=10, k=27, red=2, out=p: \
        lib.d3d_table_pool_forward(feat, src, c, dtype, tab, rows, k, red, out, None, None, None)
    bwd = lambda g=p, orows=10, c=4, dtype=0, tab=p, rows=10, k=27, red=4, arg=None, count=None, out=p: \
        lib.d3d_table_pool_backward(g, orows, c, dtype, tab, rows, k, 0, red, arg, count, out, None)
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    assert [fwd(src=-1), fwd(rows=-1), fwd(c=0), fwd(k=0), fwd(feat=None), fwd(tab=None), fwd(out=None)] == [bad] * 7
    assert [fwd(dtype=2), fwd(dtype=3), fwd(dtype=6), fwd(red=0), fwd(red=5), fwd(k=344), fwd(rows=2 ** 31), fwd(src=2 ** 31)] == [uns] * 8
    assert [bwd(orows=-1), bwd(rows=-1), bwd(c=0), bwd(k=0), bwd(g=None), bwd(tab=None), bwd(out=None)] == [bad] * 7
    assert [bwd(red=2), bwd(red=3), bwd(red=1), bwd(red=2, count=p), bwd(red=1, arg=p)] == [bad] * 5
    assert [bwd(dtype=2), bwd(dtype=-1), bwd(red=0), bwd(red=5), bwd(k=344), bwd(rows=2 ** 31), bwd(orows=2 ** 31)] == [uns] * 7
    for dtype in (0, 1, 4, 5):
        assert fwd(dtype=dtype, rows=0, feat=None, tab=None, out=None) == _lib.OK and bwd(dtype=dtype, rows=0, g=None, tab=None, out=None) == _lib.OK
