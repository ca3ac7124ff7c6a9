"""CPU: the numpy model of d3d_amd.voxel.conv (voxel_conv_reference.py) against a brute-force table and against torch's dense conv3d
and its autograd on the densified scenes, the host-side validation of VoxelNeighbors / neighbor_gather / subm_conv3d and the
workspace query -- nothing here touches a GPU."""
import numpy as np
import pytest
import torch

import voxel_conv_cases as cases
import voxel_conv_reference as ref

EPS64 = 2.0 ** -52
CONV_SCENES = cases.SMALL + ("block12", "batches")
CONV_SHAPES = (((3, 3, 3), 1), ((1, 3, 5), (1, 2, 3)), ((5, 5, 5), 2), ((3, 1, 1), 1))


@pytest.mark.parametrize("name", cases.SMALL)
def test_model_table_is_the_brute_force_table(name):
    c, b = cases.SCENES[name]
    for ks in cases.KERNELS:
        for dil in cases.DILATIONS:
            assert np.array_equal(ref.table(c, ks, dil, b), ref.table_brute(c, ks, dil, b)), (ks, dil)


def test_model_table_keeps_batches_apart():
    c, b = cases.SCENES["batches"]
    sel = np.random.default_rng(0).permutation(len(c))[:500]
    assert np.array_equal(ref.table(c[sel], 3, 1, b[sel]), ref.table_brute(c[sel], 3, 1, b[sel]))
    tab = ref.table(c, 5, 1, b)
    has = tab >= 0
    assert np.array_equal(b[np.maximum(tab, 0)][has], np.broadcast_to(b[:, None], tab.shape)[has])
    with pytest.raises(AssertionError):
        ref.table(c, 3, 1, None)                                   # the cloud of batch 0 and 1 twice under one id


def test_column_order_on_the_lines():
    """a 40 x 1 x 1 line has neighbours in the columns that differ in ix alone, and so on: the axis and column order"""
    for axis, name in enumerate(("line_x", "line_y", "line_z")):
        c, _ = cases.SCENES[name]
        tab = ref.table(c, (3, 3, 3), 1)
        stride = (9, 3, 1)[axis]
        live = sorted({13 - stride, 13, 13 + stride})
        assert [k for k in range(27) if (tab[:, k] >= 0).any()] == live
        up = tab[:, 13 + stride]
        assert np.all(c[up[up >= 0], axis] == c[up >= 0, axis] + 1)


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_mirror_identity(name):
    c, b = cases.SCENES[name]
    for ks, dil in (((3, 3, 3), 1), ((1, 3, 5), (1, 2, 3)), ((5, 5, 5), 2)):
        tab = ref.table(c, ks, dil, b)
        k = tab.shape[1]
        assert np.array_equal(tab[:, (k - 1) // 2], np.arange(len(c)))
        v, col = np.nonzero(tab >= 0)
        assert np.array_equal(tab[tab[v, col], k - 1 - col], v)


def test_wrap_scene_crosses_the_end_of_the_hash_table():
    """a replay of the kernel's key, hash and linear probing: in `wrap` inserts must step from the last slot to slot 0 in any
    insertion order, and look-ups that hit and look-ups that miss cross the end as well"""
    c, _ = cases.SCENES["wrap"]
    absent = cases.wrap()[1]
    keys = ref.hash_keys(c)
    assert keys == c[:, 0].tolist()                                  # the line starts at 0 and y, z are constant: key = x
    log2cap = ref.hash_log2cap(len(c))
    cap = 1 << log2cap
    assert cap == 512 and cap >= 2 * len(c)
    late = [k for k in keys if ref.hash_home(k, log2cap) >= cap - cases.WRAP_WINDOW]
    assert len(late) == cases.WRAP_CHAIN                             # at most 8 of them fit before the end: the others wrap
    present = set(keys)
    for order in (keys, sorted(keys), sorted(keys, reverse=True), [keys[i] for i in np.random.default_rng(3).permutation(len(keys))]):
        slots, wrapped = ref.hash_replay(order, log2cap)
        assert wrapped >= cases.WRAP_CHAIN - cases.WRAP_WINDOW and len(slots) == len(keys)
        assert all(s in slots for s in range(cap - cases.WRAP_WINDOW, cap)) and all(s in slots for s in range(150))
        hits = [ref.hash_walk(k, slots, log2cap) for k in late if k - 1 in present]         # the +1 look-ups of the fed voxels
        assert len(hits) >= cases.WRAP_FED and all(h[0] for h in hits)
        assert sum(h[2] for h in hits) >= cases.WRAP_FED - cases.WRAP_WINDOW
        assert max(ref.hash_walk(k, slots, log2cap)[1] for k in keys) >= 100
        assert absent not in present and absent - 1 in present
        found, probes, crossed = ref.hash_walk(absent, slots, log2cap)                      # the +1 look-up of the voxel at absent - 1
        assert not found and crossed and probes >= 150
    tab = ref.table(c, (3, 1, 1), 1)
    assert (tab[:, 2] >= 0).sum() >= cases.WRAP_FED


def test_comb_keys_share_their_low_bits():
    c, _ = cases.SCENES["comb"]
    keys = ref.hash_keys(c)
    assert len(set(k & (2 ** 50 - 2) for k in keys)) == 1 and max(keys) < 2 ** 62


def _dense_conv(name, ks, dil, x, w, bias):
    """torch tensors (fp64) -> the dense conv3d of the scattered rows, read back at the active sites"""
    idx, shape = cases.dense(name)
    idx = torch.from_numpy(idx)
    k, cin, cout = w.shape
    at = tuple(idx[:, a] for a in range(4))
    grid = torch.zeros(shape + (cin,), dtype=x.dtype).index_put(at, x).permute(0, 4, 1, 2, 3)
    wd = w.reshape(ks + (cin, cout)).permute(4, 3, 0, 1, 2)
    pad = tuple((a - 1) // 2 * d for a, d in zip(ks, ref.triple(dil)))
    y = torch.nn.functional.conv3d(grid, wd, bias, padding=pad, dilation=ref.triple(dil))
    return y.permute(0, 2, 3, 4, 1)[at]


@pytest.mark.parametrize("name", CONV_SCENES)
def test_model_conv_and_backward_are_the_dense_conv3d(name):
    """within the dot-product bound of ref.bounds, derived there: (K Cin + 2) eps64 sum|x||w| per output, and the same with the
    reduction lengths K Cout (grad_features) and V (grad_weight, grad_bias) for the gradients"""
    c, b = cases.SCENES[name]
    v, cin, cout = len(c), 3, 2
    for ks, dil in CONV_SHAPES:
        tab = ref.table(c, ks, dil, b)
        r = np.random.default_rng(len(name) + ks[0])
        x, w = r.standard_normal((v, cin)), r.standard_normal((tab.shape[1], cin, cout))
        bias, g = r.standard_normal(cout), r.standard_normal((v, cout))
        xt, wt, bt = (torch.from_numpy(a).requires_grad_() for a in (x, w, bias))
        y = _dense_conv(name, ks, dil, xt, wt, bt)
        y.backward(torch.from_numpy(g))
        b_out, b_gf, b_gw, b_gb = ref.bounds(x, tab, w, g, EPS64, bias)
        gf, gw, gb = ref.conv_backward(x, tab, w, g)
        for what, got, want, bound in (("out", ref.conv(x, tab, w, bias), y.detach().numpy(), b_out), ("grad_features", gf, xt.grad.numpy(), b_gf),
                                       ("grad_weight", gw, wt.grad.numpy(), b_gw), ("grad_bias", gb, bt.grad.numpy(), b_gb)):
            assert got.shape == want.shape and np.all(np.abs(got - want) <= bound), (what, ks, dil)


def test_model_gather_backward_is_torch_autograd():
    """the gather as torch indexing: its autograd gradient (index_add: a sum in some order) within K eps64 sum|g| of the fold"""
    c, b = cases.SCENES["v65"]
    tab = ref.table(c, 3, 1, b)
    g = np.random.default_rng(1).standard_normal((65, 27, 4))
    x = torch.zeros((66, 4), dtype=torch.float64, requires_grad=True)       # row 65: the zero row of an absent neighbour
    x[torch.from_numpy(np.where(tab < 0, 65, tab).astype(np.int64))].backward(torch.from_numpy(g))
    got = ref.gather_backward(g, tab)
    mag = ref.gather_backward(np.abs(g), tab)
    assert np.all(np.abs(got - x.grad.numpy()[:65]) <= 27 * EPS64 * mag)
    f = cases.features(65, 4, np.float32)
    out = ref.gather(f, tab)
    assert out.shape == (65, 27, 4) and np.array_equal(out[:, 13], f) and np.array_equal(ref.gather(f, tab, True), out[:, ::-1])


def test_host_side_validation_without_gpu():
    from d3d_amd.voxel import VoxelNeighbors, neighbor_gather, subm_conv3d
    c = torch.zeros((6, 3), dtype=torch.int64)
    for ks in (2, 4, 0, 9, -1, (3, 3), (3, 2, 3), 3.0, (3, 3, 3, 3)):
        with pytest.raises(ValueError):
            VoxelNeighbors(c, kernel_size=ks)
    for dil in (0, -1, (1, 1), 1.5):
        with pytest.raises(ValueError):
            VoxelNeighbors(c, dilation=dil)
    for bad in (torch.zeros(6, dtype=torch.int64), torch.zeros((6, 2), dtype=torch.int64), torch.zeros((6, 3, 1), dtype=torch.int64),
                torch.zeros((6, 3)), np.zeros((6, 3), np.float64), torch.zeros((6, 3), dtype=torch.int16)):
        with pytest.raises(ValueError):
            VoxelNeighbors(bad)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros((6, 1), dtype=torch.int64), torch.zeros(6)):
        with pytest.raises(ValueError):
            VoxelNeighbors(c, batch_index=bad)
    with pytest.raises(TypeError):
        VoxelNeighbors([[0, 0, 0]])
    # a span product beyond 2^62: 2^21 + 1 per axis is 2^63 and more; with a batch span of 2 the product 2^62 * 2
    wide = np.array([[0, 0, 0], [2 ** 21, 2 ** 21, 2 ** 21]], np.int64)
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelNeighbors(wide)
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelNeighbors(torch.tensor([[-2 ** 62, 0, 0], [2 ** 62, 0, 0]]))
    edge = np.array([[0, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 0]], np.int64)  # 2^62 exactly: fits ...
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelNeighbors(edge, batch_index=np.array([0, 1]))                  # ... but not times two batches
    with pytest.raises(TypeError):
        neighbor_gather(torch.zeros((6, 3)), c)
    with pytest.raises(TypeError):
        subm_conv3d(torch.zeros((6, 3)), c, torch.zeros((27, 3, 2)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):              # no silent CPU fallback
            VoxelNeighbors(c)
        with pytest.raises(RuntimeError, match="HIP device"):
            VoxelNeighbors(edge)
        with pytest.raises(RuntimeError, match="HIP device"):
            VoxelNeighbors(np.zeros((0, 3), np.int32))


def test_workspace_query():
    from d3d_amd import _lib
    lib = _lib.load()
    sizes = (0, 1, 31, 32, 33, 1000, 4095, 4096, 4097, 10 ** 6, 2 * 10 ** 7, 2 ** 31 - 1)
    b = [lib.d3d_voxel_neighbors_workspace_bytes(v) for v in sizes]
    assert all(x > 0 and x % 256 == 0 for x in b) and b == sorted(b)
    for v, x in zip(sizes, b):
        cap = (x - 256) // 16                                       # the bounds, then key and row side by side: 16 bytes a slot
        assert cap >= 2 * v and cap & (cap - 1) == 0 and (x - 256) % 16 == 0
    assert b[8] == 2 * b[7] - 256                                   # the capacity doubles between 4096 and 4097 voxels
