"""CPU: the numpy model of d3d_amd.voxel.sparse_conv (sparse_conv_reference.py) against an O(V Vout) brute force and against torch's
dense conv3d / conv_transpose3d and their autograd on the densified scenes, the identities of the two tables, the host-side
validation of SparseConvMap / sparse_conv3d / sparse_inverse_conv3d and the workspace query -- nothing here touches a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_cases as cases
import sparse_conv_reference as ref
import voxel_conv_cases as vcases
import voxel_conv_reference as vref

EPS64 = 2.0 ** -52
DENSE_SCENES = ("v1", "v63", "v65", "negative_odd", "line_x", "block12", "batches")


def _i32x3(x):
    return (ctypes.c_int32 * 3)(*ref.triple(x))


@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
@pytest.mark.parametrize("name", cases.SMALL)
def test_model_is_the_brute_force(name, config):
    c, b = cases.SCENES[name]
    shapes = (None,) if cases.shape_of(name, config) is None else (None, cases.shape_of(name, config))
    for shape in shapes:
        got = ref.build(c, *cases.CONFIGS[config], batch=b, spatial_shape=shape)
        want = ref.build_brute(c, *cases.CONFIGS[config], batch=b, spatial_shape=shape)
        for a, e in zip(got, want):
            assert np.array_equal(a, e), shape


def test_model_keeps_batches_apart():
    c, b = cases.SCENES["batches_negative"]
    sel = np.random.default_rng(0).permutation(len(c))[:120]
    for a, e in zip(ref.build(c[sel], 3, 2, 1, 1, b[sel]), ref.build_brute(c[sel], 3, 2, 1, 1, b[sel])):
        assert np.array_equal(a, e)
    oc, ob, t_out, _ = cases.model("batches_negative", "k3s2p1")
    has = t_out >= 0
    assert np.array_equal(b[np.maximum(t_out, 0)][has], np.broadcast_to(ob[:, None], t_out.shape)[has])
    assert sorted(set(ob.tolist())) == [0, 1, 5] and len(set(zip(ob.tolist(), *oc.T.tolist()))) == len(oc)
    with pytest.raises(AssertionError):
        ref.build(c, 3, 2, 1, 1, None)                              # the cloud of batch 0 and 1 twice under one id


def test_negative_coordinates_floor():
    """`negative_odd` tells a floor division from a truncating one.  k2 s2 p0 sends input i to output floor(i / 2) (through column
    i mod 2, the mathematical one); rounding the quotient towards zero instead merges the cells -1 and 0 of every axis"""
    c, _ = cases.SCENES["negative_odd"]
    assert c.min() < 0 and np.any(c[c < 0] % 2 != 0) and np.any(c[c < 0] % 3 != 0)
    oc, _, t_out, t_in = cases.model("negative_odd", "k2s2p0")
    assert np.array_equal(oc[t_in.max(1)], c // 2) and np.array_equal(np.argmax(t_in >= 0, 1), (c % 2) @ np.array([4, 2, 1]))
    truncated = np.trunc(c / 2).astype(np.int64)
    assert np.any(truncated != c // 2) and len(np.unique(truncated, axis=0)) < len(np.unique(oc, axis=0))
    # k3 s3 p0: output floor(i / 3) through column i mod 3; C's remainder of a negative i is negative: no column at all
    oc, _, t_out, t_in = cases.model("negative_odd", "k3s3p0")
    assert np.array_equal(oc[t_in.max(1)], c // 3) and np.any(np.fmod(c, 3) < 0)


@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_duality_and_row_order(name, config):
    """table_out[r, k] == v <=> table_in[v, k] == r; the rows are numbered by their first candidate; every output has an input"""
    c, b = cases.SCENES[name]
    for with_shape in (False, True) if cases.shape_of(name, config) else (False,):
        oc, ob, t_out, t_in = cases.model(name, config, with_shape)
        kk = t_out.shape[1]
        assert t_in.shape == (len(c), kk) and (t_in >= 0).sum() == (t_out >= 0).sum() and np.all((t_out >= 0).any(1))
        v, col = np.nonzero(t_in >= 0)
        assert np.array_equal(t_out[t_in[v, col], col], v)
        r, col = np.nonzero(t_out >= 0)
        assert np.array_equal(t_in[t_out[r, col], col], r)
        first = np.full(len(oc), np.iinfo(np.int64).max)
        np.minimum.at(first, t_in[v, np.nonzero(t_in >= 0)[1]], v * kk + np.nonzero(t_in >= 0)[1])
        assert np.all(np.diff(first) > 0)
        ks, st, pad, dil = (np.array(ref.triple(x)) for x in cases.CONFIGS[config])
        assert np.array_equal(oc[r] * st - pad + ref.columns(cases.CONFIGS[config][0])[col] * dil, c[t_out[r, col]])
        if b is not None:
            assert np.array_equal(ob[r], b[t_out[r, col]])


@pytest.mark.parametrize("name", ("v65", "batches", "negative_odd", "far_away", "fill32"))
def test_stride_one_is_the_submanifold_table(name):
    """stride 1 with centred padding: every input site is an output, and table_out[table_in[:, centre]] is VoxelNeighbors' table"""
    c, b = cases.SCENES[name]
    for ks, dil in ((3, 1), ((1, 3, 5), (1, 2, 3)), (5, 2)):
        pad = tuple((k - 1) // 2 * d for k, d in zip(ref.triple(ks), ref.triple(dil)))
        oc, ob, t_out, t_in = ref.build(c, ks, 1, pad, dil, b)
        centre = (t_out.shape[1] - 1) // 2
        rows = t_in[:, centre]
        assert np.all(rows >= 0) and np.array_equal(oc[rows], c)
        assert np.array_equal(t_out[rows], vref.table(c, ks, dil, b))


@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
def test_shift_by_a_multiple_of_the_stride(config):
    c, b = cases.SCENES["batches_negative"]
    ks, st, pad, dil = cases.CONFIGS[config]
    steps = np.array([3, -2, 5], np.int64)
    oc, ob, t_out, t_in = cases.model("batches_negative", config)
    oc2, ob2, t_out2, t_in2 = ref.build(c + steps * np.array(ref.triple(st)), ks, st, pad, dil, b)
    assert np.array_equal(oc2, oc + steps) and np.array_equal(ob2, ob) and np.array_equal(t_out2, t_out) and np.array_equal(t_in2, t_in)


# ---------------------------------------------------------------- against torch's dense operators

def _dense(c, b):
    ids = np.zeros(len(c), np.int64) if b is None else np.unique(b, return_inverse=True)[1]
    local = c - c.min(0)
    return np.concatenate([ids[:, None], local], 1), (int(ids.max()) + 1,) + tuple(int(a) for a in local.max(0) + 1)


@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
@pytest.mark.parametrize("name", DENSE_SCENES)
def test_model_is_the_dense_convolution(name, config):
    """on the scene moved to the origin, with spatial_shape its box (+1 on x, so that the shape is not the tightest one, and widened to the kernel's reach where the scene is thinner): the active
    outputs are the support of the all-ones conv3d of the indicator; forward and autograd equal conv3d's; the inverse equals
    conv_transpose3d at the input sites with the output_padding that restores the input shape.  Bounds: sparse_conv_reference.bounds,
    (n + 2) eps64 sum|a||b| with n = K Cin, K Cout, rows"""
    c, b = cases.SCENES[name]
    idx, shape = _dense(c, b)
    ks, st, pad, dil = (ref.triple(x) for x in cases.CONFIGS[config])
    need = tuple(d * (k - 1) + 1 - 2 * p for k, p, d in zip(ks, pad, dil))      # the smallest shape with a dense output
    shape = (shape[0], max(shape[1] + 1, need[0]), max(shape[2], need[1]), max(shape[3], need[2]))
    local, ids = idx[:, 1:], idx[:, 0]
    oc, ob, t_out, t_in = ref.build(local, ks, st, pad, dil, ids, spatial_shape=shape[1:])
    osize = ref.out_shape(shape[1:], ks, st, pad, dil)
    at = tuple(torch.from_numpy(idx[:, a]) for a in range(4))
    at_out = (torch.from_numpy(ob),) + tuple(torch.from_numpy(oc[:, a]) for a in range(3))
    f = torch.nn.functional
    ones = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.float64)
    ones[at[0], 0, at[1], at[2], at[3]] = 1
    support = f.conv3d(ones, torch.ones((1, 1) + ks, dtype=torch.float64), stride=st, padding=pad, dilation=dil)
    assert tuple(support.shape[2:]) == osize
    want_active = set(map(tuple, torch.nonzero(support[:, 0] > 0).tolist()))
    assert want_active == set(zip(ob.tolist(), *oc.T.tolist())) and len(want_active) == len(oc)
    assert np.array_equal((t_out >= 0).sum(1), support[:, 0][at_out].numpy().astype(np.int64))

    v, cin, cout, kk = len(c), 3, 2, t_out.shape[1]
    r = np.random.default_rng(len(name) + kk)
    x, w, bias, g = r.standard_normal((v, cin)), r.standard_normal((kk, cin, cout)), r.standard_normal(cout), r.standard_normal((len(oc), cout))
    xt, wt, bt = (torch.from_numpy(a).requires_grad_() for a in (x, w, bias))
    grid = torch.zeros(shape + (cin,), dtype=torch.float64).index_put(at, xt).permute(0, 4, 1, 2, 3)
    y = f.conv3d(grid, wt.reshape(ks + (cin, cout)).permute(4, 3, 0, 1, 2), bt, stride=st, padding=pad, dilation=dil)
    y = y.permute(0, 2, 3, 4, 1)[at_out]
    y.backward(torch.from_numpy(g))
    got = (ref.conv(x, t_out, w, bias),) + ref.conv_backward(x, t_out, t_in, w, g)
    want = (y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy())
    for what, a, e, bound in zip(("out", "grad_features", "grad_weight", "grad_bias"), got, want, ref.bounds(x, t_out, t_in, w, g, EPS64, bias)):
        assert a.shape == e.shape and np.all(np.abs(a - e) <= bound), what

    # the inverse: rows on the output sites -> the ORIGINAL input sites
    z, wi, gi = r.standard_normal((len(oc), cin)), r.standard_normal((kk, cin, cout)), r.standard_normal((v, cout))
    zt, wit, bit = (torch.from_numpy(a).requires_grad_() for a in (z, wi, bias))
    grid = torch.zeros((shape[0],) + osize + (cin,), dtype=torch.float64).index_put(at_out, zt).permute(0, 4, 1, 2, 3)
    opad = tuple(n - ((o - 1) * s - 2 * p + d * (k - 1) + 1) for n, o, s, p, d, k in zip(shape[1:], osize, st, pad, dil, ks))
    up = f.conv_transpose3d(grid, wit.reshape(ks + (cin, cout)).permute(3, 4, 0, 1, 2), bit, stride=st, padding=pad, output_padding=opad, dilation=dil)
    assert tuple(up.shape[2:]) == shape[1:]
    up = up.permute(0, 2, 3, 4, 1)[at]
    up.backward(torch.from_numpy(gi))
    got = (ref.conv(z, t_in, wi, bias),) + ref.conv_backward(z, t_in, t_out, wi, gi)
    want = (up.detach().numpy(), zt.grad.numpy(), wit.grad.numpy(), bit.grad.numpy())
    for what, a, e, bound in zip(("out", "grad_features", "grad_weight", "grad_bias"), got, want, ref.bounds(z, t_in, t_out, wi, gi, EPS64, bias)):
        assert a.shape == e.shape and np.all(np.abs(a - e) <= bound), "inverse " + what


# ---------------------------------------------------------------- the hash table, replayed

def test_wrap_scene_crosses_the_end_of_the_hash_table():
    """k1 s1 p0: the outputs are the inputs, the output box is the input box, so `wrap`'s keys (x itself) and its probe chain across
    the end of the table are the strided map's as well -- as long as the capacity is the one the scene was searched for, which is
    asserted, not assumed: V P = 213 (P = 1) is below the 2^15 cells of the box"""
    c, _ = cases.SCENES["wrap"]
    ks, st, pad, dil = cases.CONFIGS["k1s1p0"]
    assert ref.fanout(ks, st, dil) == 1
    oc, ob, t_out, t_in = cases.model("wrap", "k1s1p0")
    assert np.array_equal(oc, c) and np.array_equal(t_out[:, 0], np.arange(len(c))) and np.array_equal(t_in, t_out)
    fr = ref.frame(c, ks, st, pad, dil)
    assert fr[1] == [vcases.WRAP_LINE, 1, 1] and fr[4] == 9 and 1 << fr[4] >= 2 * len(c)
    keys = ref.out_keys(oc, ob, fr)
    assert keys == c[:, 0].tolist()
    cap = 1 << fr[4]
    late = [k for k in keys if vref.hash_home(k, fr[4]) >= cap - vcases.WRAP_WINDOW]
    assert len(late) == vcases.WRAP_CHAIN
    for order in (keys, sorted(keys), [keys[i] for i in np.random.default_rng(3).permutation(len(keys))]):
        slots, wrapped = vref.hash_replay(order, fr[4])
        assert wrapped >= vcases.WRAP_CHAIN - vcases.WRAP_WINDOW and len(slots) == len(keys)
        walks = [vref.hash_walk(k, slots, fr[4]) for k in late]     # the look-ups of the number and the table passes
        assert all(w[0] for w in walks) and sum(w[2] for w in walks) >= vcases.WRAP_CHAIN - vcases.WRAP_WINDOW
        assert max(w[1] for w in walks) >= 100


def test_capacity_steps():
    """V P steps over 4096 between vp512 and vp513 (k3s2p1, P = 8); a full block's capacity comes from its cells instead"""
    ks, st, pad, dil = cases.CONFIGS["k3s2p1"]
    assert ref.fanout(ks, st, dil) == 8 and ref.fanout(7, 2) == 64 and ref.fanout(3, 1) == 27 and ref.fanout(2, 2) == 1
    assert ref.fanout((3, 1, 2), (2, 1, 3), (2, 1, 1)) == 3 * 1 * 1 and ref.fanout(3, 3) == 1 and ref.fanout(5, 2) == 27
    caps = [ref.frame(cases.SCENES["vp%d" % v][0], ks, st, pad, dil)[4] for v in (511, 512, 513)]
    assert caps == [13, 13, 14]
    for v in (511, 512, 513):
        fr = ref.frame(cases.SCENES["vp%d" % v][0], ks, st, pad, dil)
        assert fr[1][0] * fr[1][1] * fr[1][2] > 8 * v
        assert len(cases.model("vp%d" % v, "k3s2p1")[0]) <= min(8 * v, fr[1][0] * fr[1][1] * fr[1][2])
    c, _ = cases.SCENES["block12"]
    fr = ref.frame(c, ks, st, pad, dil)
    assert fr[1] == [7, 7, 7] and fr[4] == 10 and len(cases.model("block12", "k3s2p1")[0]) == 343


# ---------------------------------------------------------------- the library's host side

def test_host_side_validation_without_gpu():
    from d3d_amd.voxel import SparseConvMap, sparse_conv3d, sparse_inverse_conv3d
    c = torch.zeros((6, 3), dtype=torch.int64)
    for ks in (0, 8, -1, (3, 3), 3.0, (3, 3, 3, 3)):
        with pytest.raises(ValueError):
            SparseConvMap(c, ks, 2)
    for st in (0, -1, (1, 1), 1.5, 2 ** 24 + 1):
        with pytest.raises(ValueError):
            SparseConvMap(c, 3, st)
    for pad in (-1, (1, 1), 0.5):
        with pytest.raises(ValueError):
            SparseConvMap(c, 3, 2, padding=pad)
    for dil in (0, (1, 1), 1.5):
        with pytest.raises(ValueError):
            SparseConvMap(c, 3, 2, dilation=dil)
    for shape in (5, (4, 4), (0, 4, 4), (4, 4, 2 ** 31), (2, 4, 4)):                  # (2, 4, 4): k3 p0 has no output on x
        with pytest.raises(ValueError):
            SparseConvMap(c, 3, 2, spatial_shape=shape)
    for bad in (torch.zeros(6, dtype=torch.int64), torch.zeros((6, 2), dtype=torch.int64), torch.zeros((6, 3)),
                np.zeros((6, 3), np.float64), torch.zeros((6, 3), dtype=torch.int16)):
        with pytest.raises(ValueError):
            SparseConvMap(bad, 3, 2)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros((6, 1), dtype=torch.int64), torch.zeros(6)):
        with pytest.raises(ValueError):
            SparseConvMap(c, 3, 2, batch_index=bad)
    with pytest.raises(TypeError):
        SparseConvMap([[0, 0, 0]], 3, 2)
    # V P beyond 2^31 - 1: refused before anything is copied (a [V, 3] view of one row: no memory behind it)
    many = torch.zeros((1, 3), dtype=torch.int64).expand(2 ** 31 // 27 + 1, 3)
    with pytest.raises(ValueError, match="candidates"):
        SparseConvMap(many, 3, 1, 1)
    for fn in (sparse_conv3d, sparse_inverse_conv3d):
        with pytest.raises(TypeError):
            fn(torch.zeros((6, 3)), c, torch.zeros((27, 3, 2)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):      # no silent CPU fallback
            SparseConvMap(c, 3, 2, 1)
        with pytest.raises(RuntimeError, match="HIP device"):
            SparseConvMap(np.zeros((0, 3), np.int32), 2, 2)


def test_workspace_query_and_refusals_without_launching():
    from d3d_amd import _lib
    lib = _lib.load()
    sizes = (0, 1, 31, 32, 33, 1000, 4095, 4096, 4097, 10 ** 6, 2 * 10 ** 7, (2 ** 31 - 1) // 8)
    for ks, st, dil in ((3, 2, 1), (2, 2, 1), (3, 1, 1), (7, 2, 1), ((3, 1, 2), (2, 1, 3), (2, 1, 1))):
        p, kk = ref.fanout(ks, st, dil), int(np.prod(ref.triple(ks)))
        b = [lib.d3d_sparse_conv_map_workspace_bytes(v, _i32x3(ks), _i32x3(st), _i32x3(dil)) for v in sizes if v * p <= 2 ** 31 - 1]
        assert all(x > 0 and x % 256 == 0 for x in b) and b == sorted(b)
        for v, x in zip(sizes, b):
            scan = max(-(-(v * kk) // 1024), 1) * 8                 # 8 bytes per 1024 candidate numbers, in 256-byte units
            cap = (x - 512 - -(-scan // 256) * 256) // 16           # bounds, frame, then key and first side by side: 16 bytes a slot
            assert cap >= 2 * v * p and cap >= 64 and cap & (cap - 1) == 0 and (cap == 64 or cap < 4 * v * p)
    q = lambda v, ks=3, st=2, dil=1: lib.d3d_sparse_conv_map_workspace_bytes(v, _i32x3(ks), _i32x3(st), _i32x3(dil))      # noqa: E731
    assert q(2 ** 31 // 8 + 1) == 0 and q(10, ks=8) == 0 and q(10, st=0) == 0 and q(10, dil=0) == 0 and q(10, ks=(3, 0, 3)) == 0
    # O(V P), not O(V K): k7 s7 (P = 1, K = 343) takes less than a tenth of k7 s1 (P = 343)
    assert 10 * q(10 ** 5, ks=7, st=7) < q(10 ** 5, ks=7, st=1)

    i64x3 = lambda *t: (ctypes.c_int64 * 3)(*t)                     # noqa: E731
    count = lambda v=0, ks=3, st=2, pad=1, dil=1, shape=None, counts=None: lib.d3d_sparse_conv_map_count(      # noqa: E731
        None, None, v, _i32x3(ks), _i32x3(st), _i32x3(pad), _i32x3(dil), shape, counts, None, 0, None)
    emit = lambda v=0, ks=3, st=2, pad=1, dil=1, shape=None, num_out=0: lib.d3d_sparse_conv_map_emit(      # noqa: E731
        None, None, v, _i32x3(ks), _i32x3(st), _i32x3(pad), _i32x3(dil), shape, num_out, None, None, None, None, None, None, 0, None)
    for call in (count, emit):
        assert call(v=-1) == _lib.ERR_BAD_ARG and call(ks=0) == _lib.ERR_BAD_ARG and call(ks=(3, 8, 3)) == _lib.ERR_BAD_ARG
        assert call(st=0) == _lib.ERR_BAD_ARG and call(pad=-1) == _lib.ERR_BAD_ARG and call(dil=(1, 1, 0)) == _lib.ERR_BAD_ARG
        assert call(shape=i64x3(4, 0, 4)) == _lib.ERR_BAD_ARG and call(pad=0, shape=i64x3(2, 4, 4)) == _lib.ERR_BAD_ARG
        assert call(st=2 ** 24 + 1) == _lib.ERR_UNSUPPORTED and call(shape=i64x3(4, 4, 2 ** 31)) == _lib.ERR_UNSUPPORTED
        assert call(v=2 ** 31 // 8 + 1) == _lib.ERR_UNSUPPORTED and call(v=2 ** 31) == _lib.ERR_UNSUPPORTED
        assert call(v=0) == _lib.ERR_BAD_ARG                        # no counts
        assert call(v=5) == _lib.ERR_BAD_ARG                        # no coords
    assert emit(num_out=-1) == _lib.ERR_BAD_ARG and emit(v=0, num_out=1) == _lib.ERR_BAD_ARG
