"""GPU: sparse_pool3d and the two entries behind it (csrc/vtpool.hip) against the numpy model of sparse_pool_reference.py.  Every
comparison is bit for bit (a NaN equal to any NaN: the rules say where one is, not which payload it carries)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparse_pool_cases as cases
import sparse_pool_reference as ref

pytestmark = pytest.mark.gpu


def T(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared tables are read-only)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def owner(scene, kind, what):
    return cases.owner(scene, kind, what, T)


def pool(x, where, red, g):
    """tensors of one dtype -> (out, grad_features) of sparse_pool3d"""
    from d3d_amd.voxel import sparse_pool3d
    x = x.detach().clone().requires_grad_()
    out = sparse_pool3d(x, where, red)
    out.backward(g)
    return out.detach(), x.grad


def model(x, g, tables, red, kind):
    """the fold-type arrays of features and gradient -> the model's (out, grad_features) as CPU tensors of `kind`"""
    fwd, back, mirrored = tables
    out, arg, count = ref.forward(x, fwd, red, kind)
    return ref.to_tensor(out, kind), ref.to_tensor(ref.backward(g, back, mirrored, red, kind, arg, count), kind)


def check(scene, where, kind, c, reds=ref.REDUCTIONS, seed=0):
    tables = cases.tables(scene, *where)
    (xt, x), (gt, g) = (ref.of_kind(cases.randoms(len(t), c, seed + i), kind) for i, t in enumerate((tables[1], tables[0])))
    for red in reds:
        out, gf = pool(xt.cuda(), owner(scene, *where), red, gt.cuda())
        want, want_gf = model(x, g, tables, red, kind)
        assert out.is_cuda and gf.is_cuda
        assert ref.equal_bits(out, want), (red, "out")
        assert ref.equal_bits(gf, want_gf), (red, "grad_features")


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("where", cases.WHERES, ids=lambda w: "%s-%s" % w)
@pytest.mark.parametrize("scene", cases.SCENES)
def test_forward_and_backward_are_the_model(scene, where, kind):
    """12 channels: the vector path of fp32 (three lanes of a group of four) and fp64 (six of eight), the scalar path of the half types"""
    check(scene, where, kind, 12)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("c", cases.CHANNELS)
def test_channel_counts(c, kind):
    check("v65", ("map", "k3s2p1"), kind, c, seed=c)
    check("v65", ("nbrs", (3, 3, 3)), kind, c, reds=(ref.MAX, ref.MEAN), seed=c + 1)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_misaligned_features_give_the_same_bits(kind):
    """features and gradient one element past a 16-byte boundary take the scalar path: the bits of the aligned call"""
    where, c = ("map", "k3s2p1"), 16
    tables = cases.tables("v65", *where)
    (xt, _), (gt, _) = (ref.of_kind(cases.randoms(len(t), c, 3 + i), kind) for i, t in enumerate((tables[1], tables[0])))

    def shifted(t):
        s = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
        s.copy_(t)
        assert s.is_contiguous() and s.data_ptr() % 16 == t.element_size()
        return s
    for red in ref.REDUCTIONS:
        a, ga = pool(xt.cuda(), owner("v65", *where), red, gt.cuda())
        x = shifted(xt).requires_grad_()
        from d3d_amd.voxel import sparse_pool3d
        b = sparse_pool3d(x, owner("v65", *where), red)
        b.backward(shifted(gt))
        assert ref.equal_bits(a, b.detach()) and ref.equal_bits(ga, x.grad), red


@pytest.mark.parametrize("kind", ("f32", "f16"))
def test_kernel_size_7_names_columns_beyond_255(kind):
    from d3d_amd.voxel import VoxelNeighbors
    c, feat, tab = cases.large_kernel()
    xt, x = ref.of_kind(feat, kind)
    gt, g = ref.of_kind(cases.randoms(512, feat.shape[1], 5), kind)
    _, arg, _ = ref.forward(x, tab, ref.MAX, kind)
    assert arg.max() > 255                                                   # a condition on the inputs
    nb = VoxelNeighbors(T(c), 7)
    assert np.array_equal(nb.table.cpu().numpy(), tab)
    for red in ref.REDUCTIONS:
        out, gf = pool(xt.cuda(), nb, red, gt.cuda())
        want, want_gf = model(x, g, (tab, tab, True), red, kind)
        assert ref.equal_bits(out, want) and ref.equal_bits(gf, want_gf), red
    far = np.nonzero(arg[:, 0] > 255)[0]                                     # the max's gradient of channel 0 lands where those rows point
    _, gf = pool(xt.cuda(), nb, ref.MAX, torch.ones_like(gt).cuda())
    assert len(far) and bool((gf[torch.from_numpy(tab[far, arg[far, 0].astype(np.int64)]).long().cuda(), 0] > 0).all())


# ---------------------------------------------------------------- the raw entries

def raw_forward(feat, table, red, want_arg=True, want_count=True, kind=None, rows=None):
    """d3d_table_pool_forward by hand -> (rc, out, arg, count), the outputs prefilled with sentinels"""
    from d3d_amd import _lib
    rows = table.shape[0] if rows is None else rows
    c = feat.shape[1]
    out = torch.full((table.shape[0], c), -7.0, dtype=feat.dtype, device="cuda")
    arg = torch.full((table.shape[0], c), -7, dtype=torch.int16, device="cuda") if want_arg else None
    count = torch.full((table.shape[0],), -7, dtype=torch.int32, device="cuda") if want_count else None
    code = ref.CODES[kind] if isinstance(kind, str) else kind
    rc = _lib.load().d3d_table_pool_forward(P(feat), feat.shape[0], c, code, P(table), rows, table.shape[1], ref.RED_CODES.get(red, red),
                                            P(out), P(arg), P(count), stream())
    return rc, out, arg, count


def raw_backward(grad, back, mirrored, red, arg, count, kind):
    from d3d_amd import _lib
    out = torch.full((back.shape[0], grad.shape[1]), -7.0, dtype=grad.dtype, device="cuda")
    rc = _lib.load().d3d_table_pool_backward(P(grad), grad.shape[0], grad.shape[1], ref.CODES[kind], P(back), back.shape[0], back.shape[1],
                                             int(mirrored), ref.RED_CODES[red], P(arg), P(count), P(out), stream())
    return rc, out


SPECIAL = np.array([[1.0, -0.0, np.nan, -np.inf, 5.0, 0.0, 3.0, 3.0], [1.0, 0.0, 2.0, np.inf, np.nan, -0.0, -3.0, 3.0],
                    [2.0, -0.0, np.nan, np.inf, 7.0, 0.0, 3.0, -3.0]])
SPECIAL = np.concatenate([SPECIAL, SPECIAL, SPECIAL[:1]])      # rows 3 .. 5 repeat rows 0 .. 2; row 6 is read by nobody
SPECIAL_TABLE = np.array([[0, 1, 2], [2, -1, 3], [-1, -1, -1], [-1, 4, -1], [1, 0, 5], [5, 2, 1]], np.int32)


def transposed(table, src_rows):
    """back[v, kk] == r <=> table[r, kk] == v (no column names a row twice)"""
    back = np.full((src_rows, table.shape[1]), -1, np.int32)
    for r, kk in zip(*np.nonzero(table >= 0)):
        assert back[table[r, kk], kk] == -1
        back[table[r, kk], kk] = r
    return back


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("wide", (False, True))
def test_nan_infinities_signed_zeros_ties_and_rows_without_entries(kind, wide):
    """NaN, +-inf, -0.0 against +0.0 and equal values (the lowest column wins, forward and backward); an all -1 row gives 0 / -1 / 0
    and, on the way back, a row that nobody reads zeros.  8 channels (one vector of the half types) or, tiled, 24"""
    feat = np.tile(SPECIAL, (1, 3)) if wide else SPECIAL
    xt, x = ref.of_kind(feat, kind)
    gt, g = ref.of_kind(cases.randoms(len(SPECIAL_TABLE), feat.shape[1], 6), kind)
    special_back = transposed(SPECIAL_TABLE, len(SPECIAL))
    assert np.all(SPECIAL_TABLE[2] == -1) and np.all(special_back[6] == -1)
    tab, back = T(SPECIAL_TABLE), T(special_back)
    for red in ref.REDUCTIONS:
        rc, out, arg, count = raw_forward(xt.cuda(), tab, red, kind=kind)
        want, want_arg, want_count = ref.forward(x, SPECIAL_TABLE, red, kind)
        assert rc == 0 and ref.equal_bits(out, ref.to_tensor(want, kind)), red
        assert np.array_equal(count.cpu().numpy(), want_count) and want_count[2] == 0
        extreme = red in (ref.MAX, ref.MIN)
        assert np.array_equal(arg.cpu().numpy(), want_arg if extreme else np.full_like(want_arg, -7)), red
        assert not out[2].any() and not torch.signbit(out[2]).any() and (not extreme or bool((arg[2] == -1).all()))
        rc, gf = raw_backward(gt.cuda(), back, False, red, T(want_arg), T(want_count), kind)
        want_gf = ref.backward(g, special_back, False, red, kind, want_arg, want_count)
        assert rc == 0 and ref.equal_bits(gf, ref.to_tensor(want_gf, kind)), red
        assert not gf[6].any() and not torch.signbit(gf[6]).any()


@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_a_rows_bits_do_not_depend_on_its_position_or_the_run(kind):
    t_out, _, _ = cases.tables("batches", "map", "k3s2p1")
    xt, _ = ref.of_kind(cases.randoms(len(cases.tables("batches", "map", "k3s2p1")[1]), 20, 7), kind)
    perm = np.random.default_rng(8).permutation(len(t_out))
    for red in ref.REDUCTIONS:
        _, a, arg_a, n_a = raw_forward(xt.cuda(), T(t_out), red, kind=kind)
        _, b, arg_b, n_b = raw_forward(xt.cuda(), T(t_out[perm]), red, kind=kind)
        _, again, arg_again, _ = raw_forward(xt.cuda(), T(t_out), red, kind=kind)
        p = torch.from_numpy(perm).cuda()
        assert ref.equal_bits(a[p], b) and torch.equal(arg_a[p], arg_b) and torch.equal(n_a[p], n_b), red
        assert ref.equal_bits(a, again) and torch.equal(arg_a, arg_again), red


def test_offsets_past_2_31():
    """rows * c = 2^31 + 512 elements of fp16 (4.3 GB each for out, arg and grad_feat), K = 1, 1000 feature rows named again and
    again: 64 rows straddling element 2^31 and the last 64 rows, against torch indexing on the device"""
    c, v = 8, 1000
    rows = 2 ** 31 // c + 64
    mid = 2 ** 31 // c
    assert rows * c > 2 ** 31 and (mid - 32) * c < 2 ** 31 < (mid + 32) * c
    gen = torch.Generator(device="cuda").manual_seed(11)
    table = torch.randint(-1, v, (rows, 1), dtype=torch.int32, device="cuda", generator=gen)
    feat = torch.randn((v, c), device="cuda", generator=gen).half()
    padded = torch.cat([feat, torch.zeros((1, c), dtype=torch.float16, device="cuda")])
    rc, out, arg, count = raw_forward(feat, table, ref.MAX, kind="f16")
    assert rc == 0
    for r0 in (rows - 64, mid - 32):
        t = table[r0:r0 + 64, 0]
        assert torch.equal(out[r0:r0 + 64].view(torch.int16), padded[torch.where(t < 0, v, t).long()].view(torch.int16)), r0
        assert torch.equal(arg[r0:r0 + 64], torch.where(t < 0, -1, 0).to(torch.int16)[:, None].expand(64, c)), r0
        assert torch.equal(count[r0:r0 + 64], (t >= 0).int()), r0
    del out, arg
    rc, gf = raw_backward(feat, table, False, ref.SUM, None, None, "f16")
    assert rc == 0
    for r0 in (rows - 64, mid - 32):
        t = table[r0:r0 + 64, 0]
        assert torch.equal(gf[r0:r0 + 64].view(torch.int16), padded[torch.where(t < 0, v, t).long()].view(torch.int16)), r0


def test_refusals_touch_nothing():
    from d3d_amd import _lib
    lib = _lib.load()
    feat, table = torch.zeros((65, 4), device="cuda"), torch.zeros((65, 27), dtype=torch.int32, device="cuda")
    out = torch.full((65, 4), -7.0, device="cuda")
    arg, count = torch.full((65, 4), -7, dtype=torch.int16, device="cuda"), torch.full((65,), -7, dtype=torch.int32, device="cuda")
    f = lambda fe=P(feat), src=65, c=4, dtype=0, t=P(table), rows=65, k=27, red=2, o=P(out): \
        lib.d3d_table_pool_forward(fe, src, c, dtype, t, rows, k, red, o, P(arg), P(count), stream())
    b = lambda g=P(feat), orows=65, c=4, dtype=0, t=P(table), rows=65, k=27, red=4, a=P(arg), n=P(count), o=P(out): \
        lib.d3d_table_pool_backward(g, orows, c, dtype, t, rows, k, 1, red, a, n, o, stream())
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    assert [f(fe=None), f(t=None), f(o=None), f(src=-1), f(rows=-1), f(c=0), f(k=0)] == [bad] * 7
    assert [f(dtype=2), f(dtype=3), f(dtype=6), f(red=0), f(red=5), f(k=344), f(rows=2 ** 31), f(src=2 ** 31)] == [uns] * 8
    assert [b(g=None), b(t=None), b(o=None), b(orows=-1), b(rows=-1), b(c=0), b(k=0), b(red=2, a=None), b(red=3, a=None), b(red=1, n=None)] == [bad] * 10
    assert [b(dtype=2), b(dtype=6), b(red=0), b(red=5), b(k=344), b(rows=2 ** 31), b(orows=2 ** 31)] == [uns] * 7
    assert f(rows=0) == 0 and b(rows=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((arg == -7).all()) and bool((count == -7).all())


# ---------------------------------------------------------------- the operator

@pytest.mark.parametrize("red", ref.REDUCTIONS)
@pytest.mark.parametrize("where", (("map", "k3s2p1"), ("nbrs", (3, 3, 3))), ids=("map", "nbrs"))
def test_gradcheck(where, red):
    """fp64, distinct values a multiple of 1 / 7 apart: the winner of a max or min does not change inside the probe's step"""
    from d3d_amd.voxel import sparse_pool3d
    v = len(cases.tables("v63", *where)[1])
    x = torch.from_numpy(np.random.default_rng(9).permutation(v * 3).reshape(v, 3) / 7.0).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: sparse_pool3d(t, owner("v63", *where), red), (x,), eps=1e-6, atol=1e-7, rtol=1e-7, nondet_tol=0.0)


def test_numpy_and_host_tensors_come_back_where_they_came_from():
    from d3d_amd.voxel import sparse_avg_pool3d, sparse_max_pool3d, sparse_pool3d
    tables = cases.tables("v65", "map", "k2s2p0")
    where = owner("v65", "map", "k2s2p0")
    (xt, x), (gt, g) = (ref.of_kind(cases.randoms(len(t), 5, 10 + i), "f32") for i, t in enumerate((tables[1], tables[0])))
    want, want_gf = model(x, g, tables, ref.MEAN, "f32")
    got = sparse_avg_pool3d(xt.numpy(), where)
    assert isinstance(got, np.ndarray) and ref.equal_bits(torch.from_numpy(got), want)
    out, gf = pool(xt, where, "MEAN", gt)
    assert not out.is_cuda and not gf.is_cuda and ref.equal_bits(out, want) and ref.equal_bits(gf, want_gf)
    assert ref.equal_bits(sparse_max_pool3d(xt.cuda(), where), sparse_pool3d(xt.cuda(), where))
    with pytest.raises(ValueError, match="live on"):
        _wrong_device(where, xt)
    # nothing to pool: no rows, no channels
    from d3d_amd.voxel import VoxelNeighbors
    nb = VoxelNeighbors(torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
    x0 = torch.zeros((0, 4), device="cuda", requires_grad=True)
    y0 = sparse_pool3d(x0, nb, "sum")
    y0.sum().backward()
    assert y0.shape == (0, 4) and x0.grad.shape == (0, 4)
    assert sparse_pool3d(torch.zeros((len(tables[1]), 0), device="cuda"), where).shape == (len(tables[0]), 0)


def _wrong_device(where, xt):
    """features on a GPU that is not the owner's: refused before anything is launched (with one GPU: an owner that claims another)"""
    import copy
    from d3d_amd.voxel import sparse_pool3d
    other = copy.copy(where)
    other.device = torch.device("cuda", where.device.index + 1)
    return sparse_pool3d(xt.cuda(), other)


def test_bf16_chain_of_convolutions_and_a_max_pool():
    """subm_conv3d -> sparse_max_pool3d -> subm_conv3d on the pooled out_coords, in bf16: runs, backpropagates, and the pooling stage in
    the middle is the model's"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_max_pool3d, subm_conv3d
    import sparse_conv_cases as scases
    c, b = scases.SCENES["batches"]
    nb = VoxelNeighbors(T(c), 3, batch_index=T(b))
    cmap = SparseConvMap(T(c), 3, 2, 1, batch_index=T(b))
    nb2 = VoxelNeighbors(cmap.out_coords, 3, batch_index=cmap.out_batch)
    gen = torch.Generator().manual_seed(12)
    x = (torch.randn((len(c), 16), generator=gen) / 4).bfloat16().cuda().requires_grad_()
    w1 = (torch.randn((27, 16, 32), generator=gen) / 8).bfloat16().cuda().requires_grad_()
    w2 = (torch.randn((27, 32, 16), generator=gen) / 8).bfloat16().cuda().requires_grad_()
    y = subm_conv3d(x, nb, w1)
    z = sparse_max_pool3d(y, cmap)
    out = subm_conv3d(z, nb2, w2)
    assert out.shape == (cmap.num_out, 16) and out.dtype == torch.bfloat16
    out.backward(torch.ones_like(out))
    for t in (x, w1, w2):
        assert t.grad is not None and t.grad.dtype == torch.bfloat16 and bool(torch.isfinite(t.grad.float()).all()) and bool(t.grad.any())
    t_out, _, _ = cases.tables("batches", "map", "k3s2p1")
    want, _, _ = ref.forward(y.detach().float().cpu().numpy(), t_out, ref.MAX, "bf16")
    assert ref.equal_bits(z.detach(), ref.to_tensor(want, "bf16"))
