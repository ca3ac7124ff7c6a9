"""GPU: VoxelNeighbors / neighbor_gather / subm_conv3d (vnbr.hip) against the numpy model (voxel_conv_reference.py): the table and
the gathers EXACTLY (bit for bit), the convolution within the derived dot-product bound of voxel_conv_reference.bounds."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import voxel_conv_cases as cases
import voxel_conv_reference as ref

pytestmark = pytest.mark.gpu

EPS = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}
CHANNELS = (1, 3, 4, 5, 16, 63, 64, 65, 128)


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def model_table(name, ks=(3, 3, 3), dil=1):
    c, b = cases.SCENES[name]
    tab = ref.table(c, ks, dil, b)
    return tab


def raw_table(c, b, ks, dil, fill=-7):
    """d3d_voxel_neighbors by hand, its table one int32 past a 16-byte boundary -> (rc, table, counts)"""
    from d3d_amd import _lib
    lib = _lib.load()
    v, (ks, dil) = len(c), (ref.triple(ks), ref.triple(dil))
    k = ks[0] * ks[1] * ks[2]
    slab = torch.full((v * k + 1,), fill, dtype=torch.int32, device="cuda")
    table = slab[1:].view(v, k)
    assert table.data_ptr() % 16 == 4
    counts = torch.full((3,), fill, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.d3d_voxel_neighbors_workspace_bytes(v), dtype=torch.uint8, device="cuda")
    ct, bt = T(c), T(b)                                             # (held until the results are back)
    rc = lib.d3d_voxel_neighbors(P(ct), P(bt), v, *ks, *dil, P(table), P(counts), P(ws), ws.numel(), stream())
    return rc, N(table), N(counts).tolist()


@pytest.mark.parametrize("dil", cases.DILATIONS, ids=str)
@pytest.mark.parametrize("ks", cases.KERNELS, ids=str)
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_table_is_the_model_table(name, ks, dil):
    """the class, then the C entry: with the scene's batch (NULL where it has none), and with a batch value the scene lacks"""
    from d3d_amd.voxel import VoxelNeighbors
    c, b = cases.SCENES[name]
    want = ref.table(c, ks, dil, b)
    entries = int((want >= 0).sum())
    nb = VoxelNeighbors(T(c), ks, dil, T(b))
    assert nb.table.dtype == torch.int32 and nb.table.is_cuda and nb.table.shape == want.shape and np.array_equal(N(nb.table), want)
    assert nb.num_entries == entries and nb.num_voxels == len(c) and nb.kernel_size == ref.triple(ks) and nb.dilation == ref.triple(dil)
    rc, tab, counts = raw_table(c, b, ks, dil)
    assert rc == 0 and counts == [entries, 0, 0] and np.array_equal(tab, want)
    rc, tab, counts = raw_table(c, b if b is not None else np.full(len(c), -3, np.int64), ks, dil)
    assert rc == 0 and counts == [entries, 0, 0] and np.array_equal(tab, want)


def test_inputs_of_every_kind_build_the_same_table():
    from d3d_amd.voxel import VoxelNeighbors
    c, b = cases.SCENES["batches"]
    want = model_table("batches")
    for ct, bt in ((T(c), T(b)), (c, b), (torch.from_numpy(c), torch.from_numpy(b)), (T(c.astype(np.int32)), T(b.astype(np.int32))),
                   (T(c)[:, [2, 1, 0]].flip(1), b)):
        nb = VoxelNeighbors(ct, batch_index=bt)
        assert nb.table.is_cuda and np.array_equal(N(nb.table), want)
    assert np.array_equal(N(VoxelNeighbors(T(c), 3, (1, 1, 1), T(b)).table), want)


def test_duplicates_are_refused():
    from d3d_amd.voxel import VoxelNeighbors
    c, _ = cases.SCENES["v65"]
    twice = np.concatenate([c, c[7:8]])
    with pytest.raises(ValueError, match="1 rows"):
        VoxelNeighbors(T(twice))
    rc, tab, counts = raw_table(twice, None, 3, 1)
    assert rc == 0 and counts[1:] == [1, 0] and tab.min() >= -1 and tab.max() < 66 and counts[0] == int((tab >= 0).sum())
    c, b = cases.SCENES["batches"]                                  # without the batch ids: the cloud of batch 0 and 1 twice
    dups = len(c) - len(np.unique(c, axis=0))
    assert dups >= 1500
    with pytest.raises(ValueError, match="%d rows" % dups):
        VoxelNeighbors(T(c))
    rc, tab, counts = raw_table(c, None, (1, 3, 5), 2)
    assert rc == 0 and counts[1:] == [dups, 0] and tab.min() >= -1 and tab.max() < len(c)
    assert np.array_equal(N(VoxelNeighbors(T(c), batch_index=T(b)).table), model_table("batches"))      # the next call is as good as ever


def test_span_overflow_touches_nothing():
    from d3d_amd.voxel import VoxelNeighbors
    wide = np.array([[0, 0, 0], [2 ** 21, 2 ** 21, 2 ** 21], [5, 5, 5]], np.int64)
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelNeighbors(T(wide))
    rc, tab, counts = raw_table(wide, None, 3, 1)
    assert rc == 0 and counts == [0, 0, 1] and np.all(tab == -7)
    whole = np.array([[-2 ** 63, 0, 0], [2 ** 63 - 1, 0, 0]], np.int64)      # a span of 2^64
    rc, tab, counts = raw_table(whole, None, 3, 1)
    assert rc == 0 and counts == [0, 0, 1] and np.all(tab == -7)
    edge = np.array([[0, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 0], [1, 0, 0]], np.int64)      # 2^62 exactly: fits
    assert np.array_equal(N(VoxelNeighbors(T(edge)).table), ref.table(edge))
    rc, tab, counts = raw_table(edge, np.array([0, 1, 0]), 3, 1)             # times two batches: does not
    assert rc == 0 and counts == [0, 0, 1] and np.all(tab == -7)


def test_nothing_to_do():
    from d3d_amd import _lib
    from d3d_amd.voxel import VoxelNeighbors, neighbor_gather, subm_conv3d
    nb = VoxelNeighbors(torch.zeros((0, 3), dtype=torch.int64, device="cuda"), (1, 3, 5))
    assert nb.table.shape == (0, 15) and nb.num_entries == 0 and nb.num_voxels == 0
    assert VoxelNeighbors(np.zeros((0, 3), np.int32), batch_index=np.zeros(0, np.int64)).table.shape == (0, 27)
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    assert _lib.load().d3d_voxel_neighbors(None, None, 0, 3, 3, 3, 1, 1, 1, None, P(counts), None, 0, stream()) == 0
    assert N(counts).tolist() == [0, 0, 0]
    f = torch.zeros((0, 4), device="cuda", requires_grad=True)
    w = torch.ones((15, 4, 2), device="cuda", requires_grad=True)
    assert neighbor_gather(f, nb).shape == (0, 15, 4)
    out = subm_conv3d(f, nb, w, torch.ones(2, device="cuda"))
    assert out.shape == (0, 2)
    out.sum().backward()
    assert f.grad.shape == (0, 4) and w.grad.shape == (15, 4, 2) and not w.grad.any()


def test_two_builds_give_the_same_table():
    from d3d_amd.voxel import VoxelNeighbors
    for name in ("fill32", "comb", "batches"):
        c, b = cases.SCENES[name]
        a = VoxelNeighbors(T(c), 3, 1, T(b))
        torch.empty(1 << 22, device="cuda").normal_()                # (other work in between)
        assert torch.equal(a.table, VoxelNeighbors(T(c), 3, 1, T(b)).table) and np.array_equal(raw_table(c, b, 3, 1)[1], N(a.table))


def test_entries_refuse_without_launching():
    from d3d_amd import _lib
    lib = _lib.load()
    c, _ = cases.SCENES["v65"]
    ct = T(c)
    table = torch.full((65, 27), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    need = lib.d3d_voxel_neighbors_workspace_bytes(65)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    call = lambda co=P(ct), v=65, ks=(3, 3, 3), dil=(1, 1, 1), t=P(table), cn=P(counts), w=P(ws), nb=need: \
        lib.d3d_voxel_neighbors(co, None, v, *ks, *dil, t, cn, w, nb, stream())
    assert call(co=None) == _lib.ERR_BAD_ARG and call(t=None) == _lib.ERR_BAD_ARG and call(cn=None) == _lib.ERR_BAD_ARG
    assert call(v=-1) == _lib.ERR_BAD_ARG and call(ks=(3, 2, 3)) == _lib.ERR_BAD_ARG and call(ks=(9, 3, 3)) == _lib.ERR_BAD_ARG
    assert call(ks=(3, 3, 0)) == _lib.ERR_BAD_ARG and call(dil=(1, 0, 1)) == _lib.ERR_BAD_ARG
    assert call(w=None) == _lib.ERR_WORKSPACE and call(nb=need - 1) == _lib.ERR_WORKSPACE
    assert call(v=2 ** 31) == _lib.ERR_UNSUPPORTED
    f = torch.zeros((65, 4), device="cuda")
    out = torch.full((65, 27, 4), -7.0, device="cuda")
    g = lambda fe=P(f), c=4, dtype=0, cols=1, t=P(table), r=65, k=27, o=P(out): lib.d3d_neighbor_gather(fe, 65, c, dtype, cols, t, r, k, 0, o, stream())
    assert g(fe=None) == _lib.ERR_BAD_ARG and g(t=None) == _lib.ERR_BAD_ARG and g(o=None) == _lib.ERR_BAD_ARG and g(c=0) == _lib.ERR_BAD_ARG
    assert g(cols=2) == _lib.ERR_BAD_ARG and g(r=-1) == _lib.ERR_BAD_ARG and g(k=0) == _lib.ERR_BAD_ARG
    assert g(dtype=3) == _lib.ERR_UNSUPPORTED and g(r=2 ** 31) == _lib.ERR_UNSUPPORTED and g(k=344, cols=344) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((table == -7).all()) and bool((counts == -7).all()) and bool((out == -7).all()) and not ws.any()


# ---------------------------------------------------------------- the gather

def raw_gather(feat, table, k, mirrored, cols=1, v=None, shift_out=False):
    """d3d_neighbor_gather by hand into a NaN-filled `out` (one element past a 16-byte boundary with shift_out)"""
    from d3d_amd import _lib
    r, c = table.numel() // k, feat.shape[-1]
    slab = torch.full((r * k * c + 1,), float("nan"), dtype=feat.dtype, device="cuda")
    out = slab[1:].view(r, k, c) if shift_out else slab[:-1].view(r, k, c)
    assert out.data_ptr() % 16 == (feat.element_size() if shift_out else 0)
    rc = _lib.load().d3d_neighbor_gather(P(feat), feat.shape[0] if v is None else v, c, 0 if feat.dtype == torch.float32 else 1, cols, P(table),
                                         r, k, int(mirrored), P(out), stream())
    assert rc == 0
    return out


@pytest.mark.parametrize("c", CHANNELS)
def test_gather_is_indexing(c):
    """vector rows (4, 16, 64, 128) and scalar rows (1, 3, 5, 63, 65), plain and mirrored, the whole table and the rows from an
    odd one on, an aligned feat and one an element past a 16-byte boundary, and an aligned feat into an `out` an element past one
    (element by element, the same bits)"""
    tab = model_table("v4097")
    v, k = tab.shape
    table = T(tab)
    for dtype in (np.float32, np.float64):
        f = cases.features(v, c, dtype, c)
        slab = torch.zeros(f.size + 1, dtype=T(f).dtype, device="cuda")
        shifted = slab[1:].view(v, c)
        shifted.copy_(T(f))
        assert shifted.data_ptr() % 16 == f.itemsize
        for mirrored in (False, True):
            want = ref.gather(f, tab, mirrored)
            for ft in (T(f), shifted):
                assert ref.same_bits(N(raw_gather(ft, table, k, mirrored)), want), (dtype, mirrored)
                part = raw_gather(ft, table[1001:3000], k, mirrored)
                assert ref.same_bits(N(part), want[1001:3000]), (dtype, mirrored)
            assert ref.same_bits(N(raw_gather(T(f), table, k, mirrored, shift_out=True)), want), (dtype, mirrored)


def test_gather_of_a_column_of_its_own():
    """feat_cols = K: row [e, k] of a [V, K, C] feat -- the gradient of the plain gather before its fold"""
    tab = model_table("v65", (1, 3, 5), (1, 2, 3))
    g = np.random.default_rng(3).standard_normal((65, 15, 4)).astype(np.float32)
    src = tab[:, ::-1].astype(np.int64)
    want = g[np.maximum(src, 0), np.arange(15)[None, :]]
    want[src < 0] = 0
    assert ref.same_bits(N(raw_gather(T(g), T(tab), 15, True, cols=15)), want)


def test_gather_offsets_past_2_31():
    """R = 330 000 rows of a random table into 1000 feature rows, K = 27, C = 256, fp32: 2.28e9 output elements (9.1 GB).  The last
    64 output rows and 64 rows straddling element 2^31, against torch indexing on the device"""
    r, k, c, v = 330_000, 27, 256, 1000
    gen = torch.Generator(device="cuda").manual_seed(11)
    table = torch.randint(-1, v, (r, k), dtype=torch.int32, device="cuda", generator=gen)
    feat = torch.randn((v, c), device="cuda", generator=gen)
    padded = torch.cat([feat, torch.zeros((1, c), device="cuda")])              # row v: the zero row of a -1
    mid = 2 ** 31 // (k * c)
    assert r * k * c > 2 ** 31 and mid * k * c < 2 ** 31 < (mid + 1) * k * c
    for mirrored in (False, True):
        out = raw_gather(feat, table, k, mirrored)
        for r0 in (r - 64, mid - 32):
            t = table[r0:r0 + 64].flip(1) if mirrored else table[r0:r0 + 64]
            want = padded[torch.where(t < 0, v, t).long()]
            assert torch.equal(out[r0:r0 + 64].view(torch.int32), want.view(torch.int32)), (mirrored, r0)
        del out


@pytest.mark.parametrize("name,ks,dil", [("fill32", (3, 3, 3), 1), ("v65", (1, 3, 5), (1, 2, 3)), ("batches", (3, 1, 1), 2)])
def test_neighbor_gather_and_its_fixed_order_backward(name, ks, dil):
    from d3d_amd.voxel import VoxelNeighbors, neighbor_gather
    c, b = cases.SCENES[name]
    tab = model_table(name, ks, dil)
    nb = VoxelNeighbors(T(c), ks, dil, T(b))
    v, k = tab.shape
    for dtype, ch in ((np.float32, 4), (np.float32, 5), (np.float64, 2), (np.float64, 3)):
        f = cases.features(v, ch, dtype, ch)
        g = np.random.default_rng(ch + 9).standard_normal((v, k, ch)).astype(dtype)
        want = ref.gather_backward(g, tab)
        grads = []
        for _ in range(2):
            ft = T(f).requires_grad_()
            out = neighbor_gather(ft, nb)
            assert out.shape == (v, k, ch) and ref.same_bits(N(out), ref.gather(f, tab))
            out.backward(T(g))
            grads.append(N(ft.grad))
        assert ref.same_bits(grads[0], want) and ref.same_bits(grads[1], want), (dtype, ch)


# ---------------------------------------------------------------- the convolution

def conv_case(name, ks, dil, cin, cout, dtype, seed):
    c, b = cases.SCENES[name]
    tab = model_table(name, ks, dil)
    r = np.random.default_rng(seed)
    x, w = r.standard_normal((len(c), cin)).astype(dtype), r.standard_normal((tab.shape[1], cin, cout)).astype(dtype)
    bias, g = r.standard_normal(cout).astype(dtype), r.standard_normal((len(c), cout)).astype(dtype)
    return c, b, tab, x, w, bias, g


def run_conv(nb, x, w, bias, g, **kw):
    from d3d_amd.voxel import subm_conv3d
    xt, wt, bt = T(x).requires_grad_(), T(w).requires_grad_(), T(bias).requires_grad_()
    out = subm_conv3d(xt, nb, wt, bt, **kw)
    out.backward(T(g))
    return N(out), N(xt.grad), N(wt.grad), N(bt.grad)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name,ks,dil", [("v4097", (3, 3, 3), 1), ("batches", (1, 3, 5), (1, 2, 3)), ("block12", (5, 5, 5), 1)])
def test_subm_conv3d_against_the_fp64_model(name, ks, dil, dtype):
    """forward and the three gradients within ref.bounds: (K Cin + 2) eps sum|x||w| per output, the reduction lengths K Cout for
    grad_features and V for grad_weight and grad_bias; eps = 2^-52 in fp64, 2^-23 in fp32 (the model runs in fp64 on the same
    fp32 inputs)"""
    from d3d_amd.voxel import VoxelNeighbors
    c, b, tab, x, w, bias, g = conv_case(name, ks, dil, 5, 7, dtype, 21)
    nb = VoxelNeighbors(T(c), ks, dil, T(b))
    got = run_conv(nb, x, w, bias, g)
    want = (ref.conv(x, tab, w, bias),) + ref.conv_backward(x, tab, w, g)
    for what, a, e, bound in zip(("out", "grad_features", "grad_weight", "grad_bias"), got, want, ref.bounds(x, tab, w, g, EPS[dtype], bias)):
        err = np.abs(a.astype(np.float64) - e)
        print("%s: worst |err| / bound = %.4f" % (what, np.max(err[bound > 0] / bound[bound > 0])))
        assert a.dtype == dtype and a.shape == e.shape and np.all(err <= bound), what
    plain = run_conv(nb, x, w, np.zeros_like(bias), g)[0]            # and without a bias
    from d3d_amd.voxel import subm_conv3d
    assert ref.same_bits(N(subm_conv3d(T(x), nb, T(w))) + np.zeros_like(plain), plain)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_chunk_rows(dtype):
    """chunk_rows = 1000 against the default: all four results within the bound; forward and grad_features, whose rows do not depend
    on the chunking, exactly.  (4097 voxels are one GEMM call of 8192 rows and chunk_rows is rounded up to whole calls, so both runs
    make the same calls here; test_chunk_rows_with_many_gemm_calls splits them.)"""
    from d3d_amd.voxel import VoxelNeighbors
    c, b, tab, x, w, bias, g = conv_case("v4097", (3, 3, 3), 1, 16, 16, dtype, 5)
    nb = VoxelNeighbors(T(c), 3, 1, T(b))
    whole, parts = run_conv(nb, x, w, bias, g), run_conv(nb, x, w, bias, g, chunk_rows=1000)
    bound = ref.bounds(x, tab, w, g, EPS[dtype], bias)
    for what, a, e, lim in zip(("out", "grad_features", "grad_weight", "grad_bias"), parts, whole, bound):
        print("%s %s: worst |difference| = %.3g" % (dtype.__name__, what, np.max(np.abs(a - e))))
        assert np.all(np.abs(a.astype(np.float64) - e) <= lim), what
    assert ref.same_bits(parts[0], whole[0]) and ref.same_bits(parts[1], whole[1])


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_chunk_rows_with_many_gemm_calls(dtype, monkeypatch):
    """the same with GEMM calls of 256 rows, as on a frame beyond 65536 voxels: the default is one chunk of 17 calls (the last one
    padded with zero rows), chunk_rows = 1000 becomes 1024 = five chunks of four calls, chunk_rows = 1 one chunk per call.  torch's
    GEMM alone gives the same rows other last bits in calls of 4097 and of 1000 rows (fp32, K Cin = 432: up to 9e-05 on an MI355X);
    with one call shape the rows are bit-equal"""
    from d3d_amd.voxel import VoxelNeighbors, conv
    monkeypatch.setattr(conv, "_GEMM_TILE_ROWS", (256, 256))
    c, b, tab, x, w, bias, g = conv_case("v4097", (3, 3, 3), 1, 16, 16, dtype, 5)
    nb = VoxelNeighbors(T(c), 3, 1, T(b))
    assert conv._chunk_rows(1000, nb, 16, 16, x.itemsize) == 1024 and conv._chunk_rows(1, nb, 16, 16, x.itemsize) == 256
    whole = run_conv(nb, x, w, bias, g)
    bound = ref.bounds(x, tab, w, g, EPS[dtype], bias)
    want = (ref.conv(x, tab, w, bias),) + ref.conv_backward(x, tab, w, g)
    for rows in (1000, 1):
        parts = run_conv(nb, x, w, bias, g, chunk_rows=rows)
        for what, a, e, m, lim in zip(("out", "grad_features", "grad_weight", "grad_bias"), parts, whole, want, bound):
            assert np.all(np.abs(a.astype(np.float64) - e) <= lim) and np.all(np.abs(a.astype(np.float64) - m) <= lim), (what, rows)
        assert ref.same_bits(parts[0], whole[0]) and ref.same_bits(parts[1], whole[1]), rows


def test_gradcheck_fp64():
    from d3d_amd.voxel import VoxelNeighbors, neighbor_gather, subm_conv3d
    c = cases.fill((5, 5, 5), 60, 12)
    nb = VoxelNeighbors(T(c))
    assert nb.num_entries > 300
    r = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn((60, 3), dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    w = torch.randn((27, 3, 2), dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    bias = torch.randn(2, dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b_, c_: subm_conv3d(a, nb, b_, c_), (x, w, bias))
    assert torch.autograd.gradcheck(lambda a, b_: subm_conv3d(a, nb, b_, chunk_rows=7), (x, w))
    assert torch.autograd.gradcheck(lambda a: neighbor_gather(a, nb), (x,))


def test_host_tensors_and_numpy_arrays():
    from d3d_amd.voxel import VoxelNeighbors, neighbor_gather, subm_conv3d
    c, b, tab, x, w, bias, g = conv_case("batches", (3, 3, 3), 1, 5, 3, np.float32, 8)
    nb = VoxelNeighbors(c, batch_index=b)
    want = N(subm_conv3d(T(x), nb, T(w), T(bias)))
    a = subm_conv3d(x, nb, w, bias)
    assert isinstance(a, np.ndarray) and ref.same_bits(a, want)
    xt, wt, bt = (torch.from_numpy(t).requires_grad_() for t in (x, w, bias))
    out = subm_conv3d(xt.t().contiguous().t(), nb, wt, bt)               # a non-contiguous view
    assert out.device.type == "cpu" and ref.same_bits(out.detach().numpy(), want)
    out.backward(torch.from_numpy(g))
    dev = run_conv(nb, x, w, bias, g)
    assert all(t.grad.device.type == "cpu" for t in (xt, wt, bt))
    assert ref.same_bits(xt.grad.numpy(), dev[1]) and ref.same_bits(wt.grad.numpy(), dev[2]) and ref.same_bits(bt.grad.numpy(), dev[3])
    ga = neighbor_gather(x.astype(np.float64), nb)
    assert isinstance(ga, np.ndarray) and ref.same_bits(ga, ref.gather(x.astype(np.float64), tab))
    ht = torch.from_numpy(x).requires_grad_()
    hg = neighbor_gather(ht, nb)
    assert hg.device.type == "cpu"
    hg.backward(torch.ones_like(hg))
    assert ht.grad.device.type == "cpu" and ref.same_bits(ht.grad.numpy(), ref.gather_backward(np.ones((len(c), 27, 5), np.float32), tab))
    with pytest.raises(ValueError):
        subm_conv3d(T(x), nb, T(w.astype(np.float64)))
    with pytest.raises(ValueError):
        subm_conv3d(T(x), nb, T(w[:26]))
    with pytest.raises(ValueError):
        subm_conv3d(T(x[:-1]), nb, T(w))
    with pytest.raises(ValueError):
        neighbor_gather(T(x).half(), nb)
