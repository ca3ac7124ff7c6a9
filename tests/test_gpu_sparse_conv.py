"""GPU: SparseConvMap / sparse_conv3d / sparse_inverse_conv3d (vstride.hip, the gather of vnbr.hip) against the numpy model
(sparse_conv_reference.py): the output rows, both tables and the counts EXACTLY, the convolutions within the derived dot-product
bound of sparse_conv_reference.bounds."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_cases as cases
import sparse_conv_reference as ref
import voxel_conv_reference as vref

pytestmark = pytest.mark.gpu

EPS = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}
FILL = -7


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def i32x3(x):
    return (ctypes.c_int32 * 3)(*ref.triple(x))


def shifted(numel, dtype):
    """a buffer of `numel` elements one int32 (int64 for int64) past a 16-byte boundary, prefilled with FILL"""
    slab = torch.full((numel + 1,), FILL, dtype=dtype, device="cuda")
    assert numel == 0 or (slab.data_ptr() % 16 == 0 and slab[1:].data_ptr() % 16 == slab.element_size())
    return slab[1:]


def raw_map(c, b, config, shape=None, num_out=None):
    """d3d_sparse_conv_map_count, one read, d3d_sparse_conv_map_emit by hand
    -> (rc of count, rc of emit, counts after emit, out_coords, out_batch, table_in, table_out, counts after count)"""
    from d3d_amd import _lib
    lib = _lib.load()
    ks, st, pad, dil = (ref.triple(x) for x in config)
    v, k = len(c), int(np.prod(ks))
    shape_arg = None if shape is None else (ctypes.c_int64 * 3)(*shape)
    counts = torch.full((5,), FILL, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.d3d_sparse_conv_map_workspace_bytes(v, i32x3(ks), i32x3(st), i32x3(dil)), dtype=torch.uint8, device="cuda")
    ct, bt = T(c), T(b)                                             # (held until the results are back)
    args = (P(ct), P(bt), v, i32x3(ks), i32x3(st), i32x3(pad), i32x3(dil), shape_arg)
    rc1 = lib.d3d_sparse_conv_map_count(*args, P(counts), P(ws), ws.numel(), stream())
    first = N(counts).tolist()
    vout = first[0] if num_out is None else num_out
    oc, ob = shifted(vout * 3, torch.int64).view(vout, 3), shifted(vout, torch.int64)
    t_in, t_out = shifted(v * k, torch.int32).view(v, k), shifted(vout * k, torch.int32).view(vout, k)
    rc2 = lib.d3d_sparse_conv_map_emit(*args, vout, P(oc), P(ob), P(t_in), P(t_out), P(counts), P(ws), ws.numel(), stream())
    return rc1, rc2, N(counts).tolist(), N(oc), N(ob), N(t_in), N(t_out), first


def overflows(name, config, shape):
    """does the output box of this case pass 2^62 cells (`comb`: 2^61 along x, times the kernel's reach on y and z)?"""
    c, b = cases.SCENES[name]
    _, span, _, b_span, _ = ref.frame(c, *cases.CONFIGS[config], batch=b, spatial_shape=shape)
    return span[0] * span[1] * span[2] * b_span > 2 ** 62


@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_map_is_the_model_map(name, config):
    """the class, then the C entries (with the scene's batch; NULL where it has none), without and with a spatial_shape"""
    from d3d_amd.voxel import SparseConvMap
    c, b = cases.SCENES[name]
    ks, st, pad, dil = cases.CONFIGS[config]
    for with_shape in (False, True) if cases.shape_of(name, config) else (False,):
        shape = cases.shape_of(name, config) if with_shape else None
        if overflows(name, config, shape):
            with pytest.raises(ValueError, match="2\\^62"):
                SparseConvMap(T(c), ks, st, pad, dil, T(b), shape)
            rc1, rc2, counts, oc, ob, t_in, t_out, _ = raw_map(c, b, cases.CONFIGS[config], shape)
            assert (rc1, rc2) == (0, 0) and counts == [0, 0, 0, 1, 0] and np.all(t_in == FILL) and oc.size == 0 and t_out.size == 0
            continue
        want_oc, want_ob, want_out, want_in = cases.model(name, config, with_shape)
        entries = int((want_in >= 0).sum())
        m = SparseConvMap(T(c), ks, st, pad, dil, T(b), shape)
        assert m.out_coords.dtype == torch.int64 and m.table_out.dtype == torch.int32 and m.table_in.dtype == torch.int32
        assert all(t.is_cuda for t in (m.out_coords, m.table_out, m.table_in))
        assert np.array_equal(N(m.out_coords), want_oc) and np.array_equal(N(m.table_out), want_out) and np.array_equal(N(m.table_in), want_in)
        assert (m.out_batch is None) == (b is None) and (b is None or np.array_equal(N(m.out_batch), want_ob))
        assert (m.num_voxels, m.num_out, m.num_entries, m.kernel_volume) == (len(c), len(want_oc), entries, want_in.shape[1])
        assert (m.kernel_size, m.stride, m.padding, m.dilation, m.spatial_shape) == tuple(ref.triple(x) for x in (ks, st, pad, dil)) + (shape,)
        rc1, rc2, counts, oc, ob, t_in, t_out, first = raw_map(c, b, cases.CONFIGS[config], shape)
        assert (rc1, rc2) == (0, 0) and first == counts == [len(want_oc), entries, 0, 0, 0]
        assert np.array_equal(oc, want_oc) and np.array_equal(t_in, want_in) and np.array_equal(t_out, want_out)
        assert np.array_equal(ob, want_ob) if b is not None else np.all(ob == FILL)


def test_two_builds_give_the_same_bits():
    from d3d_amd.voxel import SparseConvMap
    for name, config in (("fill32", "k3s2p1"), ("batches_negative", "k5s2p2"), ("voxelizer_range", "k2s2p0")):
        c, b = cases.SCENES[name]
        a = SparseConvMap(T(c), *cases.CONFIGS[config], batch_index=T(b))
        torch.empty(1 << 22, device="cuda").normal_()                # (other work in between)
        again = SparseConvMap(T(c), *cases.CONFIGS[config], batch_index=T(b))
        raw = raw_map(c, b, cases.CONFIGS[config])
        for x, y, z in ((a.out_coords, again.out_coords, raw[3]), (a.table_in, again.table_in, raw[5]), (a.table_out, again.table_out, raw[6])):
            assert torch.equal(x, y) and np.array_equal(N(x), z)


def test_inputs_of_every_kind_build_the_same_map():
    from d3d_amd.voxel import SparseConvMap
    c, b = cases.SCENES["batches_negative"]
    want = cases.model("batches_negative", "k3s2p1")
    for ct, bt in ((T(c), T(b)), (c, b), (torch.from_numpy(c), torch.from_numpy(b)), (T(c.astype(np.int32)), T(b.astype(np.int32))),
                   (T(c)[:, [2, 1, 0]].flip(1), b)):
        m = SparseConvMap(ct, 3, 2, 1, batch_index=bt)
        assert m.out_coords.is_cuda and m.out_coords.dtype == torch.int64 and m.out_batch.dtype == torch.int64
        for got, e in zip((m.out_coords, m.out_batch, m.table_out, m.table_in), want):
            assert np.array_equal(N(got), e)
    m = SparseConvMap(T(c), (3, 3, 3), [2, 2, 2], (1, 1, 1), (1, 1, 1), T(b))
    assert np.array_equal(N(m.table_in), want[3])


def test_duplicates_are_refused():
    from d3d_amd.voxel import SparseConvMap
    c, _ = cases.SCENES["v65"]
    twice = np.concatenate([c, c[7:8]])
    with pytest.raises(ValueError, match="another row already has"):
        SparseConvMap(T(twice), 3, 2, 1)
    rc1, rc2, counts, oc, ob, t_in, t_out, first = raw_map(twice, None, cases.CONFIGS["k3s2p1"])
    good = cases.model("v65", "k3s2p1")
    assert (rc1, rc2) == (0, 0) and first[2:] == [0, 0, 0] and counts[3:] == [0, 0]
    assert counts[2] == int((good[3][7] >= 0).sum())               # every candidate of the second copy loses its claim
    assert counts[0] == len(good[0]) and counts[1] == int((good[3] >= 0).sum()) + counts[2] and np.array_equal(oc, good[0])
    assert t_in.min() >= -1 and t_in.max() < counts[0] and t_out.min() >= -1 and t_out.max() < 66
    c, b = cases.SCENES["batches"]                                  # without the batch ids: the cloud of batch 0 and 1 twice
    with pytest.raises(ValueError, match="another row already has"):
        SparseConvMap(T(c), 2, 2)
    rc1, rc2, counts, oc, ob, t_in, t_out, _ = raw_map(c, None, cases.CONFIGS["k312s213d211"])
    once = int((ref.build(np.unique(c, axis=0), *cases.CONFIGS["k312s213d211"])[3] >= 0).sum())
    assert (rc1, rc2) == (0, 0) and counts[2] == counts[1] - once > 500           # every candidate of a second copy loses its claim
    assert t_in.min() >= -1 and t_in.max() < counts[0] and t_out.min() >= -1 and t_out.max() < len(c)
    m = SparseConvMap(T(c), 3, 2, 1, batch_index=T(b))             # the next call is as good as ever
    assert np.array_equal(N(m.table_out), cases.model("batches", "k3s2p1")[2])


def test_span_overflow_touches_nothing():
    from d3d_amd.voxel import SparseConvMap
    wide = np.array([[0, 0, 0], [2 ** 21, 2 ** 21, 2 ** 21], [5, 5, 5]], np.int64)      # an output box of (2^21 + 3)^3 cells
    half = np.array([[-2 ** 62, 0, 0], [2 ** 62, 0, 0]], np.int64)                       # inputs that span 2^63 on x
    whole = np.array([[-2 ** 63, 0, 0], [2 ** 63 - 1, 0, 0]], np.int64)
    for c, config in ((wide, (3, 1, 1, 1)), (half, (2, 2 ** 24, 0, 1)), (whole, (1, 1, 0, 1)), (whole, (3, 2, 1, 1))):
        with pytest.raises(ValueError, match="2\\^62"):
            SparseConvMap(T(c), *config)
        rc1, rc2, counts, oc, ob, t_in, t_out, first = raw_map(c, None, config)
        assert (rc1, rc2) == (0, 0) and first == counts == [0, 0, 0, 1, 0] and np.all(t_in == FILL)
        rc1, rc2, counts, oc, ob, t_in, t_out, _ = raw_map(c, None, config, num_out=2)  # and with a num_out the counts do not back
        assert (rc1, rc2) == (0, 0) and counts == [0, 0, 0, 1, 0] and np.all(t_in == FILL) and np.all(oc == FILL) and np.all(ob == FILL)
        assert np.all(t_out == -1)                                  # (the prefill of the rows the caller asked for)
    edge = np.array([[0, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 0], [1, 0, 0]], np.int64)      # k1 s1: 2^62 cells exactly: fits
    m = SparseConvMap(T(edge), 1, 1)
    assert np.array_equal(N(m.out_coords), edge) and N(m.table_in).ravel().tolist() == [0, 1, 2]
    rc1, rc2, counts, *_ = raw_map(edge, np.array([0, 1, 0]), (1, 1, 0, 1))               # times two batches: does not
    assert (rc1, rc2) == (0, 0) and counts == [0, 0, 0, 1, 0]


def test_inputs_outside_the_spatial_shape_are_refused():
    from d3d_amd.voxel import SparseConvMap
    c, _ = cases.SCENES["v65"]                                      # inside (6, 6, 6)
    for bad, shape in ((c, (6, 5, 6)), (c - np.array([0, 0, 1]), (6, 6, 6)), (c, (3, 40, 40))):
        assert bad.min() < 0 or np.any(bad.max(0) >= np.array(shape))
        with pytest.raises(ValueError, match="outside spatial_shape"):
            SparseConvMap(T(bad), 3, 2, 1, spatial_shape=shape)
        rc1, rc2, counts, oc, ob, t_in, t_out, first = raw_map(bad, None, cases.CONFIGS["k3s2p1"], shape)
        assert (rc1, rc2) == (0, 0) and first == counts == [0, 0, 0, 0, 1] and np.all(t_in == FILL)
    m = SparseConvMap(T(c), 3, 2, 1, spatial_shape=(6, 6, 6))
    assert np.array_equal(N(m.table_out), ref.build(c, 3, 2, 1, 1, None, (6, 6, 6))[2])


def test_too_many_candidates_are_refused_without_launching():
    from d3d_amd import _lib
    from d3d_amd.voxel import SparseConvMap
    lib = _lib.load()
    many = torch.zeros((1, 3), dtype=torch.int64, device="cuda").expand(2 ** 31 // 8 + 1, 3)      # one row behind every index
    with pytest.raises(ValueError, match="candidates"):
        SparseConvMap(many, 3, 2, 1)
    c, _ = cases.SCENES["v65"]
    ct = T(c)
    counts = torch.full((5,), FILL, dtype=torch.int64, device="cuda")
    need = lib.d3d_sparse_conv_map_workspace_bytes(65, i32x3(3), i32x3(2), i32x3(1))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    t_in, t_out = torch.full((65, 27), FILL, dtype=torch.int32, device="cuda"), torch.full((99, 27), FILL, dtype=torch.int32, device="cuda")
    oc = torch.full((99, 3), FILL, dtype=torch.int64, device="cuda")

    def count(co=P(ct), v=65, ks=3, st=2, pad=1, dil=1, shape=None, cn=P(counts), w=P(ws), nb=need):
        return lib.d3d_sparse_conv_map_count(co, None, v, i32x3(ks), i32x3(st), i32x3(pad), i32x3(dil), shape, cn, w, nb, stream())

    def emit(co=P(ct), v=65, ks=3, st=2, num_out=99, o=P(oc), ti=P(t_in), to=P(t_out), cn=P(counts), w=P(ws), nb=need):
        return lib.d3d_sparse_conv_map_emit(co, None, v, i32x3(ks), i32x3(st), i32x3(1), i32x3(1), None, num_out, o, None, ti, to, cn, w, nb, stream())

    for call in (count, emit):
        assert call(v=2 ** 31 // 8 + 1) == _lib.ERR_UNSUPPORTED and call(v=2 ** 31) == _lib.ERR_UNSUPPORTED
        assert call(ks=(3, 3, 8)) == _lib.ERR_BAD_ARG and call(st=0) == _lib.ERR_BAD_ARG and call(co=None) == _lib.ERR_BAD_ARG
        assert call(cn=None) == _lib.ERR_BAD_ARG and call(w=None) == _lib.ERR_WORKSPACE and call(nb=need - 1) == _lib.ERR_WORKSPACE
    assert count(shape=(ctypes.c_int64 * 3)(6, 6, 0)) == _lib.ERR_BAD_ARG and count(pad=2 ** 24 + 1) == _lib.ERR_UNSUPPORTED
    assert emit(num_out=-1) == _lib.ERR_BAD_ARG and emit(num_out=65 * 8 + 1) == _lib.ERR_BAD_ARG
    assert emit(o=None) == _lib.ERR_BAD_ARG and emit(ti=None) == _lib.ERR_BAD_ARG and emit(to=None) == _lib.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((counts == FILL).all()) and bool((t_in == FILL).all()) and bool((t_out == FILL).all()) and bool((oc == FILL).all()) and not ws.any()


def test_nothing_to_do():
    from d3d_amd import _lib
    from d3d_amd.voxel import SparseConvMap, sparse_conv3d, sparse_inverse_conv3d
    lib = _lib.load()
    m = SparseConvMap(torch.zeros((0, 3), dtype=torch.int64, device="cuda"), (3, 1, 2), 2, 1)
    assert m.table_in.shape == (0, 6) and m.table_out.shape == (0, 6) and m.out_coords.shape == (0, 3) and m.out_batch is None
    assert (m.num_voxels, m.num_out, m.num_entries) == (0, 0, 0)
    m = SparseConvMap(np.zeros((0, 3), np.int32), 2, 2, batch_index=np.zeros(0, np.int64), spatial_shape=(4, 4, 4))
    assert m.out_batch.shape == (0,) and m.table_out.shape == (0, 8)
    counts = torch.full((5,), FILL, dtype=torch.int64, device="cuda")
    assert lib.d3d_sparse_conv_map_count(None, None, 0, i32x3(3), i32x3(2), i32x3(1), i32x3(1), None, P(counts), None, 0, stream()) == 0
    assert N(counts).tolist() == [0, 0, 0, 0, 0]
    assert lib.d3d_sparse_conv_map_emit(None, None, 0, i32x3(3), i32x3(2), i32x3(1), i32x3(1), None, 0, None, None, None, None, P(counts),
                                        None, 0, stream()) == 0
    # Vout == 0 with V > 0: k2 s2 p0 on a (7, 2, 2) grid has the outputs 0 .. 2 on x, and x = 6 belongs to output 3; the other
    # voxel feeds the kept output (0, 0, 0)
    clipped = np.array([[6, 0, 0], [6, 1, 1]], np.int64)
    m = SparseConvMap(T(clipped), 2, 2, spatial_shape=(7, 2, 2))
    assert (m.num_out, m.num_entries) == (0, 0) and m.table_out.shape == (0, 8) and bool((m.table_in == -1).all())
    rc1, rc2, counts, oc, ob, t_in, t_out, _ = raw_map(clipped, None, (2, 2, 0, 1), (7, 2, 2))
    assert (rc1, rc2) == (0, 0) and counts == [0, 0, 0, 0, 0] and np.all(t_in == -1)
    both = np.array([[6, 0, 0], [1, 1, 1]], np.int64)
    m2 = SparseConvMap(T(both), 2, 2, spatial_shape=(7, 2, 2))
    assert N(m2.out_coords).tolist() == [[0, 0, 0]] and N(m2.table_in).tolist() == [[-1] * 8, [-1] * 7 + [0]]
    # no candidate at all without any clipping: k1 s2 reads the even coordinates only
    m3 = SparseConvMap(T(np.array([[1, 0, 0], [3, 5, 2]], np.int64)), 1, 2)
    assert m3.num_out == 0 and N(m3.table_in).tolist() == [[-1], [-1]]
    for mm, cin in ((m, 4), (m3, 3)):
        k = mm.kernel_volume
        f = torch.ones((2, cin), device="cuda", requires_grad=True)
        w = torch.ones((k, cin, 2), device="cuda", requires_grad=True)
        out = sparse_conv3d(f, mm, w, torch.ones(2, device="cuda"))
        assert out.shape == (0, 2)
        out.sum().backward()
        assert f.grad.shape == (2, cin) and not f.grad.any() and w.grad.shape == (k, cin, 2) and not w.grad.any()
        up = sparse_inverse_conv3d(torch.zeros((0, cin), device="cuda"), mm, w.detach(), torch.full((2,), 3.0, device="cuda"))
        assert up.shape == (2, 2) and bool((up == 3).all())


# ---------------------------------------------------------------- the convolutions

def conv_case(name, config, cin, cout, dtype, seed, inverse=False):
    """-> (the SparseConvMap, the table the rows are read through, its transposed one, x, w, bias, grad_out)"""
    from d3d_amd.voxel import SparseConvMap
    c, b = cases.SCENES[name]
    _, _, t_out, t_in = cases.model(name, config)
    tab, back = (t_in, t_out) if inverse else (t_out, t_in)
    r = np.random.default_rng(seed)
    x, w = r.standard_normal((len(back), cin)).astype(dtype), r.standard_normal((tab.shape[1], cin, cout)).astype(dtype)
    bias, g = r.standard_normal(cout).astype(dtype), r.standard_normal((len(tab), cout)).astype(dtype)
    return SparseConvMap(T(c), *cases.CONFIGS[config], batch_index=T(b)), tab, back, x, w, bias, g


def run_conv(fn, m, x, w, bias, g, **kw):
    xt, wt, bt = T(x).requires_grad_(), T(w).requires_grad_(), T(bias).requires_grad_()
    out = fn(xt, m, wt, bt, **kw)
    out.backward(T(g))
    return N(out), N(xt.grad), N(wt.grad), N(bt.grad)


@pytest.mark.parametrize("inverse", (False, True), ids=("conv", "inverse"))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("name,config", [("v4097", "k3s2p1"), ("batches", "k312s213d211"), ("batches_negative", "k2s2p0"), ("negative_odd", "k5s2p2")])
def test_convolutions_against_the_fp64_model(name, config, dtype, inverse):
    """forward and the three gradients within ref.bounds: (K Cin + 2) eps sum|x||w| per output, the reduction lengths K Cout for
    grad_features and the output's row count for grad_weight and grad_bias; eps = 2^-52 in fp64, 2^-23 in fp32 (the model runs in
    fp64 on the same fp32 inputs).  Odd channel counts: 5 -> 7"""
    from d3d_amd.voxel import sparse_conv3d, sparse_inverse_conv3d
    fn = sparse_inverse_conv3d if inverse else sparse_conv3d
    m, tab, back, x, w, bias, g = conv_case(name, config, 5, 7, dtype, 21, inverse)
    got = run_conv(fn, m, x, w, bias, g)
    want = (ref.conv(x, tab, w, bias),) + ref.conv_backward(x, tab, back, w, g)
    assert got[0].shape == (len(tab), 7) and got[1].shape == x.shape
    for what, a, e, bound in zip(("out", "grad_features", "grad_weight", "grad_bias"), got, want, ref.bounds(x, tab, back, w, g, EPS[dtype], bias)):
        err = np.abs(a.astype(np.float64) - e)
        print("%s: worst |err| / bound = %.4f" % (what, np.max(err[bound > 0] / bound[bound > 0])))
        assert a.dtype == dtype and a.shape == e.shape and np.all(err <= bound), what
    plain = run_conv(fn, m, x, w, np.zeros_like(bias), g)[0]         # and without a bias: the bits of the zero-bias run
    assert ref.same_bits(N(fn(T(x), m, T(w))) + np.zeros_like(plain), plain)


@pytest.mark.parametrize("inverse", (False, True), ids=("conv", "inverse"))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_chunk_rows(dtype, inverse, monkeypatch):
    """GEMM calls of 256 rows, as on a frame beyond 65536 voxels: chunk_rows = 1000 (rounded up to 1024) and 1 (one call per
    chunk) against the default.  Forward and grad_features, whose rows do not depend on the chunking, bit for bit; grad_weight, a
    sum over the chunks, within the bound -- of each other and of the model"""
    from d3d_amd.voxel import conv, sparse_conv3d, sparse_inverse_conv3d
    fn = sparse_inverse_conv3d if inverse else sparse_conv3d
    monkeypatch.setattr(conv, "_GEMM_TILE_ROWS", (256, 256))
    m, tab, back, x, w, bias, g = conv_case("v4097", "k3s2p1", 16, 16, dtype, 5, inverse)
    assert len(tab) > 1024 and len(back) > 1024
    whole = run_conv(fn, m, x, w, bias, g)
    bound = ref.bounds(x, tab, back, w, g, EPS[dtype], bias)
    want = (ref.conv(x, tab, w, bias),) + ref.conv_backward(x, tab, back, w, g)
    for rows in (1000, 1):
        parts = run_conv(fn, m, x, w, bias, g, chunk_rows=rows)
        for what, a, e, mod, lim in zip(("out", "grad_features", "grad_weight", "grad_bias"), parts, whole, want, bound):
            print("%s %s chunk_rows=%d: worst |difference| = %.3g" % (dtype.__name__, what, rows, np.max(np.abs(a - e))))
            assert np.all(np.abs(a.astype(np.float64) - e) <= lim) and np.all(np.abs(a.astype(np.float64) - mod) <= lim), (what, rows)
        assert ref.same_bits(parts[0], whole[0]) and ref.same_bits(parts[1], whole[1]), rows


def test_gradcheck_fp64():
    from d3d_amd.voxel import SparseConvMap, sparse_conv3d, sparse_inverse_conv3d
    c = cases.fill((5, 5, 5), 60, 12, shift=(-3, 0, 2))
    m = SparseConvMap(T(c), 3, 2, 1)
    assert m.num_entries > 150 and 1 < m.num_out < 60
    r = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn((60, 3), dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    z = torch.randn((m.num_out, 3), dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    w = torch.randn((27, 3, 2), dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    bias = torch.randn(2, dtype=torch.float64, device="cuda", generator=r, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b_, c_: sparse_conv3d(a, m, b_, c_), (x, w, bias))
    assert torch.autograd.gradcheck(lambda a, b_: sparse_conv3d(a, m, b_, chunk_rows=7), (x, w))
    assert torch.autograd.gradcheck(lambda a, b_, c_: sparse_inverse_conv3d(a, m, b_, c_), (z, w, bias))
    assert torch.autograd.gradcheck(lambda a, b_: sparse_inverse_conv3d(a, m, b_, chunk_rows=7), (z, w))


def test_host_tensors_and_numpy_arrays():
    from d3d_amd.voxel import SparseConvMap, sparse_conv3d, sparse_inverse_conv3d
    for inverse, fn in ((False, sparse_conv3d), (True, sparse_inverse_conv3d)):
        m, tab, back, x, w, bias, g = conv_case("batches_negative", "k3s2p1", 5, 3, np.float32, 8, inverse)
        want = N(fn(T(x), m, T(w), T(bias)))
        a = fn(x, m, w, bias)
        assert isinstance(a, np.ndarray) and ref.same_bits(a, want)
        xt, wt, bt = (torch.from_numpy(t).requires_grad_() for t in (x, w, bias))
        out = fn(xt.t().contiguous().t(), m, wt, bt)                 # a non-contiguous view
        assert out.device.type == "cpu" and ref.same_bits(out.detach().numpy(), want)
        out.backward(torch.from_numpy(g))
        dev = run_conv(fn, m, x, w, bias, g)
        assert all(t.grad.device.type == "cpu" for t in (xt, wt, bt))
        assert ref.same_bits(xt.grad.numpy(), dev[1]) and ref.same_bits(wt.grad.numpy(), dev[2]) and ref.same_bits(bt.grad.numpy(), dev[3])
        with pytest.raises(ValueError):
            fn(T(x), m, T(w.astype(np.float64)))
        with pytest.raises(ValueError):
            fn(T(x), m, T(w[:26]))
        with pytest.raises(ValueError):
            fn(T(x[:-1]), m, T(w))
        with pytest.raises(ValueError):
            fn(T(x).half(), m, T(w).half())
    c, b = cases.SCENES["batches_negative"]
    host = SparseConvMap(c, 3, 2, 1, batch_index=b)                  # a map from host arrays lives on the GPU all the same
    assert host.table_in.is_cuda and torch.equal(host.table_in, m.table_in)


def test_chain_down_and_up_again():
    """subm_conv3d -> sparse_conv3d (k3 s2 p1) -> VoxelNeighbors(out_coords, out_batch) -> subm_conv3d -> sparse_inverse_conv3d back
    on the input rows, fp32, against the fp64 model chain.  The chain is linear, so the bound of a stage's output is its own
    dot-product bound on the magnitudes it sees (|x| + the error so far) plus the error so far carried through |W|; the input
    gradient runs the transposed chain the same way"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d
    c, b = cases.SCENES["batches_negative"]
    oc, ob, t_out, t_in = cases.model("batches_negative", "k3s2p1")
    tab1, tab2 = vref.table(c, 3, 1, b), vref.table(oc, 3, 1, ob)
    r = np.random.default_rng(17)
    chans = (4, 6, 8, 8, 5)
    x = r.standard_normal((len(c), chans[0])).astype(np.float32)
    ws = [(r.standard_normal((27, chans[i], chans[i + 1])) / 4).astype(np.float32) for i in range(4)]
    g = r.standard_normal((len(c), chans[4])).astype(np.float32)
    nb1, m = VoxelNeighbors(T(c), batch_index=T(b)), SparseConvMap(T(c), 3, 2, 1, batch_index=T(b))
    nb2 = VoxelNeighbors(m.out_coords, batch_index=m.out_batch)
    assert np.array_equal(N(nb2.table), tab2)
    xt = T(x).requires_grad_()
    y = sparse_inverse_conv3d(subm_conv3d(sparse_conv3d(subm_conv3d(xt, nb1, T(ws[0])), m, T(ws[1])), nb2, T(ws[2])), m, T(ws[3]))
    y.backward(T(g))
    eps = EPS[np.float32]
    # forward tables, and the tables of the transposed stages (a submanifold table transposes into its mirrored columns)
    fwd = (tab1, t_out, tab2, t_in)
    bwd = (tab1[:, ::-1], t_in, tab2[:, ::-1], t_out)

    def walk(val, tabs, weights):
        err = np.zeros_like(val, dtype=np.float64)
        val = val.astype(np.float64)
        for tab, w in zip(tabs, weights):
            k, cin, _ = w.shape
            aw = np.abs(w.astype(np.float64))
            err = (k * cin + 2) * eps * ref.conv(np.abs(val) + err, tab, aw) + ref.conv(err, tab, aw)
            val = ref.conv(val, tab, w)
        return val, err

    want, bound = walk(x, fwd, ws)
    err = np.abs(N(y).astype(np.float64) - want)
    print("chain out: worst |err| / bound = %.4f" % np.max(err / bound))
    assert y.shape == (len(c), chans[4]) and np.all(err <= bound)
    want_g, bound_g = walk(g, bwd[::-1], [np.ascontiguousarray(w.transpose(0, 2, 1)) for w in ws[::-1]])
    err = np.abs(N(xt.grad).astype(np.float64) - want_g)
    print("chain grad: worst |err| / bound = %.4f" % np.max(err / bound_g))
    assert xt.grad.shape == x.shape and np.all(err <= bound_g)
