"""GPU: the fused table convolution (csrc/vconv.hip; method="fused" of subm_conv3d / sparse_conv3d / sparse_inverse_conv3d) against
the fp64 model of table_conv_reference.py: bit for bit on integer data, within the fp32-accumulation bound on random data, the same
bits for a row wherever it sits and on every run, the routing of `method`, and one list of malformed calls that all three operators
refuse alike."""
import functools

import numpy as np
import pytest
import torch

import sparse_conv_cases as scases
import table_conv_cases as cases
import table_conv_reference as ref
import voxel_conv_cases as vcases
import voxel_conv_reference as vref

pytestmark = pytest.mark.gpu

KINDS = ("f32", "f16", "bf16")
NAMES = [c[0] for c in cases.CASES]
# the bound test: every small case, one of several workgroups and one of two weight-gradient slabs
BOUND_NAMES = list(cases.SMALL) + ["block12-k27", "v4097-k27"]


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def operator(op, scene, kernel):
    """-> fn(features, weight, bias, **kw) of a case on a freshly built table, and the table's owner"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d
    c, b = cases.SCENES[scene]
    if op == "subm":
        owner = VoxelNeighbors(T(c), kernel, batch_index=T(b))
        return (lambda x, w, bias=None, **kw: subm_conv3d(x, owner, w, bias, **kw)), owner
    owner = SparseConvMap(T(c), *scases.CONFIGS[kernel], batch_index=T(b))
    f = sparse_conv3d if op == "down" else sparse_inverse_conv3d
    return (lambda x, w, bias=None, **kw: f(x, owner, w, bias, **kw)), owner


@functools.lru_cache(maxsize=None)
def built(name):
    _, op, scene, kernel, _, _ = cases.BY_NAME[name]
    return operator(op, scene, kernel)[0]


def run(fn, x, w, bias, g, **kw):
    """tensors of one dtype on the GPU -> (out, grad_features, grad_weight, grad_bias), detached"""
    xs = [t.detach().clone().requires_grad_() for t in (x, w, bias)]
    out = fn(*xs, **kw)
    out.backward(g)
    return (out.detach(),) + tuple(t.grad for t in xs)


def as_kind(arrays, kind):
    """float arrays -> GPU tensors of `kind` (rounded), and what they hold as float64 arrays"""
    ts = [torch.from_numpy(np.array(a, np.float32)).to(ref.TORCH[kind]).cuda() for a in arrays]
    return ts, [t.double().cpu().numpy() for t in ts]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_on_integers(name, kind):
    """every partial sum is an exact integer in fp32: forward, grad_features, grad_weight and grad_bias are RNE(exact), bit for bit"""
    fwd, back, _, _ = cases.tables(name)
    x, w, bias, g = cases.integers(name)
    ts, _ = as_kind((x, w, bias, g), kind)
    got = run(built(name), *ts, method="fused")
    want = (ref.conv(x, fwd, w, bias),) + ref.conv_backward(x, fwd, back, w, g)
    for what, a, b in zip(("out", "grad_features", "grad_weight", "grad_bias"), got, want):
        assert a.dtype == ref.TORCH[kind] and a.is_cuda
        assert ref.equal_bits(a, ref.round_to(b, kind)), what
    assert ref.equal_bits(built(name)(ts[0], ts[1], method="fused"), ref.round_to(ref.conv(x, fwd, w), kind)), "no bias"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", BOUND_NAMES)
def test_random_within_the_bound(name, kind):
    """|got - exact| <= E (1 + u) + u |exact| with E = (n + 2) 2^-24 sum|a||b|: n = K Cin for the forward, K Cout for grad_features,
    the rows for grad_weight and grad_bias; u the unit roundoff of the output type (none for fp32)"""
    fwd, back, _, rows = cases.tables(name)
    ts, (x, w, bias, g) = as_kind(cases.randoms(name), kind)
    got = run(built(name), *ts, method="fused")
    k, cin, cout = w.shape
    want = (ref.conv(x, fwd, w, bias),) + ref.conv_backward(x, fwd, back, w, g)
    mags = ref.magnitudes(x, fwd, back, w, g, bias)
    for what, n, a, b, m in zip(("out", "grad_features", "grad_weight", "grad_bias"), (k * cin, k * cout, rows, rows), got, want, mags):
        err, bound = np.abs(a.double().cpu().numpy() - b), ref.result_bound(n, m, b, kind)
        print("%s %s %s: worst |err| / bound = %.4f" % (name, kind, what, np.max(err / np.maximum(bound, 1e-300), initial=0)))
        assert np.all(err <= bound), what


def _rows_of(coords, batch):
    b = np.zeros(len(coords), np.int64) if batch is None else batch
    return {key: i for i, key in enumerate(zip(b.tolist(), *np.asarray(coords).T.tolist()))}


@pytest.mark.parametrize("kind", ("f32", "bf16"))
@pytest.mark.parametrize("op,scene,kernel,cin,cout", [("subm", "far_away", (3, 3, 3), 48, 16), ("subm", "batches", (3, 3, 3), 16, 32),
                                                       ("down", "negative_odd", "k3s2p1", 16, 32), ("up", "batches_negative", "k2s2p0", 32, 16)])
def test_rows_do_not_depend_on_their_position(op, scene, kernel, cin, cout, kind):
    """the voxels permuted (coords, batch, features): every output row and every grad_features row keeps its bits"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d
    c, b = cases.SCENES[scene]
    perm = np.random.default_rng(11).permutation(len(c))
    r = np.random.default_rng(12)
    dt = ref.TORCH[kind]
    results = []
    for order in (np.arange(len(c)), perm):
        co, bo = c[order], None if b is None else b[order]
        if op == "subm":
            owner = VoxelNeighbors(T(co), kernel, batch_index=T(bo))
            src, dst = (co, bo), (co, bo)
            fn = subm_conv3d
        else:
            owner = SparseConvMap(T(co), *scases.CONFIGS[kernel], batch_index=T(bo))
            oc, ob = owner.out_coords.cpu().numpy(), None if bo is None else owner.out_batch.cpu().numpy()
            src, dst = ((co, bo), (oc, ob)) if op == "down" else ((oc, ob), (co, bo))
            fn = sparse_conv3d if op == "down" else sparse_inverse_conv3d
        results.append((fn, owner, _rows_of(*src), _rows_of(*dst)))
    k = results[0][1].kernel_volume
    (_, _, src0, dst0), (_, _, src1, dst1) = results
    assert set(src0) == set(src1) and set(dst0) == set(dst1)
    x0 = torch.from_numpy(r.standard_normal((len(src0), cin)).astype(np.float32)).to(dt).cuda()
    g0 = torch.from_numpy(r.standard_normal((len(dst0), cout)).astype(np.float32)).to(dt).cuda()
    w = torch.from_numpy((r.standard_normal((k, cin, cout)) / 4).astype(np.float32)).to(dt).cuda()
    bias = torch.from_numpy(r.standard_normal(cout).astype(np.float32)).to(dt).cuda()
    # row i of the second run is row src_map[i] / dst_map[i] of the first
    inv_src, inv_dst = {i: key for key, i in src1.items()}, {i: key for key, i in dst1.items()}
    src_map = torch.tensor([src0[inv_src[i]] for i in range(len(src1))], device="cuda")
    dst_map = torch.tensor([dst0[inv_dst[i]] for i in range(len(dst1))], device="cuda")
    a = run(lambda *t, **kw: results[0][0](t[0], results[0][1], t[1], t[2], **kw), x0, w, bias, g0, method="fused")
    p = run(lambda *t, **kw: results[1][0](t[0], results[1][1], t[1], t[2], **kw), x0[src_map], w, bias, g0[dst_map], method="fused")
    assert ref.equal_bits(p[0], a[0][dst_map]) and ref.equal_bits(p[1], a[1][src_map])
    assert float(a[0].float().abs().max()) > 0 and float(a[1].float().abs().max()) > 0


@pytest.mark.parametrize("name,kind", [("v4097-k27", "f32"), ("v4097-k27", "bf16"), ("negative_odd-down-k3s2", "f16"),
                                       ("block12-k27", "bf16")])
def test_two_runs_give_the_same_bits(name, kind):
    ts, _ = as_kind(cases.randoms(name, seed=1), kind)
    first, second = run(built(name), *ts, method="fused"), run(built(name), *ts, method="fused")
    for a, b in zip(first, second):
        assert ref.equal_bits(a, b)


@pytest.mark.parametrize("name", ["far_away-k27", "negative_odd-down-k3s2", "negative_odd-up-k2s2", "v4097-k27"])
def test_fp32_routes(name):
    """method=None is the gather route, bit for bit; the fused route is within 2 E of it, the gradients too (there is no fp64
    fused route for gradcheck: the gather route's gradients have one)"""
    fwd, back, _, rows = cases.tables(name)
    ts, (x, w, bias, g) = as_kind(cases.randoms(name, seed=2), "f32")
    default, gather, fused = (run(built(name), *ts, method=m) for m in (None, "gather", "fused"))
    for a, b in zip(default, gather):
        assert ref.equal_bits(a, b)
    k, cin, cout = w.shape
    mags = ref.magnitudes(x, fwd, back, w, g, bias)
    for what, n, a, b, m in zip(("out", "grad_features", "grad_weight", "grad_bias"), (k * cin, k * cout, rows, rows), fused, gather, mags):
        err = np.abs(a.double().cpu().numpy() - b.double().cpu().numpy())
        print("%s %s: worst |fused - gather| / 2E = %.4f" % (name, what, np.max(err / (2 * ref.dot_bound(n, m)))))
        assert np.all(err <= 2 * ref.dot_bound(n, m)), what
    assert ref.equal_bits(run(built(name), *ts, method="fused", chunk_rows=7)[0], fused[0])       # checked and ignored
    with pytest.raises(ValueError):
        built(name)(*ts[:3], method="fused", chunk_rows=0)


def test_refusals():
    fn = built("far_away-k27")                                       # Cin = 48, Cout = 16
    _, _, src_rows, _ = cases.tables("far_away-k27")
    x, w = torch.zeros((src_rows, 48), device="cuda"), torch.zeros((27, 48, 16), device="cuda")
    with pytest.raises(ValueError):
        fn(x.double(), w.double(), method="fused")
    with pytest.raises(ValueError):
        fn(x[:, :5].contiguous(), w[:, :5].contiguous(), method="fused")
    with pytest.raises(ValueError):
        fn(x[:, :5].contiguous().bfloat16(), w[:, :5].contiguous().bfloat16())
    with pytest.raises(ValueError):
        fn(x.half(), w.half(), method="gather")
    with pytest.raises(ValueError):
        fn(x.half(), w)                                              # mixed dtypes
    with pytest.raises(ValueError):
        fn(x.bfloat16(), w.half())
    with pytest.raises(ValueError):
        fn(x.bfloat16(), w.bfloat16(), torch.zeros(16, device="cuda"))
    with pytest.raises(ValueError):
        fn(x, w, method="mfma")
    with pytest.raises(ValueError):
        fn(x.to(torch.int32), w.to(torch.int32))
    assert fn(x.bfloat16(), w.bfloat16()).dtype == torch.bfloat16 and fn(x.half(), w.half(), method="fused").dtype == torch.float16


BOTH = ("gather", "fused")
# (what is wrong, the exception, the methods it is tried with, (x [rows, 16], w [27, 16, 32], b [32], all fp32) -> (features, weight, bias, kw))
MALFORMED = (
    ("features 1-D", ValueError, BOTH, lambda x, w, b: (x[:, 0], w, b, {})),
    ("features of one row too few", ValueError, BOTH, lambda x, w, b: (x[:-1], w, b, {})),
    ("features int32", ValueError, BOTH, lambda x, w, b: (x.to(torch.int32), w, b, {})),
    ("weight with K - 1 slices", ValueError, BOTH, lambda x, w, b: (x, w[:-1], b, {})),
    ("weight with Cin + 1", ValueError, BOTH, lambda x, w, b: (x, torch.cat([w, w[:, :1]], 1), b, {})),
    ("weight in another dtype", ValueError, BOTH, lambda x, w, b: (x, w.double(), b, {})),
    ("bias of Cout + 1", ValueError, BOTH, lambda x, w, b: (x, w, torch.cat([b, b[:1]]), {})),
    ("bias in another dtype", ValueError, BOTH, lambda x, w, b: (x, w, b.double(), {})),
    ("chunk_rows = 0", ValueError, BOTH, lambda x, w, b: (x, w, b, {"chunk_rows": 0})),
    ("an unknown method", ValueError, ("mfma",), lambda x, w, b: (x, w, b, {})),
    ("fp64 on the fused route", ValueError, ("fused",), lambda x, w, b: (x.double(), w.double(), b.double(), {})),
    ("fp16 on the gather route", ValueError, ("gather",), lambda x, w, b: (x.half(), w.half(), b.half(), {})),
    ("Cin = 24 on the fused route", ValueError, ("fused",), lambda x, w, b: (torch.cat([x, x[:, :8]], 1), torch.cat([w, w[:, :8]], 1), b, {})),
    ("host features with a weight that is no tensor", TypeError, BOTH, lambda x, w, b: (x.cpu(), w.tolist(), b, {})),
)


def test_one_argument_check_serves_all_three_operators():
    """every malformed call is refused with the same exception type by subm_conv3d, sparse_conv3d and sparse_inverse_conv3d, on
    both routes where the call leaves the route open; the well-formed call passes on each"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d
    coords = T(vcases.fill((5, 5, 5), 60, 12))
    nbrs, cmap = VoxelNeighbors(coords, 3), SparseConvMap(coords, 3, 2, 1)
    w, b = torch.ones((27, 16, 32), device="cuda"), torch.ones(32, device="cuda")
    for op, owner, rows, out_rows in ((subm_conv3d, nbrs, 60, 60), (sparse_conv3d, cmap, 60, cmap.num_out),
                                      (sparse_inverse_conv3d, cmap, cmap.num_out, 60)):
        x = torch.ones((rows, 16), device="cuda")
        for method in BOTH:
            assert op(x, owner, w, b, method=method).shape == (out_rows, 32)
        for what, exception, methods, bend in MALFORMED:
            for method in methods:
                features, weight, bias, kw = bend(x, w, b)
                with pytest.raises(exception):
                    op(features, owner, weight, bias, method=method, **kw)
                    pytest.fail("%s, method=%r: %s took it" % (what, method, op.__name__))


def test_host_tensors_numpy_and_empty_inputs():
    from d3d_amd.voxel import VoxelNeighbors, subm_conv3d
    name = "line65-k27-16x32"
    fwd, back, _, _ = cases.tables(name)
    x, w, bias, g = cases.integers(name)
    want = ref.round_to(ref.conv(x, fwd, w, bias), "f16")
    out = built(name)(x.astype(np.float16), w.astype(np.float16), bias.astype(np.float16))
    assert isinstance(out, np.ndarray) and out.dtype == np.float16 and ref.equal_bits(torch.from_numpy(out), want)
    xs = [torch.from_numpy(a.copy()).bfloat16().requires_grad_() for a in (x, w, bias)]
    out = built(name)(*xs)
    out.backward(torch.from_numpy(g.copy()).bfloat16())
    wants = (ref.conv(x, fwd, w, bias),) + ref.conv_backward(x, fwd, back, w, g)
    for a, b in zip((out,) + tuple(t.grad for t in xs), wants):
        assert a.device.type == "cpu" and ref.equal_bits(a, ref.round_to(b, "bf16"))
    empty = VoxelNeighbors(torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
    xe = torch.zeros((0, 16), dtype=torch.bfloat16, device="cuda", requires_grad=True)
    we = torch.ones((27, 16, 32), dtype=torch.bfloat16, device="cuda", requires_grad=True)
    out = subm_conv3d(xe, empty, we)
    out.sum().backward()
    assert out.shape == (0, 32) and xe.grad.shape == (0, 16) and float(we.grad.float().abs().max()) == 0


def test_no_gathered_buffer():
    """forward and grad_features of the fused route allocate their results and nothing of the size of [V, K * C]"""
    name = "v4097-k27"
    ts, _ = as_kind(cases.randoms(name), "f32")
    fn, x, w = built(name), ts[0].requires_grad_(), ts[1]
    fn(x, w, method="fused").backward(ts[3])                         # (warm: the library is loaded)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(x, w, method="fused").backward(ts[3])
    torch.cuda.synchronize()
    fused = torch.cuda.max_memory_allocated() - base
    gathered = 4097 * 27 * 16 * 4
    print("peak above the inputs: fused %d bytes; one gathered buffer %d bytes" % (fused, gathered))
    assert fused < gathered / 4


def test_chain_down_and_up_again_bf16():
    """subm_conv3d -> sparse_conv3d (k3 s2 p1) -> subm_conv3d -> sparse_inverse_conv3d in bf16 against the fp64 model chain on the
    bf16 inputs.  A stage computes on what the stage before delivered (the model's value + the error so far): its own bound on
    those magnitudes, the error so far carried through |W|, and the rounding of its result to bf16"""
    from d3d_amd.voxel import SparseConvMap, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d
    import sparse_conv_reference as sref
    c, b = cases.SCENES["batches_negative"]
    oc, ob, t_out, t_in = scases.model("batches_negative", "k3s2p1")
    tab1, tab2 = vref.table(c, 3, 1, b), vref.table(oc, 3, 1, ob)
    r = np.random.default_rng(17)
    chans = (16, 32, 16, 16, 48)
    (xt, gt, *wts), (x, g, *ws) = as_kind([r.standard_normal((len(c), chans[0])), r.standard_normal((len(c), chans[4]))] +
                                          [r.standard_normal((27, chans[i], chans[i + 1])) / 8 for i in range(4)], "bf16")
    nb1, m = VoxelNeighbors(T(c), batch_index=T(b)), SparseConvMap(T(c), 3, 2, 1, batch_index=T(b))
    nb2 = VoxelNeighbors(m.out_coords, batch_index=m.out_batch)
    xt.requires_grad_()
    y = sparse_inverse_conv3d(subm_conv3d(sparse_conv3d(subm_conv3d(xt, nb1, wts[0]), m, wts[1]), nb2, wts[2]), m, wts[3])
    y.backward(gt)
    assert y.dtype == torch.bfloat16 and xt.grad.dtype == torch.bfloat16
    u = ref.U["bf16"]
    fwd = (tab1, t_out, tab2, t_in)
    bwd = (tab1[:, ::-1], t_in, tab2[:, ::-1], t_out)

    def walk(val, tabs, weights):
        err = np.zeros_like(val)
        for tab, wk in zip(tabs, weights):
            k, cin, _ = wk.shape
            aw = np.abs(wk)
            carried = sref.conv(err, tab, aw)
            own = ref.dot_bound(k * cin, sref.conv(np.abs(val) + err, tab, aw))
            val = sref.conv(val, tab, wk)
            err = (own + carried) * (1 + u) + u * np.abs(val)
        return val, err

    want, bound = walk(x, fwd, ws)
    err = np.abs(y.detach().double().cpu().numpy() - want)
    print("bf16 chain out: worst |err| / bound = %.4f" % np.max(err / bound))
    assert y.shape == (len(c), chans[4]) and np.all(err <= bound)
    want_g, bound_g = walk(g, bwd[::-1], [np.ascontiguousarray(wk.transpose(0, 2, 1)) for wk in ws[::-1]])
    err = np.abs(xt.grad.double().cpu().numpy() - want_g)
    print("bf16 chain grad: worst |err| / bound = %.4f" % np.max(err / bound_g))
    assert xt.grad.shape == x.shape and np.all(err <= bound_g)


@pytest.mark.parametrize("kind", KINDS)
def test_buffers_off_a_16_byte_boundary(kind):
    """the C ABI on feat, weight and grad_out that start one element past a 16-byte boundary: the element-wise loads give the bits
    of the 16-byte ones"""
    import ctypes
    from d3d_amd import _lib
    lib, name = _lib.load(), "negative_odd-down-k3s2"                # Cin = 48, Cout = 16: the padded MFMA depth too
    fwd, _, src_rows, rows = cases.tables(name)
    (x, w, bias, g), _ = as_kind(cases.randoms(name, seed=3), kind)
    k, cin, cout = w.shape
    table, code = torch.from_numpy(fwd.copy()).cuda(), {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}[kind]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def shifted(t):
        slab = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
        slab[1:] = t.reshape(-1)
        assert slab.data_ptr() % 16 == 0 and slab[1:].data_ptr() % 16 == t.element_size()
        return slab[1:]

    def both(xs, ws, gs):
        out, gw = torch.empty((rows, cout), dtype=x.dtype, device="cuda"), torch.empty_like(w)
        rc = lib.d3d_table_conv(_lib.ptr(xs), src_rows, cin, _lib.ptr(table), rows, k, 0, _lib.ptr(ws), _lib.ptr(bias), cout, code,
                                _lib.ptr(out), stream)
        assert rc == _lib.OK
        ws_bytes = lib.d3d_table_conv_wgrad_workspace_bytes(rows, k, cin, cout)
        scratch = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        rc = lib.d3d_table_conv_wgrad(_lib.ptr(xs), src_rows, cin, _lib.ptr(table), rows, k, 0, _lib.ptr(gs), cout, code, _lib.ptr(gw),
                                      _lib.ptr(scratch), ws_bytes, stream)
        assert rc == _lib.OK
        assert lib.d3d_table_conv_wgrad(_lib.ptr(xs), src_rows, cin, _lib.ptr(table), rows, k, 0, _lib.ptr(gs), cout, code, _lib.ptr(gw),
                                        _lib.ptr(scratch), ws_bytes - 1, stream) == _lib.ERR_WORKSPACE
        torch.cuda.synchronize()
        return out, gw

    aligned, off = both(x, w, g), both(shifted(x), shifted(w), shifted(g))
    assert ref.equal_bits(aligned[0], off[0]) and ref.equal_bits(aligned[1], off[1])
    assert float(aligned[0].float().abs().max()) > 0 and float(aligned[1].float().abs().max()) > 0
