"""GPU: FrustumMap, lift_splat, lift_splat_bev and the entries behind them (csrc/vlift.hip) against the numpy model of
lift_reference.py on the scenes of lift_cases.py.  The map, the forward and grad_feat are compared bit for bit (a NaN equal to any NaN);
grad_depth, whose summation order is the kernel's own, against a bound."""
import functools

import numpy as np
import pytest
import torch

import lift_cases as cases
import lift_reference as ref

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 4, 8, 20, 64, 260)
U_ACC = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "f16": 2.0 ** -24, "bf16": 2.0 ** -24}       # the accumulation type's unit roundoff
U_OUT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}        # one rounding of the output dtype ...
TINY = {"f32": 2.0 ** -150, "f64": 0.0, "f16": 2.0 ** -25, "bf16": 2.0 ** -134}            # ... where it is subnormal: half a step


def build(name, perm=None):
    from d3d_amd.voxel import FrustumMap
    sc = cases.scene(name)
    pre, post = (sc["pre"], sc["post"]) if perm is None else (sc["pre"][perm], sc["post"][perm])
    us, vs, ds, pre, post = (np.array(a) for a in (sc["us"], sc["vs"], sc["ds"], pre, post))      # (copies: the shared scenes are read-only)
    return FrustumMap(us, vs, ds, pre, post, sc["bounds"], sc["shape"], sc["cams"])


@functools.lru_cache(maxsize=None)
def owner(name):
    return build(name)


def same(t, a):
    got = t.cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and np.array_equal(got, a)


def misaligned(t):
    """the same values 'contiguous' at an address that is no multiple of 16"""
    buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def data(name, c, kind, values=cases.randoms, seed=0):
    """-> ((depth, feat, grad) tensors of `kind` on the host, the same in the fold type as numpy)"""
    s, _, k = cases.sizes(name)
    d, h, w = cases.frustum(name)
    v = cases.model(name)["V"]
    pairs = [ref.of_kind(values(shape, seed + i), kind) for i, shape in enumerate(((s, d, h, w), (s, h, w, c), (v, c)))]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def depth_bound(exact, scale, c, kind):
    first = (c + 1) * U_ACC[kind] * scale.astype(np.float64)
    return first + U_OUT[kind] * (np.abs(exact.astype(np.float64)) + first) + TINY[kind]


def check(name, kind, c, values=cases.randoms, seed=0, paths=False):
    """forward and both gradients on scene `name` through autograd against the model; paths: the three entries again on misaligned
    views (the element-by-element path), the same bits"""
    from d3d_amd.voxel import lift, lift_splat
    fmap, m, fr = owner(name), cases.model(name), cases.frustum(name)
    s = cases.sizes(name)[0]
    (dt, ft, gt), (dx, fx, gx) = data(name, c, kind, values, seed)
    depth, feat = dt.cuda().requires_grad_(), ft.cuda().requires_grad_()
    out = lift_splat(depth, feat, fmap)
    out.backward(gt.cuda())
    assert out.is_cuda and out.shape == (m["V"], c) and depth.grad.shape == depth.shape and feat.grad.shape == feat.shape
    want = ref.to_tensor(ref.forward(dx.reshape(-1), fx.reshape(-1, c), m["mapping"], m["V"], fr, kind), kind)
    assert ref.equal_bits(out.detach(), want), ("forward", name, kind, c)
    want_gf = ref.to_tensor(ref.backward_feat(gx, dx.reshape(-1), m["mapping"], s, fr, kind), kind).reshape(ft.shape)
    assert ref.equal_bits(feat.grad, want_gf), ("grad_feat", name, kind, c)
    exact, scale = ref.backward_depth_exact(gx, fx.reshape(-1, c), m["mapping"], fr)
    bound = depth_bound(exact, scale, c, kind)

    def depth_check(t, what):
        got = t.detach().cpu().to(torch.float64).numpy().reshape(-1)
        err = np.abs(got.astype(ref.EXACT) - exact).astype(np.float64)     # (the difference itself in long double: fp64 results too)
        worst = int(np.argmax(err / np.maximum(bound, 2.0 ** -1000)))
        print("%s %s %s c=%d: error %.3e at a bound of %.3e where the two are closest" % (what, name, kind, c, err[worst], bound[worst]))
        assert np.all(err <= bound), (what, name, kind, c, err[worst], bound[worst])
        assert np.all(got[m["mapping"] < 0] == 0), what
    depth_check(depth.grad, "grad_depth")
    if paths and m["V"]:
        d1, f1, g1 = misaligned(depth.detach()), misaligned(feat.detach()), misaligned(gt.cuda())
        assert ref.equal_bits(lift._forward(d1, f1, fmap), out.detach()), ("forward, misaligned", name, kind, c)
        assert ref.equal_bits(lift._backward_feat(g1, d1, fmap), feat.grad), ("grad_feat, misaligned", name, kind, c)
        depth_check(lift._backward_depth(g1, f1, fmap), "grad_depth, misaligned")
    return out.detach(), depth.grad, feat.grad


@pytest.mark.parametrize("name", cases.SCENES)
def test_map_is_the_model(name):
    fmap, m, sc = build(name), cases.model(name), cases.scene(name)
    s, b, k = cases.sizes(name)
    assert (fmap.num_voxels, fmap.num_points, fmap.num_members) == (m["V"], k, int(m["member"].sum()))
    assert (fmap.num_cameras, fmap.batch_size, fmap.cams_per_sample, fmap.frustum, fmap.shape) == (s, b, sc["cams"], cases.frustum(name), sc["shape"])
    assert fmap.mapping.is_cuda and same(fmap.mapping, m["mapping"])
    assert same(fmap.coords, m["coords"]) and same(fmap.batch_index, m["batch_index"])
    idx = fmap.index
    assert idx.mapping is fmap.mapping and idx.num_voxels == m["V"] and idx.num_mapped == int(m["member"].sum())
    order = np.nonzero(m["member"])[0]
    order = order[np.argsort(m["mapping"][order], kind="stable")]
    assert same(idx.order, order.astype(np.int32))
    assert same(idx.offsets, np.concatenate([[0], np.cumsum(np.bincount(m["mapping"][m["member"]], minlength=m["V"]))]).astype(np.int64))
    dmap = fmap.dense_map()
    assert dmap is fmap.dense_map() and dmap.batch_size == b and dmap.dense_shape == sc["shape"][::-1] and dmap.num_voxels == m["V"]


def test_map_takes_tensors_from_either_side():
    sc, m = cases.scene("ring_3x5"), cases.model("ring_3x5")
    from d3d_amd.voxel import FrustumMap
    dev = [torch.from_numpy(np.array(sc[key])).cuda() for key in ("us", "vs", "ds", "pre", "post")]
    host = [torch.from_numpy(np.array(sc[key])).double() for key in ("us", "vs", "ds", "pre", "post")]     # (fp32 values in fp64: cast back)
    for args in (dev, host):
        fmap = FrustumMap(*args, np.array(sc["bounds"]), list(sc["shape"]), sc["cams"])
        assert same(fmap.mapping, m["mapping"]) and same(fmap.coords, m["coords"])


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_operator_follows_the_models_fold_order(name, kind):
    """random data; 20 channels: the vector path of fp32 and fp64, the element path of the half types; 8: the vector path of all four"""
    check(name, kind, 20)
    check(name, kind, 8, seed=3)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", ("int_3x5", "spoiled_4x16"))
def test_every_channel_count_on_both_paths(name, kind):
    for c in CHANNELS:
        check(name, kind, c, seed=c, paths=True)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", cases.INTEGER)
def test_integer_data_gives_rne_of_the_exact_value(name, kind):
    """integers in [-4, 4]: every product and every partial sum (at most 16 x 2125) is exact in fp32, so the result is the exact value
    rounded once to the dtype -- taken here from the fp64 model, in which the same sums are exact as well"""
    c = 12
    out, _, gf = check(name, kind, c, values=cases.integers, seed=1)
    m, fr = cases.model(name), cases.frustum(name)
    _, (dx, fx, gx) = data(name, c, kind, cases.integers, 1)
    exact = ref.forward(dx.reshape(-1).astype(np.float64), fx.reshape(-1, c).astype(np.float64), m["mapping"], m["V"], fr, "f64")
    assert ref.equal_bits(out, ref.to_tensor(exact, kind))
    exact = ref.backward_feat(gx.astype(np.float64), dx.reshape(-1).astype(np.float64), m["mapping"], cases.sizes(name)[0], fr, "f64")
    assert ref.equal_bits(gf, ref.to_tensor(exact, kind).reshape(gf.shape))


@pytest.mark.parametrize("kind", ("f32", "f64"))
@pytest.mark.parametrize("name", ("ring_3x5", "spoiled_4x16", "crowded", "empty"))
def test_forward_is_voxel_pool_of_the_materialised_product(name, kind):
    from d3d_amd.voxel import lift_splat, voxel_pool
    fmap = owner(name)
    s, _, k = cases.sizes(name)
    d, h, w = cases.frustum(name)
    for c in (4, 7):
        (dt, ft, _), _ = data(name, c, kind, seed=c)
        depth, feat = dt.cuda(), ft.cuda()
        product = depth.reshape(-1, 1) * feat[:, None].expand(s, d, h, w, c).reshape(k, c)
        assert ref.equal_bits(lift_splat(depth, feat, fmap), voxel_pool(product, fmap.index, reduction="sum"))


def test_gradcheck_in_both_inputs():
    from d3d_amd.voxel import lift_splat
    fmap = owner("ring_3x5")
    (dt, ft, _), _ = data("ring_3x5", 2, "f64", seed=4)
    depth, feat = dt.cuda().requires_grad_(), ft.cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: lift_splat(a, b, fmap), (depth, feat), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


def test_each_gradient_is_computed_only_when_needed(monkeypatch):
    from d3d_amd.voxel import lift, lift_splat
    fmap = owner("int_3x5")
    (dt, ft, gt), _ = data("int_3x5", 4, "f32")
    calls = []
    for fn in ("_backward_feat", "_backward_depth"):
        monkeypatch.setattr(lift, fn, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(lift, fn), fn))
    for need_depth, need_feat in ((True, False), (False, True), (True, True)):
        del calls[:]
        depth, feat = dt.cuda().requires_grad_(need_depth), ft.cuda().requires_grad_(need_feat)
        lift_splat(depth, feat, fmap).backward(gt.cuda())
        assert sorted(calls) == sorted(n for n, need in (("_backward_depth", need_depth), ("_backward_feat", need_feat)) if need)
        assert (depth.grad is not None) == need_depth and (feat.grad is not None) == need_feat
    assert not lift_splat(dt.cuda(), ft.cuda(), fmap).requires_grad


def test_permuting_cameras_with_their_matrices_keeps_every_cells_members():
    """cameras swapped inside their samples: the cells and their numbering stay, every point keeps its row, and on data where fp32 is
    exact (multiples of 1/8) the outputs are the same bits although the fold order changed"""
    from d3d_amd.voxel import lift_splat
    name, perm = "ring_3x5", np.array([1, 0, 3, 2])
    a, b = owner(name), build(name, perm)
    s = cases.sizes(name)[0]
    assert torch.equal(a.coords, b.coords) and torch.equal(a.batch_index, b.batch_index)
    assert torch.equal(b.mapping.view(s, -1), a.mapping.view(s, -1)[torch.from_numpy(perm).cuda()])
    (dt, ft, gt), _ = data(name, 8, "f32", cases.dyadic)
    outs = []
    for fmap, order in ((a, np.arange(s)), (b, perm)):
        depth, feat = dt[order].cuda().requires_grad_(), ft[order].cuda().requires_grad_()
        out = lift_splat(depth, feat, fmap)
        out.backward(gt.cuda())
        inverse = np.argsort(order)
        outs.append((out.detach(), depth.grad[inverse], feat.grad[inverse]))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_two_runs_give_the_same_bits():
    runs = [check("crowded", kind, 20, seed=7) for kind in ("f32", "bf16") for _ in range(2)]
    for first, second in (runs[:2], runs[2:]):
        assert all(ref.equal_bits(x, y) for x, y in zip(first, second))
    assert same(build("spoiled_4x16").mapping, owner("spoiled_4x16").mapping.cpu().numpy())


def test_five_dimensional_inputs_host_inputs_and_numpy():
    from d3d_amd.voxel import lift_splat
    name = "int_4x16"
    fmap = owner(name)
    s, b, _ = cases.sizes(name)
    (dt, ft, _), _ = data(name, 4, "f32")
    want = lift_splat(dt.cuda(), ft.cuda(), fmap)
    assert torch.equal(lift_splat(dt.cuda().unflatten(0, (b, s // b)), ft.cuda().unflatten(0, (b, s // b)), fmap), want)
    host = lift_splat(dt, ft, fmap)
    assert not host.is_cuda and torch.equal(host, want.cpu())
    got = lift_splat(dt.numpy(), ft.numpy(), fmap)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy())
    for bad in ((dt.cuda()[:, :-1], ft.cuda()), (dt.cuda(), ft.cuda()[:, :-1]), (dt.cuda().double(), ft.cuda()), (dt, ft.cuda()),
                (dt.cuda().int(), ft.cuda().int())):
        with pytest.raises(ValueError):
            lift_splat(bad[0], bad[1], fmap)


@pytest.mark.parametrize("name", ("int_4x16", "ring_3x5", "empty"))
def test_bev_is_the_rows_scattered_by_index_put(name):
    from d3d_amd.voxel import lift_splat, lift_splat_bev
    fmap, sc = owner(name), cases.scene(name)
    b = cases.sizes(name)[1]
    n0, n1, n2 = sc["shape"]
    for kind, c in (("f32", 5), ("bf16", 8)):
        (dt, ft, _), _ = data(name, c, kind, seed=2)
        rows = lift_splat(dt.cuda(), ft.cuda(), fmap)
        bev = lift_splat_bev(dt.cuda(), ft.cuda(), fmap)
        x, y, z = fmap.coords.unbind(1)
        grid = rows.new_zeros((b, n2, n1, n0, c)).index_put((fmap.batch_index, z, y, x), rows)
        assert bev.shape == (b, c * n2, n1, n0) and ref.equal_bits(bev, grid.permute(0, 4, 1, 2, 3).reshape(b, c * n2, n1, n0))


def test_forward_never_holds_the_product():
    """K C 4 = 32 MiB: the peak over the forward stays below inputs + outputs + 8 MiB (the inputs and the map are allocated before the
    window opens, so the window may grow by the output and the allowance)"""
    from d3d_amd.voxel import FrustumMap, lift_splat, voxel_pool
    s, d, h, w, c = 2, 32, 32, 64, 64
    assert s * d * h * w * c * 4 == 32 << 20
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    us, vs, ds = np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32), (1 + np.arange(d) / 8).astype(np.float32)
    fmap = FrustumMap(us, vs, ds, np.stack([eye, eye]), np.stack([eye, eye]), (0, 256, 0, 128, 0, 8), (64, 64, 1), 1)
    assert fmap.num_members > s * d * h * w // 2 and fmap.num_voxels > 2000
    gen = torch.Generator().manual_seed(0)
    depth, feat = torch.rand((s, d, h, w), generator=gen).cuda(), torch.randn((s, h, w, c), generator=gen).cuda()
    lift_splat(depth, feat, fmap)                                         # (the library and the allocator are warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = lift_splat(depth, feat, fmap)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out_bytes = out.numel() * 4
    print("forward: peak %d bytes over the inputs, the output is %d" % (peak, out_bytes))
    assert peak <= out_bytes + (8 << 20)
    product = depth.reshape(-1, 1) * feat[:, None].expand(s, d, h, w, c).reshape(-1, c)
    assert torch.equal(out, voxel_pool(product, fmap.index, reduction="sum"))
