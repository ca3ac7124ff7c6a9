"""GPU: VoxelInterp, voxel_interpolate, voxel_splat and the entries behind them (csrc/vnbr.hip's corner table, csrc/vinterp.hip)
against the numpy model of voxel_interp_reference.py.  Every comparison is bit for bit (a NaN equal to any NaN)."""
import functools

import numpy as np
import pytest
import torch

import voxel_interp_cases as cases
import voxel_interp_reference as ref

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f64": torch.float64}


def T(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared scenes are read-only)


def build(name, dtype, mode="linear", normalize=False, perm=None):
    from d3d_amd.voxel import VoxelInterp
    c, b, _, pb = cases.scene(name)
    p = cases.positions(name, dtype)
    if perm is not None:
        p, pb = p[perm], (None if pb is None else pb[perm])
    return VoxelInterp(T(c), T(p), T(b), T(pb), mode=mode, normalize=normalize)


@functools.lru_cache(maxsize=None)
def owner(name, dtype, mode="linear", normalize=False):
    return build(name, dtype, mode, normalize)


def same_bytes(t, a):
    """a device tensor against a numpy array: shape, dtype and bytes"""
    got = t.cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("name", cases.SCENES)
def test_table_and_weights_are_the_model(name, dtype):
    for mode in ref.MODES:
        for normalize in (False, True):
            itp = build(name, dtype, mode, normalize)
            t, w = cases.table(name, dtype, mode, normalize)
            what = (mode, normalize)
            assert itp.table.is_cuda and itp.weights.dtype == TORCH[dtype] and itp.num_corners == ref.MODES[mode], what
            assert (itp.num_points, itp.num_voxels, itp.num_entries) == (len(t), len(cases.scene(name)[0]), int((t >= 0).sum())), what
            assert same_bytes(itp.table, t), what
            assert same_bytes(itp.weights, w), what


def run(fn, x, itp, g):
    """tensors of one dtype -> (out, grad) of voxel_interpolate or voxel_splat"""
    x = x.detach().clone().requires_grad_()
    out = fn(x, itp)
    out.backward(g)
    return out.detach(), x.grad


def check(name, dtype, kind, c, values=cases.randoms, mode="linear", normalize=False, seed=0):
    """both operators, forward and gradient, on scene `name` against the model"""
    from d3d_amd.voxel import voxel_interpolate, voxel_splat
    itp = owner(name, dtype, mode, normalize)
    t, w = cases.table(name, dtype, mode, normalize)
    k, v = len(t), itp.num_voxels
    (vt, vx), (pt, px) = (ref.of_kind(values(n, c, seed + i), kind) for i, n in enumerate((v, k)))
    out, gv = run(voxel_interpolate, vt.cuda(), itp, pt.cuda())
    assert out.is_cuda and gv.is_cuda
    assert ref.equal_bits(out, ref.to_tensor(ref.forward(vx, t, w, kind), kind)), "interpolate"
    assert ref.equal_bits(gv, ref.to_tensor(ref.transpose(px, t, w, v, kind), kind)), "interpolate: gradient"
    out, gp = run(voxel_splat, pt.cuda(), itp, vt.cuda())
    assert ref.equal_bits(out, ref.to_tensor(ref.transpose(px, t, w, v, kind), kind)), "splat"
    assert ref.equal_bits(gp, ref.to_tensor(ref.forward(vx, t, w, kind), kind)), "splat: gradient"
    return vx, px, t, w


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_operators_follow_the_models_fold_order(name, kind):
    """random data, 12 channels: the vector path of fp32 and fp64, the scalar path of the half types.  fp64 positions under the other
    three kinds: the weights are cast once"""
    check(name, "f32", kind, 12)
    check(name, "f64", kind, 12, normalize=True, seed=2)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_integer_features_at_quarter_steps_are_exact(kind):
    """weights that are multiples of 1 / 64 and integers in -8 .. 8: every product and partial sum is exact, so the result is the exact
    value rounded once to nearest even -- computed here in fp64 with numpy's own dot products, not by the model's fold"""
    vx, px, t, w = check("quarters", "f32", kind, 16, values=cases.small_integers)
    k, v = len(t), len(vx)
    m = np.zeros((k, v))
    np.add.at(m, (np.nonzero(t >= 0)[0], t[t >= 0]), w[t >= 0].astype(np.float64))
    assert set(np.unique(m * 64) % 1) == {0.0}
    from d3d_amd.voxel import voxel_interpolate, voxel_splat
    itp = owner("quarters", "f32")
    vt, pt = (torch.from_numpy(a).to(ref.pref.TORCH[kind]).cuda() for a in (vx, px))
    assert ref.equal_bits(voxel_interpolate(vt, itp), ref.to_tensor(m @ vx.astype(np.float64), kind))
    assert ref.equal_bits(voxel_splat(pt, itp), ref.to_tensor(m.T @ px.astype(np.float64), kind))


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("c", cases.CHANNELS)
def test_channel_counts(c, kind):
    check("random", "f32", kind, c, seed=c)
    check("crowded", "f32", kind, c, seed=c + 1)
    check("random", "f32", kind, c, mode="nearest", seed=c + 2)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_misaligned_rows_give_the_same_bits(kind):
    """features and gradient one element past a 16-byte boundary take the scalar path: the bits of the aligned call"""
    from d3d_amd.voxel import voxel_interpolate, voxel_splat
    itp = owner("crowded", "f32")
    (vt, _), (pt, _) = (ref.of_kind(cases.randoms(n, 16, 3 + i), kind) for i, n in enumerate((itp.num_voxels, itp.num_points)))

    def shifted(t):
        s = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
        s.copy_(t)
        assert s.is_contiguous() and s.data_ptr() % 16 == t.element_size()
        return s
    for fn, x, g in ((voxel_interpolate, vt, pt), (voxel_splat, pt, vt)):
        a, ga = run(fn, x.cuda(), itp, g.cuda())
        b, gb = run(fn, shifted(x), itp, shifted(g))
        assert ref.equal_bits(a, b) and ref.equal_bits(ga, gb), fn.__name__


@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_permuted_points_and_two_runs(kind):
    """Permuting the points permutes the interpolated rows.  The splat folds a voxel's entries in ascending entry number of the PERMUTED
    table, so its bits may move with the order of the points: what holds is that it is the model's fold on the permuted input -- and
    that two runs of anything give the same bits"""
    from d3d_amd.voxel import voxel_interpolate, voxel_splat
    name, c = "crowded", 20
    itp = owner(name, "f32")
    perm = np.random.default_rng(4).permutation(itp.num_points)
    other = build(name, "f32", perm=perm)
    t, w = cases.table(name, "f32")
    assert same_bytes(other.table, t[perm]) and same_bytes(other.weights, w[perm])
    (vt, _), (pt, px) = (ref.of_kind(cases.randoms(n, c, 5 + i), kind) for i, n in enumerate((itp.num_voxels, itp.num_points)))
    a = voxel_interpolate(vt.cuda(), itp)
    assert ref.equal_bits(a[torch.from_numpy(perm).cuda()], voxel_interpolate(vt.cuda(), other))
    s = voxel_splat(pt[perm].cuda(), other)
    assert ref.equal_bits(s, ref.to_tensor(ref.transpose(px[perm], t[perm], w[perm], itp.num_voxels, kind), kind))
    assert ref.equal_bits(a, voxel_interpolate(vt.cuda(), itp)) and ref.equal_bits(s, voxel_splat(pt[perm].cuda(), other))
    again = build(name, "f32")
    assert torch.equal(again.table, itp.table) and torch.equal(again.weights, itp.weights)
    assert torch.equal(again.transpose().order, itp.transpose().order) and itp.transpose() is itp.transpose()
    assert itp.transpose().mapping is None and itp.transpose().num_mapped == itp.num_entries       # (no widened copy of the table is kept)


def test_output_past_2_31_elements():
    """K = 2^24 + 3 points, C = 128 in fp16: out has 2^31 + 384 elements.  65 voxels named again and again; the model on a seeded sample
    of rows, the rows around element 2^31 (the very last ones) among them"""
    from d3d_amd.voxel import VoxelInterp, voxel_interpolate
    c, k = 128, 2 ** 24 + 3
    assert k * c > 2 ** 31 and (k - 4) * c < 2 ** 31
    coords = cases.scene("random")[0]
    gen = torch.Generator(device="cuda").manual_seed(6)
    lo = torch.tensor([-1.0, -1.0, -1.0], device="cuda")
    pos = torch.rand((k, 3), device="cuda", generator=gen) * torch.tensor([b + 1.0 for b in cases.BOX], device="cuda") + lo
    itp = VoxelInterp(T(coords), pos)
    ft, fx = ref.of_kind(cases.randoms(len(coords), c, 7), "f16")
    out = voxel_interpolate(ft.cuda(), itp)
    assert out.shape == (k, c) and out.numel() > 2 ** 31
    rows = np.concatenate([np.random.default_rng(8).integers(0, k, 500), np.arange(k - 8, k), np.arange(8)])
    at = torch.from_numpy(rows).cuda()
    t, w = ref.corners(coords, pos[at].cpu().numpy())
    assert same_bytes(itp.table[at], t) and same_bytes(itp.weights[at], w) and (t >= 0).sum() > 500
    assert ref.equal_bits(out[at], ref.to_tensor(ref.forward(fx, t, w, "f16"), "f16"))


@pytest.mark.parametrize("fn", ("voxel_interpolate", "voxel_splat"))
def test_gradcheck(fn):
    import d3d_amd.voxel as voxel
    itp = owner("random", "f64")
    rows = itp.num_voxels if fn == "voxel_interpolate" else itp.num_points
    x = torch.from_numpy(cases.randoms(rows, 3, 9)).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: getattr(voxel, fn)(t, itp), (x,), eps=1e-6, atol=1e-7, rtol=1e-7, nondet_tol=0.0)


def test_numpy_host_tensors_and_nothing_to_do():
    from d3d_amd.voxel import VoxelInterp, voxel_interpolate, voxel_splat
    name = "random"
    c, p = np.array(cases.scene(name)[0]), cases.positions(name, "f32")    # (copies: the shared scene is read-only)
    t, w = cases.table(name, "f32")
    itp = VoxelInterp(c, p)                                                  # numpy in: built on the current device
    assert itp.table.is_cuda and same_bytes(itp.table, t) and same_bytes(itp.weights, w)
    (vt, vx), (pt, px) = (ref.of_kind(cases.randoms(n, 5, 10 + i), "f32") for i, n in enumerate((len(c), len(p))))
    want, want_t = ref.to_tensor(ref.forward(vx, t, w, "f32"), "f32"), ref.to_tensor(ref.transpose(px, t, w, len(c), "f32"), "f32")
    got = voxel_interpolate(vt.numpy(), itp)
    assert isinstance(got, np.ndarray) and ref.equal_bits(torch.from_numpy(got), want)
    out, g = run(voxel_interpolate, vt, itp, pt)
    assert not out.is_cuda and not g.is_cuda and ref.equal_bits(out, want) and ref.equal_bits(g, want_t)
    assert ref.equal_bits(voxel_splat(pt, itp), want_t)
    import copy
    other = copy.copy(itp)
    other.device = torch.device("cuda", itp.device.index + 1)
    with pytest.raises(ValueError, match="live on"):
        voxel_interpolate(vt.cuda(), other)
    # duplicates and a span overflow that only the device can see
    with pytest.raises(ValueError, match="already has"):
        VoxelInterp(T(np.concatenate([c, c[:2]])), T(p))
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelInterp(T(np.array([[0, 0, 0], [2 ** 31, 2 ** 31, 2 ** 31]], np.int64)), T(p))
    # no points, no voxels, no channels
    for empty in ("no_points", "no_voxels"):
        e = owner(empty, "f32")
        x = torch.zeros((e.num_voxels, 4), device="cuda", requires_grad=True)
        y = voxel_interpolate(x, e)
        y.sum().backward()
        assert y.shape == (e.num_points, 4) and not y.any() and x.grad.shape == x.shape and not x.grad.any()
        assert voxel_splat(torch.ones((e.num_points, 4), device="cuda"), e).shape == (e.num_voxels, 4)
    assert voxel_interpolate(torch.zeros((len(c), 0), device="cuda"), itp).shape == (len(p), 0)


def test_chain_pool_conv_interpolate_reaches_the_point_features():
    """voxel_pool -> subm_conv3d (bf16, fused) -> voxel_interpolate at the original points: runs, and the gradient reaches the point
    features"""
    from d3d_amd.voxel import VoxelIndex, VoxelInterp, VoxelNeighbors, subm_conv3d, voxel_interpolate, voxel_pool
    r = np.random.default_rng(11)
    pts = r.uniform(0, 6, (400, 3))
    cell = np.floor(pts).astype(np.int64)
    coords, mapping = np.unique(cell, axis=0, return_inverse=True)
    gen = torch.Generator().manual_seed(12)
    pf = (torch.randn((400, 16), generator=gen) / 4).cuda().requires_grad_()
    w = (torch.randn((27, 16, 32), generator=gen) / 8).bfloat16().cuda().requires_grad_()
    vf = voxel_pool(pf, VoxelIndex(T(mapping.reshape(-1)), len(coords)), reduction="mean")
    y = subm_conv3d(vf.bfloat16(), VoxelNeighbors(T(coords)), w, method="fused")
    itp = VoxelInterp(T(coords), T((pts - 0.5).astype(np.float32)))
    out = voxel_interpolate(y, itp)
    assert out.shape == (400, 32) and out.dtype == torch.bfloat16 and itp.num_entries > 400
    out.backward(torch.ones_like(out))
    for t in (pf, w):
        assert t.grad is not None and bool(torch.isfinite(t.grad.float()).all()) and bool(t.grad.any())
    assert bool(pf.grad.any(1).all())                                        # every point's voxel feeds some interpolated row
    t, wts = ref.corners(coords, (pts - 0.5).astype(np.float32))
    want = ref.forward(y.detach().float().cpu().numpy(), t, wts, "bf16")
    assert ref.equal_bits(out.detach(), ref.to_tensor(want, "bf16"))
