"""CPU: the numpy model of the frustum map and the lift-splat folds (lift_reference.py) against exact arithmetic, a brute-force loop and
LSS's own formulation in torch; frustum_matrices against LSS's step-by-step geometry; every refusal of the C entries and of the Python
layer, none of which needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import lift_cases as cases
import lift_reference as ref

_BAD, _UNSUP, _WS = -1, -2, -3


# ---------------------------------------------------------------- the geometry model
@pytest.mark.parametrize("name", cases.INTEGER)
def test_geometry_model_is_exact_arithmetic_on_integer_scenes(name):
    """Python Fractions, point by point: membership and cells equal for EVERY point of the scene"""
    sc, m = cases.scene(name), cases.model(name)
    member, cell = ref.cells_exact(sc["us"], sc["vs"], sc["ds"], sc["pre"], sc["post"], m["lo"], m["size"], sc["shape"], sc["cams"])
    assert len(member) == cases.sizes(name)[2]
    assert np.array_equal(member, m["member"])
    assert np.array_equal(cell, m["cell"])


def test_band_below_zero_is_outside_where_truncation_would_keep_it():
    m = cases.model("int_3x5")
    t = m["t"].astype(np.float64)
    band = np.any((t > -1) & (t < 0), 1)
    truncated_in = np.all((np.trunc(t) >= 0) & (np.trunc(t) < np.array(cases.scene("int_3x5")["shape"])), 1)
    assert np.any(band & truncated_in) and not np.any(band & m["member"])


@pytest.mark.parametrize("name", cases.SCENES)
def test_rows_are_numbered_by_ascending_sample_and_coordinate(name):
    sc, m = cases.scene(name), cases.model(name)
    n = sc["shape"]
    key = ((m["batch_index"] * n[0] + m["coords"][:, 0]) * n[1] + m["coords"][:, 1]) * n[2] + m["coords"][:, 2]
    assert np.all(np.diff(key) > 0)                                       # ascending, no cell twice
    assert m["coords"].shape == (m["V"], 3) and np.all(m["coords"] >= 0) and np.all(m["coords"] < np.array(n))
    assert np.all((m["batch_index"] >= 0) & (m["batch_index"] < cases.sizes(name)[1]))
    inside = m["mapping"] >= 0
    assert np.array_equal(inside, m["member"]) and np.array_equal(np.unique(m["mapping"][inside]), np.arange(m["V"]))
    assert np.array_equal(m["coords"][m["mapping"][inside]], m["cell"][inside, 1:])
    assert np.array_equal(m["batch_index"][m["mapping"][inside]], m["cell"][inside, 0])


# ---------------------------------------------------------------- the fold models
def _data(name, c, kind, values, seed=0):
    s, _, k = cases.sizes(name)
    d, h, w = cases.frustum(name)
    (_, depth), (_, feat) = (ref.of_kind(values(shape, seed + i), kind) for i, shape in enumerate(((k,), (s * h * w, c))))
    return depth, feat


@pytest.mark.parametrize("kind", ("f32", "f64"))
@pytest.mark.parametrize("name", ("int_3x5", "ring_3x5", "one_bin", "crowded"))
def test_forward_model_is_the_dictionary_loop(name, kind):
    m = cases.model(name)
    depth, feat = _data(name, 3, kind, cases.randoms)
    got = ref.forward(depth, feat, m["mapping"], m["V"], cases.frustum(name), kind)
    want = ref.forward_brute(depth, feat, m["cell"], m["member"], cases.frustum(name))
    assert len(want) == m["V"]
    for r in range(m["V"]):
        row = want[(int(m["batch_index"][r]),) + tuple(int(a) for a in m["coords"][r])]
        assert np.array_equal(np.array(row, got.dtype), got[r]), r


def _lss(name, depth, feat, grad):
    """LSS's voxel pooling in torch fp64: index_add_ of depth[..., None] * feat over the kept points, and its autograd"""
    m = cases.model(name)
    s, _, k = cases.sizes(name)
    d, h, w = cases.frustum(name)
    dt = torch.from_numpy(depth.astype(np.float64)).reshape(s, d, h, w).requires_grad_()
    ft = torch.from_numpy(feat.astype(np.float64)).reshape(s, h, w, -1).requires_grad_()
    prod = (dt[..., None] * ft[:, None]).reshape(k, -1)
    kept = torch.from_numpy(m["mapping"] >= 0)
    rows = torch.from_numpy(np.array(m["mapping"]))                      # (a copy: the shared model is read-only)
    out = torch.zeros((m["V"], feat.shape[1]), dtype=torch.float64).index_add_(0, rows[kept], prod[kept])
    out.backward(torch.from_numpy(grad.astype(np.float64)))
    return out.detach().numpy(), dt.grad.reshape(-1).numpy(), ft.grad.reshape(s * h * w, -1).numpy()


@pytest.mark.parametrize("name", [n for n in cases.SCENES if n != "empty"])
def test_fold_models_equal_lss_in_fp64_on_dyadic_data(name):
    """multiples of 1/8: every product and sum is exact in fp32, so the fp32 models must EQUAL torch's fp64 result and gradients"""
    m = cases.model(name)
    s = cases.sizes(name)[0]
    depth, feat = _data(name, 5, "f32", cases.dyadic)
    grad = ref.of_kind(cases.dyadic((m["V"], 5), 9), "f32")[1]
    out, gd, gf = _lss(name, depth, feat, grad)
    assert np.array_equal(ref.forward(depth, feat, m["mapping"], m["V"], cases.frustum(name), "f32").astype(np.float64), out)
    assert np.array_equal(ref.backward_feat(grad, depth, m["mapping"], s, cases.frustum(name), "f32").astype(np.float64), gf)
    exact, scale = ref.backward_depth_exact(grad, feat, m["mapping"], cases.frustum(name))
    assert np.array_equal(exact.astype(np.float64), gd) and np.all(scale >= np.abs(exact))


# ---------------------------------------------------------------- frustum_matrices
def test_frustum_matrices_follow_lss_get_geometry():
    """(pre, post) applied in fp64 against LSS's get_geometry step by step in fp64 (BEVFusion's extra rotation and translation last).
    The only error is the ONE rounding of the 24 matrix entries to fp32, relative u = 2^-24 each:
      |dq_i| <= u Q_i,            Q_i = sum_j |pre_ij| |a_j|               (a = (u, v, d, 1))
      |de_0| <= |q0| dq2 + |q2| dq0 + dq0 dq2,  likewise e_1;  de_2 = dq2
      |dx_i| <= sum_j |post_ij| (1 + u) de_j + u sum_j |post_ij| |e_j|      (e_3 = 1, de_3 = 0)
    What fp64 itself contributes (two association orders of well-conditioned 3 x 3 products: some tens of 2^-53 of the same sums) is
    below 2^-20 of that bound; the factor 1 + 2^-8 covers it."""
    from d3d_amd.voxel import frustum_matrices
    rng = np.random.default_rng(5)
    b, n = 2, 3

    def rot(scale=1.0):
        q, _ = np.linalg.qr(rng.standard_normal((b, n, 3, 3)))
        return q * scale
    rots, trans = rot(), rng.uniform(-2, 2, (b, n, 3))
    intrins = np.zeros((b, n, 3, 3))
    intrins[..., 0, 0], intrins[..., 1, 1], intrins[..., 2, 2] = rng.uniform(200, 300, (b, n)), rng.uniform(200, 300, (b, n)), 1
    intrins[..., 0, 2], intrins[..., 1, 2] = 176, 64
    post_rots = rot(0.5)
    post_rots[..., 2, :], post_rots[..., :, 2] = 0, 0
    post_rots[..., 2, 2] = 1
    post_rots[..., :2, :2] = np.array([[0.48, -0.02], [0.02, 0.48]])
    post_trans = np.concatenate([rng.uniform(-20, 20, (b, n, 2)), np.zeros((b, n, 1))], -1)
    extra_rots = np.linalg.qr(rng.standard_normal((b, 3, 3)))[0]
    extra_trans = rng.uniform(-1, 1, (b, 3))
    pre, post = frustum_matrices(rots, trans, intrins, post_rots, post_trans, extra_rots, extra_trans)
    assert isinstance(pre, np.ndarray) and pre.shape == post.shape == (b * n, 3, 4) and pre.dtype == post.dtype == np.float32
    tp, tq = frustum_matrices(*(torch.from_numpy(a) for a in (rots, trans, intrins, post_rots, post_trans, extra_rots, extra_trans)))
    assert torch.is_tensor(tp) and np.array_equal(tp.numpy(), pre) and np.array_equal(tq.numpy(), post)
    plain = frustum_matrices(rots, trans, intrins, post_rots, post_trans)
    eye = frustum_matrices(rots, trans, intrins, post_rots, post_trans, np.broadcast_to(np.eye(3), (b, n, 3, 3)).copy(), np.zeros((b, n, 3)))
    assert np.array_equal(plain[0], eye[0]) and np.array_equal(plain[1], eye[1])
    us, vs, ds = np.linspace(0, 351, 7), np.linspace(0, 127, 5), np.linspace(1, 60, 6)
    frustum = np.stack(np.meshgrid(us, vs, ds, indexing="ij"), -1).reshape(-1, 3)                # (u, v, d) rows
    u = 2.0 ** -24
    for s in range(b * n):
        i, j = divmod(s, n)
        # LSS, step by step
        p = frustum - post_trans[i, j]
        p = (np.linalg.inv(post_rots[i, j]) @ p.T).T
        p = np.concatenate([p[:, :2] * p[:, 2:3], p[:, 2:3]], 1)
        p = ((rots[i, j] @ np.linalg.inv(intrins[i, j])) @ p.T).T + trans[i, j]
        want = (extra_rots[i] @ p.T).T + extra_trans[i]
        # the two matrices, in fp64
        m, q4 = pre[s].astype(np.float64), post[s].astype(np.float64)
        a = np.concatenate([frustum, np.ones((len(frustum), 1))], 1)
        q = a @ m.T
        e = np.stack([q[:, 0] * q[:, 2], q[:, 1] * q[:, 2], q[:, 2], np.ones(len(q))], 1)
        got = e @ q4.T
        dq = u * (np.abs(a) @ np.abs(m).T)
        de = np.stack([np.abs(q[:, 0]) * dq[:, 2] + np.abs(q[:, 2]) * dq[:, 0] + dq[:, 0] * dq[:, 2],
                       np.abs(q[:, 1]) * dq[:, 2] + np.abs(q[:, 2]) * dq[:, 1] + dq[:, 1] * dq[:, 2], dq[:, 2], np.zeros(len(q))], 1)
        bound = ((1 + u) * (de @ np.abs(q4).T) + u * (np.abs(e) @ np.abs(q4).T)) * (1 + 2.0 ** -8)
        assert np.all(np.abs(got - want) <= bound), s
        assert np.max(np.abs(got - want) / bound) > 1e-3                  # (the bound is of the error's own size, not a blanket)
    with pytest.raises(ValueError):
        frustum_matrices(rots[0], trans, intrins, post_rots, post_trans)
    with pytest.raises(ValueError):
        frustum_matrices(rots, trans, intrins, post_rots, post_trans, extra_rots[:1], extra_trans)
    with pytest.raises(ValueError):
        frustum_matrices(rots[..., :2], trans, intrins, post_rots, post_trans)


# ---------------------------------------------------------------- refusals: the C entries
def _map_args(**wrong):
    """the arguments of d3d_frustum_map_count for 2 cameras of 5 x 3 pixels and 4 bins in a 4 x 4 x 2 grid, one host buffer standing in
    for every device pointer; `wrong` replaces arguments by name"""
    arena = (ctypes.c_char * (1 << 20))()
    dev = ctypes.addressof(arena)
    a = dict(us=dev, w=5, vs=dev, h=3, ds=dev, d=4, pre=dev, post=dev, s=2, cams=1, lo=(ctypes.c_float * 3)(0, 0, 0),
             size=(ctypes.c_float * 3)(1, 1, 1), shape=(ctypes.c_int32 * 3)(4, 4, 2), counts=dev, workspace=dev, workspace_bytes=len(arena),
             stream=None)
    a.update(wrong)
    return a, arena


def _addr(v):
    return ctypes.addressof(v) if isinstance(v, ctypes.Array) else v


_COUNT_ORDER = "us w vs h ds d pre post s cams lo size shape counts workspace workspace_bytes stream".split()
_EMIT_ORDER = "w h d s cams shape v mapping coords batch_index workspace workspace_bytes stream".split()
_F3, _I3 = ctypes.c_float * 3, ctypes.c_int32 * 3
_MAP_REFUSALS = [
    (dict(size=_F3(0, 1, 1)), _BAD), (dict(size=_F3(1, -1, 1)), _BAD), (dict(size=_F3(1, 1, float("inf"))), _BAD),
    (dict(size=_F3(float("nan"), 1, 1)), _BAD), (dict(shape=_I3(0, 4, 2)), _BAD), (dict(shape=_I3(4, 4, -1)), _BAD),
    (dict(s=3, cams=2), _BAD), (dict(cams=0), _BAD), (dict(w=-1), _BAD), (dict(s=-2), _BAD), (dict(lo=None), _BAD), (dict(size=None), _BAD),
    (dict(shape=None), _BAD), (dict(counts=None), _BAD), (dict(pre=None), _BAD), (dict(us=None), _BAD),
    (dict(s=1 << 20, w=1 << 10, h=2, d=1), _UNSUP),                          # K = 2^31
    (dict(w=46341, h=46341, d=1, s=1), _UNSUP),                              # K just above 2^31 - 1
    (dict(s=1 << 40, w=1 << 30, h=1 << 30, d=1 << 30), _UNSUP),              # K far beyond 64 bits
    (dict(shape=_I3(1 << 15, 1 << 15, 1)), _UNSUP),                          # B n0 n1 n2 = 2^31
    (dict(shape=_I3(2047, 1 << 10, 1 << 10), s=2), _UNSUP),                  # the samples count in the cells
    (dict(workspace=None), _WS), (dict(workspace_bytes=64), _WS),
    (dict(size=_F3(0, 1, 1), shape=_I3(1 << 15, 1 << 15, 1)), _BAD),         # a bad argument wins over an unsupported size
    (dict(shape=_I3(1 << 15, 1 << 15, 1), workspace=None), _UNSUP),
]


def test_frustum_map_entries_refuse_before_any_hip_call():
    """one wrong argument per call (and pairs, for which code wins); the pointers are host memory and there may be no device at all,
    so an entry that reached a HIP call would answer D3D_ERR_HIP or fault"""
    from d3d_amd import _lib
    lib = _lib.load()
    assert lib.d3d_frustum_map_workspace_bytes(2 * 4 * 3 * 5, 2 * 32) < (1 << 20)
    assert lib.d3d_frustum_map_workspace_bytes(1000, 64) < lib.d3d_frustum_map_workspace_bytes(100000, 64)
    assert lib.d3d_frustum_map_workspace_bytes(1000, 64) < lib.d3d_frustum_map_workspace_bytes(1000, 1 << 24)
    wrong = []
    for case, code in _MAP_REFUSALS:
        a, arena = _map_args(**case)
        rc = lib.d3d_frustum_map_count(*[_addr(a[n]) for n in _COUNT_ORDER])
        if rc != code:
            wrong.append(("count", {k: (list(v) if isinstance(v, ctypes.Array) else v) for k, v in case.items()}, code, rc))
        if not set(case) - set(_EMIT_ORDER):
            a.update(v=3, mapping=a["us"], coords=a["us"], batch_index=a["us"])
            rc = lib.d3d_frustum_map_emit(*[_addr(a[n]) for n in _EMIT_ORDER])
            if rc != code:
                wrong.append(("emit", case, code, rc))
    for case, code in ((dict(v=-1), _BAD), (dict(v=2 * 32 + 1), _BAD), (dict(mapping=None), _BAD), (dict(coords=None), _BAD),
                       (dict(batch_index=None), _BAD)):
        a, arena = _map_args()
        a.update(v=3, mapping=a["us"], coords=a["us"], batch_index=a["us"])
        a.update(case)
        rc = lib.d3d_frustum_map_emit(*[_addr(a[n]) for n in _EMIT_ORDER])
        if rc != code:
            wrong.append(("emit", case, code, rc))
    assert not wrong, wrong


_FOLD_REFUSALS = [
    (dict(c=0), _BAD), (dict(s=-1), _BAD), (dict(d=-1), _BAD), (dict(v=-1), _BAD), (dict(dtype=2), _UNSUP), (dict(dtype=3), _UNSUP),
    (dict(dtype=9), _UNSUP), (dict(s=1 << 20, d=1 << 11, h=1, w=1), _UNSUP), (dict(v=1 << 31), _UNSUP), (dict(c=0, dtype=9), _BAD),
    (dict(out=None), _BAD), (dict(a=None), _BAD), (dict(b=None), _BAD),
]


def test_fold_entries_refuse_before_any_hip_call():
    from d3d_amd import _lib
    lib = _lib.load()
    arena = (ctypes.c_char * (1 << 16))()
    dev = ctypes.addressof(arena)
    wrong = []
    for case, code in _FOLD_REFUSALS:
        a = dict(a=dev, b=dev, idx=dev, idx2=dev, s=2, d=4, h=3, w=5, c=8, dtype=0, v=7, out=dev)
        a.update(case)
        rcs = dict(
            forward=lib.d3d_lift_pool_forward(a["a"], a["b"], a["s"], a["d"], a["h"], a["w"], a["c"], a["dtype"], a["idx"], a["idx2"], a["v"],
                                              a["out"], None),
            backward_feat=lib.d3d_lift_pool_backward_feat(a["a"], a["v"], a["b"], a["idx"], a["s"], a["d"], a["h"], a["w"], a["c"], a["dtype"],
                                                          a["out"], None),
            backward_depth=lib.d3d_lift_pool_backward_depth(a["a"], a["v"], a["b"], a["idx"], a["s"], a["d"], a["h"], a["w"], a["c"], a["dtype"],
                                                            a["out"], None))
        wrong += [(entry, case, code, rc) for entry, rc in rcs.items() if rc != code]
    # nothing to do: D3D_OK before any HIP call, with no pointer at all
    assert lib.d3d_lift_pool_forward(None, None, 2, 4, 3, 5, 8, 0, None, None, 0, None, None) == 0
    assert lib.d3d_lift_pool_backward_feat(None, 7, None, None, 0, 4, 3, 5, 8, 0, None, None) == 0
    assert lib.d3d_lift_pool_backward_depth(None, 7, None, None, 2, 0, 3, 5, 8, 0, None, None) == 0
    assert not wrong, wrong


# ---------------------------------------------------------------- refusals: the Python layer
def test_python_layer_refuses_before_a_gpu_is_needed():
    from d3d_amd.voxel import FrustumMap, lift_splat
    from d3d_amd.voxel.lift import grid_of
    sc = {key: (np.array(a) if isinstance(a, np.ndarray) else a) for key, a in cases.scene("int_3x5").items()}      # (copies: writable)
    good = dict(us=sc["us"], vs=sc["vs"], ds=sc["ds"], pre=sc["pre"], post=sc["post"], bounds=sc["bounds"], shape=sc["shape"],
                cams_per_sample=2)
    for case in (dict(shape=(0, 4, 4)), dict(shape=(4, 4)), dict(shape=(4.0, 4, 4)), dict(bounds=(0, 0, 0, 1, 0, 1)),
                 dict(bounds=(0, -1, 0, 1, 0, 1)), dict(bounds=(0, float("inf"), 0, 1, 0, 1)), dict(bounds=(0, float("nan"), 0, 1, 0, 1)),
                 dict(bounds=(0, 1, 0, 1)), dict(cams_per_sample=0), dict(cams_per_sample=True), dict(cams_per_sample=1.0),
                 dict(pre=sc["pre"][:1]), dict(pre=np.concatenate([sc["pre"]] * 2)[:3], post=np.concatenate([sc["post"]] * 2)[:3]),
                 dict(pre=sc["pre"].reshape(2, 12)), dict(post=sc["post"][:, :, :3]), dict(us=sc["us"].reshape(1, -1)),
                 dict(ds=np.arange(5)), dict(shape=(1 << 11, 1 << 10, 1 << 10)),
                 dict(us=np.zeros(1 << 16, np.float32), vs=np.zeros(1 << 15, np.float32))):
        with pytest.raises(ValueError):
            FrustumMap(**dict(good, **case))
    with pytest.raises(TypeError):
        FrustumMap(**dict(good, pre=[[1.0]]))
    lo, size, shape = grid_of((0, 70.4, -40, 40, -3, 1), (704, 800, 40))
    assert lo.dtype == size.dtype == np.float32 and shape == (704, 800, 40)
    assert lo.tolist() == [0, -40, -3] and np.array_equal(size, np.array([70.4 / 704, 80 / 800, 4 / 40]).astype(np.float32))
    for name in cases.SCENES:                                              # the model's grid is the layer's
        g = grid_of(cases.scene(name)["bounds"], cases.scene(name)["shape"])
        assert np.array_equal(g[0], cases.model(name)["lo"]) and np.array_equal(g[1], cases.model(name)["size"])
    with pytest.raises(TypeError):
        lift_splat(torch.zeros(2, 5, 3, 5), torch.zeros(2, 3, 5, 4), "no map")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):              # no silent CPU fallback
            FrustumMap(**good)
