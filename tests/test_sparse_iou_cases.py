"""CPU: the sparse IoU operators (box2d_iou_sparse / iou3d_sparse) without a device -- what every scene of sparse_iou_cases.py
claims, on the oracle alone (oracle.box2d_iou / oracle.iou3d through nonzero is the model); the bindings; the return codes of the
C entries for null and zero-size calls; the host-side errors."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import sparse_iou_cases as sc
from d3d_amd import _lib
from d3d_amd import box as dbox
from d3d_amd.box import box2d_iou_sparse, iou3d_sparse


def oracle_dense(scene, method):
    if scene["dims"] == 2:
        return oracle.box2d_iou(scene["b1"], scene["b2"], method, precise=True)
    return oracle.iou3d(scene["b1"], scene["b2"], method)


def stored_threshold(dense):
    """one stored value of the scene: the median of its positive entries"""
    hits = np.sort(dense[dense > 0])
    return float(hits[len(hits) // 2])


@pytest.mark.parametrize("scene", sc.SCENES, ids=lambda s: s["name"])
def test_scene_claims(scene):
    n, m = len(scene["b1"]), len(scene["b2"])
    assert 1 <= n <= 320 and 1 <= m <= 320 and scene["b1"].shape[1] == scene["b2"].shape[1] == (5 if scene["dims"] == 2 else 7)
    claims = scene["claims"]
    for method in sc.METHODS:
        d = oracle_dense(scene, method)
        pairs, values, offsets = sc.model(d, 0.0)
        k = len(pairs)
        assert offsets[-1] == k and len(values) == k
        if claims.get("hits"):
            assert k > 0
        if claims.get("no_hits"):
            assert k == 0 and not offsets.any()
        if claims.get("all_hit"):
            assert k == n * m and len(sc.model(d, 0.5)[0]) == n * m
        if "row_over_64" in claims:
            r = claims["row_over_64"]
            assert (d[r, :64] > 0).sum() == 64 and (d[r] > 0).sum() > 64
        if "hit_rows" in claims:
            rows = np.flatnonzero((d > 0).any(1))
            assert np.array_equal(rows, claims["hit_rows"]) and rows[0] > 0 and rows[-1] < n - 1
        if "dead_rows" in claims:
            dead_r, dead_c = list(claims["dead_rows"]), list(claims["dead_cols"])
            if method == "box":                                   # the bounding box of a rectangle without area may have one: NaN rows only
                dead_r, dead_c = [r for r in dead_r if np.isnan(scene["b1"][r]).any()], [c for c in dead_c if np.isnan(scene["b2"][c]).any()]
            assert not (d[dead_r] > 0).any() and not (d[:, dead_c] > 0).any()
        if "zero_candidates" in claims:
            ci, cj = oracle.aabb_candidate_pairs(scene["b1"], scene["b2"])
            zero = d[ci, cj] <= sc.TIE
            assert zero.sum() >= claims["zero_candidates"]
            assert (d[ci, cj][zero] == 0).all()                   # exactly 0, so absent at threshold 0 -- no tie either
        if claims.get("z_groups"):
            bev = oracle.box2d_iou(scene["b1"][:, [0, 1, 3, 4, 6]], scene["b2"][:, [0, 1, 3, 4, 6]], method, precise=True)
            i = np.arange(n)
            assert (bev[i, i] > 0).all()
            assert (d[i, i][i % 3 == 0] > 0).all() and (d[i, i][i % 3 != 0] == 0).all()
        # the rounding ties the GPU test leaves undecided stay under the cap, at every threshold it runs
        thresholds = list(sc.THRESHOLDS) + ([stored_threshold(d)] if scene["stored"] else [])
        for t in thresholds:
            assert sc.ties(d, t).sum() <= sc.TIE_CAP * n * m, (scene["name"], method, t)
        if scene["stored"]:
            t = thresholds[-1]
            assert (d == np.asarray(t, d.dtype)).any() and len(sc.model(d, t)[0]) < k      # strictness drops that pair


def test_names_and_bindings():
    for name in ("box2d_iou_sparse", "iou3d_sparse"):
        assert name in dbox.__all__ and callable(getattr(dbox, name))
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t
    inputs = [vp, i64, vp, i64, i32, i32, i32, ctypes.c_double]
    assert _lib.SIGNATURES["d3d_iou_sparse_workspace_bytes"] == (sz, [i64, i64])
    assert _lib.SIGNATURES["d3d_iou_sparse_count"] == (ctypes.c_int, inputs + [vp, vp, sz, vp])
    assert _lib.SIGNATURES["d3d_iou_sparse_emit"] == (ctypes.c_int, inputs + [vp, i64, vp, vp, vp, sz, vp])


def test_c_entries_without_a_device():
    lib = _lib.load()
    count = lambda n, m, cols, kind, dtype, thr: lib.d3d_iou_sparse_count(None, n, None, m, cols, kind, dtype, thr, None, None, 0, None)      # noqa: E731
    emit = lambda n, m, cols, kind, dtype, thr, cap=0: lib.d3d_iou_sparse_emit(None, n, None, m, cols, kind, dtype, thr, None, cap, None,      # noqa: E731
                                                                               None, None, 0, None)
    for fn in (count, emit):
        for n, m in ((0, 0), (0, 7), (7, 0)):                     # zero sizes: OK without a launch, null pointers allowed
            assert fn(n, m, 5, 2, _lib.F64, 0.0) == _lib.OK
            assert fn(n, m, 5, 1, _lib.F32_WIDE, 0.5) == _lib.OK
            assert fn(n, m, 7, 2, _lib.F32, 0.0) == _lib.OK
        assert fn(-1, 3, 5, 2, _lib.F64, 0.0) == _lib.ERR_BAD_ARG
        assert fn(3, -1, 5, 2, _lib.F64, 0.0) == _lib.ERR_BAD_ARG
        assert fn(1 << 31, 3, 5, 2, _lib.F64, 0.0) == _lib.ERR_BAD_ARG
        assert fn(0, 0, 6, 2, _lib.F64, 0.0) == _lib.ERR_BAD_ARG
        for kind in (0, 3, 4, 5, 6, 9):
            assert fn(0, 0, 5, kind, _lib.F64, 0.0) == _lib.ERR_UNSUPPORTED
        assert fn(0, 0, 5, 2, _lib.F64_M32, 0.0) == _lib.ERR_UNSUPPORTED
        assert fn(0, 0, 5, 2, 9, 0.0) == _lib.ERR_UNSUPPORTED
        for dtype in (_lib.F64, _lib.F32_WIDE, _lib.F64_M32):      # 7 columns: fp32 only, as iou3d
            assert fn(0, 0, 7, 2, dtype, 0.0) == _lib.ERR_UNSUPPORTED
        for thr in (-0.5, float("nan"), float("inf"), -float("inf")):
            assert fn(0, 0, 5, 2, _lib.F64, thr) == _lib.ERR_BAD_ARG
        assert fn(4, 4, 5, 2, _lib.F64, 0.0) == _lib.ERR_BAD_ARG   # null pointers with work to do
        assert fn(4, 4, 7, 1, _lib.F32, 0.0) == _lib.ERR_BAD_ARG
    assert emit(0, 0, 5, 2, _lib.F64, 0.0, cap=-1) == _lib.ERR_BAD_ARG
    # O(n + m), never O(n * m); a carve on a null base: a multiple of 256, monotone
    q = lib.d3d_iou_sparse_workspace_bytes
    sizes = [0, 1, 63, 64, 65, 1000, 4097, 100000]
    for n in sizes:
        for m in sizes:
            assert q(n, m) % 256 == 0 and 0 < q(n, m) <= 16 * m + n // 128 + 1024
            assert q(n + 1, m) >= q(n, m) and q(n, m + 1) >= q(n, m)
    assert q(200000, 200000) < 4 << 20


def test_host_side_errors():
    z5, z7 = torch.zeros(3, 5), torch.zeros(3, 7)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "x"):
        with pytest.raises(ValueError, match="threshold"):
            box2d_iou_sparse(z5, z5, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            iou3d_sparse(z7, z7, threshold=bad)
    for method in ("grbox", "drbox"):
        with pytest.raises(ValueError, match="Unsupported iou type!"):
            box2d_iou_sparse(z5, z5, method=method)
        with pytest.raises(ValueError, match="Unsupported iou type!"):
            iou3d_sparse(z7, z7, method=method)
    with pytest.raises(AttributeError):
        box2d_iou_sparse(z5, z5, method="circle")                 # like box2d_iou
    with pytest.raises(ValueError, match="Unrecognized iou type!"):
        iou3d_sparse(z7, z7, method="circle")                     # like iou3d
    with pytest.raises(ValueError, match="Nx2 tensors"):
        box2d_iou_sparse(torch.zeros(5), z5)
    for a, b in ((torch.zeros(3, 4), z5), (z5, z7), (z7, z7)):
        with pytest.raises(ValueError, match="5 fields"):
            box2d_iou_sparse(a, b)
    for a, b in ((z5, z7), (z7, z5), (torch.zeros(7), z7)):
        with pytest.raises(ValueError, match="7 fields"):
            iou3d_sparse(a, b)
    with pytest.raises(AssertionError, match="both numpy"):
        box2d_iou_sparse(np.zeros((3, 5)), z5)
    with pytest.raises(RuntimeError, match="same dtype"):
        box2d_iou_sparse(z5, z5.double(), precise=False)
    with pytest.raises(RuntimeError, match="float32 or float64"):
        box2d_iou_sparse(z5.int(), z5.int(), precise=False)


@pytest.mark.parametrize("numpy_in", [False, True])
def test_empty_inputs_need_no_device(numpy_in):
    for n, m in ((0, 4), (4, 0), (0, 0)):
        for dtype in (torch.float32, torch.float64):
            a, b = torch.ones(n, 5, dtype=dtype), torch.ones(m, 5, dtype=dtype)
            a3, b3 = torch.ones(n, 7, dtype=dtype), torch.ones(m, 7, dtype=dtype)
            if numpy_in:
                a, b, a3, b3 = a.numpy(), b.numpy(), a3.numpy(), b3.numpy()
            for out, vdtype in ((box2d_iou_sparse(a, b, return_offsets=True), dtype), (iou3d_sparse(a3, b3, return_offsets=True), torch.float32)):
                assert len(out) == 3 and all(isinstance(t, np.ndarray if numpy_in else torch.Tensor) for t in out)
                pairs, values, offsets = (torch.from_numpy(t) if numpy_in else t for t in out)
                assert pairs.shape == (0, 2) and pairs.dtype == torch.int64 and values.shape == (0,) and values.dtype == vdtype
                assert offsets.shape == (n + 1,) and offsets.dtype == torch.int64 and not offsets.any()
            assert len(box2d_iou_sparse(a, b)) == 2


def test_no_silent_cpu_fallback():
    if not torch.cuda.is_available():                              # (with a GPU the calls below simply run: test_gpu_sparse_iou.py)
        with pytest.raises(RuntimeError, match="HIP device"):
            box2d_iou_sparse(torch.ones(3, 5), torch.ones(3, 5))
        with pytest.raises(RuntimeError, match="HIP device"):
            iou3d_sparse(np.ones((3, 7)), np.ones((3, 7)), method="box")
