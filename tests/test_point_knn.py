"""CPU: the numpy models of knn_query, the kNN weights and the weighted fold against exact arithmetic and their own properties, and
every host-side refusal of the four C entries and of the Python layer.  No GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import point_knn_cases as cases
import point_knn_reference as ref
from d3d_amd import _lib
from d3d_amd.point import PointInterp, knn_query, point_interpolate

DTYPES = (np.float32, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_model_equals_exact_arithmetic(dtype):
    """every q of these scenes is exact in fp32: model and brute force agree in every row and every bit"""
    for name, pts, ctr, poffs, coffs in cases.exact_scenes():
        assert np.abs(pts).max() <= 1000 and np.array_equal(pts * 64, np.round(pts * 64)), name
        for k in (1, 3, 16, 64):
            table, dist2 = ref.knn_model(pts.astype(dtype), ctr.astype(dtype), k, poffs, coffs)
            want_table, want_dist2 = ref.knn_exact(pts, ctr, k, poffs, coffs)
            assert table.dtype == np.int32 and dist2.dtype == dtype
            assert table.tolist() == want_table, (name, k)
            got = [[None if np.isinf(q) else Fraction(float(q)) for q in row] for row in dist2]
            assert got == want_dist2, (name, k)


def test_knn_model_on_values_that_are_not_finite():
    by_name = {s[0]: s for s in cases.scenes()}
    _, pts, ctr, _, _ = by_name["nonfinite"]
    table, dist2 = ref.knn_model(pts.astype(np.float32), ctr.astype(np.float32), 300)
    nan_rows = set(np.nonzero(np.isnan(pts[:, :3]).any(1))[0].tolist())
    inf_rows = set(np.nonzero(np.isinf(pts[:, :3]).any(1))[0].tolist()) - nan_rows
    assert len(nan_rows) == 3 and len(inf_rows) == 6
    for c in range(12):                                  # a finite centre: NaN rows are out, infinite rows come last with q = +inf
        rows = table[c][table[c] >= 0].tolist()
        assert set(rows) == set(range(300)) - nan_rows and rows[-6:] == sorted(inf_rows)
        assert np.all(np.isinf(dist2[c, len(rows) - 6:len(rows)])) and np.all(np.diff(dist2[c, :len(rows) - 6]) >= 0)
    assert np.all(table[12] == -1) and np.all(np.isinf(dist2[12]))               # the NaN centre
    for c, col in ((13, 1), (14, 2)):                    # an infinite centre: a row infinite in that column the same way is NaN
        same = {r for r in inf_rows if pts[r, col] == ctr[c, col]}
        assert same and set(table[c][table[c] >= 0].tolist()) == set(range(300)) - nan_rows - same
    _, pts, ctr, _, _ = by_name["huge"]
    table, dist2 = ref.knn_model(pts.astype(np.float32), ctr.astype(np.float32), 200)
    assert np.all(table[:4] >= 0) and np.all(np.isinf(dist2[:4, 67:])) and np.all(np.isfinite(dist2[:4, :67]))
    assert np.all(np.diff(table[:4, 67:].astype(np.int64), axis=1) > 0)         # equal q = +inf: by row
    t64, d64 = ref.knn_model(pts, ctr, 200)
    assert np.all(np.isfinite(d64)) and np.all(t64 >= 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("power", (1, 2))
def test_weights_model_properties(dtype, power):
    rng = np.random.default_rng(31)
    ulp = np.finfo(dtype).eps
    for name, pts, ctr, poffs, coffs in cases.exact_scenes():
        table, dist2 = ref.knn_model(pts.astype(dtype), ctr.astype(dtype), 5, poffs, coffs)
        w = ref.knn_weights_model(table, dist2, power, 1e-8)
        assert w.dtype == dtype and np.all(w[table < 0] == 0) and np.all(w >= 0), name
        has = (table >= 0).any(1)
        s = np.zeros(len(w), dtype)
        for j in range(w.shape[1]):
            s = s + w[:, j]
        assert np.all(np.abs(s[has] - 1) <= 2 * ulp) and np.all(s[~has] == 0), name   # (the sum of <= 5 quotients u / s, each within 1/2 ulp)
        assert np.all(np.diff(np.where(table >= 0, w, 0), axis=1) <= 0), name          # nearer rows weigh no less
        w0 = ref.knn_weights_model(table, dist2, power, 0.0)
        hit = ((dist2 == 0) & (table >= 0)).any(1)
        assert np.all(w0[hit] == 0) and np.all((w0[has & ~hit] > 0).any(1)), name      # an exact hit with eps = 0: u = inf, all zero
    q = rng.uniform(0.5, 4.0, (6, 3)).astype(dtype)
    t = np.array([[0, 1, 2], [3, -1, 4], [-1, -1, 5], [-1, -1, -1], [6, 7, -1], [-1, 8, -1]], np.int32)
    w = ref.knn_weights_model(t, q, power, 0.0)
    assert np.all(w[t < 0] == 0) and w[2, 2] == 1 and w[5, 1] == 1 and np.all(w[3] == 0)
    u = 1 / (np.sqrt(q[1, [0, 2]]) if power == 1 else q[1, [0, 2]])
    assert np.array_equal(w[1, [0, 2]], u / (dtype(0) + u[0] + u[1]))
    q[0, 2] = np.inf                                     # u = 0 for a row at q = +inf; all of a row at +inf: s == 0, all zero
    q[4, :2] = np.inf
    w = ref.knn_weights_model(t, q, power, 1e-8)
    assert w[0, 2] == 0 and w[0, 0] > 0 and np.all(w[4] == 0)


def test_fold_transpose_model_is_the_transpose():
    """<fold(F), G> == <F, transpose(G)> on small integers: every product and sum is exact, so the two sides are equal"""
    rng = np.random.default_rng(32)
    for v, r, j, c in ((40, 70, 3, 5), (9, 33, 16, 2), (1, 8, 1, 4), (25, 10, 64, 3)):
        table = rng.integers(-1, v, (r, j)).astype(np.int32)
        w = rng.integers(-4, 5, (r, j)).astype(np.float64)
        f, g = rng.integers(-8, 9, (v, c)).astype(np.float64), rng.integers(-8, 9, (r, c)).astype(np.float64)
        out, back = ref.wfold_model(f, table, w), ref.wfold_transpose_model(g, table, w, v)
        assert (out * g).sum() == (f * back).sum()
        dense = np.zeros((r, v))
        for rr in range(r):
            for jj in range(j):
                if table[rr, jj] >= 0:
                    dense[rr, table[rr, jj]] += w[rr, jj]
        assert np.array_equal(out, dense @ f) and np.array_equal(back, dense.T @ g)
    assert np.all(ref.wfold_model(f, np.full((4, 3), -1, np.int32), np.ones((4, 3))) == 0)


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """pointers that are never followed: each call returns before its first HIP call"""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    knn = lambda **k: lib.d3d_knn_query(*[k.get(a, v) for a, v in (  # noqa: E731
        ("points", p), ("n", 10), ("pstride", 3), ("centers", p), ("m", 4), ("cstride", 3), ("dtype", _lib.F32), ("poffs", None),
        ("coffs", None), ("segments", 0), ("k", 3), ("table", p), ("dist2", None), ("stream", None))])
    for wrong in (dict(n=-1), dict(m=-1), dict(segments=-1), dict(pstride=2), dict(cstride=0), dict(k=0), dict(k=-3), dict(poffs=p),
                  dict(coffs=p), dict(poffs=p, coffs=p, segments=0), dict(table=None), dict(centers=None), dict(points=None)):
        assert knn(**wrong) == bad, wrong
    for wrong in (dict(dtype=_lib.F16), dict(dtype=_lib.BF16), dict(n=2 ** 31), dict(m=2 ** 31), dict(poffs=p, coffs=p, segments=2 ** 31),
                  dict(k=_lib.KNN_MAX + 1)):
        assert knn(**wrong) == uns, wrong
    assert knn(m=0, centers=None, table=None) == _lib.OK and knn(m=0, k=_lib.KNN_MAX, points=None, centers=None, table=None) == _lib.OK
    wts = lambda t=p, q=p, m=4, k=3, dtype=_lib.F32, power=1, eps=1e-8, w=p: lib.d3d_knn_weights(t, q, m, k, dtype, power, eps, w, None)  # noqa: E731
    assert [wts(m=-1), wts(k=0), wts(power=0), wts(power=3), wts(eps=-1e-9), wts(eps=float("nan")), wts(eps=float("inf")), wts(eps=1e39),
            wts(t=None), wts(q=None), wts(w=None)] == [bad] * 11
    assert [wts(dtype=_lib.F16), wts(dtype=7), wts(k=_lib.KNN_MAX + 1), wts(m=2 ** 30)] == [uns] * 4
    assert wts(eps=1e39, dtype=_lib.F64, m=0, t=None, q=None, w=None) == _lib.OK and wts(m=0, eps=0.0, t=None, q=None, w=None) == _lib.OK
    fwd = lambda feat=p, v=10, c=4, dtype=0, t=p, w=p, rows=5, j=3, out=p: lib.d3d_knn_interp_forward(feat, v, c, dtype, t, w, rows, j, out, None)  # noqa: E731
    bwd = lambda g=p, rows=5, c=4, dtype=0, o=p, off=p, w=p, j=3, v=10, out=p: lib.d3d_knn_interp_backward(g, rows, c, dtype, o, off, w, j, v, out, None)  # noqa: E731
    assert [fwd(v=-1), fwd(rows=-1), fwd(c=0), fwd(j=0), fwd(j=-1), fwd(feat=None), fwd(t=None), fwd(w=None), fwd(out=None)] == [bad] * 9
    assert [fwd(dtype=2), fwd(dtype=3), fwd(dtype=6), fwd(v=2 ** 31), fwd(rows=2 ** 30), fwd(rows=2 ** 31, j=1), fwd(j=_lib.KNN_MAX + 1)] == [uns] * 7
    assert [bwd(v=-1), bwd(rows=-1), bwd(c=0), bwd(j=0), bwd(g=None), bwd(o=None), bwd(off=None), bwd(w=None), bwd(out=None)] == [bad] * 9
    assert [bwd(dtype=2), bwd(dtype=-1), bwd(v=2 ** 31), bwd(rows=2 ** 30), bwd(rows=2 ** 31, j=1), bwd(j=_lib.KNN_MAX + 1)] == [uns] * 6
    for dtype in (_lib.F32, _lib.F64, _lib.F16, _lib.BF16):
        for j in (1, 3, 8, _lib.KNN_MAX):
            assert fwd(dtype=dtype, j=j, rows=0, feat=None, t=None, w=None, out=None) == _lib.OK
            assert bwd(dtype=dtype, j=j, v=0, g=None, o=None, off=None, w=None, out=None) == _lib.OK
    # the fixed-width entries keep their own refusals
    assert lib.d3d_table_interp_forward(p, 10, 4, 0, p, p, 5, 3, p, None) == bad
    assert lib.d3d_table_interp_backward(p, 5, 4, 0, p, p, p, 3, 10, p, None) == bad


def test_python_layer_refuses_before_a_gpu_is_needed():
    pts, ctr = torch.zeros(10, 3), torch.zeros(4, 3)
    for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(k=3.0), dict(k=True), dict(k="3"), dict(point_offsets=[0, 10]), dict(center_offsets=[0, 4]),
               dict(point_offsets=[0, 10], center_offsets=[0, 2, 4]), dict(point_offsets=[0, 11], center_offsets=[0, 4]),
               dict(point_offsets=[0, 10], center_offsets=[1, 4]), dict(point_offsets=[0, 6, 4, 10], center_offsets=[0, 1, 2, 4]),
               dict(point_offsets=[[0, 10]], center_offsets=[0, 4]), dict(point_offsets=[0.0, 10.0], center_offsets=[0, 4]),
               dict(point_offsets=torch.tensor([0.0, 10.0]), center_offsets=[0, 4])):
        with pytest.raises(ValueError):
            knn_query(pts, ctr, **dict(dict(k=3), **kw))
        with pytest.raises(ValueError):
            PointInterp(pts, ctr, **{dict(point_offsets="known_offsets", center_offsets="unknown_offsets").get(a, a): v
                                     for a, v in dict(dict(k=3), **kw).items()})
    for bad_pts, bad_ctr in ((pts, ctr.double()), (pts, torch.zeros(4, 2)), (pts.half(), ctr.half()), (torch.zeros(10), ctr), (pts, torch.zeros(2, 4, 3)),
                             (pts.long(), ctr.long()), (np.zeros((10, 2), np.float32), np.zeros((4, 3), np.float32))):
        with pytest.raises(ValueError):
            knn_query(bad_pts, bad_ctr, 3)
        with pytest.raises(ValueError):
            PointInterp(bad_pts, bad_ctr)
    with pytest.raises(TypeError):
        knn_query([[0.0, 0.0, 0.0]], ctr, 1)
    for kw in (dict(power=0), dict(power=3), dict(power=1.5), dict(power=True), dict(eps=-1e-8), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(eps="1e-8"), dict(eps=1e39)):
        with pytest.raises(ValueError):
            PointInterp(pts, ctr, **kw)
    # nothing to launch: no centres
    table, dist2 = knn_query(pts, torch.zeros(0, 5), 4)
    assert table.shape == (0, 4) and table.dtype == torch.int32 and dist2.shape == (0, 4) and dist2.dtype == torch.float32
    table = knn_query(np.zeros((10, 4)), np.zeros((0, 3)), 2, return_distances=False)
    assert isinstance(table, np.ndarray) and table.shape == (0, 2) and table.dtype == np.int32
    # from_table
    t, w = torch.zeros((5, 3), dtype=torch.int32), torch.zeros((5, 3))
    for bad_t, bad_w, nk in ((torch.zeros((5, 65), dtype=torch.int32), torch.zeros((5, 65)), 4), (torch.zeros((5, 0), dtype=torch.int32), torch.zeros((5, 0)), 4),
                             (t.long(), w, 4), (t[0], w[0], 4), (t, w[:, :2], 4), (t, w.half(), 4), (t, w, -1), (t, w, 2 ** 31), (t, w, 0), (t - 2, w, 4),
                             (t + 4, w, 4), (t, w, 4.0)):
        with pytest.raises(ValueError):
            PointInterp.from_table(bad_t, bad_w, nk)
    with pytest.raises(TypeError):
        PointInterp.from_table([[0]], w, 4)
    with pytest.raises(TypeError):
        point_interpolate(torch.zeros(4, 2), object())
    # the operator's own refusals, on a PointInterp put together by hand (building one needs a GPU): 6 known rows, 5 query rows
    itp = PointInterp.__new__(PointInterp)
    itp._set(torch.device("cuda", 0), t, None, w, 6)
    assert (itp.num_known, itp.num_points, itp.k) == (6, 5, 3)
    with pytest.raises(TypeError):
        point_interpolate([[0.0] * 4] * 6, itp)
    for bad in (torch.zeros((6, 4), dtype=torch.int32), np.zeros((6, 4), np.int64), torch.zeros((6, 4), dtype=torch.complex64)):
        with pytest.raises(ValueError, match="float32, float64, float16 or bfloat16"):
            point_interpolate(bad, itp)
    for bad in (torch.zeros(6), torch.zeros((6, 4, 1))):
        with pytest.raises(ValueError, match="2-D"):
            point_interpolate(bad, itp)
    for bad in (torch.zeros((7, 4)), torch.zeros((5, 4), dtype=torch.bfloat16), np.zeros((0, 4), np.float16)):
        with pytest.raises(ValueError, match="rows"):
            point_interpolate(bad, itp)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):                                  # no CPU fallback
            knn_query(pts, ctr, 3)
        with pytest.raises(RuntimeError, match="HIP device"):
            PointInterp(pts, ctr)
        with pytest.raises(RuntimeError, match="HIP device"):
            PointInterp.from_table(t, w, 4)
