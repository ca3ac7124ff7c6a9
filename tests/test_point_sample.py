"""CPU: the numpy models of furthest_point_sample / ball_query against an independent implementation in Python integers, the
models' own properties, the pure host entries (d3d_fps_plan, the workspace query) and every host-side refusal.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import point_sample_cases as cases
import point_sample_reference as ref
from d3d_amd import _lib
from d3d_amd.point import ball_query, fps_plan, furthest_point_sample

DTYPES = (np.float32, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_model_equals_integer_arithmetic(dtype):
    """|x| <= 1000: every q is an integer below 2^24, exact in fp32 -- model and exact implementation agree in every index and bit"""
    for name, pts, m, offs in cases.integer_fps_scenes():
        assert np.abs(pts).max() <= 1000 and np.array_equal(pts, np.round(pts)), name
        idx, dist = ref.fps_model(pts.astype(dtype), m, offs)
        want_idx, want_dist = ref.fps_exact(pts, m, offs)
        assert idx.tolist() == want_idx, name
        assert dist.dtype == dtype and dist.tolist() == [np.inf if d is None else float(d) for d in want_dist], name


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_model_equals_integer_arithmetic(dtype):
    for name, pts, ctr, r, poffs, coffs in cases.integer_ball_scenes():
        for nsample, pad in ((1, "none"), (5, "first"), (16, "none"), (64, "first")):
            table, counts = ref.ball_model(pts.astype(dtype), ctr.astype(dtype), r, nsample, poffs, coffs, pad)
            want_table, want_counts = ref.ball_exact(pts, ctr, r, nsample, poffs, coffs, pad)
            assert table.tolist() == want_table and counts.tolist() == want_counts, (name, nsample, pad)
    # a lattice row at exactly r from a lattice centre is outside
    lat = np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 1, 1], [0.0, -2, 0]])
    table, counts = ref.ball_model(lat.astype(dtype), lat[:1].astype(dtype), 2, 4)
    assert table.tolist() == [[0, 2, -1, -1]] and counts.tolist() == [2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_properties(dtype):
    for name, pts, m, offs in cases.fps_scenes(big_rows=2100):
        pts = pts.astype(dtype)
        trace = []
        idx, dist = ref.fps_model(pts, m, offs, trace)
        segs = [0, len(pts)] if offs is None else offs
        ms = [m] * (len(segs) - 1) if np.isscalar(m) else m
        assert len(idx) == len(dist) == len(trace) == sum(ms), name
        at = 0
        for b, mb in enumerate(ms):
            d_seg = dist[at:at + mb]
            if mb and not np.isnan(d_seg).any():
                assert d_seg[0] == np.inf and np.all(d_seg[2:] <= d_seg[1:-1]), name         # non-increasing after step 0
            for s in range(at, at + mb):
                start, d = trace[s]
                assert start == segs[b] and segs[b] <= idx[s] < segs[b + 1], name
                if (d >= 0).any():                      # the pick holds the maximum, and no lower row does
                    c = idx[s] - start
                    assert d[c] == d.max() and not (d[:c] == d.max()).any() and dist[s] == d[c], name
                else:
                    assert idx[s] == start and np.isnan(dist[s]), name
            at += mb
    for name, pts, ctr, r, poffs, coffs in cases.ball_scenes():
        pts, ctr = pts.astype(dtype), ctr.astype(dtype)
        r2 = dtype(r) * dtype(r)
        psegs = [0, len(pts)] if poffs is None else poffs
        csegs = [0, len(ctr)] if coffs is None else coffs
        for nsample, pad in ((3, "none"), (33, "first")):
            table, counts = ref.ball_model(pts, ctr, r, nsample, poffs, coffs, pad)
            for c in range(len(ctr)):
                b = int(np.searchsorted(csegs, c, side="right")) - 1
                with np.errstate(invalid="ignore", over="ignore"):
                    inside = (ref._q(pts, ctr[c]) < r2)
                inside[:psegs[b]] = False
                inside[psegs[b + 1]:] = False
                rows = table[c, :counts[c]]
                assert counts[c] == min(int(inside.sum()), nsample), (name, c)
                assert np.all(np.diff(rows) > 0) and inside[rows].all(), (name, c)            # ascending, all inside ...
                if len(rows):
                    assert inside[:rows[-1] + 1].sum() == len(rows), (name, c)                # ... and no inside row skipped
                assert np.all(table[c, counts[c]:] == (rows[0] if (pad == "first" and len(rows)) else -1)), (name, c)


_plan, fps_boundaries = cases.fps_plan_of, cases.fps_boundaries


def test_fps_plan_and_workspace_are_pure_and_monotone():
    lib = _lib.load()
    for code, size in ((_lib.F32, 4), (_lib.F64, 8)):
        bounds = fps_boundaries(code)
        assert [r for r, _ in bounds] == list(range(len(bounds))) and bounds[-1][0] == _lib.FPS_ROUTE_LDS
        caps = [c for _, c in bounds]
        assert caps == sorted(set(caps)) and all(c % 64 == 0 for c in caps)
        last = (0, 0)
        for n in sorted({0, 1, 2, 1000, 10 ** 6, 2 ** 31 - 1} | {c + k for c in caps for k in (-1, 0, 1)}):
            got = _plan(n, code)
            assert got == _plan(n, code) and got[0] >= last[0] and got[1] >= last[1] and got[1] >= n, (code, n)
            last = got
        assert _plan(2 ** 31 - 1, code) == (_lib.FPS_ROUTE_STREAM, 2 ** 31 - 1)
        route, cap = ctypes.c_int32(-7), ctypes.c_int32(-7)
        assert lib.d3d_fps_plan(-1, code, ctypes.byref(route), ctypes.byref(cap)) == _lib.ERR_BAD_ARG
        assert lib.d3d_fps_plan(2 ** 31, code, ctypes.byref(route), ctypes.byref(cap)) == _lib.ERR_UNSUPPORTED
        assert lib.d3d_fps_plan(5, _lib.F16, ctypes.byref(route), ctypes.byref(cap)) == _lib.ERR_UNSUPPORTED
        assert (route.value, cap.value) == (-7, -7)
        sizes = [lib.d3d_fps_workspace_bytes(n, 3, code) for n in (0, 1, 1000, 10 ** 6, 10 ** 8)]
        assert sizes == sorted(sizes) and sizes[-1] >= 10 ** 8 * size and all(s % 256 == 0 for s in sizes)
        assert lib.d3d_fps_workspace_bytes(1000, 3, code) == lib.d3d_fps_workspace_bytes(1000, 3, code)
    # the KITTI keypoint case stays on chip in fp32, and fp64 holds half of what fp32 holds
    assert _plan(16384, _lib.F32)[0] <= _lib.FPS_ROUTE_LDS and fps_plan(16384) == _plan(16384, _lib.F32)
    assert fps_boundaries(_lib.F32)[-1][1] >= 16384 and fps_boundaries(_lib.F64)[-1][1] * 2 == fps_boundaries(_lib.F32)[-1][1]


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """a host buffer stands in for every device pointer: each call returns before its first HIP call"""
    lib = _lib.load()
    arena = (ctypes.c_char * 4096)()
    p = ctypes.addressof(arena)
    fps = lambda **k: lib.d3d_furthest_point_sample(*[k.get(a, v) for a, v in (  # noqa: E731
        ("points", p), ("n", 10), ("stride", 3), ("dtype", _lib.F32), ("poffs", p), ("soffs", p), ("segments", 1), ("indices", p),
        ("distances", None), ("ws", p), ("ws_bytes", 4096), ("stream", None))])
    assert fps(n=-1) == _lib.ERR_BAD_ARG and fps(stride=2) == _lib.ERR_BAD_ARG and fps(poffs=None) == _lib.ERR_BAD_ARG
    assert fps(indices=None) == _lib.ERR_BAD_ARG and fps(points=None) == _lib.ERR_BAD_ARG and fps(segments=-1) == _lib.ERR_BAD_ARG
    assert fps(dtype=_lib.F16) == _lib.ERR_UNSUPPORTED and fps(segments=2 ** 31) == _lib.ERR_UNSUPPORTED
    assert fps(ws=None) == _lib.ERR_WORKSPACE and fps(ws_bytes=16) == _lib.ERR_WORKSPACE
    assert fps(segments=0, poffs=None, soffs=None, indices=None, ws=None) == _lib.OK          # nothing to do, nothing launched
    bq = lambda **k: lib.d3d_ball_query(*[k.get(a, v) for a, v in (  # noqa: E731
        ("points", p), ("n", 10), ("pstride", 3), ("centers", p), ("m", 4), ("cstride", 3), ("dtype", _lib.F32), ("poffs", None),
        ("coffs", None), ("segments", 0), ("radius", 1.0), ("nsample", 8), ("pad", 0), ("table", p), ("counts", p), ("stream", None))])
    for wrong in (dict(n=-1), dict(m=-1), dict(pstride=2), dict(cstride=0), dict(nsample=0), dict(nsample=1025), dict(radius=0.0),
                  dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(poffs=p), dict(coffs=p),
                  dict(table=None), dict(counts=None), dict(centers=None), dict(points=None), dict(poffs=p, coffs=p, segments=0)):
        assert bq(**wrong) == _lib.ERR_BAD_ARG, wrong
    assert bq(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED and bq(n=2 ** 31) == _lib.ERR_UNSUPPORTED
    assert bq(m=0, centers=None, table=None, counts=None) == _lib.OK


def test_python_layer_refuses_before_a_gpu_is_needed():
    pts = torch.zeros(10, 3)
    for offsets in ([1, 10], [0, 9], [0, 6, 4, 10], [], [[0, 10]], [0.0, 10.0], torch.tensor([0.0, 10.0])):
        with pytest.raises(ValueError):
            furthest_point_sample(pts, 2, offsets)
    with pytest.raises(ValueError):                      # a segment without rows cannot give samples
        furthest_point_sample(pts, [1, 1], [0, 0, 10])
    with pytest.raises(ValueError):
        furthest_point_sample(pts, 2, [0, 10, 10])
    with pytest.raises(ValueError):
        furthest_point_sample(torch.zeros(0, 3), 1)
    with pytest.raises(ValueError):                      # a segment above 2^31 - 1 rows (an expanded view: no memory behind it)
        furthest_point_sample(torch.zeros(1, 3).expand(2 ** 31, 3), 1)
    for bad in (torch.zeros(10, 3, dtype=torch.float16), torch.zeros(10, 3, dtype=torch.int64), torch.zeros(10, 2), torch.zeros(10),
                torch.zeros(2, 5, 3), np.zeros((10, 2), np.float32)):
        with pytest.raises(ValueError):
            furthest_point_sample(bad, 1)
    with pytest.raises(ValueError):
        furthest_point_sample(pts, -1)
    with pytest.raises(ValueError):
        furthest_point_sample(pts, [2, -1], [0, 5, 10])
    with pytest.raises(ValueError):
        furthest_point_sample(pts, [2, 2, 2], [0, 5, 10])
    with pytest.raises(TypeError):
        furthest_point_sample([[0.0, 0.0, 0.0]], 1)
    # valid, and nothing to launch: M = 0, B = 0
    assert furthest_point_sample(pts, 0).shape == (0,) and furthest_point_sample(pts, 0).dtype == torch.int64
    idx, dist = furthest_point_sample(np.zeros((0, 4)), 3, [0], return_distances=True)
    assert idx.shape == dist.shape == (0,) and idx.dtype == np.int64 and dist.dtype == np.float64
    assert furthest_point_sample(pts, [0, 0], [0, 0, 10]).numel() == 0

    ctr = torch.zeros(4, 3)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="1"),
               dict(radius=torch.tensor(1.0)), dict(nsample=0), dict(nsample=1025), dict(pad="last"), dict(point_offsets=[0, 10]),
               dict(center_offsets=[0, 4]), dict(point_offsets=[0, 10], center_offsets=[0, 2, 4]),
               dict(point_offsets=[0, 11], center_offsets=[0, 4]), dict(point_offsets=[0, 10], center_offsets=[1, 4])):
        with pytest.raises(ValueError):
            ball_query(pts, ctr, **dict(dict(radius=1.0, nsample=4), **kw))
    with pytest.raises(ValueError):
        ball_query(pts, ctr.double(), 1.0, 4)
    with pytest.raises(ValueError):
        ball_query(pts, torch.zeros(4, 2), 1.0, 4)
    with pytest.raises(ValueError):
        ball_query(pts.half(), ctr.half(), 1.0, 4)
    table, counts = ball_query(pts, torch.zeros(0, 5), 1.0, 4)
    assert table.shape == (0, 4) and table.dtype == torch.int32 and counts.shape == (0,) and counts.dtype == torch.int32
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):                                  # no CPU fallback
            furthest_point_sample(pts, 2)
        with pytest.raises(RuntimeError, match="HIP device"):
            ball_query(pts, ctr, 1.0, 4)
