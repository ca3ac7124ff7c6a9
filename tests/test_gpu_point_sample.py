"""GPU: furthest_point_sample and ball_query (csrc/psample.hip) against the numpy models of point_sample_reference.py, bit for bit:
indices, tables and counts with array_equal, distances by their bits.  Shapes sit around every boundary d3d_fps_plan reports."""
import ctypes

import numpy as np
import pytest
import torch

import point_sample_cases as cases
import point_sample_reference as ref
from d3d_amd import _lib
from d3d_amd.point import ball_query, furthest_point_sample

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
CODE = {np.float32: _lib.F32, np.float64: _lib.F64}
fps_boundaries = cases.fps_boundaries


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def gpu_fps(pts, m, offs=None):
    idx, dist = furthest_point_sample(torch.from_numpy(np.ascontiguousarray(pts)).cuda(), m, offs, return_distances=True)
    assert idx.is_cuda and dist.is_cuda and idx.dtype == torch.int64
    return idx.cpu().numpy(), dist.cpu().numpy()


def assert_fps(pts, m, offs=None, what=None):
    want_idx, want_dist = ref.fps_model(pts, m, offs)
    idx, dist = gpu_fps(pts, m, offs)
    assert np.array_equal(idx, want_idx), what
    assert dist.dtype == pts.dtype and np.array_equal(bits(dist), bits(want_dist)), what


def assert_ball(pts, ctr, r, nsample, poffs=None, coffs=None, what=None):
    for pad in ("none", "first"):
        want_table, want_counts = ref.ball_model(pts, ctr, r, nsample, poffs, coffs, pad)
        table, counts = ball_query(torch.from_numpy(np.ascontiguousarray(pts)).cuda(), torch.from_numpy(np.ascontiguousarray(ctr)).cuda(),
                                   float(r), nsample, poffs, coffs, pad=pad)
        assert table.is_cuda and table.dtype == torch.int32 and counts.dtype == torch.int32
        assert np.array_equal(counts.cpu().numpy(), want_counts), (what, pad)
        assert np.array_equal(table.cpu().numpy(), want_table), (what, pad)


@pytest.fixture(scope="module")
def cloud():
    """one LiDAR-like cloud the size tests slice their first n rows from (float64; a test casts it)"""
    rng = np.random.default_rng(5)
    big = max(cap for code in CODE.values() for _, cap in fps_boundaries(code)) + 1100
    pts = rng.uniform(-1.0, 1.0, (big, 4)) * np.array([50.0, 50.0, 2.0, 1.0])
    return np.round(pts * 64) / 64


# ---------------------------------------------------------------- furthest point sampling
@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_around_every_boundary(cloud, dtype):
    """wave, workgroup and every route's capacity (from d3d_fps_plan), each at -1, +0, +1; the LDS route also with a partly filled
    last plane row; the first size past the on-chip capacity streams"""
    bounds = fps_boundaries(CODE[dtype])
    sizes = {1, 2, 63, 64, 65, 1023, 1024, 1025}
    for _, cap in bounds:
        sizes |= {cap - 1, cap, cap + 1}
    sizes |= {bounds[-2][1] + 1024 + 37, bounds[-1][1] + 1024 + 37}
    lib = _lib.load()
    seen = set()
    for n in sorted(sizes):
        route, cap = ctypes.c_int32(), ctypes.c_int32()
        assert lib.d3d_fps_plan(n, CODE[dtype], ctypes.byref(route), ctypes.byref(cap)) == 0
        seen.add(route.value)
        assert_fps(cloud[:n].astype(dtype), 24, what=(n, route.value))
    assert seen == set(range(_lib.FPS_ROUTE_STREAM + 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_full_length(cloud, dtype):
    assert_fps(cloud[:4096].astype(dtype), 4096)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_more_samples_than_rows_and_one_sample(cloud, dtype):
    pts = cloud[:50].astype(dtype)
    idx, _ = gpu_fps(pts, 130)
    assert len(set(idx[:50].tolist())) == 50 and np.all(idx[50:] == 0)          # every row once, then the lowest row repeats
    assert_fps(pts, 130)
    assert_fps(pts, 1)
    assert_fps(cloud[:3000].astype(dtype), 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_scenes(dtype):
    big = fps_boundaries(CODE[dtype])[-1][1] + 1
    for name, pts, m, offs in cases.fps_scenes(big):
        assert_fps(pts.astype(dtype), m, offs, what=name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_view_with_an_element_aligned_base(dtype):
    """[N, 3] starting one row into an allocation: the base is aligned to 12 (24) bytes only"""
    scenes = {s[0]: s[1] for s in cases.fps_scenes(2000)}
    pts = scenes["lidar_d3"].astype(dtype)
    assert pts.shape[1] == 3
    full = torch.from_numpy(np.concatenate([np.zeros((1, 3), dtype), pts])).cuda()
    view = full[1:]
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    idx, dist = furthest_point_sample(view, 40, return_distances=True)
    want_idx, want_dist = ref.fps_model(pts, 40)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(bits(dist.cpu().numpy()), bits(want_dist))
    wide = torch.from_numpy(scenes["lidar_d5"].astype(dtype)).cuda()               # [N, 5]: columns 1 .. 3 as they lie
    idx = furthest_point_sample(wide[:, 1:4], 40)
    assert np.array_equal(idx.cpu().numpy(), ref.fps_model(wide[:, 1:4].cpu().numpy(), 40)[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_mixed_routes_in_one_call_equal_per_segment_calls(dtype):
    big = fps_boundaries(CODE[dtype])[-1][1] + 1
    name, pts, ms, offs = cases.fps_scenes(big)[-1]
    assert name == "mixed_routes"
    pts = pts.astype(dtype)
    idx, dist = gpu_fps(pts, ms, offs)
    at = 0
    for b, m in enumerate(ms):
        if m:
            one_idx, one_dist = gpu_fps(pts[offs[b]:offs[b + 1]], m)
            assert np.array_equal(idx[at:at + m], one_idx + offs[b]) and np.array_equal(bits(dist[at:at + m]), bits(one_dist)), b
        at += m
    assert at == len(idx)
    want_idx, want_dist = ref.fps_model(pts, ms, offs)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(dist), bits(want_dist))


def test_fps_host_and_numpy_in_and_out(cloud):
    pts = cloud[:700].astype(np.float32)
    want_idx, want_dist = ref.fps_model(pts, [10, 20], [0, 300, 700])
    idx, dist = furthest_point_sample(pts, [10, 20], np.array([0, 300, 700]), return_distances=True)
    assert isinstance(idx, np.ndarray) and isinstance(dist, np.ndarray) and idx.dtype == np.int64 and dist.dtype == np.float32
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(dist), bits(want_dist))
    idx = furthest_point_sample(torch.from_numpy(pts), torch.tensor([10, 20]), torch.tensor([0, 300, 700]))
    assert torch.is_tensor(idx) and not idx.is_cuda and np.array_equal(idx.numpy(), want_idx)
    idx = furthest_point_sample(torch.from_numpy(pts).cuda(), [10, 20], torch.tensor([0, 300, 700]).cuda())   # (offsets read back)
    assert idx.is_cuda and np.array_equal(idx.cpu().numpy(), want_idx)
    table, counts = ball_query(pts, pts[:5], 6.0, 8)
    assert isinstance(table, np.ndarray) and isinstance(counts, np.ndarray)
    want = ref.ball_model(pts, pts[:5], 6.0, 8)
    assert np.array_equal(table, want[0]) and np.array_equal(counts, want[1])
    table, counts = ball_query(torch.from_numpy(pts), torch.from_numpy(pts[:5]), 6.0, 8)
    assert not table.is_cuda and not counts.is_cuda and np.array_equal(table.numpy(), want[0])


def test_fps_repeats_its_bits(cloud):
    pts = torch.from_numpy(cloud[:5000].astype(np.float32)).cuda()
    first = furthest_point_sample(pts, 64, [0, 1000, 5000], return_distances=True)
    second = furthest_point_sample(pts, 64, [0, 1000, 5000], return_distances=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1].view(torch.int32), second[1].view(torch.int32))


def test_fps_raw_entry_without_distances(cloud):
    lib = _lib.load()
    pts_np = cloud[:900].astype(np.float32)
    pts = torch.from_numpy(pts_np).cuda()
    poffs, soffs = torch.tensor([0, 400, 900]).cuda(), torch.tensor([0, 7, 30]).cuda()
    idx = torch.full((30,), -5, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.d3d_fps_workspace_bytes(900, 2, _lib.F32), dtype=torch.uint8, device="cuda")
    rc = lib.d3d_furthest_point_sample(_lib.ptr(pts), 900, 4, _lib.F32, _lib.ptr(poffs), _lib.ptr(soffs), 2, _lib.ptr(idx), None,
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == _lib.OK
    assert np.array_equal(idx.cpu().numpy(), ref.fps_model(pts_np, [7, 23], [0, 400, 900])[0])


# ---------------------------------------------------------------- ball query
@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_query_around_tile_multiples(cloud, dtype):
    """a wavefront walks 64 rows per tile, 4 tiles per round"""
    ctr = cloud[[3, 40, 64, 100, 200, 255, 256, 500], :3].astype(dtype)
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):
        assert_ball(cloud[:n].astype(dtype), ctr, 40.0, 16, what=n)
        assert_ball(cloud[:n].astype(dtype), ctr, 40.0, 1024, what=n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_query_nsample_below_and_above_the_rows_inside(cloud, dtype):
    pts = cloud[:1500].astype(dtype)
    ctr = cloud[1500:1540, :3].astype(dtype)
    inside_small = ref.ball_model(pts, ctr, 6.0, 1024)[1]
    inside_all = ref.ball_model(pts, ctr, 500.0, 1500)[1]
    assert 1 < inside_small.min() < 16 < inside_small.max() < 33 and np.all(inside_all == 1500)
    for nsample in (1, 16, 33, 64, 1024):
        assert_ball(pts, ctr, 6.0, nsample, what=("small", nsample))
        assert_ball(pts, ctr, 500.0, nsample, what=("all", nsample))
    assert_ball(pts, ctr, 30.0, 33, what="middle")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_query_scenes(dtype):
    """points at exactly r (outside), empty balls, rows and centres that are not finite, ragged segments with an empty point segment"""
    for name, pts, ctr, r, poffs, coffs in cases.ball_scenes():
        for nsample in (5, 64):
            assert_ball(pts.astype(dtype), ctr.astype(dtype), r, nsample, poffs, coffs, what=(name, nsample))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_query_strides(cloud, dtype):
    rng = np.random.default_rng(6)
    for d in (3, 4, 5):
        for dc in (3, 4, 5):
            pts = np.concatenate([cloud[:300, :3], rng.normal(size=(300, d - 3))], 1).astype(dtype)
            ctr = np.concatenate([cloud[300:320, :3], rng.normal(size=(20, dc - 3))], 1).astype(dtype)
            assert_ball(pts, ctr, 25.0, 16, what=(d, dc))
    wide = torch.from_numpy(cloud[:300].astype(dtype)).cuda()                   # a column slice of [N, 4] rows: read as it lies
    table, counts = ball_query(wide[:, :3], wide[:7, :3], 25.0, 16)
    want = ref.ball_model(cloud[:300, :3].astype(dtype), cloud[:7, :3].astype(dtype), 25.0, 16)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])


def test_ball_query_raw_table_feeds_table_pool(cloud):
    """the raw entry with pad_first; its table goes straight into d3d_table_pool_forward (max): repeats of the first entry do not
    change a maximum, an empty ball gives the zero row"""
    lib = _lib.load()
    rng = np.random.default_rng(7)
    n, m, k, c = 1500, 30, 16, 8
    pts_np = cloud[:n].astype(np.float32)
    ctr_np = np.concatenate([cloud[n:n + m - 1, :3], [[900.0, 900.0, 900.0]]]).astype(np.float32)     # (the last ball is empty)
    feat_np = rng.normal(size=(n, c)).astype(np.float32)
    pts, ctr, feat = (torch.from_numpy(a).cuda() for a in (pts_np, ctr_np, feat_np))
    table = torch.full((m, k), -9, dtype=torch.int32, device="cuda")
    counts = torch.full((m,), -9, dtype=torch.int32, device="cuda")
    rc = lib.d3d_ball_query(_lib.ptr(pts), n, 4, _lib.ptr(ctr), m, 3, _lib.F32, None, None, 0, 6.0, k, 1, _lib.ptr(table), _lib.ptr(counts),
                            _lib.stream_ptr())
    assert rc == _lib.OK
    want_table, want_counts = ref.ball_model(pts_np, ctr_np, 6.0, k, pad="first")
    assert np.array_equal(table.cpu().numpy(), want_table) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert want_counts[-1] == 0 and want_counts.max() == k and 0 < want_counts[:-1].min() < k
    out = torch.empty((m, c), dtype=torch.float32, device="cuda")
    rc = lib.d3d_table_pool_forward(_lib.ptr(feat), n, c, _lib.F32, _lib.ptr(table), m, k, _lib.REDUCE_MAX, _lib.ptr(out), None, None,
                                    _lib.stream_ptr())
    assert rc == _lib.OK
    want = np.stack([feat_np[want_table[i, :want_counts[i]]].max(0) if want_counts[i] else np.zeros(c, np.float32) for i in range(m)])
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_then_ball_query(cloud, dtype):
    """every keypoint finds a row at distance 0 (itself, or a lower row with its coordinates) as the first entry of its ball"""
    pts_np = np.concatenate([cloud[:2500], cloud[100:600]]).astype(dtype)       # with duplicates
    pts = torch.from_numpy(pts_np).cuda()
    idx = furthest_point_sample(pts, 128)
    # coordinates lie on a 1/64 grid: within r = 1/128 of a keypoint are the rows with its coordinates and no others
    table, counts = ball_query(pts, pts[idx], 1.0 / 128, 16)
    first = table[:, 0].long()
    assert bool((counts >= 1).all()) and torch.equal(pts[first, :3], pts[idx, :3]) and bool((first <= idx).all())
    assert int(counts.max()) == 2 and int(counts.min()) == 1                    # (a duplicated row was picked: both copies are inside)
    # a wider ball holds the keypoint among its rows
    table, counts = ball_query(pts, pts[idx], 1.5, 16)
    assert bool(((table == idx[:, None]).any(1) | (counts == 16)).all())
    want = ref.ball_model(pts_np, pts_np[idx.cpu().numpy()], 1.5, 16)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
