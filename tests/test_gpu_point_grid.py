"""GPU: PointGrid and the grid routes of ball_query / knn_query (csrc/pgrid.hip): the index against the numpy model of
point_grid_reference.py, and the grid route == the brute-force route == the numpy models of the queries, bit for bit (tables with
array_equal, dist2 by its bits), on every scene of point_grid_cases.py and on the scenes of the brute-force routes' own tests."""
import numpy as np
import pytest
import torch

import point_grid_cases as cases
import point_grid_reference as ref
from d3d_amd import _lib
from d3d_amd.point import PointGrid, PointInterp, ball_query, knn_query, point_interpolate
from point_knn_reference import knn_model
from point_sample_reference import ball_model

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
CODE = {np.float32: _lib.F32, np.float64: _lib.F64}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def cloud():
    """one LiDAR-like cloud on a 1/64 grid the tests slice rows from (float64; a test casts it)"""
    rng = np.random.default_rng(51)
    pts = rng.uniform(-1.0, 1.0, (4096, 4)) * np.array([20.0, 20.0, 2.0, 1.0])
    return np.round(pts * 64) / 64


_MODELS = {}


def models(sc, dtype):
    """the numpy models of one scene in one dtype, computed once and shared: ball tables per (nsample, pad), kNN tables per k"""
    key = (sc["name"], dtype)
    if key not in _MODELS:
        pts, ctr = sc["points"].astype(dtype), sc["centers"].astype(dtype)
        wide = ball_model(pts, ctr, sc["radius"], 64, sc["poffs"], sc["coffs"])
        knn = knn_model(pts, ctr, 64, sc["poffs"], sc["coffs"])
        _MODELS[key] = dict(pts=pts, ctr=ctr, ball=wide, knn=knn)
    return _MODELS[key]


def ball_want(model, nsample, pad):
    """ball_model's answer for nsample <= 64 out of its 64-wide table (the first nsample inside rows are a prefix)"""
    table, counts = model["ball"]
    count = np.minimum(counts, nsample)
    out = table[:, :nsample].copy()
    if pad == "first":
        for c in range(len(out)):
            if count[c]:
                out[c, count[c]:] = out[c, 0]
    return out, count.astype(np.int32)


def knn_want(model, k):
    return model["knn"][0][:, :k], model["knn"][1][:, :k]


def build(sc, dtype, cell):
    return PointGrid(cuda(models(sc, dtype)["pts"]), cell, sc["poffs"], sc["cap"])


# ---------------------------------------------------------------- the index
@pytest.mark.parametrize("dtype", DTYPES)
def test_index_equals_the_model_on_every_scene(dtype):
    for sc in cases.scenes():
        pts = models(sc, dtype)["pts"]
        for cell in sc["cell_sizes"]:
            want = ref.grid_model(pts, cell, sc["poffs"], sc["cap"])
            grid = build(sc, dtype, cell)
            what = (sc["name"], cell)
            assert grid.num_cells == want["total"] and grid.num_points == len(pts), what
            assert grid.cell_size == tuple(g["h"] for g in want["plan"]) and grid.dims == tuple(g["dims"] for g in want["plan"]), what
            assert grid.bases == tuple(g["base"] for g in want["plan"]) and grid.lo == tuple(g["lo"] for g in want["plan"]), what
            assert np.array_equal(host(grid.mapping), want["mapping"]), what
            assert grid.order.dtype == torch.int32 and np.array_equal(host(grid.order), want["order"]), what
            assert grid.offsets.dtype == torch.int64 and np.array_equal(host(grid.offsets), want["offsets"]), what
            assert host(grid.packed).dtype == dtype and np.array_equal(bits(host(grid.packed)), bits(want["packed"])), what
    capped = [sc for sc in cases.scenes() if sc["name"] == "capped"][0]
    assert build(capped, dtype, 0.5).cell_size[0] >= 32.0                      # the cap doubled h


def test_bounds_entry_on_a_ragged_batch():
    sc = [s for s in cases.scenes() if s["name"] == "ragged"][0]
    for dtype in DTYPES:
        pts = sc["points"].astype(dtype)
        want_bounds, want_rows = ref.bounds_model(pts, sc["poffs"])
        s = len(sc["poffs"]) - 1
        p, offs = cuda(pts), torch.tensor(sc["poffs"]).cuda()
        for _ in range(2):                               # twice: the same bits
            bounds, rows = torch.full((s, 6), 7.0, dtype=torch.float64, device="cuda"), torch.full((s,), -3, dtype=torch.int64, device="cuda")
            rc = _lib.load().d3d_point_grid_bounds(_lib.ptr(p), len(pts), pts.shape[1], CODE[dtype], _lib.ptr(offs), s, _lib.ptr(bounds),
                                                   _lib.ptr(rows), _lib.stream_ptr())
            assert rc == _lib.OK and np.array_equal(host(rows), want_rows) and np.array_equal(bits(host(bounds)), bits(want_bounds))


# ---------------------------------------------------------------- ball query
@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_grid_equals_brute_force_and_model_on_every_scene(dtype):
    for sc in cases.scenes() + cases.borrowed_ball_scenes():
        model = models(sc, dtype)
        pts, ctr = cuda(model["pts"]), cuda(model["ctr"])
        for cell in sc["cell_sizes"]:
            grid = PointGrid(pts, cell, sc["poffs"], sc["cap"])
            for nsample in (1, 16, 63, 64):
                for pad in ("none", "first"):
                    what = (sc["name"], cell, nsample, pad)
                    table, counts = ball_query(grid, ctr, sc["radius"], nsample, center_offsets=sc["coffs"], pad=pad)
                    assert table.is_cuda and table.dtype == torch.int32 and table.shape == (len(model["ctr"]), nsample), what
                    brute = ball_query(pts, ctr, sc["radius"], nsample, sc["poffs"], sc["coffs"], pad=pad)
                    assert torch.equal(table, brute[0]) and torch.equal(counts, brute[1]), what
                    want = ball_want(model, nsample, pad)
                    assert np.array_equal(host(table), want[0]) and np.array_equal(host(counts), want[1]), what


def test_ball_grid_cluster_counts():
    """63 .. 257 candidates in one run of cells, 63 .. 257 rows inside one ball"""
    sc = [s for s in cases.scenes() if s["name"] == "clusters"][0]
    model = models(sc, np.float32)
    full, counts = ball_model(model["pts"], model["ctr"], sc["radius"], 300)
    assert counts.tolist() == list(cases.CLUSTERS)
    grid = build(sc, np.float32, 4.0)
    runs = (grid.offsets[1:] - grid.offsets[:-1]).cpu().tolist()
    assert sorted(r for r in runs if r) == [1] + sorted(cases.CLUSTERS)         # every cluster is one cell (and the lone row at lo)
    table, got = ball_query(grid, cuda(model["ctr"]), sc["radius"], 64)
    assert got.tolist() == [63, 64, 64, 64, 64, 64] and np.array_equal(host(table)[1:], full[1:, :64])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_grid_sizes_strides_host_and_numpy(cloud, dtype):
    rng = np.random.default_rng(52)
    r = 3.0
    for d, dc, m in ((3, 3, 1), (4, 3, 3), (5, 4, 4), (3, 5, 5), (4, 4, 67)):
        pts = np.concatenate([cloud[:1500, :3], rng.normal(size=(1500, d - 3))], 1).astype(dtype)
        ctr = np.concatenate([cloud[1500:1500 + m, :3], rng.normal(size=(m, dc - 3))], 1).astype(dtype)
        want = ball_model(pts, ctr, r, 16)
        grid = PointGrid(cuda(pts), r)
        table, counts = ball_query(grid, cuda(ctr), r, 16)
        assert np.array_equal(host(table), want[0]) and np.array_equal(host(counts), want[1]), (d, dc, m)
    wide = cuda(cloud[:1500].astype(dtype))                                      # a column slice of [N, 4] rows: read as it lies
    want = ball_model(cloud[:1500, :3].astype(dtype), cloud[:9, :3].astype(dtype), r, 16)
    table, counts = ball_query(PointGrid(wide[:, :3], 1.7), wide[:9, :3], r, 16)
    assert np.array_equal(host(table), want[0]) and np.array_equal(host(counts), want[1])
    pts, ctr = cloud[:1500].astype(dtype), cloud[:9, :3].astype(dtype)
    grid = PointGrid(pts, 2.0)                                                   # numpy in, numpy out: the side the points came from
    table, counts = ball_query(grid, ctr, r, 16)
    assert isinstance(table, np.ndarray) and isinstance(counts, np.ndarray) and np.array_equal(table, want[0]) and np.array_equal(counts, want[1])
    table, counts = ball_query(grid, cuda(ctr), r, 16, pad="first")
    assert isinstance(table, np.ndarray) and np.array_equal(table, ball_model(pts, ctr, r, 16, pad="first")[0])
    grid = PointGrid(torch.from_numpy(pts), 2.0)                                 # a host tensor: host tensors back
    table, counts = ball_query(grid, torch.from_numpy(ctr), r, 16)
    assert torch.is_tensor(table) and not table.is_cuda and not counts.is_cuda and np.array_equal(table.numpy(), want[0])
    nearest, _ = knn_query(grid, ctr, 3)
    assert torch.is_tensor(nearest) and not nearest.is_cuda and np.array_equal(nearest.numpy(), knn_model(pts, ctr, 3)[0])


def test_one_grid_three_radii_permuted_centres_and_repeat(cloud):
    pts, ctr = cloud[:4096].astype(np.float32), cloud[:300, :3].astype(np.float32) + np.float32(0.125)
    grid = PointGrid(cuda(pts), 1.0)
    for r in (0.4, 1.0, 3.5):                            # cells larger than, equal to and smaller than the ball
        want = ball_model(pts, ctr, r, 32)
        table, counts = ball_query(grid, cuda(ctr), r, 32)
        assert np.array_equal(host(table), want[0]) and np.array_equal(host(counts), want[1]), r
    perm = np.random.default_rng(53).permutation(len(ctr))
    table, counts = ball_query(grid, cuda(ctr), 1.0, 32)
    again = ball_query(grid, cuda(ctr[perm]), 1.0, 32)
    assert torch.equal(again[0], table[cuda(perm)]) and torch.equal(again[1], counts[cuda(perm)])
    near, dist2 = knn_query(grid, cuda(ctr), 16)
    again = knn_query(grid, cuda(ctr[perm]), 16)
    assert torch.equal(again[0], near[cuda(perm)]) and torch.equal(again[1].view(torch.int32), dist2[cuda(perm)].view(torch.int32))
    other = PointGrid(cuda(pts), 1.0)                    # two builds, two runs: the same bits
    assert torch.equal(other.mapping, grid.mapping) and torch.equal(other.order, grid.order) and torch.equal(other.offsets, grid.offsets)
    assert torch.equal(other.packed.view(torch.int32), grid.packed.view(torch.int32))
    twice = knn_query(other, cuda(ctr), 16)
    assert torch.equal(twice[0], near) and torch.equal(twice[1].view(torch.int32), dist2.view(torch.int32))


# ---------------------------------------------------------------- k nearest rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_grid_equals_brute_force_and_model_on_every_scene(dtype):
    """the scenes of the grid, and the brute-force route's own: tie lattices, duplicates, rows sorted by ascending and descending
    distance, fewer rows than k, rows and centres that are not finite, q = +inf, short and empty segments"""
    for sc in cases.scenes() + cases.borrowed_knn_scenes():
        model = models(sc, dtype)
        pts, ctr = cuda(model["pts"]), cuda(model["ctr"])
        for cell in sc["cell_sizes"][:2]:
            grid = PointGrid(pts, cell, sc["poffs"], sc["cap"])
            for k in (1, 3, 16, 63, 64):
                what = (sc["name"], cell, k)
                table, dist2 = knn_query(grid, ctr, k, center_offsets=sc["coffs"])
                assert table.is_cuda and table.dtype == torch.int32 and table.shape == dist2.shape == (len(model["ctr"]), k), what
                brute = knn_query(pts, ctr, k, sc["poffs"], sc["coffs"])
                assert torch.equal(table, brute[0]) and np.array_equal(bits(host(dist2)), bits(host(brute[1]))), what
                want = knn_want(model, k)
                assert np.array_equal(host(table), want[0]) and np.array_equal(bits(host(dist2)), bits(want[1])), what


@pytest.mark.parametrize("k", (1, 3, 16, 63, 64))
def test_knn_grid_rows_around_k(cloud, k):
    for n in sorted({1, 2, k - 1, k, k + 1, 65, 257} - {0}):
        for m in (1, 5):
            pts, ctr = cloud[:n].astype(np.float32), cloud[2000:2000 + m, :3].astype(np.float32)
            want = knn_model(pts, ctr, k)
            table, dist2 = knn_query(PointGrid(cuda(pts), 4.0), cuda(ctr), k)
            assert np.array_equal(host(table), want[0]) and np.array_equal(bits(host(dist2)), bits(want[1])), (n, m)


def test_raw_entries(cloud):
    pts, ctr = cloud[:700].astype(np.float32), cloud[700:740, :3].astype(np.float32)
    grid, c = PointGrid(cuda(pts), 2.5), cuda(ctr)
    lib = _lib.load()
    head = (_lib.ptr(c), 40, 3, _lib.F32, None, 1, _lib.ptr(grid._plan), _lib.ptr(grid._order), _lib.ptr(grid.offsets), _lib.ptr(grid._packed), 700)
    raw = torch.full((40, 6), -9, dtype=torch.int32, device="cuda")
    assert lib.d3d_knn_query_grid(*head, 6, _lib.ptr(raw), None, _lib.stream_ptr()) == _lib.OK                 # dist2 = NULL
    assert np.array_equal(host(raw), knn_model(pts, ctr, 6)[0])
    table, counts = torch.full((40, 16), -9, dtype=torch.int32, device="cuda"), torch.full((40,), -9, dtype=torch.int32, device="cuda")
    assert lib.d3d_ball_query_grid(*head, 6.0, 16, 1, _lib.ptr(table), _lib.ptr(counts), _lib.stream_ptr()) == _lib.OK
    want = ball_model(pts, ctr, 6.0, 16, pad="first")
    assert np.array_equal(host(table), want[0]) and np.array_equal(host(counts), want[1])
    assert lib.d3d_ball_query_grid(*head, 6.0, 65, 1, _lib.ptr(table), _lib.ptr(counts), _lib.stream_ptr()) == _lib.ERR_UNSUPPORTED


def test_interp_chain_through_the_grid(cloud):
    """PointGrid -> PointInterp -> point_interpolate in bf16: the chain without the grid, bit for bit"""
    known, unknown = cuda(cloud[:600, :3].astype(np.float32)), cuda(cloud[600:1600, :3].astype(np.float32))
    poffs, uoffs = [0, 250, 600], [0, 400, 1000]
    feats = torch.randn((600, 24), generator=torch.Generator().manual_seed(5)).cuda().bfloat16()
    for offs in ((None, None), (poffs, uoffs)):
        plain = PointInterp(known, unknown, k=3, known_offsets=offs[0], unknown_offsets=offs[1])
        through = PointInterp(PointGrid(known, 2.0, offs[0]), unknown, k=3, unknown_offsets=offs[1])
        assert through.num_known == 600 and torch.equal(through.table, plain.table)
        assert torch.equal(through.dist2.view(torch.int32), plain.dist2.view(torch.int32))
        assert torch.equal(through.weights.view(torch.int32), plain.weights.view(torch.int32))
        out, want = point_interpolate(feats, through), point_interpolate(feats, plain)
        assert out.dtype == torch.bfloat16 and torch.equal(out.view(torch.int16), want.view(torch.int16))
