"""GPU: RoiGrid, roiaware_pool3d, group_pool and roipoint_pool3d (csrc/roipool.hip, csrc/vtpool.hip) against the numpy models of
roi_pool_reference.py, bit for bit: tables with array_equal, floats by their bits (a NaN equal to any NaN).  The one exception is
gradcheck (fp64, torch's defaults)."""
import numpy as np
import pytest
import torch

import oracle
import roi_pool_cases as cases
import roi_pool_reference as ref
import sparse_pool_reference as pref
from d3d_amd.point import (RoiGrid, ball_query, furthest_point_sample, group_pool, knn_query, roi_grid_max_cells, roi_grid_plan,
                           roiaware_pool3d, roipoint_pool3d)

pytestmark = pytest.mark.gpu
F = np.float32
PADS = ("none", "cycle")
SPECIAL = dict(cases.special_scenes())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_grid(sc, pad="none", max_points=None, out_size=None, points=None, what=None):
    """the three outputs of a RoiGrid over the scene against the model; -> (grid, (table, counts, inside) of the model)"""
    p = sc.max_points if max_points is None else max_points
    size = sc.out_size if out_size is None else out_size
    want = ref.grid_model(sc.points, sc.boxes, size, p, sc.point_offsets, sc.box_offsets, pad)
    grid = RoiGrid(cuda(sc.points) if points is None else points, cuda(sc.boxes), size, p, sc.point_offsets, sc.box_offsets, pad)
    m, dims = len(sc.boxes), ref.triple(size)
    g = dims[0] * dims[1] * dims[2]
    assert grid.table.is_cuda and grid.table.dtype == grid.counts.dtype == grid.inside.dtype == torch.int32
    assert grid.table.shape == (m,) + dims + (p,) and grid.counts.shape == (m,) + dims and grid.inside.shape == (m,)
    assert (grid.num_points, grid.num_boxes, grid.out_size, grid.max_points_per_cell) == (len(sc.points), m, dims, p)
    assert np.array_equal(grid.inside.cpu().numpy(), want[2]), (what, "inside")
    assert np.array_equal(grid.counts.cpu().numpy().reshape(m, g), want[1]), (what, "counts")
    assert np.array_equal(grid.table.cpu().numpy().reshape(m, g, p), want[0]), (what, "table")
    return grid, want


@pytest.fixture(scope="module")
def cloud():
    """4096 rows around six boxes: the tests slice segments off its front"""
    return cases.random_scene(4096, 6, 51, out_size=3, max_points=16, spread=4.0)


# ---------------------------------------------------------------- the table
def test_table_segment_lengths_around_the_plan(cloud):
    lengths = {1, 2}
    for base in (64, 512, 1500, 4096):
        tile, slab, rnd = roi_grid_plan(base, 27)
        lengths |= {tile - 1, tile, tile + 1, slab - 1, slab, slab + 1, 2 * slab - 1, 2 * slab, 2 * slab + 1, rnd - 1, rnd, rnd + 1}
    assert {63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049} <= lengths and max(lengths) <= 4096
    for n in sorted(lengths):
        for pad in PADS:
            assert_grid(cases.scene(cloud.points[:n], cloud.boxes, 3, 16), pad, what=(n, pad))


def test_table_empty_inputs(cloud):
    grid, _ = assert_grid(cases.scene(np.zeros((0, 3), F), cloud.boxes, 3, 4))
    assert int(grid.inside.sum()) == 0 and bool((grid.table == -1).all())
    grid, _ = assert_grid(cases.scene(cloud.points[:100], np.zeros((0, 7), F), 3, 4))
    assert grid.table.shape == (0, 3, 3, 3, 4) and grid.transpose().order.numel() == 0
    out = roiaware_pool3d(torch.zeros(100, 5).cuda(), grid)
    assert out.shape == (0, 3, 3, 3, 5)
    for pad in PADS:
        assert_grid(SPECIAL["ragged"], pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("p", (1, 2, 128, 1024))
def test_table_caps(cloud, p, pad):
    for size in (1, 2):
        assert_grid(cloud, pad, max_points=p, out_size=size, what=(p, size))


@pytest.mark.parametrize("pad", PADS)
def test_table_grids(cloud, pad):
    for size in (1, (1, 2, 3), (3, 2, 1), 12):
        assert_grid(cases.scene(cloud.points[:1500], cloud.boxes, size, 8), pad, what=size)
    assert 16 ** 3 == roi_grid_max_cells()
    big = cases.random_scene(4096, 2, 52, out_size=16, max_points=128, spread=2.0)      # G = 4096, once, with two boxes
    grid, want = assert_grid(big, pad)
    assert (want[1] > 0).sum() > 300


def test_table_strides_and_views(cloud):
    rng = np.random.default_rng(53)
    xyz = cloud.points[:700, :3]
    want = ref.grid_model(xyz, cloud.boxes, 3, 16)
    for d in (3, 4, 5):
        pts = np.concatenate([xyz, rng.normal(size=(700, d - 3)).astype(F)], 1)
        assert_grid(cases.scene(pts, cloud.boxes, 3, 16), what=d)
        flat = torch.zeros(700 * d + 1, dtype=torch.float32).cuda()
        flat[1:] = cuda(pts).view(-1)
        view = flat[1:].view(700, d)                                               # a base aligned to one element only
        assert view.data_ptr() % 16 == 4
        assert_grid(cases.scene(pts, cloud.boxes, 3, 16), points=view, what=("view", d))
    wide = cuda(np.concatenate([xyz, rng.normal(size=(700, 2)).astype(F)], 1))
    grid = RoiGrid(wide[:, :3], cuda(cloud.boxes), 3, 16)                          # a column slice of [N, 5] rows: read as it lies
    assert np.array_equal(grid.table.cpu().numpy().reshape(want[0].shape), want[0])
    host = RoiGrid(np.ascontiguousarray(xyz), cloud.boxes, 3, 16)                  # numpy in: the grid still lives on the GPU
    assert host.table.is_cuda and np.array_equal(host.table.cpu().numpy().reshape(want[0].shape), want[0])


@pytest.mark.parametrize("name,sc", cases.angle_scenes())
def test_table_angles(name, sc):
    for pad in PADS:
        _, want = assert_grid(sc, pad, what=name)
    assert want[2].min() > 0


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_table_special_scenes(name, pad):
    sc = SPECIAL[name]
    _, want = assert_grid(sc, pad, what=name)
    if name == "nonfinite_points":                       # the NaN z row: inside for crop_points, a member of nothing here
        assert not (want[0] == sc.nan_z_row).any()
    if name in ("early_cap", "overflow", "two_cells", "cap"):
        assert (want[1] == sc.max_points).any()


@pytest.mark.parametrize("name", ("r_small", "r_mid", "r_big"))
def test_table_random_scenes(name):
    sc = cases.random_scene(*cases.RANDOM_SCENES[name])
    assert_grid(sc, what=name)


def test_table_agrees_with_crop_points():
    """with P large enough the union of a box's cells, and inside, are crop_points on the finite rows"""
    for sc in (SPECIAL["nonfinite_points"], SPECIAL["faces"], SPECIAL["bad_boxes"], cases.random_scene(2000, 12, 54, spread=6.0)):
        grid = RoiGrid(cuda(sc.points), cuda(sc.boxes), 2, 1024)
        xyz = np.ascontiguousarray(sc.points[:, :3])
        mask = oracle.crop_points(sc.boxes, xyz) & np.isfinite(xyz).all(1)[None, :]
        table = grid.table.cpu().numpy().reshape(len(sc.boxes), -1)
        assert np.array_equal(grid.inside.cpu().numpy(), mask.sum(1))
        for i in range(len(sc.boxes)):
            got = np.sort(table[i][table[i] >= 0])
            assert np.array_equal(got, np.flatnonzero(mask[i])), i
        assert np.array_equal(grid.counts.cpu().numpy().reshape(len(sc.boxes), -1).sum(1), mask.sum(1))


def test_table_rows_follow_their_boxes_and_runs_repeat():
    sc = cases.random_scene(3000, 32, 55, out_size=4, max_points=32, spread=6.0)
    pts, boxes = cuda(sc.points), cuda(sc.boxes)
    a = RoiGrid(pts, boxes, 4, 32, pad="cycle")
    b = RoiGrid(pts, boxes, 4, 32, pad="cycle")
    for x, y in ((a.table, b.table), (a.counts, b.counts), (a.inside, b.inside)):
        assert torch.equal(x, y)
    perm = torch.from_numpy(np.random.default_rng(56).permutation(32)).cuda()
    c = RoiGrid(pts, boxes[perm], 4, 32, pad="cycle")
    assert torch.equal(c.table, a.table[perm]) and torch.equal(c.counts, a.counts[perm]) and torch.equal(c.inside, a.inside[perm])


# ---------------------------------------------------------------- the pooling and its gradient
class Pooled:
    """one scene of overlapping boxes, its grid on the GPU and the model's table"""

    def __init__(self):
        self.sc = sc = cases.random_scene(600, 6, 57, out_size=3, max_points=8, spread=2.0)
        self.n = len(sc.points)
        self.table = ref.grid_model(sc.points, sc.boxes, 3, 8)[0]
        self.grid = RoiGrid(cuda(sc.points), cuda(sc.boxes), 3, 8)
        named = np.bincount(self.table[self.table >= 0], minlength=self.n)
        assert named.max() >= 3 and (named == 0).any()                             # a gradient of >= 3 terms, and rows nobody names
        assert ref.members(sc.points, sc.boxes).sum(0).max() >= 3

    def values(self, data, c, seed):
        rng = np.random.default_rng(seed)
        if data == "random":
            return rng.normal(size=(self.n, c))
        x = rng.integers(-3, 4, (self.n, c)).astype(np.float64)                    # small integers: ties, and every sum exact
        if data == "special":
            x[rng.random((self.n, c)) < 0.05] = np.nan
            x[rng.random((self.n, c)) < 0.1] = -0.0
        return x


@pytest.fixture(scope="module")
def pooled():
    return Pooled()


def check_pool(fn, table, n, values, grads, reduction, kind, view=None):
    """fn(features on the GPU) -> pooled rows; forward and gradient against the model"""
    t, x = pref.of_kind(values, kind)
    g_t, g_x = pref.of_kind(grads, kind)
    want, arg, count = ref.pool_forward(x, table, reduction, kind)
    want_grad = ref.pool_backward(g_x, table, n, reduction, kind, arg, count)
    feat = (t.cuda() if view is None else view(t)).requires_grad_()
    out = fn(feat)
    c = t.shape[1]
    assert out.is_cuda and out.dtype == t.dtype
    assert pref.equal_bits(out.detach().cpu().reshape(-1, c), pref.to_tensor(want, kind)), "forward"
    out.backward(g_t.cuda().view_as(out))
    assert pref.equal_bits(feat.grad.cpu(), pref.to_tensor(want_grad, kind)), "backward"


@pytest.mark.parametrize("kind", pref.KINDS)
@pytest.mark.parametrize("reduction", pref.REDUCTIONS)
def test_roiaware_pool(pooled, reduction, kind):
    rows = pooled.table.shape[0] * pooled.table.shape[1]
    for k, data in enumerate(("integers", "random", "special")):
        for c in (1, 3, 4, 16):
            rng = np.random.default_rng(100 + c)
            grads = rng.integers(-2, 3, (rows, c)).astype(np.float64) if data != "random" else rng.normal(size=(rows, c))
            check_pool(lambda f: roiaware_pool3d(f, pooled.grid, reduction), pooled.table, pooled.n, pooled.values(data, c, 60 + k), grads,
                       reduction, kind)


@pytest.mark.parametrize("kind", pref.KINDS)
def test_roiaware_pool_wide_rows_and_misaligned_views(pooled, kind):
    rows = pooled.table.shape[0] * pooled.table.shape[1]
    rng = np.random.default_rng(61)
    for reduction in ("max", "mean"):
        check_pool(lambda f: roiaware_pool3d(f, pooled.grid, reduction), pooled.table, pooled.n, pooled.values("random", 260, 62),
                   rng.normal(size=(rows, 260)), reduction, kind)

        def view(t):                                   # the same rows at a base that is aligned to one element only
            flat = torch.zeros(t.numel() + 1, dtype=t.dtype).cuda()
            flat[1:] = t.cuda().view(-1)
            v = flat[1:].view(t.shape)
            assert v.data_ptr() % 16 != 0
            return v.detach()
        check_pool(lambda f: roiaware_pool3d(f, pooled.grid, reduction), pooled.table, pooled.n, pooled.values("random", 8, 63),
                   rng.normal(size=(rows, 8)), reduction, kind, view)


def test_roiaware_pool_fronts(pooled):
    feat = np.random.default_rng(64).normal(size=(pooled.n, 4)).astype(F)
    want = pref.to_tensor(ref.pool_forward(feat, pooled.table, "max", "f32")[0], "f32").numpy().reshape(6, 3, 3, 3, 4)
    out = roiaware_pool3d(feat, pooled.grid)                                       # numpy in, numpy out
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    out = roiaware_pool3d(torch.from_numpy(feat), pooled.grid, "MAX")              # host in, host out
    assert not out.is_cuda and np.array_equal(out.numpy(), want)
    with pytest.raises(ValueError):
        roiaware_pool3d(feat[:-1], pooled.grid)
    with pytest.raises(ValueError):
        roiaware_pool3d(feat, pooled.grid, "median")
    wide = RoiGrid(cuda(pooled.sc.points), cuda(pooled.sc.boxes), 1, 344)
    with pytest.raises(ValueError):
        roiaware_pool3d(feat, wide)
    order, offsets = pooled.grid.transpose().order, pooled.grid.transpose().offsets
    assert order.dtype == torch.int32 and offsets.dtype == torch.int64 and offsets.shape == (pooled.n + 1,)
    assert order.numel() == int((pooled.table >= 0).sum()) == int(offsets[-1]) and pooled.grid.transpose().order is order
    flat = pooled.table.reshape(-1)
    assert np.array_equal(flat[order.cpu().numpy()], np.repeat(np.arange(pooled.n), np.diff(offsets.cpu().numpy())))


@pytest.mark.parametrize("reduction", pref.REDUCTIONS)
def test_roiaware_pool_gradcheck(reduction):
    sc = cases.random_scene(40, 2, 65, out_size=2, max_points=4, spread=1.5)
    grid = RoiGrid(cuda(sc.points), cuda(sc.boxes), 2, 4)
    assert int(grid.counts.sum()) > 8
    feat = torch.from_numpy(np.random.default_rng(66).permutation(80).reshape(40, 2) / 8.0).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda f: roiaware_pool3d(f, grid, reduction), (feat,))


@pytest.mark.parametrize("kind", pref.KINDS)
@pytest.mark.parametrize("reduction", pref.REDUCTIONS)
def test_group_pool_on_query_tables(cloud, reduction, kind):
    pts = cuda(cloud.points[:800])
    idx = furthest_point_sample(pts, 40)
    ball, counts = ball_query(pts, pts[idx], 0.8, 16, pad="first")
    knn = knn_query(pts, pts[idx], 16, return_distances=False)
    assert int(counts.min()) < 16                                                  # some ball is padded with its first entry
    rng = np.random.default_rng(67)
    for table in (ball, knn):
        for c in (3, 8):
            check_pool(lambda f: group_pool(f, table, reduction), table.cpu().numpy(), 800, rng.integers(-3, 4, (800, c)).astype(np.float64),
                       rng.normal(size=(40, c)), reduction, kind)
    with pytest.raises(ValueError):
        group_pool(torch.zeros(10, 3).cuda(), ball, reduction)                     # rows 10 .. 799 are out of range


# ---------------------------------------------------------------- roipoint_pool3d
@pytest.mark.parametrize("kind", pref.KINDS)
def test_roipoint_pool(kind):
    sc = SPECIAL["overlap"]
    n = len(sc.points)
    inside = ref.members(sc.points, sc.boxes).sum(1)
    rng = np.random.default_rng(68)
    t, x = pref.of_kind(rng.integers(-8, 9, (n, 5)).astype(np.float64), kind)
    for s in (3, 64, 512):
        assert inside[3] == 0 and 3 < inside[:3].min() and inside[:3].max() < 512            # S above and below inside, an empty box
        want, empty, table = ref.roipoint_model(sc.points, t.numpy() if kind in ("f32", "f64") else x, sc.boxes, s)
        feat = t.cuda().requires_grad_()
        pooled, got_empty = roipoint_pool3d(cuda(sc.points), feat, cuda(sc.boxes), s)
        assert pooled.shape == (4, s, 8) and pooled.dtype == t.dtype and got_empty.dtype == torch.bool
        assert got_empty.cpu().numpy().tolist() == empty.tolist()
        want_t = torch.from_numpy(np.ascontiguousarray(want)).to(t.dtype)
        assert pref.equal_bits(pooled.detach().cpu().reshape(-1, 8), want_t.reshape(-1, 8))
        # the gradient against torch's autograd of the dense gather: exact on integer data
        g_t, _ = pref.of_kind(rng.integers(-2, 3, (4, s, 8)).astype(np.float64), kind)
        pooled.backward(g_t.cuda())
        leaf = t.to(torch.float64).clone().requires_grad_()
        rows = torch.from_numpy(np.maximum(table, 0).astype(np.int64))
        dense = torch.where(torch.from_numpy(table >= 0)[:, :, None], leaf[rows], torch.zeros(()).double())
        dense.backward(g_t[:, :, 3:].double())
        assert torch.equal(feat.grad.cpu(), leaf.grad.to(t.dtype))                  # (integers: every partial sum is exact in fp32)


def test_roipoint_pool_ragged_and_numpy():
    sc = SPECIAL["ragged"]
    feat = np.random.default_rng(69).normal(size=(len(sc.points), 3)).astype(F)
    want, empty, _ = ref.roipoint_model(sc.points, feat, sc.boxes, 32, sc.point_offsets, sc.box_offsets)
    pooled, got_empty = roipoint_pool3d(sc.points, feat, sc.boxes, 32, sc.point_offsets, sc.box_offsets)
    assert isinstance(pooled, np.ndarray) and np.array_equal(pooled, want) and got_empty.tolist() == empty.tolist() and empty.any()


# ---------------------------------------------------------------- one chain
def test_chain_fps_grid_pool_linear():
    sc = cases.random_scene(3000, 4, 70, d=4, spread=8.0)
    pts = cuda(sc.points)
    idx = furthest_point_sample(pts, 24)
    boxes = torch.cat([pts[idx, :3], torch.tensor([4.2, 1.8, 1.6], device="cuda").expand(24, 3),
                       torch.linspace(-3.0, 3.0, 24, device="cuda")[:, None]], 1)
    grads = []
    for _ in range(2):
        torch.manual_seed(71)
        layer = torch.nn.Linear(16, 8).cuda().to(torch.bfloat16)
        feat = torch.randn(3000, 16, device="cuda").to(torch.bfloat16).requires_grad_()
        grid = RoiGrid(pts, boxes, 6, 32)
        out = layer(roiaware_pool3d(feat, grid, "max").view(-1, 16))
        out.float().square().sum().backward()
        assert int(grid.inside.min()) > 0 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(feat.grad).all())
        assert float(feat.grad.float().abs().sum()) > 0
        grads.append((out.detach().clone(), feat.grad.clone(), layer.weight.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
