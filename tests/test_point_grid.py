"""CPU: d3d_point_grid_plan against the numpy model of the grid; the two facts the grid routes rest on -- every row inside a ball lies
in the box of cells the ball query walks, every one of the k nearest rows in the rings the kNN walks before its bound stops it --
on every scene, against ball_model / knn_model; and every host-side refusal of the C entries and of the Python layer.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import point_grid_cases as cases
import point_grid_reference as ref
from d3d_amd import _lib
from d3d_amd.point import PointGrid, PointInterp, ball_query, grid_plan, knn_query
from d3d_amd.point.grid import _Segment
from point_knn_reference import knn_model
from point_sample_reference import ball_model

DTYPES = (np.float32, np.float64)
ALL_SCENES = cases.scenes() + cases.borrowed_ball_scenes() + cases.borrowed_knn_scenes()


def _segment_of(offs, c):
    return 0 if offs is None else int(np.searchsorted(np.asarray(offs), c, side="right")) - 1


def _plan_matches(points, sc, cell):
    bounds, rows = ref.bounds_model(points, sc["poffs"])
    want, want_total = ref.plan_model(bounds, rows, cell, sc["cap"])
    got, total = grid_plan(bounds, rows, cell, sc["cap"])
    assert total == want_total and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (sc["name"], cell, g, w)              # lo, h, inv_h as the same doubles; dims and base as the same ints
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_equals_the_model_on_every_scene(dtype):
    for sc in ALL_SCENES:
        pts = sc["points"].astype(dtype)
        for cell in sc["cell_sizes"]:
            plan = _plan_matches(pts, sc, cell)
            assert _plan_matches(pts, sc, cell) == plan                          # pure: the same answer again
            for g in plan:
                cells = g["dims"][0] * g["dims"][1] * g["dims"][2]
                assert g["h"] >= cell and np.log2(g["h"] / cell) == np.round(np.log2(g["h"] / cell)) and g["inv_h"] == 1.0 / g["h"]
                assert all(d >= 1 for d in g["dims"]) and cells <= 8 * max(64, sc["cap"] * len(pts))
    capped = [sc for sc in ALL_SCENES if sc["name"] == "capped"][0]
    plan = _plan_matches(capped["points"].astype(dtype), capped, 0.5)
    assert plan[0]["h"] >= 32.0 and plan[0]["dims"][0] * plan[0]["dims"][1] * plan[0]["dims"][2] <= 100   # 0.5 doubled six times and more
    huge = [sc for sc in ALL_SCENES if sc["name"] == "huge"][0]
    assert _plan_matches(huge["points"].astype(dtype), huge, 1.0)[0]["h"] >= 2.0 ** 60


def test_plan_is_monotone_and_refuses():
    bounds, rows = np.array([[0.0, -1.0, 2.0, 10.0, 7.5, 2.0]]), np.array([1000])
    last = None
    for cell in [0.013 * 2 ** j for j in range(14)]:                             # up one ladder of doublings: never more cells
        plan, total = grid_plan(bounds, rows, cell)
        cells = int(np.prod(plan[0]["dims"]))
        assert total == cells + 1 and cells <= 2000 and (last is None or cells <= last) and plan[0]["dims"][2] == 1
        last = cells
    # extents 10, 8.5 and 0: 11 x 9 x 1 cells of 1 fit a cap of 100 (and of 1000), a cap of 64 doubles h once: 6 x 5 x 1
    assert [grid_plan(bounds, rows, 1.0, cap)[1] for cap in (0.01, 0.1, 1.0)] == [6 * 5 * 1 + 1, 11 * 9 * 1 + 1, 11 * 9 * 1 + 1]
    plan, total = grid_plan(np.zeros((3, 6)), [0, 5, 0], 0.5)                    # no finite row: lo = 0, one cell; and zero extent
    assert [g["dims"] for g in plan] == [(1, 1, 1)] * 3 and [g["base"] for g in plan] == [0, 2, 4] and total == 6
    assert grid_plan(np.zeros((0, 6)), [], 1.0) == ([], 0)
    wide = np.array([[0.0, 0.0, 0.0, 1e6, 1e6, 1e6]])
    with pytest.raises(ValueError, match="2\\^31"):                              # one segment above 2^31 - 1 cells
        grid_plan(wide, [2 ** 31 - 1], 1.0, 4.0)
    # 2^30 rows, a cap of 1.5 * 2^30: h = 1024, 977^3 = 0.93e9 cells a segment -- two fit below 2^31, the sum of three does not
    with pytest.raises(ValueError, match="2\\^31"):
        grid_plan(np.concatenate([wide] * 3), [2 ** 30] * 3, 1.0, 1.5)
    with pytest.raises(ValueError):
        ref.plan_model(np.concatenate([wide] * 3), [2 ** 30] * 3, 1.0, 1.5)
    assert grid_plan(np.concatenate([wide] * 2), [2 ** 30] * 2, 1.0, 1.5)[1] == 2 * (977 ** 3 + 1)
    with pytest.raises(ValueError, match="2\\^31"):                              # fp64 rows at both ends of the range
        grid_plan(np.array([[-1.5e308, 0, 0, 1.5e308, 0, 0]]), [2], 1.0)
    for kw in (dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=float("nan")), dict(cell_size=float("inf")), dict(cell_size="1"),
               dict(cell_size=True), dict(max_cells_per_point=0.0), dict(max_cells_per_point=float("inf")), dict(finite_rows=[-1]),
               dict(bounds=np.array([[0.0, 0, 0, -1.0, 0, 0]])), dict(bounds=np.array([[0.0, 0, 0, np.nan, 0, 0]])),
               dict(bounds=np.zeros((2, 6)))):
        with pytest.raises(ValueError):
            grid_plan(**dict(dict(bounds=bounds, finite_rows=rows, cell_size=1.0, max_cells_per_point=2.0), **kw))


def test_the_cell_of_a_coordinate_is_monotone():
    rng = np.random.default_rng(43)
    for inv_h, dim in ((1.0, 7), (3.7, 100), (2.0 ** -60, 4), (1e3, 2 ** 31 - 1)):
        t = np.sort(np.concatenate([rng.uniform(-3, dim + 3, 400) / inv_h, np.arange(-2, 9) / inv_h, [-np.inf, np.inf, 0.0, -0.0]]))
        cells = [ref.cell_rel(v, inv_h, dim) for v in t]
        assert cells == sorted(cells) and cells[0] == 0 and cells[-1] == dim - 1
    assert ref.cell_rel(np.nan, 1.0, 5) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ball_box_holds_every_inside_row(dtype):
    """what d3d_ball_query_grid rests on: ball_model's inside rows (all of them: nsample = n) are among the rows of the box"""
    checked = 0
    for sc in ALL_SCENES:
        pts, ctr = sc["points"].astype(dtype), sc["centers"].astype(dtype)
        for radius in (sc["radius"], sc["radius"] * 0.37):
            table, counts = ball_model(pts, ctr, radius, max(len(pts), 1), sc["poffs"], sc["coffs"])
            for cell in sc["cell_sizes"]:
                grid = ref.grid_model(pts, cell, sc["poffs"], sc["cap"])
                for c in range(len(ctr)):
                    inside = table[c, :counts[c]]
                    got = ref.ball_candidates(grid, _segment_of(sc["coffs"], c), ctr[c], radius, dtype)
                    missing = np.setdiff1d(inside, got)
                    assert len(missing) == 0, (sc["name"], cell, radius, c, missing)
                    checked += len(inside)
    assert checked > 10000


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_knn_rings_hold_the_k_nearest_rows(dtype):
    """what d3d_knn_query_grid rests on: knn_model's entries are among the rows the rings (and the overflow cell) give before the
    bound stops the walk; and the bound does stop it where the cloud allows"""
    early = 0
    for sc in ALL_SCENES:
        pts, ctr = sc["points"].astype(dtype), sc["centers"].astype(dtype)
        for k in (1, 3, 16, 64):
            table, _ = knn_model(pts, ctr, k, sc["poffs"], sc["coffs"])
            for cell in sc["cell_sizes"][:2]:
                grid = ref.grid_model(pts, cell, sc["poffs"], sc["cap"])
                for c in range(len(ctr)):
                    s = _segment_of(sc["coffs"], c)
                    got, rings = ref.knn_candidates(grid, s, ctr[c], k, pts, dtype)
                    want = table[c][table[c] >= 0]
                    missing = np.setdiff1d(want, got)
                    assert len(missing) == 0, (sc["name"], cell, k, c, missing)
                    early += rings < max(grid["plan"][s]["dims"])
    assert early > 500


def test_grid_model_index_is_the_inverted_mapping():
    for sc in cases.scenes():
        grid = ref.grid_model(sc["points"].astype(np.float32), sc["cell_sizes"][0], sc["poffs"], sc["cap"])
        m, order, offs = grid["mapping"], grid["order"], grid["offsets"]
        assert len(offs) == grid["total"] + 1 and offs[-1] == len(order) == (m >= 0).sum() and m.max(initial=-1) < grid["total"]
        for cell in np.unique(m[m >= 0]):
            rows = order[offs[cell]:offs[cell + 1]]
            assert np.array_equal(rows, np.nonzero(m == cell)[0])                # ascending row inside a cell
        nan = np.isnan(sc["points"][:, :3].astype(np.float32)).any(1)
        inf = np.isinf(sc["points"][:, :3].astype(np.float32)).any(1) & ~nan
        assert np.array_equal(m < 0, nan)
        over = {g["base"] + int(np.prod(g["dims"])) for g in grid["plan"]}
        assert all(int(v) in over for v in m[inf]) and not any(int(v) in over for v in m[~inf & ~nan])


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """pointers that are never followed: each call returns before its first HIP call"""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    bad, uns, ws = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE

    def call(fn, names, **k):
        return getattr(lib, fn)(*[k.get(a, v) for a, v in names])

    bnd = (("points", p), ("n", 10), ("stride", 3), ("dtype", _lib.F32), ("poffs", None), ("segments", 0), ("bounds", p), ("rows", p),
           ("stream", None))
    for wrong in (dict(n=-1), dict(segments=-1), dict(stride=2), dict(poffs=p, segments=0), dict(bounds=None), dict(rows=None), dict(points=None)):
        assert call("d3d_point_grid_bounds", bnd, **wrong) == bad, wrong
    for wrong in (dict(dtype=_lib.F16), dict(dtype=_lib.BF16), dict(n=2 ** 31), dict(poffs=p, segments=2 ** 31)):
        assert call("d3d_point_grid_bounds", bnd, **wrong) == uns, wrong
    assert call("d3d_point_grid_bounds", bnd, n=0, poffs=p, segments=0, points=None, bounds=None, rows=None) == _lib.OK

    total = ctypes.c_int64()
    b6, r1, seg = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1), (ctypes.c_int64 * 1)(8), (_Segment * 1)()
    pln = (("bounds", b6), ("rows", r1), ("segments", 1), ("cell", 0.5), ("cap", 2.0), ("plan", ctypes.addressof(seg)), ("total", ctypes.byref(total)))
    plan_call = lambda **k: lib.d3d_point_grid_plan(*[ctypes.addressof(v) if isinstance(v, ctypes.Array) else v  # noqa: E731
                                                      for v in (k.get(a, d) for a, d in pln)])
    assert plan_call() == _lib.OK and total.value == 3 * 3 * 3 + 1 and tuple(seg[0].dim) == (3, 3, 3) and seg[0].h == 0.5
    for wrong in (dict(segments=-1), dict(bounds=None), dict(rows=None), dict(plan=None), dict(total=None), dict(cell=0.0), dict(cell=float("nan")),
                  dict(cap=-1.0), dict(cap=float("inf")), dict(rows=(ctypes.c_int64 * 1)(-1)), dict(bounds=(ctypes.c_double * 6)(0, 0, 0, -1, 0, 0))):
        assert plan_call(**wrong) == bad, wrong
    assert plan_call(segments=2 ** 31) == uns
    assert plan_call(segments=0, bounds=None, rows=None, plan=None) == _lib.OK and total.value == 0

    assert lib.d3d_point_grid_workspace_bytes(1000, 300) == lib.d3d_voxel_index_workspace_bytes(1000, 300) > 0
    bld = (("points", p), ("n", 10), ("stride", 3), ("dtype", _lib.F32), ("poffs", None), ("segments", 0), ("plan", p), ("total", 28), ("mapping", p),
           ("order", p), ("offsets", p), ("counts", p), ("packed", p), ("ws", p), ("ws_bytes", 1 << 20), ("stream", None))
    for wrong in (dict(n=-1), dict(segments=-1), dict(stride=1), dict(total=0), dict(poffs=p, segments=0), dict(plan=None), dict(offsets=None),
                  dict(counts=None), dict(points=None), dict(mapping=None), dict(order=None), dict(packed=None)):
        assert call("d3d_point_grid_build", bld, **wrong) == bad, wrong
    for wrong in (dict(dtype=_lib.F16), dict(n=2 ** 31), dict(total=2 ** 31), dict(poffs=p, segments=2 ** 31)):
        assert call("d3d_point_grid_build", bld, **wrong) == uns, wrong
    for wrong in (dict(ws=None), dict(ws_bytes=16)):
        assert call("d3d_point_grid_build", bld, **wrong) == ws, wrong

    head = (("centers", p), ("m", 4), ("cstride", 3), ("dtype", _lib.F32), ("coffs", None), ("segments", 0), ("plan", p), ("order", p),
            ("cells", p), ("packed", p), ("n", 10))
    bq = head + (("radius", 1.0), ("nsample", 8), ("pad", 0), ("table", p), ("counts", p), ("stream", None))
    kq = head + (("k", 3), ("table", p), ("dist2", None), ("stream", None))
    common_bad = (dict(n=-1), dict(m=-1), dict(segments=-1), dict(cstride=2), dict(coffs=p, segments=0), dict(centers=None), dict(table=None),
                  dict(plan=None), dict(cells=None), dict(order=None), dict(packed=None))
    common_uns = (dict(dtype=_lib.F16), dict(dtype=_lib.BF16), dict(n=2 ** 31), dict(m=2 ** 31), dict(coffs=p, segments=2 ** 31))
    for wrong in common_bad + (dict(nsample=0), dict(nsample=1025), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
                               dict(radius=float("inf")), dict(counts=None)):
        assert call("d3d_ball_query_grid", bq, **wrong) == bad, wrong
    for wrong in common_uns + (dict(nsample=_lib.KNN_MAX + 1), dict(nsample=1024)):
        assert call("d3d_ball_query_grid", bq, **wrong) == uns, wrong
    for wrong in common_bad + (dict(k=0), dict(k=-3)):
        assert call("d3d_knn_query_grid", kq, **wrong) == bad, wrong
    for wrong in common_uns + (dict(k=_lib.KNN_MAX + 1),):
        assert call("d3d_knn_query_grid", kq, **wrong) == uns, wrong
    none = dict(m=0, centers=None, table=None, plan=None, cells=None, order=None, packed=None)
    assert call("d3d_ball_query_grid", bq, counts=None, nsample=_lib.KNN_MAX, **none) == _lib.OK
    assert call("d3d_knn_query_grid", kq, k=_lib.KNN_MAX, **none) == _lib.OK
    # the brute-force siblings keep their own limits
    assert lib.d3d_ball_query(p, 10, 3, p, 0, 3, _lib.F32, None, None, 0, 1.0, 1024, 0, None, None, None) == _lib.OK


def _hand_grid(offs=None, dtype=torch.float32):
    """a PointGrid put together by hand (building one needs a GPU): 10 rows, one cell per segment"""
    segs = 1 if offs is None else len(offs) - 1
    plan = (_Segment * segs)()
    for s in range(segs):
        plan[s].h, plan[s].inv_h, plan[s].base = 1.0, 1.0, 2 * s
        plan[s].dim[:] = [1, 1, 1]
    grid = PointGrid.__new__(PointGrid)
    e = torch.zeros(0, dtype=torch.int64)
    grid._set(torch.device("cuda", 0), torch.zeros((10, 3), dtype=dtype), offs, list(plan), 2 * segs, None, e, e.int(), e, torch.zeros(0, dtype=dtype), e)
    return grid


def test_python_layer_refuses_before_a_gpu_is_needed():
    pts, ctr = torch.zeros(10, 3), torch.zeros(4, 3)
    for kw in (dict(cell_size=0), dict(cell_size=-0.5), dict(cell_size=float("nan")), dict(cell_size=float("inf")), dict(cell_size="0.5"),
               dict(cell_size=True), dict(max_cells_per_point=0), dict(max_cells_per_point=float("inf")), dict(max_cells_per_point=None),
               dict(offsets=[0, 11]), dict(offsets=[1, 10]), dict(offsets=[0, 6, 4, 10]), dict(offsets=[[0, 10]]), dict(offsets=[0.0, 10.0])):
        with pytest.raises(ValueError):
            PointGrid(pts, **dict(dict(cell_size=0.5), **kw))
    for bad in (torch.zeros(10, 2), pts.half(), torch.zeros(10), pts.long(), np.zeros((10, 2), np.float32)):
        with pytest.raises(ValueError):
            PointGrid(bad, 0.5)
    with pytest.raises(TypeError):
        PointGrid([[0.0, 0.0, 0.0]], 0.5)
    grid, ragged = _hand_grid(), _hand_grid([0, 4, 10])
    assert grid.num_points == 10 and grid.num_cells == 2 and grid.cell_size == (1.0,) and grid.dims == ((1, 1, 1),) and grid.point_offsets is None
    assert ragged.num_segments == 2 and ragged.bases == (0, 2) and ragged.point_offsets == [0, 4, 10]
    queries = (lambda g, c, **kw: ball_query(g, c, 0.5, kw.pop("width", 8), **kw), lambda g, c, **kw: knn_query(g, c, kw.pop("width", 8), **kw),
               lambda g, c, **kw: PointInterp(g, c, k=kw.pop("width", 3), **{dict(point_offsets="known_offsets", center_offsets="unknown_offsets")[a]: v
                                                                             for a, v in kw.items()}))
    for query in queries:
        with pytest.raises(ValueError, match="brute-force" if query is queries[0] else "1 .. 64"):    # the grid route stops at 64; k
            query(grid, ctr, width=65)                                                                # stops there on both routes
        with pytest.raises(ValueError, match="own segments"):
            query(grid, ctr, point_offsets=[0, 10])
        with pytest.raises(ValueError, match="own segments"):
            query(ragged, ctr, point_offsets=[0, 4, 10], center_offsets=[0, 2, 4])
        with pytest.raises(ValueError, match="required iff"):
            query(grid, ctr, center_offsets=[0, 4])
        with pytest.raises(ValueError, match="required iff"):
            query(ragged, ctr)
        for coffs in ([0, 4], [0, 1, 2, 4], [0, 3, 2, 4], [0, 2, 5], [1, 2, 4]):
            with pytest.raises(ValueError):
                query(ragged, ctr, center_offsets=coffs)
        for bad in (ctr.double(), torch.zeros(4, 2), ctr.half(), torch.zeros(2, 4, 3)):
            with pytest.raises(ValueError):
                query(grid, bad)
        with pytest.raises(ValueError):
            query(_hand_grid(dtype=torch.float64), ctr)                          # the centres' dtype must be the grid's
        with pytest.raises(TypeError):
            query(grid, [[0.0, 0.0, 0.0]])
        with pytest.raises(ValueError):
            query(grid, ctr, width=0)
    for kw in (dict(radius=0.0), dict(radius=float("nan")), dict(radius="1"), dict(nsample=1025), dict(pad="last")):
        with pytest.raises(ValueError):
            ball_query(grid, ctr, **dict(dict(radius=0.5, nsample=8), **kw))
    assert "1024" in str(pytest.raises(ValueError, ball_query, grid, ctr, 0.5, 65).value)
    # nothing to launch: no centres
    table, counts = ball_query(grid, torch.zeros(0, 3), 0.5, 8)
    assert table.shape == (0, 8) and table.dtype == torch.int32 and counts.shape == (0,)
    table, dist2 = knn_query(ragged, torch.zeros(0, 5), 4, center_offsets=[0, 0, 0])
    assert table.shape == (0, 4) and dist2.shape == (0, 4) and dist2.dtype == torch.float32
    # an array in the place of the points behaves as before
    with pytest.raises(ValueError):
        ball_query(pts, ctr, 0.5, 8, point_offsets=[0, 10])
    assert ball_query(pts, torch.zeros(0, 3), 0.5, 1024)[0].shape == (0, 1024)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):                    # no CPU fallback
            PointGrid(pts, 0.5)
