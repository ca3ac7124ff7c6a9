"""CPU: the numpy model of the RoI pooling operators (roi_pool_reference.py) against a brute force in Python loops and against torch's
autograd, the pure-host entries (plan, limits), every refusal of the C entries and of the Python layer, and every scene of
roi_pool_cases.py against the property it exists for.  No GPU: the kernels run in tests/test_gpu_roi_pool.py."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
import roi_pool_cases as cases
import roi_pool_reference as ref
from d3d_amd import _lib
from d3d_amd.point import RoiGrid, group_pool, roi_grid_max_cells, roi_grid_plan, roiaware_pool3d, roipoint_pool3d

F = np.float32
_OK, _BAD, _UNSUP = 0, -1, -2
SPECIAL = dict(cases.special_scenes())


# ---------------------------------------------------------------- the model against loops
def brute_table(sc, p, pad):
    """rz = 0 only, exact rational arithmetic, one Python loop over boxes and points"""
    ox, oy, oz = ref.triple(sc.out_size)
    m = len(sc.boxes)
    table = [[[] for _ in range(ox * oy * oz)] for _ in range(m)]
    inside = [0] * m
    for i, b in enumerate(sc.boxes.tolist()):
        assert b[6] == 0
        c, ext = [Fraction(v) for v in b[:3]], [Fraction(v) for v in b[3:6]]
        for j, row in enumerate(sc.points[:, :3].tolist()):
            idx = []
            for a, o in enumerate((ox, oy, oz)):
                d = Fraction(row[a]) - c[a]
                if not -ext[a] / 2 <= d <= ext[a] / 2:
                    break
                idx.append(min(int((d / ext[a] + Fraction(1, 2)) * o), o - 1))
            else:
                inside[i] += 1
                cell = table[i][(idx[0] * oy + idx[1]) * oz + idx[2]]
                if len(cell) < p:
                    cell.append(j)
    counts = [[len(cell) for cell in box] for box in table]
    full = [[cell + ([cell[k % len(cell)] for k in range(len(cell), p)] if pad == "cycle" and cell else [-1] * (p - len(cell)))
             for cell in box] for box in table]
    return np.array(full, np.int32).reshape(m, -1, p), np.array(counts, np.int32), np.array(inside, np.int32)


@pytest.mark.parametrize("name", ("lattice", "cap"))
@pytest.mark.parametrize("pad", ("none", "cycle"))
def test_model_against_brute_force(name, pad):
    sc = SPECIAL[name]
    for p in (1, sc.max_points, sc.max_points + 1, 64):
        want = brute_table(sc, p, pad)
        got = ref.grid_model(sc.points, sc.boxes, sc.out_size, p, pad=pad)
        for g, w, what in zip(got, want, ("table", "counts", "inside")):
            assert g.dtype == np.int32 and np.array_equal(g, w), (what, p)
    assert want[2].min() > 0


def test_lattice_scene_sits_on_faces_and_corners():
    sc = SPECIAL["lattice"]
    b = sc.boxes[0]
    on_face = np.isclose(np.abs(sc.points[:, :3] - b[:3]), b[3:6] / 2).any(1) & ref.members(sc.points, sc.boxes)[0]
    corner = np.isclose(np.abs(sc.points[:, :3] - b[:3]), b[3:6] / 2).all(1)
    assert on_face.sum() >= 8 and corner.any()
    assert len(np.unique(sc.points, axis=0)) < len(sc.points)              # duplicates


# ---------------------------------------------------------------- the model's fold and its gradient against torch's autograd
def dense_pool(feat, table, reduction):
    """[N, C] fp64 tensor, table [R, K] -> [R, C] by a dense [R, K, C] gather and torch's own reductions"""
    t = torch.from_numpy(np.asarray(table).reshape(-1, table.shape[-1]).astype(np.int64))
    here = (t >= 0)[:, :, None]
    x = feat[t.clamp(min=0)]
    n = here.sum(1)
    if reduction in ("sum", "mean"):
        s = torch.where(here, x, torch.zeros_like(x)).sum(1)
        return s if reduction == "sum" else torch.where(n > 0, s / n.clamp(min=1), s)
    fill = float("-inf") if reduction == "max" else float("inf")
    x = torch.where(here, x, torch.full_like(x, fill))
    best = x.max(1).values if reduction == "max" else x.min(1).values
    return torch.where(n > 0, best, torch.zeros_like(best))


@pytest.mark.parametrize("reduction", ("sum", "mean", "max", "min"))
def test_model_pool_and_gradient_against_torch_autograd(reduction):
    sc = cases.random_scene(300, 5, 11, out_size=3, max_points=8, spread=4.0)
    table, _, _ = ref.grid_model(sc.points, sc.boxes, sc.out_size, sc.max_points)
    assert (ref.members(sc.points, sc.boxes).sum(0) >= 2).any()
    rng = np.random.default_rng(3)
    feat = rng.normal(size=(len(sc.points), 5))
    grad = rng.normal(size=(table.shape[0] * table.shape[1], 5))
    out, arg, count = ref.pool_forward(feat, table, reduction, "f64")
    gfeat = ref.pool_backward(grad, table, len(feat), reduction, "f64", arg, count)
    leaf = torch.from_numpy(feat).requires_grad_()
    want = dense_pool(leaf, table, reduction)
    want.backward(torch.from_numpy(grad))
    assert np.allclose(out, want.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(gfeat, leaf.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert np.abs(gfeat).sum() > 0


def test_roipoint_model_fills_cyclically():
    sc = SPECIAL["overlap"]
    feat = np.arange(len(sc.points) * 2, dtype=F).reshape(-1, 2)
    for s in (3, 64, 512):
        pooled, empty, table = ref.roipoint_model(sc.points, feat, sc.boxes, s)
        inside = ref.members(sc.points, sc.boxes).sum(1)
        assert empty.tolist() == (inside == 0).tolist() and empty[3] and not empty[:3].any()
        for i in range(3):
            rows = np.flatnonzero(ref.members(sc.points, sc.boxes)[i])[:s]
            assert table[i].tolist() == [int(rows[j % len(rows)]) for j in range(s)]
            assert np.array_equal(pooled[i, :, :3], sc.points[table[i], :3]) and np.array_equal(pooled[i, :, 3:], feat[table[i]])
        assert not pooled[3].any() and (table[3] == -1).all()


# ---------------------------------------------------------------- pure host entries
def test_plan_and_limits():
    assert roi_grid_max_cells() >= 4096
    for cells in (1, 1728, roi_grid_max_cells()):
        last = 0
        for rows in (0, 1, 63, 64, 65, 511, 512, 513, 4096, 150000, 2 ** 31 - 1):
            tile, slab, rnd = roi_grid_plan(rows, cells)
            assert tile == 64 and slab >= tile and slab % tile == 0 and rnd > slab and rnd % slab == 0 and rnd >= last
            last = rnd
    lib = _lib.load()
    a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    ra, rb, rc = ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)
    assert lib.d3d_roi_grid_plan(-1, 8, ra, rb, rc) == _BAD and lib.d3d_roi_grid_plan(10, 0, ra, rb, rc) == _BAD
    assert lib.d3d_roi_grid_plan(10, 8, None, rb, rc) == _BAD and lib.d3d_roi_grid_plan(10, 8, ra, None, rc) == _BAD
    assert lib.d3d_roi_grid_plan(10, 8, ra, rb, None) == _BAD
    assert lib.d3d_roi_grid_plan(2 ** 31, 8, ra, rb, rc) == _UNSUP and lib.d3d_roi_grid_plan(10, roi_grid_max_cells() + 1, ra, rb, rc) == _UNSUP
    with pytest.raises(ValueError):
        roi_grid_plan(-1, 8)


# ---------------------------------------------------------------- refusals of the C entries (none launches, none reads a pointer)
_GRID_ARGS = "points n point_stride boxes m box_stride box_offset dtype point_offsets box_offsets segments out_size max_points pad table counts inside stream"
_GRID_REFUSALS = [
    (dict(n=-1), _BAD), (dict(m=-1), _BAD), (dict(segments=-1), _BAD), (dict(point_stride=2), _BAD), (dict(box_stride=6), _BAD),
    (dict(box_offset=-1), _BAD), (dict(box_offset=2), _BAD), (dict(box_offset=2, box_stride=9, boxes=None), _BAD),
    (dict(points=None), _BAD), (dict(boxes=None), _BAD), (dict(table=None), _BAD), (dict(counts=None), _BAD), (dict(inside=None), _BAD),
    (dict(point_offsets=True), _BAD), (dict(box_offsets=True), _BAD), (dict(point_offsets=True, box_offsets=True, segments=0), _BAD),
    (dict(out_size=None), _BAD), (dict(out_size=(0, 2, 2)), _BAD), (dict(out_size=(2, -1, 2)), _BAD), (dict(out_size=(2, 2, 0)), _BAD),
    (dict(max_points=0), _BAD), (dict(max_points=1025), _BAD), (dict(max_points=-3), _BAD), (dict(pad=2), _BAD), (dict(pad=-1), _BAD),
    (dict(dtype=1), _UNSUP), (dict(dtype=4), _UNSUP), (dict(dtype=5), _UNSUP), (dict(out_size=(17, 16, 16)), _UNSUP),
    (dict(out_size=(4097, 1, 1)), _UNSUP), (dict(out_size=(2 ** 30, 2 ** 30, 2 ** 30)), _UNSUP), (dict(n=2 ** 31), _UNSUP),
    (dict(m=2 ** 31), _UNSUP), (dict(segments=2 ** 31, point_offsets=True, box_offsets=True), _UNSUP),
    (dict(m=2 ** 31 // (8 * 128) + 1), _UNSUP), (dict(m=5000, out_size=(16, 16, 16), max_points=1024), _UNSUP),
    (dict(m=0), _OK), (dict(m=0, points=None, boxes=None, table=None, counts=None, inside=None), _OK),
]
_BWD_ARGS = "grad_out rows c dtype order offsets src_rows k reduction arg count grad_feat stream"
_BWD_REFUSALS = [
    (dict(rows=-1), _BAD), (dict(src_rows=-1), _BAD), (dict(c=0), _BAD), (dict(k=0), _BAD), (dict(grad_out=None), _BAD),
    (dict(order=None), _BAD), (dict(offsets=None), _BAD), (dict(grad_feat=None), _BAD), (dict(reduction=2, arg=None), _BAD),
    (dict(reduction=3, arg=None), _BAD), (dict(reduction=1, count=None), _BAD),
    (dict(dtype=2), _UNSUP), (dict(dtype=3), _UNSUP), (dict(reduction=0), _UNSUP), (dict(reduction=5), _UNSUP), (dict(k=344), _UNSUP),
    (dict(src_rows=2 ** 31), _UNSUP), (dict(rows=2 ** 31 // 7 + 1), _UNSUP),
    (dict(src_rows=0), _OK), (dict(src_rows=0, offsets=None, grad_feat=None), _OK),
]


def _refusal_codes(fn, names, defaults, cases_):
    arena = (ctypes.c_char * 4096)()
    dev = ctypes.addressof(arena)                       # stands in for every device pointer: a refused call reads none of them
    out, keep = [], []
    for wrong, expected in cases_:
        args = []
        for name in names.split():
            v = wrong.get(name, defaults.get(name, dev))
            if v is True:
                v = dev
            if isinstance(v, tuple):
                v = (ctypes.c_int32 * 3)(*v)
                keep.append(v)
                v = ctypes.addressof(v)
            args.append(v)
        out.append((wrong, expected, fn(*args)))
    return out


def test_roi_grid_table_refuses_before_any_launch():
    defaults = dict(n=100, point_stride=3, m=4, box_stride=7, box_offset=0, dtype=_lib.F32, point_offsets=None, box_offsets=None, segments=0,
                    out_size=(2, 2, 2), max_points=128, pad=0, stream=None)
    got = _refusal_codes(_lib.load().d3d_roi_grid_table, _GRID_ARGS, defaults, _GRID_REFUSALS)
    assert not [(w, "expected %d, got %d" % (x, rc)) for w, x, rc in got if rc != x]


def test_table_pool_backward_index_refuses_before_any_launch():
    defaults = dict(rows=10, c=4, dtype=_lib.F32, src_rows=20, k=7, reduction=4, stream=None)
    got = _refusal_codes(_lib.load().d3d_table_pool_backward_index, _BWD_ARGS, defaults, _BWD_REFUSALS)
    assert not [(w, "expected %d, got %d" % (x, rc)) for w, x, rc in got if rc != x]


# ---------------------------------------------------------------- refusals of the Python layer (before a GPU is needed)
def test_python_layer_refuses_without_a_gpu():
    pts, boxes = np.zeros((10, 4), F), np.zeros((2, 7), F)
    bad = [
        dict(points=np.zeros((10, 2), F)), dict(points=np.zeros((10,), F)), dict(points=pts.astype(np.float64)), dict(points=[[0, 0, 0]]),
        dict(boxes=np.zeros((2, 6), F)), dict(boxes=np.zeros((2, 9), F)), dict(boxes=boxes.astype(np.float64)), dict(boxes=np.zeros((7,), F)),
        dict(out_size=0), dict(out_size=(2, 2)), dict(out_size=(2, 2, 0)), dict(out_size=2.0), dict(out_size=True), dict(out_size=17),
        dict(out_size=(4097, 1, 1)), dict(max_points_per_cell=0), dict(max_points_per_cell=1025), dict(max_points_per_cell=1.5),
        dict(pad="first"), dict(pad=None), dict(point_offsets=[0, 10]), dict(box_offsets=[0, 2]),
        dict(point_offsets=[0, 10], box_offsets=[0, 1, 2]), dict(point_offsets=[0, 9], box_offsets=[0, 2]),
        dict(point_offsets=[0, 7, 5, 10], box_offsets=[0, 1, 1, 2]), dict(point_offsets=[1, 10], box_offsets=[0, 2]),
        dict(boxes=np.zeros((2 ** 31 // (4096 * 1024) + 1, 7), F), out_size=16, max_points_per_cell=1024),
    ]
    for kw in bad:
        args = dict(dict(points=pts, boxes=boxes), **kw)
        with pytest.raises((ValueError, TypeError)):
            RoiGrid(**args)
    for s in (0, 1025, -1):
        with pytest.raises(ValueError):
            roipoint_pool3d(pts, np.zeros((10, 3), F), boxes, num_samples=s)
    with pytest.raises(TypeError):
        roiaware_pool3d(np.zeros((10, 3), F), "grid")
    feat, table = np.zeros((10, 3), F), np.zeros((4, 5), np.int32)
    for f, t, r in ((feat, table.astype(np.int64), "max"), (feat, table[0], "max"), (feat, np.zeros((4, 344), np.int32), "max"),
                    (feat, np.zeros((4, 0), np.int32), "max"), (feat, table, "median"), (feat, table, None), (feat[0], table, "max"),
                    (feat.astype(np.int32), table, "max"), (feat, table + 10, "max"), (feat, table - 2, "max")):
        with pytest.raises(ValueError):
            group_pool(f, t, r)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):           # no silent CPU fallback
            RoiGrid(pts, boxes)
        with pytest.raises(RuntimeError):
            group_pool(feat, table, "max")


# ---------------------------------------------------------------- every scene against the property it exists for
def uncapped(sc):
    return ref.grid_model(sc.points, sc.boxes, sc.out_size, 1024, sc.point_offsets, sc.box_offsets)


def test_cap_scene_has_a_cell_at_the_cap_and_one_past_it():
    sc = SPECIAL["cap"]
    _, counts, _ = uncapped(sc)
    assert counts[0, 0] == sc.max_points and counts[0, 7] == sc.max_points + 1 and (counts[0, 1:7] > 0).any()


def test_overlap_scene_has_a_point_in_three_boxes_and_an_empty_box():
    sc = SPECIAL["overlap"]
    mask = ref.members(sc.points, sc.boxes)
    assert mask.sum(0).max() >= 3 and mask[3].sum() == 0 and (mask[:3].sum(1) > 0).all()
    sc = SPECIAL["copies"]
    assert len(sc.boxes) == 32 and (sc.boxes == sc.boxes[0]).all() and ref.members(sc.points, sc.boxes)[0].sum() > 64


def test_seam_scene_straddles_every_slab_seam():
    sc = SPECIAL["seam"]
    n = len(sc.points)
    _, slab, rnd = roi_grid_plan(n, 8)
    rows = np.flatnonzero(ref.members(sc.points, sc.boxes)[0])
    seams = list(range(slab, n, slab))
    assert len(seams) >= 2 and rnd in seams and rows.tolist() == sorted([s - 1 for s in seams] + seams)
    assert len(set(ref.cells(sc.points[rows, :3], sc.boxes[0], sc.out_size).tolist())) == 1


def test_tile_scenes():
    sc = SPECIAL["one_cell_tile"]
    mask = ref.members(sc.points, sc.boxes)[0]
    cell = ref.cells(sc.points[:, :3], sc.boxes[0], sc.out_size)
    assert mask[64:128].all() and len(set(cell[64:128].tolist())) == 1               # all 64 lanes of the second tile, one cell
    assert len(set(cell[mask].tolist())) > 2 and roi_grid_plan(len(sc.points), 8)[0] == 64
    sc = SPECIAL["two_cells"]
    mask = ref.members(sc.points, sc.boxes)[0]
    cell = ref.cells(sc.points[:, :3], sc.boxes[0], sc.out_size)
    assert mask[:192].all() and cell[0] != cell[1] and (cell[:192:2] == cell[0]).all() and (cell[1:192:2] == cell[1]).all()
    assert 96 > sc.max_points                                                         # both cells pass the cap


def test_early_cap_and_overflow_scenes():
    sc = SPECIAL["early_cap"]
    _, slab, rnd = roi_grid_plan(len(sc.points), 2)
    rows = np.flatnonzero(ref.members(sc.points, sc.boxes)[0])
    cell = ref.cells(sc.points[rows, :3], sc.boxes[0], sc.out_size)
    left, right = rows[cell == 0], rows[cell == 1]
    assert (left < slab).sum() > sc.max_points and (left >= slab).any() and (left >= rnd).any()    # the cap is reached inside the first slab
    assert (right < slab).sum() == 1 and len(right) > sc.max_points and (right // slab).tolist() == [0, 2, 3, rnd // slab + 1]
    sc = SPECIAL["overflow"]
    _, slab, rnd = roi_grid_plan(len(sc.points), 27)
    mask = ref.members(sc.points, sc.boxes)[0]
    assert mask.all() and len(mask) == 2 * rnd and uncapped(sc)[1].max() > sc.max_points      # every queue full, in two rounds


def test_nonfinite_scenes():
    sc = SPECIAL["nonfinite_points"]
    r = sc.nan_z_row
    assert np.isnan(sc.points[r, 2]) and oracle.crop_points(sc.boxes, np.ascontiguousarray(sc.points[:, :3]))[0, r]
    assert not ref.members(sc.points, sc.boxes)[:, r].any()
    assert not ref.members(sc.points, sc.boxes)[:, ~np.isfinite(sc.points[:, :3]).all(1)].any()
    sc = SPECIAL["bad_boxes"]
    mask = ref.members(sc.points, sc.boxes)
    nan_rows = np.isnan(sc.boxes).any(1)
    assert nan_rows.sum() == 4 and mask[:4].any(1).all()
    flat = np.isnan(sc.boxes[:, [0, 1, 3, 4]]).any(1)                                 # a NaN in the rectangle: crop_points holds for no point
    assert flat.sum() == 2 and not mask[flat].any()
    for i in np.flatnonzero(nan_rows & ~flat):                                        # a NaN in z or lz: the closed z test passes, t_z is NaN -> i_z = 0
        rows = np.flatnonzero(mask[i])
        assert len(rows) and (ref.cells(sc.points[rows, :3], sc.boxes[i], sc.out_size) % ref.triple(sc.out_size)[2] == 0).all()
    assert (sc.boxes[:, 3:6] <= 0).any(1).sum() >= 8 and np.isinf(sc.boxes).any()
    sc = SPECIAL["duplicates"]
    assert (sc.points[0::4] == sc.points[3::4]).all()
    sc = SPECIAL["ragged"]
    assert sc.point_offsets[1] == sc.point_offsets[2] and sc.box_offsets[2] > sc.box_offsets[1]
    assert (uncapped(sc)[2][sc.box_offsets[1]:sc.box_offsets[2]] == 0).all()


def test_faces_scene_lies_on_the_boundary():
    sc = SPECIAL["faces"]
    mask = ref.members(sc.points, sc.boxes)
    planted = mask[:, 256:]
    assert planted.any(1).all() and not planted.all()                                 # the outward twins are outside
    assert sc.boxes[0, 6] == 0 and sc.boxes[1, 6] == F(np.pi / 2) and sc.boxes[2, 6] == F(np.pi)


@pytest.mark.parametrize("name", sorted(cases.RANDOM_SCENES))
def test_random_scenes_fill_their_boxes(name):
    sc = cases.random_scene(*cases.RANDOM_SCENES[name])
    assert ref.members(sc.points, sc.boxes).any(0).mean() >= 0.1
    assert np.abs(sc.boxes[:, 6]).max() < ref.MAX_ANGLE
    for _, s in cases.angle_scenes():
        assert ref.members(s.points, s.boxes).any(0).mean() >= 0.1
