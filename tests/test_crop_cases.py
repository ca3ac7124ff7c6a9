"""The scenes of tests/crop_cases.py against the oracle, without a GPU: conditions on the INPUTS of tests/test_gpu_crop_routes.py.
A scene whose planted points missed their boxes, or whose duplicated rows never decide a painted id, would let a wrong kernel
pass there."""
import numpy as np
import pytest

import crop_cases as cc
import oracle

N = 4097
FOOT = [0, 1, 3, 4]            # centre and extents: what duplicated rows share (all seven numbers but in zero_extent)


def _first_containing(mask):
    return np.where(mask.any(0), mask.argmax(0) + 1, 0)


@pytest.mark.parametrize("name", cc.SCENES)
def test_scene_meets_its_conditions(name):
    sc = cc.scene(name, N)
    assert sc.pts.shape == (N, 6) and sc.boxes.shape == (sc.m, 7) and sc.rows9.shape == (sc.m, 9)
    mask = oracle.crop_points(sc.boxes, sc.pts)
    ids = oracle.paint_label(sc.rows9, sc.pts, sc.sem)
    assert np.array_equal(ids, oracle.paint_label(sc.boxes, sc.pts[:, :3].copy(), sc.sem, labels=sc.labels))
    assert mask.any(0).sum() >= 0.05 * N                                        # hits
    on, off = mask[sc.pairs[:, 0], sc.pairs[:, 1]], mask[sc.pairs[:, 0], sc.pairs[:, 2]]
    assert len(sc.pairs) >= 6 and on.all() and not off.any()                    # ON the boundary: inside; one step out: outside
    # the four points on the common range and their twins are the last four pairs: the twins are outside EVERY box
    assert not mask[:, sc.pairs[-4:, 2]].any() and mask[:, sc.pairs[-4:, 1]].any(0).all()
    first = _first_containing(mask)
    assert np.any((first > 0) & (ids != first))                                 # the first box that holds a point is not painted
    if sc.m >= 5:
        for lo, hi in sc.wrong:                                                 # ... because it is of another class than hi
            assert sc.labels[lo] != sc.labels[hi] and np.array_equal(sc.boxes[lo, FOOT], sc.boxes[hi, FOOT])
            assert np.any((ids == hi + 1) & mask[lo]), (lo, hi)
        for lo, hi in sc.tie:                                                   # same class, same box: the lower index is painted
            assert sc.labels[lo] == sc.labels[hi] and np.array_equal(sc.boxes[lo, FOOT], sc.boxes[hi, FOOT])
            assert np.any((ids == lo + 1) & mask[hi]) and not np.any(ids == hi + 1), (lo, hi)
    # the other two operators see hits too (strict interval along z; the rectangle alone)
    assert oracle.box3dp_crop(sc.pts[:, :3], sc.boxes).any(0).sum() >= 0.05 * N
    assert oracle.crop_2dr(sc.pts[:, :2].copy(), sc.boxes[:, [0, 1, 3, 4, 6]].copy()).any(0).sum() >= 0.05 * N


def test_large_boxes_hold_most_points():
    for name in ("g8_box", "all_list"):
        sc = cc.scene(name, N)
        big = np.flatnonzero(sc.boxes[:, 3] >= 25)
        assert oracle.crop_2dr(sc.pts[:, :2].copy(), sc.boxes[big][:, [0, 1, 3, 4, 6]].copy()).any(0).mean() > 0.5, name


def test_non_finite_rows_and_points_are_there():
    for name, col in (("all_nan", 0), ("all_inf_w", 3), ("all_inf_yaw", 6)):
        sc = cc.scene(name, N)
        assert not np.isfinite(sc.boxes[cc.SPOILED_ROW, col]) and np.isfinite(np.delete(sc.boxes, cc.SPOILED_ROW, 0)).all()
        assert not oracle.crop_points(sc.boxes, sc.pts)[cc.SPOILED_ROW].any()   # dgal_wrap.h:6-19 on such a row: no point inside
    sc = cc.scene("g32", N)
    x, y, z = sc.pts[:, 0], sc.pts[:, 1], sc.pts[:, 2]
    assert np.isnan(x).sum() == 1 and np.isnan(y).sum() == 1 and np.isnan(z).sum() == 1
    assert np.isposinf(x).sum() == 1 and np.isneginf(x).sum() == 1 and np.isposinf(z).sum() == 1 and np.isneginf(z).sum() == 1
    assert oracle.crop_points(sc.boxes, sc.pts)[:, np.isnan(z)].any()           # NaN z passes the closed interval test
    assert cc.rows11(sc.boxes).shape == (sc.m, 11)


@pytest.mark.parametrize("m,n", [(1, 1), (65, 3), (129, 1025), (4097, 300)])
def test_pairs_scene(m, n):
    sc = cc.pairs_scene(m, n)
    mask = oracle.crop_points(sc.boxes, sc.pts)
    ids = oracle.paint_label(sc.boxes, sc.pts, sc.sem, labels=sc.labels)
    assert mask.shape == (m, n) and mask.any()
    if m >= 65 and n >= 300:
        assert np.any((ids > 0) & (ids != _first_containing(mask)))
        assert mask[64:].any() and np.any(ids > 64)                             # hits and painted ids beyond the first tile


def test_paint_tile_cases():
    sc = cc.paint_early_exit()
    ids = oracle.paint_label(sc.boxes, sc.pts, sc.sem, labels=sc.labels)
    assert np.all(ids[:1024] == 1) and ids[1024] != 1
    sc = cc.paint_last_tile()
    assert np.all(oracle.paint_label(sc.boxes, sc.pts, sc.sem, labels=sc.labels) == sc.m)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_axes_scene_hits_every_axis(dtype):
    pts, boxes = cc.axes_scene(1003, dtype)
    for ax in (0, 1, 2):
        assert oracle.box3dp_crop(pts, boxes, ax).any(0).sum() >= 0.1 * len(pts), ax
