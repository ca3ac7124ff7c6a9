"""CPU: the scenes of tests/deteval_cases.py against oracle.calc_stats alone -- what each scene is there for holds in the
reference's own arithmetic, so the device tests on them cannot pass vacuously."""
import numpy as np
import pytest

import oracle
import deteval_cases as cases
from d3d_amd.benchmarks import DetectionEvaluator


def _thresholds(scene):
    return DetectionEvaluator(scene["classes"], scene["min_overlaps"], **scene["kwargs"]).score_thresholds


def _oracle(scene, literal, frames=None):
    thr, maxd = _thresholds(scene), cases.max_distance(scene)
    fr = cases.frames_of(scene)
    return [oracle.calc_stats(fr[f][0], fr[f][1], scene["classes"], maxd, thr, literal=literal)
            for f in (range(len(fr)) if frames is None else frames)]


@pytest.fixture(scope="module")
def scenes():
    return dict(a=cases.scene_a(), b=cases.scene_b(), c=cases.scene_c(), d=cases.scene_d(96), e=cases.scene_e())


def test_offsets_rise_from_zero_to_the_row_counts(scenes):
    for name, s in scenes.items():
        for off, rows in ((s["go"], s["gt"]), (s["do"], s["dt"])):
            assert off[0] == 0 and off[-1] == len(rows) and np.all(np.diff(off) >= 0), name
        assert len(s["go"]) == len(s["do"])
        assert s["gt"].dtype == np.float32 and s["dt"].dtype == np.float32 and s["gt"].shape[1] == 9 and s["dt"].shape[1] == 9
    assert len(scenes["a"]["go"]) - 1 == 24 and len(set(np.diff(scenes["a"]["go"]).tolist())) > 4
    assert len(scenes["e"]["go"]) - 1 == 300
    assert np.diff(scenes["e"]["go"]).max() <= 15 and np.diff(scenes["e"]["do"]).max() <= 30
    d = scenes["d"]
    assert np.diff(d["go"])[d["names"]["at"]] == 96 and np.diff(d["do"])[d["names"]["at"]] == 96
    assert np.diff(d["go"])[d["names"]["above"]] == 97 and np.diff(d["do"])[d["names"]["above"]] == 97
    c, sizes = scenes["c"], {}
    for name, f in c["names"].items():
        sizes[name] = (int(np.diff(c["do"])[f]), int(np.diff(c["go"])[f]))
    assert sizes["0x0"] == (0, 0) and sizes["0x5"] == (0, 5) and sizes["5x0"] == (5, 0) and sizes["1x1"] == (1, 1)
    assert sizes["65x65"] == (65, 65) and sizes["64x129"] == (64, 129)
    gt_f, dt_f = cases.frames_of(c)[c["names"]["outside"]]
    assert len(gt_f) and len(dt_f) and not np.isin(gt_f[:, 0], c["classes"]).any() and not np.isin(dt_f[:, 0], c["classes"]).any()


@pytest.mark.parametrize("name", ["a", "b"])
def test_every_class_matches_and_the_thresholds_bite(scenes, name):
    s = scenes[name]
    res = {lit: _oracle(s, lit) for lit in (True, False)}
    for lit in (True, False):
        for c in s["classes"]:
            lowest, highest = sum(r.tp[c][0] for r in res[lit]), sum(r.tp[c][-1] for r in res[lit])
            assert lowest > 0 and highest < lowest, (name, lit, c, lowest, highest)
    if name == "b":
        differ = sum(a[k][c] != b[k][c] for a, b in zip(res[True], res[False]) for k in ("tp", "fp", "fn") for c in s["classes"])
        assert differ >= 1
    if name == "a":
        assert {int(x) for x in np.unique(s["gt"][:, 0])} == {1, 2, 3} and {int(x) for x in np.unique(s["dt"][:, 0])} == {1, 2, 3}


def test_edge_frames_are_what_they_claim(scenes):
    s = scenes["c"]
    thr = _thresholds(s)
    fr = cases.frames_of(s)
    assert thr[0] > 0.19 and len(thr) == 10
    # the tie frame: more than 16 of a kind among the selected at the lowest threshold (numpy's argsort leaves insertion sort)
    dt_f = fr[s["names"]["ties"]][1]
    sel = np.isin(dt_f[:, 0], s["classes"]) & ~(dt_f[:, 1] < thr[0])
    assert np.unique(dt_f[sel, 1], return_counts=True)[1].max() > 16
    # the NaN frame: its NaN detections are counted at every threshold
    f = s["names"]["nan"]
    dt_f = fr[f][1]
    nan = np.isnan(dt_f[:, 1])
    assert nan.sum() >= 10
    got = _oracle(s, True, [f])[0]
    for c in s["classes"]:
        k = int((nan & (dt_f[:, 0] == c)).sum())
        assert k > 0 and got.ndt[c][-1] >= k and all(v >= k for v in got.ndt[c])
    # all scores below every threshold: nothing selected, every ground truth missed
    f = s["names"]["below"]
    assert fr[f][1][:, 1].max() < thr[0]
    got = _oracle(s, True, [f])[0]
    assert all(sum(got.ndt[c]) == 0 and sum(got.tp[c]) == 0 and got.fn[c][0] == got.ngt[c] > 0 for c in s["classes"])
    # the wavefront-crossing frames match ground truths beyond column 63 (and 127)
    for name, col in (("65x65", 64), ("64x129", 128)):
        gt_f, dt_f = fr[s["names"][name]]
        cache = oracle.prepare_boxes(dt_f, gt_f, True)
        _, da = oracle.score_match(cache, dt_f, gt_f, np.nonzero(np.isin(dt_f[:, 0], s["classes"]))[0],
                                   np.nonzero(np.isin(gt_f[:, 0], s["classes"]))[0], cases.max_distance(s), literal=True)
        assert max(da) >= col - 8 and len(da) > 10, (name, sorted(da))


def _cache_fp64(src_arr, dst_arr, rotated=True):
    """oracle.prepare_boxes with the IoU evaluated in fp64 (the oracle's own box2d_iou on fp64 rows) and rounded once"""
    d, g = np.asarray(src_arr, np.float32).reshape(-1, 9), np.asarray(dst_arr, np.float32).reshape(-1, 9)
    if not len(d) or not len(g):
        return np.zeros((len(d), len(g)), np.float32)
    a, b = d[:, 2:9].astype(np.float64), g[:, 2:9].astype(np.float64)
    a[:, 3:6], b[:, 3:6] = np.clip(a[:, 3:6], -1e3, 1e3), np.clip(b[:, 3:6], -1e3, 1e3)
    bev = oracle.box2d_iou(a[:, [0, 1, 3, 4, 6]], b[:, [0, 1, 3, 4, 6]], "rbox")
    az0, az1, bz0, bz1 = a[:, 2] - a[:, 5] / 2, a[:, 2] + a[:, 5] / 2, b[:, 2] - b[:, 5] / 2, b[:, 2] + b[:, 5] / 2
    zi = np.maximum(np.minimum(az1[:, None], bz1[None]) - np.maximum(az0[:, None], bz0[None]), 0)
    zu = np.maximum(np.maximum(az1[:, None], bz1[None]) - np.minimum(az0[:, None], bz0[None]), 1e-6)
    return (1 - bev * zi / zu).astype(np.float32)


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_oracles_own_rounding_stays_inside_half_the_tolerance(scenes, name, monkeypatch):
    """tests/test_gpu_deteval_batch.py compares acc_* with oracle.calc_stats at rtol=1e-4, atol=1e-5.  The oracle computes its
    IoU in fp32 as the reference does; on (a) and (b) its stats must not move by more than HALF that tolerance when its distance
    cache is evaluated in fp64 instead, in any bin, so that the comparison measures the device and not the oracle's rounding"""
    s = scenes[name]
    for literal in (True, False):
        own = _oracle(s, literal)
        with monkeypatch.context() as mp:
            mp.setattr(oracle, "prepare_boxes", _cache_fp64)
            exact = _oracle(s, literal)
        for f, (a, b) in enumerate(zip(own, exact)):
            for c in s["classes"]:
                assert all(a[k][c] == b[k][c] for k in ("ndt", "tp", "fp", "fn")), (name, literal, f, c)
                assert np.allclose(a.acc_iou[c], b.acc_iou[c], rtol=0.5e-4, atol=0.5e-5, equal_nan=True), \
                    (name, literal, f, c, np.nanmax(np.abs(np.asarray(a.acc_iou[c]) - np.asarray(b.acc_iou[c]))))
