"""GPU tests of TrackingEvaluator: whole seeded sequences frame by frame against the literal checker (tests/track_reference.py,
fed the device's distance cache so that both decide on the same fp32 distances), calc_stats_sequence against per-frame calls,
device inputs, reset and pickling mid-sequence, a large frame, and the edge cases of the carry-over rules."""
import pickle

import numpy as np
import pytest
import torch

import track_reference as tr
from track_cases import CASES, assert_stats_equal, golden, golden_case, golden_evaluator, golden_stats
from d3d_amd import synth
from d3d_amd.benchmarks import TrackingEvaluator
from d3d_amd.tracking import DistanceTypes, prepare_boxes

pytestmark = pytest.mark.gpu
CLASSES = [1, 2]


def _frames(seq):
    g, d, gi, di, go, do = seq
    return [(g[go[f]:go[f + 1]], d[do[f]:do[f + 1]], gi[go[f]:go[f + 1]], di[do[f]:do[f + 1]]) for f in range(len(go) - 1)]


def _cache(gt, dt):
    if len(gt) == 0 or len(dt) == 0:
        return np.zeros((len(dt), len(gt)), np.float32)
    return prepare_boxes(dt, gt, DistanceTypes.RIoU).cpu().numpy()


class Checker:
    def __init__(self, ev):
        self.ev, self.state = ev, tr.State(ev._pr_nsamples)
        self.md = {c: np.float32(v) for c, v in ev._max_distance.items()}

    def __call__(self, gt, dt, gi, di):
        return tr.calc_stats(self.state, gt, dt, gi, di, self.ev._classes, self.md, self.ev.score_thresholds, cache=_cache(gt, dt))


@pytest.mark.parametrize("seed,overlap", [(0, 0.5), (1, 0.3), (2, 0.7)])
def test_sequence_against_checker(seed, overlap):
    ev = TrackingEvaluator(CLASSES, overlap, pr_sample_count=16)
    ck = Checker(ev)
    frames = _frames(synth.tracking_sequence(frames=12, n_tracks=25, seed=seed))
    for f, fr in enumerate(frames):
        got, exp = ev.calc_stats(*fr), ck(*fr)
        assert_stats_equal(got, exp, CLASSES, "frame %d" % f)
        ev.add_stats(got)
    assert sum(sum(v) for v in ev.get_stats().id_switches.values()) > 0


def test_sequence_call_equals_per_frame():
    seq = synth.tracking_sequence(frames=15, n_tracks=30, seed=4)
    a, b = TrackingEvaluator(CLASSES, 0.5), TrackingEvaluator(CLASSES, 0.5)
    many = a.calc_stats_sequence(*seq)
    for f, fr in enumerate(_frames(seq)):
        assert_stats_equal(many[f], b.calc_stats(*fr), CLASSES, "frame %d" % f)
    nxt = synth.tracking_sequence(frames=2, n_tracks=30, seed=4)          # the state after the sequence is the same too
    for fr in _frames(nxt):
        assert_stats_equal(a.calc_stats(*fr), b.calc_stats(*fr), CLASSES)


def test_device_inputs_equal_host():
    seq = synth.tracking_sequence(frames=6, n_tracks=20, seed=6)
    a, b = TrackingEvaluator(CLASSES, 0.5), TrackingEvaluator(CLASSES, 0.5)
    for fr in _frames(seq):
        g, d, gi, di = fr
        dev = (torch.from_numpy(g).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(gi.astype(np.int64)).cuda(),
               torch.from_numpy(di.astype(np.int64)).cuda())
        assert_stats_equal(a.calc_stats(*dev), b.calc_stats(*fr), CLASSES)


def test_reset_and_pickle_mid_sequence():
    frames = _frames(synth.tracking_sequence(frames=10, n_tracks=20, seed=7))
    ev = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=8)
    for fr in frames[:4]:
        ev.add_stats(ev.calc_stats(*fr))
    clone = pickle.loads(pickle.dumps(ev))
    ck = Checker(TrackingEvaluator(CLASSES, 0.5, pr_sample_count=8))
    for fr in frames[:4]:
        ck(*fr)
    for f, fr in enumerate(frames[4:]):
        got, exp = ev.calc_stats(*fr), ck(*fr)
        assert_stats_equal(got, exp, CLASSES, "frame %d" % f)
        assert_stats_equal(clone.calc_stats(*fr), exp, CLASSES, "resumed frame %d" % f)
    ev.reset()
    fresh = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=8)
    for fr in frames[2:5]:
        assert_stats_equal(ev.calc_stats(*fr), fresh.calc_stats(*fr), CLASSES)
    assert ev.get_stats().tp[1] == [0] * 8


def test_large_frames_and_state_growth():
    """frames past any LDS budget (2 k gt x 5 k dt) and a state that grows between frames: sequence == per frame, counts add up"""
    small = _frames(synth.tracking_sequence(frames=2, n_tracks=10, seed=9))
    big = _frames(synth.tracking_sequence(frames=2, n_tracks=2000, seed=9, false_tracks=3000))
    ev, ref = TrackingEvaluator(CLASSES, 0.5), TrackingEvaluator(CLASSES, 0.5)
    frames = small + big
    gt = np.concatenate([f[0] for f in frames])
    dt = np.concatenate([f[1] for f in frames])
    gi = np.concatenate([f[2] for f in frames])
    di = np.concatenate([f[3] for f in frames])
    go = np.cumsum([0] + [len(f[0]) for f in frames])
    do = np.cumsum([0] + [len(f[1]) for f in frames])
    many = ev.calc_stats_sequence(gt, dt, gi, di, go, do)
    for f, fr in enumerate(frames):
        one = ref.calc_stats(*fr)
        assert_stats_equal(many[f], one, CLASSES, "frame %d" % f)
        for c in CLASSES:
            assert [a + b for a, b in zip(one.tp[c], one.fn[c])] == [one.ngt[c]] * 40
    assert len(big[0][1]) > 4000


def _box(cls, x, score=0.9, y=0.0, l=4.0):
    return [cls, score, x, y, 0.0, l, 2.0, 1.5, 0.0]


def _run_both(frames, classes=CLASSES, overlap=0.5, T=8):
    ev = TrackingEvaluator(classes, overlap, pr_sample_count=T)
    ck = Checker(ev)
    out = []
    for f, (g, d, gi, di) in enumerate(frames):
        g = np.asarray(g, np.float32).reshape(-1, 9)
        d = np.asarray(d, np.float32).reshape(-1, 9)
        gi, di = np.asarray(gi, np.uint64), np.asarray(di, np.uint64)
        got, exp = ev.calc_stats(g, d, gi, di), ck(g, d, gi, di)
        assert_stats_equal(got, exp, classes, "frame %d" % f)
        out.append(got)
    return out


def test_empty_frames():
    out = _run_both([([_box(1, 0)], [_box(1, 0.1)], [1], [11]),
                     ([], [_box(1, 0.1)], [], [11]),
                     ([_box(1, 0)], [], [1], []),
                     ([], [], [], []),
                     ([_box(1, 0)], [_box(1, 0.1)], [1], [11])])
    assert out[1].fp[1][0] == 0                     # the carried detection whose gt is absent takes no part: never fp
    assert out[2].fn[1][0] == 1


def test_vanish_return_fragments_and_gt_swaps():
    out = _run_both([([_box(1, 0), _box(1, 10)], [_box(1, 0.1, 0.9), _box(1, 10.1, 0.8)], [1, 2], [11, 12]),
                     ([_box(1, 0), _box(1, 10)], [_box(1, 10.1, 0.8)], [1, 2], [12]),                   # 11 vanishes
                     ([_box(1, 0), _box(1, 10)], [_box(1, 0.1, 0.9), _box(1, 10.1, 0.8)], [1, 2], [11, 12]),
                     ([_box(1, 0), _box(1, 10)], [_box(1, 0.1, 0.9), _box(1, 10.1, 0.8)], [2, 1], [11, 12]),   # gt ids swap
                     ([_box(1, 0), _box(1, 10)], [_box(1, 10.1, 0.9), _box(1, 0.1, 0.8)], [2, 1], [11, 12])])  # dt ids swap
    assert sum(out[3].id_switches[1]) > 0 or sum(out[4].id_switches[1]) > 0
    assert sum(sum(o.fragments[1]) for o in out) > 0


def test_drift_past_max_distance():
    # the carry-over is kept while the distance is <= max_distance and rematched past it
    frames = [([_box(1, 0)], [_box(1, 0.0)], [1], [11])] + \
             [([_box(1, 0), _box(1, 1.5 * k - 1.0)], [_box(1, 0.5 * k, 0.9), _box(1, 1.5 * k - 0.9, 0.5)], [1, 2], [11, 12])
              for k in range(1, 6)]
    _run_both(frames, overlap=0.4)


def test_carry_over_kept_at_exact_boundary():
    """dt 11 tracked gt 1; now it sits exactly at max_distance from gt 1 and within it of gt 2, and dt 13 (higher score) sits
    on gt 1.  Kept (`>` rematches): 13 overwrites the carry-over (fp) and gt 2 stays unmatched (fn).  Were the test `>=`,
    11 would be rematched: 13 takes gt 1, 11 takes gt 2, no fp and no fn."""
    g1, a = np.asarray([_box(1, 0)], np.float32), np.asarray([_box(1, 0.7, 0.5)], np.float32)
    d = float(_cache(g1, a)[0, 0])
    overlap = 1 - d
    assert np.float32(TrackingEvaluator([1], overlap)._max_distance[1]) == np.float32(d)
    frames = [([_box(1, 0)], [_box(1, 0.05, 0.5)], [1], [11]),
              ([_box(1, 0), _box(1, 1.35)], [_box(1, 0.7, 0.5), _box(1, 0.0, 0.9)], [1, 2], [11, 13])]
    out = _run_both(frames, classes=[1], overlap=overlap, T=4)
    assert float(_cache(np.asarray([_box(1, 1.35)], np.float32), a)[0, 0]) <= d
    both = np.nonzero(TrackingEvaluator([1], overlap, pr_sample_count=4).score_thresholds <= 0.5)[0]     # 11 and 13 selected
    assert len(both) >= 2
    for t in both:
        assert (out[1].fp[1][t], out[1].fn[1][t], out[1].fragments[1][t]) == (1, 1, 1), t


def test_frames_of_several_hundred_boxes_against_checker():
    """more than one 256-thread step of every compaction and a mask grid that wraps its 1024-block clamp (> 262 k cells)"""
    frames = _frames(synth.tracking_sequence(frames=2, n_tracks=500, seed=21, false_tracks=200))
    assert min(len(f[1]) for f in frames) > 512 and min(len(f[0]) * (len(f[1]) + 1) for f in frames) > 1024 * 256
    ev = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=4)
    ck = Checker(ev)
    for f, fr in enumerate(frames):
        assert_stats_equal(ev.calc_stats(*fr), ck(*fr), CLASSES, "frame %d" % f)


@pytest.mark.parametrize("name", CASES)
def test_golden_sequences(name):
    """the reference's own per-frame TrackingEvalStats (tests/golden/make_track_golden.py), frame by frame.  The goldens were
    computed on the CPU oracle's distances: counts exact, accuracies within the detection evaluator's tolerances against it
    (tests/test_gpu_boxloss.py: rtol 1e-4, atol 1e-5)"""
    z = golden()
    classes, params, frames = golden_case(z, name)
    ev = golden_evaluator(TrackingEvaluator, classes, params)
    for f, fr in enumerate(frames):
        assert_stats_equal(ev.calc_stats(*fr), golden_stats(z, name, f, classes, params["T"], True), classes, "frame %d" % f,
                           rtol=1e-4, atol=1e-5)


def test_nan_and_tied_scores():
    g = [_box(1, 3.0 * k) for k in range(8)]
    scores = [float("nan"), 0.5, 0.5, 0.5, float("nan"), 0.7, 0.5, 0.7, 0.2, 0.5]
    d = [_box(1, 3.0 * (k % 8) + 0.2 * (k // 8), s) for k, s in enumerate(scores)]
    frames = [(g, d, list(range(1, 9)), list(range(11, 21)))]
    frames.append((g, d, list(range(1, 9)), list(range(21, 31))))
    _run_both(frames)


def test_tid_reused_by_other_class_and_out_of_class_gts():
    # dt 11 tracks gt 1 (class 1); next frame tid 1 belongs to a gt of class 3 (outside classes) at the same place
    frames = [([_box(1, 0), _box(2, 10)], [_box(1, 0.1), _box(2, 10.1)], [1, 2], [11, 12]),
              ([_box(3, 0), _box(2, 10)], [_box(1, 0.1), _box(2, 10.1)], [1, 2], [11, 12]),
              ([_box(1, 0), _box(2, 10)], [_box(1, 0.1), _box(2, 10.1)], [1, 2], [11, 12])]
    _run_both(frames)


def test_invalid_tids_raise():
    ev = TrackingEvaluator(CLASSES, 0.5)
    g = np.asarray([_box(1, 0), _box(1, 5)], np.float32)
    with pytest.raises(AssertionError):
        ev.calc_stats(g, g, np.array([1, 2], np.uint64), np.array([0, 3], np.uint64))
    with pytest.raises(ValueError):
        ev.calc_stats(g, g, np.array([1, 1], np.uint64), np.array([2, 3], np.uint64))
    with pytest.raises(ValueError):
        ev.calc_stats(g, g, np.array([1, 2], np.uint64), np.array([3, 3], np.uint64))
