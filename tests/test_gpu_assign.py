"""GPU: linear_sum_assignment, HungarianMatcher and NearestNeighborMatcher against the reference's recorded results
(tests/golden/matcher_ref_cases.npz), bit for bit on the assignment, and against the literal restatement
(tests/assign_reference.py) on seeded frames.  No scipy needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases  # noqa: E402
import assign_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu


def run_gpu(kind, dist, stags, dtags, calls):
    """the matchers' bookkeeping over the array functions: NN skips boxes of earlier calls, Hungarian overwrites key by key"""
    from d3d_amd.tracking import hungarian_match, nearest_neighbor_match
    n, m = dist.shape
    d = torch.from_numpy(dist).cuda()
    sa, da, out = {}, {}, []
    for s, dd, thr in calls:
        if kind == "hungarian":
            sm, _ = hungarian_match(d, stags, dtags, thr, s, dd)
        else:
            sf, df = np.ones((n,), bool), np.ones((m,), bool)
            sf[list(sa)] = False
            df[list(da)] = False
            sm, _ = nearest_neighbor_match(d, stags, dtags, thr, s, dd, sf, df)
        sm = sm.cpu().numpy()
        for i in np.nonzero(sm >= 0)[0].tolist():
            sa[i] = int(sm[i])
            da[int(sm[i])] = i
        out.append(assign_cases.as_arrays(sa, da, n, m))
    return out


@pytest.mark.parametrize("kind", ["hungarian", "nn"])
def test_golden_cases(kind):
    for name, dist, stags, dtags, calls, exp, nn_ties in assign_cases.match_cases():
        got = run_gpu(kind, dist, stags, dtags, calls)
        ref = exp[kind] if not (kind == "nn" and nn_ties) else \
            [assign_cases.as_arrays(*x, *dist.shape) for x in _restated(kind, dist, stags, dtags, calls)]
        for k, ((gs, gd), (es, ed)) in enumerate(zip(got, ref)):
            assert np.array_equal(gs, es) and np.array_equal(gd, ed), (name, k)


def _restated(kind, dist, stags, dtags, calls):
    sa, da, out = {}, {}, []
    fn = ar.hungarian_match if kind == "hungarian" else ar.nearest_neighbor_match
    for s, d, thr in calls:
        fn(dist, stags, dtags, s, d, thr, sa, da)
        out.append((dict(sa), dict(da)))
    return out


def test_lsap_golden_cases_bit_for_bit():
    from d3d_amd.tracking import linear_sum_assignment
    seen = 0
    for key, c, rows, cols in assign_cases.lsap_cases():
        a, b = linear_sum_assignment(c)
        assert a.dtype == np.int64 and b.dtype == np.int64
        assert np.array_equal(a, rows) and np.array_equal(b, cols), key
        seen += 1
    assert seen == 6


def test_lsap_against_the_restatement_seeded():
    from d3d_amd.tracking import linear_sum_assignment
    rng = np.random.default_rng(11)
    for t in range(60):
        nr, nc = (int(x) for x in rng.integers(1, 90, 2))
        c = (rng.integers(0, 6, (nr, nc)) * 0.5).astype(np.float64 if t % 2 else np.float32)
        if t % 3 == 0:
            c = rng.random((nr, nc)).astype(np.float32)
        a, b = linear_sum_assignment(c)
        ea, eb = ar.lsap(c)
        assert np.array_equal(a, ea) and np.array_equal(b, eb), (t, c.shape, c.dtype)


def test_lsap_batch_equals_single_calls_and_host_equals_device():
    from d3d_amd.tracking import linear_sum_assignment
    rng = np.random.default_rng(3)
    for shape in ((5, 40, 40), (4, 70, 50), (3, 30, 130)):
        c = (rng.integers(0, 5, shape) * 0.25).astype(np.float32)
        ba, bb = linear_sum_assignment(c)
        assert ba.shape == (shape[0], min(shape[1:])) and bb.shape == ba.shape
        ta, tb = linear_sum_assignment(torch.from_numpy(c))
        assert ta.device.type == "cpu" and np.array_equal(ta.numpy(), ba) and np.array_equal(tb.numpy(), bb)
        da, db = linear_sum_assignment(torch.from_numpy(c).cuda())
        assert da.is_cuda and np.array_equal(da.cpu().numpy(), ba) and np.array_equal(db.cpu().numpy(), bb)
        for k in range(shape[0]):
            a, b = linear_sum_assignment(c[k])
            assert np.array_equal(a, ba[k]) and np.array_equal(b, bb[k])
            ea, eb = ar.lsap(c[k])
            assert np.array_equal(a, ea) and np.array_equal(b, eb)


def test_lsap_invalid_entries_raise():
    from d3d_amd.tracking import hungarian_match, linear_sum_assignment
    for bad in (np.array([[1.0, np.nan], [0.0, 1.0]]), np.array([[1.0, -np.inf], [0.0, 1.0]], np.float32)):
        with pytest.raises(ValueError, match="invalid numeric entries"):
            linear_sum_assignment(bad)
    c = np.full((3, 3), np.inf)
    c[0, 0] = c[1, 1] = 1.0
    with pytest.raises(ValueError, match="infeasible"):
        linear_sum_assignment(c)
    a, b = linear_sum_assignment(np.array([[np.inf, 1.0], [2.0, np.inf]]))   # +inf entries are allowed
    assert a.tolist() == [0, 1] and b.tolist() == [1, 0]
    d = np.zeros((2, 2), np.float32)
    d[1, 0] = np.nan
    with pytest.raises(ValueError):
        hungarian_match(torch.from_numpy(d).cuda(), [0, 0], [0, 0], {0: 1.0})


@pytest.mark.parametrize("metric", [1, 2, 3])
def test_matchers_on_seeded_frames(metric):
    from d3d_amd.tracking import HungarianMatcher, NearestNeighborMatcher
    rng = np.random.default_rng(100 + metric)
    thr = {1: 0.7, 2: 0.8, 3: 0.9} if metric != 3 else {1: 2.0, 2: 1.0}      # (class 3 missing from the map: 0.0)
    for frame in range(4):
        src, dst = assign_cases.boxes_frame(rng, {1: 40 + 10 * frame, 2: 25, 3: 12})
        for cls, fn in ((HungarianMatcher, ar.hungarian_match), (NearestNeighborMatcher, ar.nearest_neighbor_match)):
            mt = cls()
            mt.prepare_boxes(src, dst, metric)
            dist = mt.distance_cache.cpu().numpy()
            stags, dtags = src[:, 0].astype(np.int64), dst[:, 0].astype(np.int64)
            calls = [(list(range(0, len(src), 2)), list(range(len(dst))), thr),     # two calls without clear_match
                     (list(range(len(src)))[::-1], list(range(len(dst))), thr)]
            sa, da = {}, {}
            for s, d, t in calls:
                mt.match(s, d, t)
                fn(dist, stags, dtags, s, d, t, sa, da)
                assert all(mt.query_src_match(i) == sa.get(i, -1) for i in range(len(src))), (cls.__name__, frame)
                assert all(mt.query_dst_match(j) == da.get(j, -1) for j in range(len(dst))), (cls.__name__, frame)
                assert mt.num_of_matches() == len(sa)
            mt.clear_match()
            assert mt.num_of_matches() == 0


def test_large_frame_2k_by_5k():
    """2000 x 5000 with a planted optimum: every row's planted column costs < 0.5, every other entry >= 1 -- the unique optimal
    assignment and the nearest-neighbour greedy are both the planted pairs; a threshold of 0.25 keeps those below it"""
    from d3d_amd.tracking import hungarian_match, nearest_neighbor_match
    rng = np.random.default_rng(2025)
    n, m = 2000, 5000
    d = (1.0 + rng.random((n, m))).astype(np.float32)
    perm = rng.permutation(m)[:n]
    planted = (rng.random(n) * 0.5).astype(np.float32)
    d[np.arange(n), perm] = planted
    exp = np.where(planted <= np.float32(0.25), perm, -1)
    dev = torch.from_numpy(d).cuda()
    for fn in (hungarian_match, nearest_neighbor_match):
        sm, dm = fn(dev, np.zeros(n), np.zeros(m), {0: 0.25})
        sm, dm = sm.cpu().numpy(), dm.cpu().numpy()
        assert np.array_equal(sm, exp), fn.__name__
        assert np.array_equal(np.nonzero(dm >= 0)[0], np.sort(exp[exp >= 0]))
    from d3d_amd.tracking import linear_sum_assignment
    a, b = linear_sum_assignment(dev)
    assert np.array_equal(a.cpu().numpy(), np.arange(n)) and np.array_equal(b.cpu().numpy(), perm)
