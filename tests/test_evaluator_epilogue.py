"""CPU: the two functions every evaluator epilogue of d3d_amd.benchmarks goes through -- the accuracy terms of matched pairs
against the reference's own expressions, and the counts and means per bin against a plain loop -- bit for bit."""
import math

import numpy as np

from d3d_amd.benchmarks import _ACC_FIELDS, _bin_means, _pair_terms


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def test_pair_terms_are_the_references_expressions_bit_for_bit():
    """diffnorm3 of the positions and of the dimensions as np.linalg.norm(., axis=1) of the fp32 rows, quatdiff of two yaw
    rotations / pi as |wrap(dyaw)| / pi in fp32 (benchmarks.pyx:252-257), the IoU handed through; rows at the scales 1e-20
    (squares are denormal or 0), 1, 50 and 1e18 (squares near fp32's end), and rows holding 0, denormals, +-inf and NaN"""
    rng = np.random.default_rng(2024)
    K = 4000
    scale = np.repeat(np.array([1e-20, 1.0, 50.0, 1e18], np.float32), K // 4)[:, None]
    ga = (rng.standard_normal((K, 9)) * scale).astype(np.float32)
    da = (rng.standard_normal((K, 9)) * scale).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -3e-39, 1e18, -1e18, np.inf, -np.inf, np.nan, 1.0], np.float32)
    rows = rng.permutation(K)[:600]
    ga[rows[:400], rng.integers(2, 9, 400)] = special[rng.integers(0, len(special), 400)]
    da[rows[200:], rng.integers(2, 9, 400)] = special[rng.integers(0, len(special), 400)]
    ga[rows[:50]] = da[rows[:50]]                                    # equal rows: every term 0
    iou = rng.random(K).astype(np.float32)
    with np.errstate(all="ignore"):
        got = _pair_terms(ga, da, iou)
        dyaw = ga[:, 8] - da[:, 8]
        pi, two_pi = np.float32(np.pi), np.float32(2 * np.pi)
        want = (iou, np.abs(np.mod(dyaw + pi, two_pi) - pi) / pi,
                np.linalg.norm(ga[:, 2:5] - da[:, 2:5], axis=1), np.linalg.norm(ga[:, 5:8] - da[:, 5:8], axis=1))
    assert len(got) == 4 == len(_ACC_FIELDS) - 1 and _ACC_FIELDS[:4] == ("acc_iou", "acc_angular", "acc_dist", "acc_box")
    for name, g, w in zip(_ACC_FIELDS, got, want):
        assert g.shape == (K,) and np.array_equal(_bits(g), _bits(w)), (name, np.nonzero(_bits(g) != _bits(w))[0][:5])
    assert np.isnan(got[2]).sum() > 10 and np.isinf(got[2]).sum() > 10 and (got[2] == 0).sum() >= 50      # the specials took part
    empty = _pair_terms(ga[:0], da[:0], iou[:0])
    assert all(t.shape == (0,) and t.dtype == np.float32 for t in empty)


def test_bin_means_are_a_plain_loop_over_the_pairs():
    """per bin: the pairs counted, each term summed in float64 in the order of the pairs, one division, one rounding to fp32; a bin
    without a pair has count 0, means NaN and acc_var NaN, every other acc_var -inf.  Two bins hold sequences whose mean tells an
    fp32 accumulation ([1e8, 1, -1e8]: 0 instead of 1/3) and a reordered one ([2^60, 1, -2^60, 1]: 1/2 or 0 instead of 1/4) apart."""
    rng = np.random.default_rng(7)
    shape = (3, 5, 4)
    nbins = math.prod(shape)
    used = rng.permutation(nbins)[:40]                                # 20 bins stay empty
    single, many, probe_a, probe_b = used[:8], used[8:38], int(used[38]), int(used[39])
    key = np.concatenate([single, many[rng.integers(0, len(many), 3000)]])
    terms = [(rng.standard_normal(len(key)) * s).astype(np.float32) for s in (1.0, 1e-3, 1e6, 1e-30)]
    at = np.sort(rng.permutation(len(key))[:7])                       # the probes' pairs lie between the others, in this order
    key = np.insert(key, at, [probe_a, probe_b, probe_a, probe_b, probe_a, probe_b, probe_b])
    probe = np.array([1e8, 2.0 ** 60, 1, 1, -1e8, -2.0 ** 60, 1], np.float32)
    terms = [np.insert(t, at, probe) for t in terms]
    key = key.astype(np.int64)
    tp, acc = _bin_means(key, shape, terms)
    count = [0] * nbins
    sums = [[0.0] * nbins for _ in terms]
    for i, b in enumerate(key.tolist()):
        count[b] += 1
        for s, t in zip(sums, terms):
            s[b] += float(t[i])
    assert tp.shape == shape and tp.dtype.kind == "i" and tp.reshape(-1).tolist() == count
    assert count.count(0) == 20 and count.count(1) == 8 and count[probe_a] == 3 and count[probe_b] == 4 and max(count) > 50
    assert len(acc) == len(_ACC_FIELDS) == len(terms) + 1
    for s, got in zip(sums, acc):
        want = np.array([np.float32(s[b] / count[b]) if count[b] else np.float32(np.nan) for b in range(nbins)], np.float32)
        assert got.shape == shape
        assert np.array_equal(_bits(got).reshape(-1), _bits(want)), np.nonzero(_bits(got).reshape(-1) != _bits(want))[0]
        assert got.reshape(-1)[probe_a] == np.float32(1 / 3) and got.reshape(-1)[probe_b] == np.float32(0.25)
    var = acc[-1].reshape(-1)
    assert acc[-1].shape == shape
    assert all((math.isnan(v) if n == 0 else v == -math.inf) for v, n in zip(var.tolist(), count))
    tp0, acc0 = _bin_means(np.zeros((0,), np.int64), (2, 3), [np.zeros((0,), np.float32)] * 4)
    assert tp0.tolist() == [[0] * 3] * 2 and all(np.isnan(a).all() and a.shape == (2, 3) for a in acc0)
