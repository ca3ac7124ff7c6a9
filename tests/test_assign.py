"""CPU: the literal restatement of the reference's association steps (tests/assign_reference.py) against the reference's
recorded results and, where scipy is installed, against scipy itself; argument validation of the new entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases  # noqa: E402
import assign_reference as ar  # noqa: E402


def run_reference(kind, dist, stags, dtags, calls):
    sa, da, out = {}, {}, []
    fn = ar.hungarian_match if kind == "hungarian" else ar.nearest_neighbor_match
    for s, d, thr in calls:
        fn(dist, stags, dtags, s, d, thr, sa, da)
        out.append(assign_cases.as_arrays(sa, da, *dist.shape))
    return out


@pytest.mark.parametrize("kind", ["hungarian", "nn"])
def test_restatement_equals_the_reference_goldens(kind):
    seen = 0
    for name, dist, stags, dtags, calls, exp, nn_ties in assign_cases.match_cases():
        if kind == "nn" and nn_ties:
            continue              # the reference's unstable argsort leaves the order of equal distances open
        got = run_reference(kind, dist, stags, dtags, calls)
        for k, ((gs, gd), (es, ed)) in enumerate(zip(got, exp[kind])):
            assert np.array_equal(gs, es) and np.array_equal(gd, ed), (name, k)
        seen += 1
    assert seen >= (12 if kind == "hungarian" else 5)


def test_restatement_lsap_equals_the_recorded_scipy_results():
    for key, c, rows, cols in assign_cases.lsap_cases():
        if c.size > 300 * 300:
            continue              # (1000 x 3000: the GPU test checks it; pure Python takes minutes)
        a, b = ar.lsap(c)
        assert np.array_equal(a, rows) and np.array_equal(b, cols), key


def test_restatement_lsap_equals_scipy_on_seeded_matrices():
    sp = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    for t in range(300):
        nr, nc = (int(x) for x in rng.integers(1, 20, 2))
        kind = t % 4
        if kind == 0:
            c = rng.integers(0, 3, (nr, nc)).astype(np.float64)
        elif kind == 1:
            c = (rng.integers(0, 8, (nr, nc)) * 0.25).astype(np.float32)
        elif kind == 2:
            c = rng.random((nr, nc)).astype(np.float32)
        else:
            c = rng.integers(0, 4, (nr, nc)).astype(np.float64)
            c[rng.random((nr, nc)) < 0.3] = np.inf
        try:
            exp = sp.linear_sum_assignment(c)
        except ValueError as e:
            with pytest.raises(ValueError, match=str(e)):
                ar.lsap(c)
            continue
        a, b = ar.lsap(c)
        assert np.array_equal(a, exp[0]) and np.array_equal(b, exp[1]), (t, c)
    for bad in (np.array([[1.0, np.nan]]), np.array([[-np.inf, 1.0]])):
        with pytest.raises(ValueError):
            sp.linear_sum_assignment(bad)
        with pytest.raises(ValueError):
            ar.lsap(bad)


def test_constant_matrix_gives_the_identity():
    a, b = ar.lsap(np.ones((6, 6)))
    assert np.array_equal(a, np.arange(6)) and np.array_equal(b, np.arange(6))


def test_argument_validation_without_gpu():
    from d3d_amd.tracking import HungarianMatcher, NearestNeighborMatcher, hungarian_match, linear_sum_assignment, nearest_neighbor_match
    with pytest.raises(ValueError):
        linear_sum_assignment(np.zeros((3,)))
    with pytest.raises(ValueError):
        linear_sum_assignment(np.zeros((2, 2, 2, 2)))
    a, b = linear_sum_assignment(np.zeros((0, 4)))            # empty: nothing to solve, no device needed
    assert a.shape == (0,) and b.shape == (0,) and a.dtype == np.int64
    with pytest.raises(ValueError):
        hungarian_match(np.zeros((3,), np.float32), [0, 0, 0], [0], {0: 1.0})
    with pytest.raises(ValueError):
        nearest_neighbor_match(np.zeros((3,), np.float32), [0, 0, 0], [0], {0: 1.0})
    for cls in (HungarianMatcher, NearestNeighborMatcher):
        mt = cls()
        with pytest.raises(ValueError):
            mt.prepare_boxes(np.zeros((2, 8), np.float32), np.zeros((2, 9), np.float32), 3)
        mt.prepare_boxes(np.zeros((0, 9), np.float32), np.zeros((2, 9), np.float32), 3)     # empty: matcher.pyx:41-43
        mt.match([], [0, 1], {0: 1.0})
        assert mt.num_of_matches() == 0 and mt.query_src_match(0) == -1 and mt.query_dst_match(1) == -1


# --------------------------------------------------------------- tests/golden/lsap_route_cases.npz: the large launch routes
def test_route_goldens_regenerate_and_name_their_routes():
    g = assign_cases.route_generator()
    assert os.path.getsize(assign_cases.ROUTE_GOLDEN) < 500 * 1024
    z = np.load(assign_cases.ROUTE_GOLDEN)
    meta = __import__("json").loads(bytes(z["__meta__"]).decode())
    assert meta["scipy_version"]
    routes = set()
    for name, c, rows, cols, m in assign_cases.route_cases():
        assert tuple(m["route"]) == g.route(*c.shape), name
        k = min(c.shape)
        assert rows.shape == (k,) and cols.shape == (k,), name
        routes.add(tuple(m["route"]))
    assert routes == {(256, "lds"), (256, "workspace"), (1024, "workspace")}
    dist, stags, dtags, ssub, dsub, thr, large, rows, cols, r, k = assign_cases.route_frame()
    assert g.route(len(rows), len(cols)) == (256, "workspace") and r.shape == (min(len(rows), len(cols)),)
    for cls in (3, 12):     # the small classes take smaller routes on their own
        rr, cc, _ = g.class_block(dist, stags, dtags, ssub, dsub, cls)
        assert g.route(len(rr), len(cc)) == ((256, "lds") if cls == 3 else (64, "lds"))


def test_route_goldens_are_scipys_results():
    sp = pytest.importorskip("scipy.optimize")
    for name, c, rows, cols, m in assign_cases.route_cases():
        a, b = sp.linear_sum_assignment(c)
        assert np.array_equal(a, rows) and np.array_equal(b, cols), name
    dist, stags, dtags, ssub, dsub, thr, large, rr, cc, r, k = assign_cases.route_frame()
    a, b = sp.linear_sum_assignment(dist[np.ix_(rr, cc)])
    assert np.array_equal(a, r) and np.array_equal(b, k)


def test_restatement_equals_the_route_goldens():
    """every recorded case but the two uniform fp64 squares of 1500+ columns (minutes of pure Python): about 3 s"""
    seen = 0
    for name, c, rows, cols, m in assign_cases.route_cases():
        if m["kind"] == "uniform" and min(c.shape) > 1:
            continue
        a, b = ar.lsap(c)
        assert np.array_equal(a, rows) and np.array_equal(b, cols), name
        seen += 1
    assert seen == 9


def test_near_tie_golden_changes_when_read_as_fp32():
    """the near-tie case is only a test of the fp64 cost read if narrowing the matrix to fp32 changes scipy's answer"""
    sp = pytest.importorskip("scipy.optimize")
    for name, c, rows, cols, m in assign_cases.route_cases():
        if m["kind"] == "neartie":
            a, b = sp.linear_sum_assignment(c.astype(np.float32))
            assert not np.array_equal(b, cols), name


def _free_as_assigned(free, subset):
    """a box that is not free: a key of the assignment map (what an earlier call leaves), partner -2"""
    return {int(i): -2 for i in np.nonzero(~np.asarray(free, bool))[0]}


def test_fast_nn_restatement_equals_the_literal_one():
    rng = np.random.default_rng(41)
    for t in range(40):
        n, m = (int(x) for x in rng.integers(1, 70, 2))
        d, stags, dtags, thr, ssub, dsub, sfree, dfree = assign_cases.nn_edge_frame(rng, n, m)
        if t % 4 == 0:
            sfree[:], dfree[:] = True, True
        if t % 5 == 1:
            ssub, dsub = ssub[: 1 + t % 3], dsub[: 2]           # tiny calls: the literal's early exit applies
        sa0, da0 = _free_as_assigned(sfree, ssub), _free_as_assigned(dfree, dsub)
        lit = ar.nearest_neighbor_match(d, stags, dtags, ssub, dsub, thr, dict(sa0), dict(da0))
        fast = ar.nearest_neighbor_match_fast(d, stags, dtags, ssub, dsub, thr, dict(sa0), dict(da0))
        assert lit == fast, t
    # a chain of decreasing pairs (r0 c0 r1 c1 ...): the greedy takes the diagonal from the far end
    n = 50
    d = np.full((n, n), 1e6, np.float32)
    for k in range(n):
        d[k, k] = 2.0 * n - 2 * k
        if k + 1 < n:
            d[k + 1, k] = 2.0 * n - 2 * k - 1
    z = np.zeros(n, np.int64)
    lit = ar.nearest_neighbor_match(d, z, z, range(n), range(n), {0: 4.0 * n})
    fast = ar.nearest_neighbor_match_fast(d, z, z, range(n), range(n), {0: 4.0 * n})
    assert lit == fast and lit[0] == {k: k for k in range(n)}
