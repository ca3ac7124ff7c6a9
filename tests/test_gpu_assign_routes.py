"""GPU: every launch route of the LSAP and greedy-matcher kernels against a plain reference, assignments exact.

  * d3d_lsap_batched picks its route from the caller's stated max_rows / max_cols: 64 lanes with the solver's state in LDS,
    256 lanes in LDS, 256 lanes in the workspace, 1024 lanes in the workspace.  Stating larger bounds than a problem needs is
    legal, so the same seeded problems are solved on all four and checked against the restatement (tests/assign_reference.py);
    the large cases against scipy's recorded results (tests/golden/lsap_route_cases.npz).
  * d3d_nn_match: a chain that needs one round of k_nn_rounds per pair, the chunked column pass (more than 4 194 240 rows),
    edge values -- against the fast restatement of match_by_order.
  * d3d_score_match / _batched with the taken-bitmap in global memory (m > 262 144) -- against oracle.score_match_rows."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases  # noqa: E402
import assign_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu

def route(max_rows, max_cols):
    return assign_cases.route_generator().route(max_rows, max_cols)


# --------------------------------------------------------------------------------------------------------- LSAP launches
def lsap_launch(cost, ld, row_idx, col_idx, row_off, col_off, max_rows, max_cols, ws_bytes=None):
    """one d3d_lsap_batched call on a device matrix; the workspace is allocated at the size the library asks for, and
    `ws_bytes` (if given) is what the call is TOLD it holds.  -> (row_match, col_match) numpy int32, status int"""
    from d3d_amd import _lib
    lib = _lib.load()
    dev = cost.device
    B = len(row_off) - 1
    nrt, nct = int(row_off[-1]), int(col_off[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)      # noqa: E731
    ri, ci, ro, co = t(row_idx), t(col_idx), t(row_off), t(col_off)
    rm = torch.full((max(nrt, 1),), -7, dtype=torch.int32, device=dev)
    cm = torch.full((max(nct, 1),), -7, dtype=torch.int32, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    full = lib.d3d_lsap_batched_workspace_bytes(B, nrt, nct)
    ws = torch.empty((full,), dtype=torch.uint8, device=dev)
    rc = lib.d3d_lsap_batched(_lib.ptr(cost), _lib.F64 if cost.dtype == torch.float64 else _lib.F32, int(ld), _lib.ptr(ri),
                              _lib.ptr(ci), _lib.ptr(ro), _lib.ptr(co), B, int(max_rows), int(max_cols), _lib.ptr(rm), _lib.ptr(cm),
                              _lib.ptr(status), _lib.ptr(ws), full if ws_bytes is None else int(ws_bytes), _lib.stream_ptr())
    _lib.check(rc, "lsap_batched")
    return rm.cpu().numpy()[:nrt], cm.cpu().numpy()[:nct], int(status.cpu()[0])


class Packed:
    """problems gathered from one larger matrix: each block sits on rows / columns of its own, scattered at random; every
    other entry is NaN, so a read outside a problem's block shows as status bit 0 or a wrong result.  ld > every width."""

    def __init__(self, blocks, dtype, rng):
        R, C = sum(b.shape[0] for b in blocks) + 5, sum(b.shape[1] for b in blocks) + 3
        H = np.full((R, C), np.nan, dtype)
        rp, cp = rng.permutation(R), rng.permutation(C)
        self.rows, self.cols, r0, c0 = [], [], 0, 0
        for b in blocks:
            rr, cc = rp[r0:r0 + b.shape[0]], cp[c0:c0 + b.shape[1]]
            H[np.ix_(rr, cc)] = b
            self.rows.append(rr)
            self.cols.append(cc)
            r0, c0 = r0 + b.shape[0], c0 + b.shape[1]
        self.H = torch.from_numpy(H).cuda()
        self.ld = C

    def solve(self, which, max_rows, max_cols, ws_bytes=None):
        """problems `which` (indices into blocks) in one launch -> per problem (row_match, col_match), status"""
        rows = [self.rows[k] for k in which]
        cols = [self.cols[k] for k in which]
        ro = np.concatenate([[0], np.cumsum([r.size for r in rows])])
        co = np.concatenate([[0], np.cumsum([c.size for c in cols])])
        rm, cm, st = lsap_launch(self.H, self.ld, np.concatenate(rows), np.concatenate(cols), ro, co, max_rows, max_cols, ws_bytes)
        return [(rm[ro[k]:ro[k + 1]], cm[co[k]:co[k + 1]]) for k in range(len(which))], st


def expected(block):
    """the restatement's assignment as (row_match, col_match), or the ValueError's status bit"""
    nr, nc = block.shape
    try:
        a, b = ar.lsap(block)
    except ValueError as e:
        return np.full((nr,), -1, np.int32), np.full((nc,), -1, np.int32), 1 if "invalid" in str(e) else 2
    rm, cm = np.full((nr,), -1, np.int32), np.full((nc,), -1, np.int32)
    rm[a], cm[b] = b, a
    return rm, cm, 0


def feasible_inf(rng, shape, dtype):
    """ties with 40 % +inf entries, one full assignment kept finite"""
    c = (rng.integers(0, 8, shape) * 0.25).astype(dtype)
    c[rng.random(shape) < 0.4] = np.inf
    k = min(shape)
    r, q = rng.permutation(shape[0])[:k], rng.permutation(shape[1])[:k]
    c[r, q] = (rng.integers(0, 8, k) * 0.25).astype(dtype)
    return c


def small_problems(rng, dtype):
    """seeded problems of at most 60 a side (they fit the 64-lane route): 1xk, kx1, square, wide, tall; ties, constant, +inf,
    negative; for fp64 values 1e-13 apart on a quantized base and magnitudes near 1e300 and 1e308"""
    U = lambda *s: rng.random(s).astype(dtype)                                   # noqa: E731
    T = lambda *s: (rng.integers(0, 8, s) * 0.25).astype(dtype)                  # noqa: E731
    p = [U(1, 1), U(1, 60), U(60, 1), T(1, 45), T(45, 1), T(60, 60), T(37, 60), T(60, 41), U(23, 23), U(52, 60), U(60, 17),
         np.full((30, 45), 1.5, dtype), np.full((45, 30), 0.0, dtype), feasible_inf(rng, (40, 50), dtype),
         feasible_inf(rng, (50, 40), dtype), (T(50, 33) - 1.0).astype(dtype), (T(33, 50) - 1.75).astype(dtype)]
    if dtype == np.float64:
        near = lambda *s: 1.0 + rng.integers(0, 4, s) * 0.5 + rng.integers(0, 3, s) * 1e-13      # noqa: E731
        p += [near(40, 60), near(60, 40), near(60, 60), rng.random((30, 40)) * 1e300, rng.integers(1, 8, (40, 30)) * 2.5e307,
              rng.integers(1, 8, (25, 25)) * 2.5e307]
    return p


def medium_problems(rng, dtype):
    T = lambda *s: (rng.integers(0, 8, s) * 0.25).astype(dtype)                  # noqa: E731
    return [T(120, 200), T(200, 120), rng.random((150, 150)).astype(dtype), feasible_inf(rng, (90, 200), dtype)]


SMALL_BOUNDS = [(60, 60), (60, 1000), (60, 1600), (60, 2100)]
MEDIUM_BOUNDS = [(200, 200), (200, 1600), (200, 2100)]


def test_declared_bounds_select_every_route():
    """the host rule, recomputed: a later change of the thresholds must fail here, not silently stop covering a route"""
    assert [route(*b) for b in SMALL_BOUNDS] == [(64, "lds"), (256, "lds"), (256, "workspace"), (1024, "workspace")]
    assert [route(*b) for b in MEDIUM_BOUNDS] == [(256, "lds"), (256, "workspace"), (1024, "workspace")]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lsap_every_route_against_the_restatement(dtype):
    """the same problems, gathered from a NaN-filled matrix (ld > width, permuted row / column indices), on every route: alone
    and all in one launch; every route gives the restatement's assignment, so all routes agree"""
    rng = np.random.default_rng(7 if dtype == np.float32 else 8)
    for problems, bounds in ((small_problems(rng, dtype), SMALL_BOUNDS), (medium_problems(rng, dtype), MEDIUM_BOUNDS)):
        pk = Packed(problems, dtype, rng)
        exp = [expected(b) for b in problems]
        assert all(e[2] == 0 for e in exp)
        for mr, mc in bounds:
            got, st = pk.solve(range(len(problems)), mr, mc)
            assert st == 0, (mr, mc)
            for k, ((rm, cm), (er, ec, _)) in enumerate(zip(got, exp)):
                assert np.array_equal(rm, er) and np.array_equal(cm, ec), (route(mr, mc), k, problems[k].shape)
            for k in range(len(problems)):
                (rm, cm), = pk.solve([k], mr, mc)[0]
                assert np.array_equal(rm, exp[k][0]) and np.array_equal(cm, exp[k][1]), ("alone", route(mr, mc), k)


def test_near_ties_decide_the_answer():
    """the fp64 near-tie problems are a test of the fp64 cost read only if reading them as fp32 changes the answer"""
    rng = np.random.default_rng(8)
    near = small_problems(rng, np.float64)[-6:-3]
    assert any(not np.array_equal(ar.lsap(c)[1], ar.lsap(c.astype(np.float32))[1]) for c in near)


@pytest.mark.parametrize("bounds", [(60, 1600), (60, 2100)])
def test_lsap_status_bits_on_the_workspace_routes(bounds):
    """bit 0: a NaN at the LAST element of a problem (its four-loads-per-thread scan clamps there); bit 1: an infeasible
    problem; the problems' matches stay -1 and the others in the launch are solved"""
    rng = np.random.default_rng(9)
    ok1 = (rng.integers(0, 8, (37, 53)) * 0.25).astype(np.float64)
    nan1 = rng.random((37, 53))
    nan1[-1, -1] = np.nan
    nan2 = rng.random((32, 128))                                   # 4096 entries: four full passes of 1024 lanes
    nan2[-1, -1] = np.nan
    inf = np.full((20, 30), np.inf)
    inf[:, 0] = 1.0                                                # every row needs column 0
    ok2 = rng.random((60, 25))
    blocks = [ok1, nan1, inf, nan2, ok2]
    assert route(*bounds)[1] == "workspace"
    pk = Packed(blocks, np.float64, rng)
    got, st = pk.solve(range(len(blocks)), *bounds)
    assert st == 3, st
    for k, b in enumerate(blocks):
        er, ec, bit = expected(b)
        assert bit == {1: 1, 2: 2, 3: 1}.get(k, 0)
        assert np.array_equal(got[k][0], er) and np.array_equal(got[k][1], ec), k


@pytest.mark.parametrize("bounds", [(60, 1600), (60, 2100)])
def test_lsap_too_big_and_short_workspace_set_bit_2(bounds):
    """bit 2: a problem beyond the stated bounds (rows, or columns), or one whose state would run past the workspace -- the
    workspace is allocated in full and only its stated size is cut short, so a broken guard cannot write outside memory"""
    rng = np.random.default_rng(10)
    mr, mc = bounds
    blocks = [rng.random((30, 40)), rng.random((mr + 1, 20)), rng.random((5, mc + 1)), rng.random((50, 45))]
    pk = Packed(blocks, np.float64, rng)
    got, st = pk.solve(range(4), mr, mc)
    assert st == 4, st
    for k in (0, 3):
        er, ec, _ = expected(blocks[k])
        assert np.array_equal(got[k][0], er) and np.array_equal(got[k][1], ec), k
    for k in (1, 2):
        assert (got[k][0] == -1).all() and (got[k][1] == -1).all(), k
    # three problems: the last one's state ends at (ro + co + NR + NC) * 32 bytes
    fit = [blocks[0], blocks[3], rng.random((40, 60))]
    pk = Packed(fit, np.float64, rng)
    need = (30 + 50 + 40 + 60 + 45 + 40) * 32
    got, st = pk.solve(range(3), mr, mc, ws_bytes=need)
    assert st == 0
    for k in range(3):
        er, ec, _ = expected(fit[k])
        assert np.array_equal(got[k][0], er) and np.array_equal(got[k][1], ec), k
    got, st = pk.solve(range(3), mr, mc, ws_bytes=need - 1)
    assert st == 4, st
    for k in range(2):
        er, ec, _ = expected(fit[k])
        assert np.array_equal(got[k][0], er) and np.array_equal(got[k][1], ec), k
    assert (got[2][0] == -1).all() and (got[2][1] == -1).all()


# ---------------------------------------------------------------------------------------- large problems: scipy's goldens
def test_lsap_route_goldens_bit_for_bit():
    from d3d_amd.tracking import linear_sum_assignment
    seen = set()
    for name, c, rows, cols, m in assign_cases.route_cases():
        assert route(*c.shape) == tuple(m["route"]), name
        seen.add(route(*c.shape))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = linear_sum_assignment(c)
        dt = time.perf_counter() - t0
        assert np.array_equal(a, rows) and np.array_equal(b, cols), name
        da, db = linear_sum_assignment(torch.from_numpy(c).cuda())
        assert da.is_cuda and np.array_equal(da.cpu().numpy(), rows) and np.array_equal(db.cpu().numpy(), cols), name
        print("%s %s: %.1f ms" % (name, c.shape, dt * 1e3))
    assert seen == {(256, "lds"), (256, "workspace"), (1024, "workspace")}


def test_lsap_route_goldens_as_one_batch_on_1024_lanes():
    """the 1024-lane cases of one shape and dtype in one batch: several problems per launch on the largest route"""
    from d3d_amd.tracking import linear_sum_assignment
    cases = {name: (c, rows, cols) for name, c, rows, cols, m in assign_cases.route_cases()}
    c1, r1, k1 = cases["t500x2049"]
    c2 = np.ascontiguousarray(cases["t2049x500"][0].T)                # the tall case's transpose: scipy's answer transposed
    rt, kt = cases["t2049x500"][1:]
    a, b = linear_sum_assignment(np.stack([c1, c2]))
    assert np.array_equal(a[0], r1) and np.array_equal(b[0], k1)
    # (scipy's tall result is ordered by row: as the transposed problem it is (kt, rt), re-sorted by kt's position)
    assert np.array_equal(a[1], np.arange(500)) and np.array_equal(b[1][kt], rt)


def test_hungarian_frame_small_classes_on_the_workspace_route():
    """one frame of three classes (about 1200, 300 and 40 a side, tags interleaved, subsets shuffled): in one launch the large
    class sends the small ones through the 256-lane workspace route; each class equals its own single-class call (its own
    smaller route), the small classes the restatement, the large class scipy's recorded result"""
    from d3d_amd.tracking import hungarian_match
    dist, stags, dtags, ssub, dsub, thr, large, lrows, lcols, lr, lc = assign_cases.route_frame()
    d = torch.from_numpy(dist).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sm, dm = hungarian_match(d, stags, dtags, thr, ssub, dsub)
    sm, dm = sm.cpu().numpy(), dm.cpu().numpy()
    print("frame: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    for cls in (7, 3, 12):
        s1 = [s for s in ssub if stags[s] == cls]
        d1 = [x for x in dsub if dtags[x] == cls]
        a, b = hungarian_match(d, stags, dtags, thr, s1, d1)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(sm[s1], a[s1]) and np.array_equal(dm[d1], b[d1]), cls
    assert (sm[stags == 5] == -1).all()

    def solver(block):
        if block.shape == (len(lrows), len(lcols)):
            assert np.array_equal(block, dist[np.ix_(lrows, lcols)])
            return lr, lc
        return ar.lsap(block)
    sa, da = ar.hungarian_match(dist, stags, dtags, ssub, dsub, thr, solver=solver)
    es, ed = assign_cases.as_arrays(sa, da, *dist.shape)
    assert np.array_equal(sm, es) and np.array_equal(dm, ed)
    assert (sm[lrows] >= 0).sum() > 100 and (sm[stags == 12] >= 0).sum() > 5


# ------------------------------------------------------------------------------------------- nearest-neighbour greedy
def nn_gpu(dist, stags, dtags, thr, ssub, dsub, sfree=None, dfree=None):
    from d3d_amd.tracking import nearest_neighbor_match
    d = dist if isinstance(dist, torch.Tensor) else torch.from_numpy(dist).cuda()
    sm, dm = nearest_neighbor_match(d, stags, dtags, thr, ssub, dsub, sfree, dfree)
    return sm.cpu().numpy(), dm.cpu().numpy()


def nn_expected(dist, stags, dtags, thr, ssub, dsub, sfree=None, dfree=None):
    """the fast restatement; boxes that are not free enter as keys of the assignment maps and are dropped from the result"""
    n, m = dist.shape
    sa = {} if sfree is None else {int(i): -2 for i in np.nonzero(~sfree)[0]}
    da = {} if dfree is None else {int(j): -2 for j in np.nonzero(~dfree)[0]}
    sa, da = ar.nearest_neighbor_match_fast(dist, stags, dtags, ssub, dsub, thr, sa, da)
    return assign_cases.as_arrays({i: j for i, j in sa.items() if j >= 0}, {j: i for j, i in da.items() if i >= 0}, n, m)


def test_nn_chain_of_decreasing_pairs():
    """along one path r0 c0 r1 c1 ... every vertex's least edge is its next one: the only mutual pair is the last, so
    k_nn_rounds matches one pair per round -- 3000 rounds -- while a random background on two other tags is matched too"""
    rng = np.random.default_rng(12)
    L, nb = 3000, 400
    n = m = L + nb
    rp, cp = rng.permutation(n), rng.permutation(m)                 # path vertex k = row rp[k], column cp[k]
    dist = (rng.integers(0, 64, (n, m)) / 64.0).astype(np.float32)
    stags, dtags = np.zeros(n, np.int64), np.zeros(m, np.int64)
    stags[rp[L:]] = rng.integers(2, 4, nb)
    dtags[cp[L:]] = rng.integers(2, 4, nb)
    stags[rp[:L]] = dtags[cp[:L]] = 1
    dist[np.ix_(rp[:L], cp[:L])] = 1e5
    k = np.arange(L)
    dist[rp[k], cp[k]] = 2.0 * L - 2 * k
    dist[rp[k[1:]], cp[k[:-1]]] = 2.0 * L - 2 * k[1:] + 1
    thr = {1: 4.0 * L, 2: 0.5, 3: 0.75}
    ssub, dsub = rng.permutation(n), rng.permutation(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sm, dm = nn_gpu(dist, stags, dtags, thr, ssub, dsub)
    print("chain: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    es, ed = nn_expected(dist, stags, dtags, thr, ssub, dsub)
    assert np.array_equal(sm[rp[:L]], cp[:L])                         # the whole diagonal of the path
    assert np.array_equal(sm, es) and np.array_equal(dm, ed)


def test_nn_chunked_column_pass():
    """more than 4 194 240 source rows against 6 destinations: k_nn_propose_cols runs chunks of more than 64 rows.  The least
    pairs are planted at the last row, at the first row past 64 x 65535 and at chunk ends; ties at 0 elsewhere"""
    rng = np.random.default_rng(13)
    ns, nd = 4_200_000, 6
    dist = (rng.integers(0, 1 << 16, (ns, nd)) / 65536.0).astype(np.float32)
    stags = rng.integers(0, 2, ns).astype(np.int64)
    dtags = np.array([0, 0, 0, 1, 1, 1], np.int64)
    chunk = -(-ns // 65535)
    assert chunk > 64
    for j, r in enumerate((ns - 1, 64 * 65535, chunk * 1000 - 1, chunk * 1000, ns - 2)):
        dist[r, j] = -1.0
        stags[r] = dtags[j]
    thr = {0: 0.002, 1: 0.001}
    ssub, dsub = np.arange(ns), np.arange(nd)
    sm, dm = nn_gpu(dist, stags, dtags, thr, ssub, dsub)
    es, ed = nn_expected(dist, stags, dtags, thr, ssub, dsub)
    assert np.array_equal(dm, ed) and np.array_equal(sm, es)
    assert dm[0] == ns - 1 and dm[1] == 64 * 65535 and (dm >= 0).all()


def test_nn_edge_values_on_2k_frames():
    """-0.0 beside +0.0, +inf under an inf threshold, NaN, negative distances, a tag missing from the threshold map, free
    masks and permuted subsets, 2000 x 2000 across four tags"""
    rng = np.random.default_rng(14)
    for t in range(3):
        d, stags, dtags, thr, ssub, dsub, sfree, dfree = assign_cases.nn_edge_frame(rng, 2000, 2000)
        if t == 0:
            sfree = dfree = None
        sm, dm = nn_gpu(d, stags, dtags, thr, ssub, dsub, sfree, dfree)
        es, ed = nn_expected(d, stags, dtags, thr, ssub, dsub, sfree, dfree)
        assert np.array_equal(sm, es) and np.array_equal(dm, ed), t
        hit = d[np.nonzero(sm >= 0)[0], sm[sm >= 0]]
        assert np.isinf(hit).any() and (hit < 0).any() and (np.signbit(hit) & (hit == 0)).any(), t


# ------------------------------------------------------------------------- score-ordered greedy, bitmap in global memory
def _score_frame(rng, n, m):
    """every row's nearest destinations are nearly the same (a common base plus a little per-row noise), so later rows find
    their 64 listed candidates taken and sweep their whole row; thresholds loose enough for tens of thousands of candidates"""
    base = rng.integers(0, 4096, m) / 4096.0
    dist = (base[None, :] + rng.integers(0, 4, (n, m)) / 4096.0).astype(np.float32)
    stags = rng.integers(0, 2, n).astype(np.int64)
    dtags = rng.integers(0, 3, m).astype(np.int64)               # tag 2: not in the threshold map
    scores = (rng.permutation(n) / n).astype(np.float32)
    return dist, stags, dtags, scores, {0: 0.5, 1: 0.3}


def test_score_match_global_bitmap_route():
    import oracle
    from d3d_amd.tracking import score_match
    rng = np.random.default_rng(15)
    n, m = 300, 270_000
    assert (m + 31) // 32 * 4 > 32 * 1024
    dist, stags, dtags, scores, thr = _score_frame(rng, n, m)
    d = torch.from_numpy(dist).cuda()
    sm, dm = score_match(d, scores, stags, dtags, thr)
    esm, edm = oracle.score_match_rows(dist, np.stack([stags, scores], 1), np.stack([dtags, dtags], 1), thr)
    assert np.array_equal(sm.cpu().numpy(), esm) and np.array_equal(dm.cpu().numpy(), edm)
    assert (esm >= 0).all()
    # rows that could take none of their 64 nearest acceptable destinations: the sweep of the whole row decided them
    swept = 0
    for s in range(n):
        ok = dist[s][(dtags == stags[s]) & (dist[s] <= np.float32(thr[int(stags[s])]))]
        swept += int(dist[s, esm[s]] > np.partition(ok, 63)[63])
    assert swept > 50, swept


def test_reference_association_global_bitmap_route():
    """ReferenceAssociation at m > 262 144: match_many (d3d_score_match_batched) equals one-by-one `match`; a subset given in
    descending score order pairs every source with its own row, which is score_match"""
    from d3d_amd.tracking import matcher, score_match
    rng = np.random.default_rng(16)
    n, m = 200, 270_000
    dist, stags, dtags, scores, thr = _score_frame(rng, n, m)
    d = torch.from_numpy(dist).cuda()
    assoc = matcher.ReferenceAssociation(d, scores, stags, dtags, thr, np.arange(m))
    by_score = np.argsort(-scores, kind="stable")
    subsets = [by_score, np.nonzero(scores >= 0.5)[0], rng.permutation(n)[:120], np.array([5])]
    sm, dm = assoc.match_many(subsets)
    for t, sub in enumerate(subsets):
        s1, d1 = assoc.match(sub)
        assert torch.equal(sm[t], s1) and torch.equal(dm[t], d1), t
    ssm, sdm = score_match(d, scores, stags, dtags, thr)
    assert torch.equal(sm[0], ssm) and torch.equal(dm[0], sdm)
    assert int((sm[0] >= 0).sum()) == n
