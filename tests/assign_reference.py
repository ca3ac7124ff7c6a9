"""A literal restatement, in plain Python, of the reference's association steps -- the checker of d3d_amd's LSAP and matcher
kernels.  No scipy: scipy's solver is restated from its algorithm (the shortest augmenting path method of Crouse 2016, scipy's
rectangular_lsap), one statement per statement, in the same fp64 arithmetic and the same evaluation order.

  * lsap(cost)                           = scipy.optimize.linear_sum_assignment(cost) (maximize=False)
  * match_by_order(...)                  = BaseMatcher.match_by_order (reference d3d/tracking/matcher.pyx:90-121)
  * nearest_neighbor_match(...)          = NearestNeighborMatcher.match (:164-186), the distance order made stable
  * hungarian_match(...)                 = HungarianMatcher.match (:188-230)

The match functions take and update the two assignment dicts, as the reference's unordered_maps persist between calls."""
import math

import numpy as np


def lsap(cost):
    """-> (row_ind, col_ind) int64 arrays; raises ValueError as scipy does (NaN / -inf entries, infeasible matrix)"""
    c = np.asarray(cost, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %r array" % (c.shape,))
    nr, nc = c.shape
    if nr == 0 or nc == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    transpose = nc < nr
    if transpose:
        c = c.T
        nr, nc = nc, nr
    if np.any(np.isnan(c)) or np.any(c == -math.inf):
        raise ValueError("matrix contains invalid numeric entries")
    cost = c.tolist()
    u = [0.0] * nr
    v = [0.0] * nc
    spc = [math.inf] * nc
    path = [-1] * nc
    col4row = [-1] * nr
    row4col = [-1] * nc
    for cur in range(nr):
        # augmenting_path
        minVal = 0.0
        remaining = [nc - it - 1 for it in range(nc)]
        num_remaining = nc
        SR = [False] * nr
        SC = [False] * nc
        spc = [math.inf] * nc
        i = cur
        sink = -1
        while sink == -1:
            index = -1
            lowest = math.inf
            SR[i] = True
            ci, ui = cost[i], u[i]
            for it in range(num_remaining):
                j = remaining[it]
                r = minVal + ci[j] - ui - v[j]
                if r < spc[j]:
                    path[j] = i
                    spc[j] = r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest = spc[j]
                    index = it
            minVal = lowest
            if minVal == math.inf:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        # update the dual variables
        u[cur] += minVal
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += minVal - spc[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= minVal - spc[j]
        # augment the previous solution
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transpose:
        order = sorted(range(nr), key=lambda k: col4row[k])
        return np.array([col4row[k] for k in order], np.int64), np.array(order, np.int64)
    return np.arange(nr, dtype=np.int64), np.array(col4row, np.int64)


def _thr(distance_threshold, tag):
    """unordered_map<int, float>::operator[]: a missing key reads as 0.0 (fp32)"""
    return float(np.float32(distance_threshold.get(int(tag), 0.0)))


def match_by_order(src_order, dst_order, distance, src_tags, dst_tags, distance_threshold, src_assignment, dst_assignment):
    """BaseMatcher.match_by_order, statement for statement; distance is the full fp32 cache, the tags per box"""
    assert len(src_order) == len(dst_order)
    for i in range(len(src_order)):
        src_idx, dst_idx = int(src_order[i]), int(dst_order[i])
        if src_idx in src_assignment:
            continue
        if dst_idx in dst_assignment:
            continue
        src_tag, dst_tag = int(src_tags[src_idx]), int(dst_tags[dst_idx])
        if src_tag != dst_tag:
            continue
        if float(distance[src_idx, dst_idx]) <= _thr(distance_threshold, dst_tag):
            src_assignment[src_idx] = dst_idx
            dst_assignment[dst_idx] = src_idx
        if len(src_assignment) == len(src_order):
            break
        if len(dst_assignment) == len(src_order):
            break


def nearest_neighbor_match(distance, src_tags, dst_tags, src_subset, dst_subset, distance_threshold,
                           src_assignment=None, dst_assignment=None):
    """NearestNeighborMatcher.match with a STABLE distance order (ties: row-major over the subset positions)"""
    src_assignment = {} if src_assignment is None else src_assignment
    dst_assignment = {} if dst_assignment is None else dst_assignment
    src_subset, dst_subset = [int(x) for x in src_subset], [int(x) for x in dst_subset]
    if not src_subset or not dst_subset:
        return src_assignment, dst_assignment
    sub = np.asarray(distance)[np.ix_(src_subset, dst_subset)]
    order = np.argsort(sub, axis=None, kind="stable")
    si, di = np.unravel_index(order, (len(src_subset), len(dst_subset)))
    match_by_order([src_subset[k] for k in si], [dst_subset[k] for k in di], distance, src_tags, dst_tags, distance_threshold,
                   src_assignment, dst_assignment)
    return src_assignment, dst_assignment


def nearest_neighbor_match_fast(distance, src_tags, dst_tags, src_subset, dst_subset, distance_threshold,
                                src_assignment=None, dst_assignment=None):
    """nearest_neighbor_match for large frames: match_by_order over the ACCEPTABLE free pairs only (tags agree, distance <=
    the threshold of the dst tag, neither side assigned before the call), stably sorted by (distance, src position, dst
    position).  The pairs left out never change match_by_order's state, so the result is the same -- except where
    match_by_order's early exit (an assignment map exactly as long as the whole pair list) can fire; such a small call is
    handed to the literal version."""
    src_assignment = {} if src_assignment is None else src_assignment
    dst_assignment = {} if dst_assignment is None else dst_assignment
    ssub, dsub = np.asarray(src_subset, np.int64).reshape(-1), np.asarray(dst_subset, np.int64).reshape(-1)
    if ssub.size == 0 or dsub.size == 0:
        return src_assignment, dst_assignment
    total = ssub.size * dsub.size
    if max(len(src_assignment), len(dst_assignment)) + min(ssub.size, dsub.size) >= total:
        return nearest_neighbor_match(distance, src_tags, dst_tags, ssub, dsub, distance_threshold, src_assignment, dst_assignment)
    st, dt = np.asarray(src_tags, np.int64)[ssub], np.asarray(dst_tags, np.int64)[dsub]
    thr = np.array([_thr(distance_threshold, t) for t in dt], np.float64)
    sfree = np.array([int(s) not in src_assignment for s in ssub])
    dfree = np.array([int(d) not in dst_assignment for d in dsub])
    sub = np.asarray(distance)[np.ix_(ssub, dsub)]
    ok = (st[:, None] == dt[None, :]) & (sub.astype(np.float64) <= thr[None, :]) & sfree[:, None] & dfree[None, :]
    si, di = np.nonzero(ok)                                  # row-major: (src position, dst position) ascending
    order = np.argsort(sub[si, di], kind="stable")           # (-0.0 and +0.0 compare equal, as in the literal sort)
    left_s, left_d = int(sfree.sum()), int(dfree.sum())
    for s, d in zip(ssub[si[order]].tolist(), dsub[di[order]].tolist()):
        if s in src_assignment or d in dst_assignment:
            continue
        src_assignment[s] = d
        dst_assignment[d] = s
        left_s, left_d = left_s - 1, left_d - 1
        if left_s == 0 or left_d == 0:                       # nothing later can match
            break
    return src_assignment, dst_assignment


def hungarian_match(distance, src_tags, dst_tags, src_subset, dst_subset, distance_threshold, src_assignment=None,
                    dst_assignment=None, solver=lsap):
    """HungarianMatcher.match, statement for statement (`solver` = scipy's linear_sum_assignment where it is wanted)"""
    src_assignment = {} if src_assignment is None else src_assignment
    dst_assignment = {} if dst_assignment is None else dst_assignment
    src_classes, dst_classes = {}, {}
    for src_idx in src_subset:
        src_classes.setdefault(int(src_tags[int(src_idx)]), []).append(int(src_idx))
    for dst_idx in dst_subset:
        dst_classes.setdefault(int(dst_tags[int(dst_idx)]), []).append(int(dst_idx))
    distance = np.asarray(distance)
    for clsid in src_classes.keys():
        if clsid not in dst_classes.keys():
            continue
        src_list, dst_list = src_classes[clsid], dst_classes[clsid]
        a, b = solver(distance[np.ix_(src_list, dst_list)])
        for i in range(len(a)):
            src_idx, dst_idx = src_list[a[i]], dst_list[b[i]]
            if float(distance[src_idx, dst_idx]) <= _thr(distance_threshold, clsid):
                src_assignment[src_idx] = dst_idx
                dst_assignment[dst_idx] = src_idx
    return src_assignment, dst_assignment
