"""Generate tests/golden/lsap_route_cases.npz: scipy.optimize.linear_sum_assignment on matrices large enough to reach the
large launch routes of d3d_lsap_batched (256 lanes with the solver's state in the workspace, 1024 lanes), where the plain
Python restatement (tests/assign_reference.py) is too slow to serve as the checker.

Data only: every matrix is regenerated from (kind, shape, dtype, seed) by `matrix` below and checked against a stored
SHA-256 of its bytes; the file holds scipy's row_ind / col_ind, the scipy version and the route each case is meant to reach
(`route`, the host rule of d3d_lsap_batched for the bounds linear_sum_assignment states: max_rows = n, max_cols = m).
Plus one HungarianMatcher frame of three classes (about 1200, 300 and 40 boxes a side, tags interleaved, subsets shuffled):
scipy's assignment of its large class, in subset order.

The generators import numpy only; scipy is imported by `main`.

usage: python tests/golden/make_lsap_route_golden.py"""
import hashlib
import json
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lsap_route_cases.npz")

# (name, kind, shape, dtype, seed)
CASES = [
    ("b1117", "ties", (1117, 1117), "float32", 11),          # 256 lanes, state 49 148 B: LDS
    ("b1118", "ties", (1118, 1118), "float32", 12),          # 256 lanes, state 49 192 B: workspace
    ("w1x1535", "uniform", (1, 1535), "float64", 13),        # 256 lanes, 49 132 B: LDS
    ("w1x1536", "uniform", (1, 1536), "float64", 14),        # 256 lanes, 49 164 B: workspace
    ("t300x1600", "ties", (300, 1600), "float32", 15),       # 256 lanes, workspace, wide
    ("t1600x300", "ties", (1600, 300), "float32", 16),       # 256 lanes, workspace, tall
    ("u2048x1500", "uniform", (2048, 1500), "float64", 17),  # 256 lanes, workspace, tall
    ("u2049x2049", "uniform", (2049, 2049), "float64", 18),  # 1024 lanes
    ("t500x2049", "ties", (500, 2049), "float32", 19),       # 1024 lanes, wide
    ("t2049x500", "ties", (2049, 500), "float32", 20),       # 1024 lanes, tall
    ("n700x3000", "neartie", (700, 3000), "float64", 21),    # 1024 lanes, values 1e-13 apart
]

# the Hungarian frame: class -> (sources, destinations); class 5 has no destinations (skipped, as the reference does)
FRAME_SEED = 31
FRAME_CLASSES = {7: (1200, 1190), 3: (300, 310), 12: (40, 38), 5: (9, 0)}
FRAME_THRESHOLD = {7: 1.25, 3: 1.5, 12: 2.0}
FRAME_LARGE = 7


def matrix(kind, shape, dtype, seed):
    """uniform: U[0, 1); ties: multiples of 0.25 in [0, 2); neartie (fp64 only): 1 plus a multiple of 0.5 plus 0, 1 or 2 x
    1e-13 -- reading it as fp32 merges the near-ties and changes the optimum"""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        c = rng.random(shape)
    elif kind == "ties":
        c = rng.integers(0, 8, shape) * 0.25
    elif kind == "neartie":
        assert dtype == "float64"
        c = 1.0 + rng.integers(0, 4, shape) * 0.5 + rng.integers(0, 3, shape) * 1e-13
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(c.astype(dtype))


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def route(max_rows, max_cols):
    """d3d_lsap_batched's launch route for the stated bounds (d3d_amd/csrc/assign.hip): kc = the larger bound, kr = the smaller,
    the solver's state 32 kc + 12 kr bytes -> (lanes, "lds" | "workspace")"""
    kc, kr = max(max_rows, max_cols), min(max_rows, max_cols)
    lanes = 64 if kc <= 64 else (256 if kc <= 2048 else 1024)
    return lanes, "lds" if 32 * kc + 12 * kr <= 48 * 1024 else "workspace"


def frame(seed=FRAME_SEED):
    """-> dist f32 [n, m] (multiples of 1/16 in [0, 4)), src_tags [n], dst_tags [m], src_subset, dst_subset: the classes'
    boxes interleaved, the subsets shuffled and a few boxes left out of each"""
    rng = np.random.default_rng(seed)
    stags = np.concatenate([np.full((s,), c, np.int64) for c, (s, _) in FRAME_CLASSES.items()])
    dtags = np.concatenate([np.full((d,), c, np.int64) for c, (_, d) in FRAME_CLASSES.items()])
    stags, dtags = stags[rng.permutation(stags.size)], dtags[rng.permutation(dtags.size)]
    dist = (rng.integers(0, 64, (stags.size, dtags.size)) / 16.0).astype(np.float32)
    ssub = rng.permutation(stags.size)[:stags.size - 7]
    dsub = rng.permutation(dtags.size)[:dtags.size - 5]
    return dist, stags, dtags, ssub, dsub


def class_block(dist, stags, dtags, ssub, dsub, cls):
    """the class's rows and columns in subset order (HungarianMatcher.match's split) and its cost block"""
    rows = [int(s) for s in ssub if stags[s] == cls]
    cols = [int(d) for d in dsub if dtags[d] == cls]
    return rows, cols, dist[np.ix_(rows, cols)]


def main():
    import scipy
    from scipy.optimize import linear_sum_assignment
    arrays, meta = {}, {"scipy_version": scipy.__version__, "cases": {}}
    for name, kind, shape, dtype, seed in CASES:
        c = matrix(kind, shape, dtype, seed)
        t0 = time.perf_counter()
        r, k = linear_sum_assignment(c)
        dt = time.perf_counter() - t0
        idx = np.int16 if max(shape) < 32768 else np.int32
        arrays[name + "/rows"], arrays[name + "/cols"] = r.astype(idx), k.astype(idx)
        meta["cases"][name] = {"kind": kind, "shape": list(shape), "dtype": dtype, "seed": seed, "sha256": sha256(c),
                               "route": list(route(*shape)), "scipy_seconds": round(dt, 3)}
        print("%-12s %-10s %s: route %s, scipy %.3f s" % (name, dtype, shape, route(*shape), dt))
    dist, stags, dtags, ssub, dsub = frame()
    rows, cols, block = class_block(dist, stags, dtags, ssub, dsub, FRAME_LARGE)
    r, k = linear_sum_assignment(block)
    arrays["frame/rows"], arrays["frame/cols"] = r.astype(np.int16), k.astype(np.int16)
    meta["frame"] = {"seed": FRAME_SEED, "sha256": sha256(dist), "large_class": FRAME_LARGE, "block_shape": list(block.shape),
                     "block_sha256": sha256(block), "route": list(route(*block.shape))}
    arrays["__meta__"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
