"""Shared helpers of the LSAP / matcher tests: the goldens of tests/golden/matcher_ref_cases.npz (written by
tests/golden/make_matcher_golden.py) and seeded frames."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matcher_ref_cases.npz")


def load():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["__meta__"]).decode())
    return z, meta


def match_cases():
    z, meta = load()
    for name, m in meta.items():
        if name.startswith("lsap/") or name == "time":
            continue
        calls = [(c["src"], c["dst"], {int(k): v for k, v in c["thr"].items()}) for c in m["calls"]]
        exp = {kind: [(z["%s/%s/%d/src" % (name, kind, k)], z["%s/%s/%d/dst" % (name, kind, k)]) for k in range(len(calls))]
               for kind in ("hungarian", "nn")}
        yield name, z[name + "/dist"], z[name + "/src_tags"], z[name + "/dst_tags"], calls, exp, m["nn_ties"]


def lsap_matrix(shape, seed):
    """the generator's tie-heavy matrix: multiples of 0.25 in [0, 2), fp32"""
    return (np.random.default_rng(seed).integers(0, 8, shape) * 0.25).astype(np.float32)


def lsap_cases():
    z, meta = load()
    for key, m in meta.items():
        if not key.startswith("lsap/"):
            continue
        shape = tuple(m["shape"])
        c = lsap_matrix(shape, m["seed"])
        chk = np.array([c.astype(np.float64).sum(), float((c * np.arange(c.size).reshape(shape) % 97).sum())])
        assert np.array_equal(chk, z[key + "/checksum"]), "%s: the seeded matrix is not the generator's" % key
        if key + "/cost" in z.files:
            assert np.array_equal(c, z[key + "/cost"])
        yield key, c, z[key + "/rows"].astype(np.int64), z[key + "/cols"].astype(np.int64)


def as_arrays(src_assignment, dst_assignment, n, m):
    s, d = np.full((n,), -1, np.int32), np.full((m,), -1, np.int32)
    for i, j in src_assignment.items():
        s[i] = j
    for j, i in dst_assignment.items():
        d[j] = i
    return s, d


def boxes_frame(rng, counts, spread=30.0, jitter=1.0):
    """[n,9] src and [m,9] dst boxes of several classes: dst scattered, src = dst moved a little (some dropped, some added)"""
    src, dst = [], []
    for cls, k in counts.items():
        d = np.zeros((k, 9), np.float32)
        d[:, 0] = cls
        d[:, 1] = rng.random(k)
        d[:, 2:4] = rng.uniform(-spread, spread, (k, 2))
        d[:, 4] = rng.uniform(-1, 1, k)
        d[:, 5:8] = rng.uniform(1, 4, (k, 3))
        d[:, 8] = rng.uniform(-3, 3, k)
        s = d[rng.random(k) > 0.15].copy()
        s[:, 2:5] += rng.normal(0, jitter, (len(s), 3)).astype(np.float32)
        s[:, 8] += rng.normal(0, 0.1, len(s)).astype(np.float32)
        s[:, 1] = rng.random(len(s))
        src.append(s)
        dst.append(d)
    s, d = np.concatenate(src), np.concatenate(dst)
    return s[rng.permutation(len(s))], d[rng.permutation(len(d))]


# ------------------------------------------------------------------------ tests/golden/lsap_route_cases.npz (scipy's results)
ROUTE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsap_route_cases.npz")


def route_generator():
    """tests/golden/make_lsap_route_golden.py as a module: the matrix generators and d3d_lsap_batched's route rule (numpy only)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_lsap_route_golden",
                                                  os.path.join(os.path.dirname(ROUTE_GOLDEN), "make_lsap_route_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def route_cases():
    """-> (name, cost, rows, cols, meta) per recorded case, the matrix regenerated and checked against its SHA-256"""
    g = route_generator()
    z = np.load(ROUTE_GOLDEN)
    meta = json.loads(bytes(z["__meta__"]).decode())
    for name, m in meta["cases"].items():
        c = g.matrix(m["kind"], tuple(m["shape"]), m["dtype"], m["seed"])
        assert g.sha256(c) == m["sha256"], "%s: the regenerated matrix is not the generator's" % name
        yield name, c, z[name + "/rows"].astype(np.int64), z[name + "/cols"].astype(np.int64), m


def route_frame():
    """-> (dist, src_tags, dst_tags, src_subset, dst_subset, thresholds, large class, its rows, its cols, scipy's row_ind,
    col_ind of its block) of the recorded HungarianMatcher frame"""
    g = route_generator()
    z = np.load(ROUTE_GOLDEN)
    m = json.loads(bytes(z["__meta__"]).decode())["frame"]
    dist, stags, dtags, ssub, dsub = g.frame(m["seed"])
    assert g.sha256(dist) == m["sha256"], "the regenerated frame is not the generator's"
    rows, cols, block = g.class_block(dist, stags, dtags, ssub, dsub, m["large_class"])
    assert g.sha256(block) == m["block_sha256"]
    return (dist, stags, dtags, ssub, dsub, dict(g.FRAME_THRESHOLD), m["large_class"], rows, cols,
            z["frame/rows"].astype(np.int64), z["frame/cols"].astype(np.int64))


def nn_edge_frame(rng, n, m, tags=(1, 2, 3, 4)):
    """a nearest-neighbour frame with the edge values: distances multiples of 0.25 in [-1, 3) (negative ones, many ties),
    -0.0 beside +0.0, +inf (acceptable under an inf threshold), NaN (never acceptable); tag 4 missing from the threshold map
    (0.0: only distances <= 0 match); src_free / dst_free masks; permuted subsets without a few boxes.
    -> dist f32 [n, m], src_tags, dst_tags, thresholds, src_subset, dst_subset, src_free, dst_free"""
    stags = rng.choice(np.asarray(tags, np.int64), n)
    dtags = rng.choice(np.asarray(tags, np.int64), m)
    d = (rng.integers(-4, 12, (n, m)) * 0.25).astype(np.float32)
    u = rng.random((n, m))
    d[:, dtags == 4] = np.abs(d[:, dtags == 4])                 # the missing tag: only its zeros (of either sign) can match
    zero = (u < 0.3) & (dtags == 4)[None, :]
    d[zero & (u < 0.15)] = -0.0
    d[zero & (u >= 0.15)] = 0.0
    d[(u < 0.6) & (dtags == 2)[None, :]] = np.inf               # the inf threshold: many pairs only an inf apart,
    d[np.ix_((stags == 2) & (rng.random(n) < 0.3), dtags == 2)] = np.inf    # and rows that can only match at inf
    d[(u >= 0.6) & (u < 0.62)] = np.nan
    thr = {1: 0.5, 2: float("inf"), 3: -0.25}
    ssub = rng.permutation(n)[:n - n // 20]
    dsub = rng.permutation(m)[:m - m // 20]
    sfree, dfree = rng.random(n) > 0.1, rng.random(m) > 0.1
    return d, stags, dtags, thr, ssub, dsub, sfree, dfree
