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
