"""linear_sum_assignment, hungarian_match and nearest_neighbor_match against the literal restatement
(tests/assign_reference.py) on seeded tie-heavy problems: quantized and constant matrices, +inf entries, rectangular shapes
both ways, several classes, missing thresholds, batches (development aid).  usage: python tests/assign_fuzz.py [seeds]"""
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import assign_reference as ar
from d3d_amd.tracking import hungarian_match, linear_sum_assignment, nearest_neighbor_match

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
bad = 0
for seed in range(7000, 7000 + seeds):
    rng = np.random.default_rng(seed)
    n, m = (int(x) for x in rng.integers(1, 160, 2))
    kind = seed % 4
    if kind == 0:
        c = (rng.integers(0, 6, (n, m)) * 0.25).astype(np.float32)
    elif kind == 1:
        c = np.full((n, m), 0.5, np.float32)
    elif kind == 2:
        c = rng.random((n, m)).astype(np.float64)
    else:
        c = rng.integers(0, 4, (n, m)).astype(np.float64)
        c[rng.random((n, m)) < 0.05] = np.inf
    try:
        exp = ar.lsap(c)
    except ValueError:
        exp = None
    try:
        got = linear_sum_assignment(torch.from_numpy(c).cuda() if seed % 2 else c)
        got = tuple(x.cpu().numpy() if torch.is_tensor(x) else x for x in got)
    except ValueError:
        got = None
    if (exp is None) != (got is None) or (exp is not None and not (np.array_equal(exp[0], got[0]) and np.array_equal(exp[1], got[1]))):
        bad += 1
        print("lsap mismatch: seed", seed, c.shape, c.dtype)
    # matchers: several classes, one of them missing from the map, subsets shuffled
    d = (rng.integers(0, 10, (n, m)) * 0.25).astype(np.float32) if seed % 3 else rng.random((n, m)).astype(np.float32) * 3
    st, dt = rng.integers(0, 4, n), rng.integers(0, 4, m)
    thr = {0: 1.0, 1: 1.5, 2: 0.5}
    ss = [int(x) for x in rng.permutation(n)[: max(1, n - int(rng.integers(0, 5)))]]
    ds = [int(x) for x in rng.permutation(m)[: max(1, m - int(rng.integers(0, 5)))]]
    dev = torch.from_numpy(d).cuda()
    for name, fg, fr in (("hungarian", hungarian_match, ar.hungarian_match), ("nn", nearest_neighbor_match, ar.nearest_neighbor_match)):
        sm, dm = fg(dev, st, dt, thr, ss, ds)
        sa, da = fr(d, st, dt, ss, ds, thr)
        es = np.full((n,), -1, np.int32)
        for i, j in sa.items():
            es[i] = j
        if not np.array_equal(sm.cpu().numpy(), es):
            bad += 1
            print(name, "mismatch: seed", seed, (n, m))
print("assign_fuzz: %d seeds, %d failures" % (seeds, bad))
sys.exit(1 if bad else 0)
