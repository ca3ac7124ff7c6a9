"""Cases for the tests of the fused table convolution: the scenes of voxel_conv_cases.py and sparse_conv_cases.py, lines cut to the
row counts around the edges of the kernel's tiles (16-row MFMA blocks, 32 rows per wavefront, 128 per workgroup), a scene whose
table has whole columns absent, tables whose source rows are not their own rows (strided, inverse), and the data of the exact test.

A case: (name, op, scene, kernel, cin, cout) with op "subm" (kernel = a VoxelNeighbors kernel size), "down" (sparse_conv3d) or "up"
(sparse_inverse_conv3d) (kernel = a name of sparse_conv_cases.CONFIGS)."""
import functools

import numpy as np

import sparse_conv_cases as scases
import voxel_conv_cases as vcases
import voxel_conv_reference as vref

LINE_ROWS = (1, 15, 16, 17, 63, 64, 65, 129)
CHANNELS = ((16, 16), (16, 32), (48, 16), (64, 64), (32, 128))


def line(v):
    """v voxels in a row along x, in a shuffled row order"""
    c = np.zeros((v, 3), np.int64)
    c[:, 0] = np.random.default_rng(v).permutation(v) - 3
    return c


def scenes():
    s = dict(scases.SCENES)
    for v in LINE_ROWS:
        s["line%d" % v] = (line(v), None)
    return s


SCENES = scenes()


def cases():
    out = []
    for v in LINE_ROWS:                                             # K = 3: the tile and MFMA block edges
        out.append(("line%d-k3" % v, "subm", "line%d" % v, (3, 1, 1), 16, 16))
    # K = 27 on a line: 24 of the 27 columns are absent in every row, the skip runs; every channel pair
    for v, (cin, cout) in zip((17, 65, 129, 64, 63), CHANNELS):
        out.append(("line%d-k27-%dx%d" % (v, cin, cout), "subm", "line%d" % v, (3, 3, 3), cin, cout))
    out.append(("v65-k27", "subm", "v65", (3, 3, 3), 16, 32))
    out.append(("far_away-k27", "subm", "far_away", (3, 3, 3), 48, 16))
    out.append(("block12-k27", "subm", "block12", (3, 3, 3), 32, 128))      # 1728 rows: 14 workgroups, every column present
    out.append(("v4097-k27", "subm", "v4097", (3, 3, 3), 16, 16))             # two row slabs in the weight gradient
    out.append(("v1-k1", "subm", "v1", (1, 1, 1), 16, 16))
    for op in ("down", "up"):                                        # src_rows != rows
        out.append(("negative_odd-%s-k2s2" % op, op, "negative_odd", "k2s2p0", 16, 32))
        out.append(("negative_odd-%s-k3s2" % op, op, "negative_odd", "k3s2p1", 48, 16))
        out.append(("negative_odd-%s-k1" % op, op, "negative_odd", "k1s1p0", 16, 16))
        out.append(("negative_odd-%s-k311" % op, op, "negative_odd", "k311s211", 64, 64))
        out.append(("line65-%s-k2s2" % op, op, "line65", "k2s2p0", 32, 128))
    out.append(("batches_negative-down-k3s2", "down", "batches_negative", "k3s2p1", 16, 16))
    return out


CASES = cases()
BY_NAME = {c[0]: c for c in CASES}
SMALL = tuple(c[0] for c in CASES if len(SCENES[c[2]][0]) <= 130)


@functools.lru_cache(maxsize=None)
def sparse_model(scene, config):
    c, b = SCENES[scene]
    import sparse_conv_reference as sref
    out = sref.build(c, *scases.CONFIGS[config], batch=b)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tables(name):
    """-> (forward table [rows, K], the transposed map [src_rows, K], src_rows, rows) of a case, from the numpy models (shared: do
    not modify)"""
    _, op, scene, kernel, _, _ = BY_NAME[name]
    c, b = SCENES[scene]
    if op == "subm":
        tab = vref.table(c, kernel, 1, b)
        fwd, back = tab, np.ascontiguousarray(tab[:, ::-1])
    else:
        _, _, t_out, t_in = sparse_model(scene, kernel)
        fwd, back = (t_out, t_in) if op == "down" else (t_in, t_out)
    for a in (fwd, back):
        a.setflags(write=False)
    return fwd, back, len(back), len(fwd)


@functools.lru_cache(maxsize=None)
def integers(name):
    """small integers for the exact test: |features| <= 3, |weight| <= 2, |bias| <= 3, |grad_out| <= 3 as float32 (shared: do not
    modify).  Every sum of |a||b| behind an output stays below 2^24, and below 65504 (test_table_conv.py checks it), so every fp32
    partial sum is an exact integer in any order and the result is RNE(exact)"""
    _, _, _, _, cin, cout = BY_NAME[name]
    fwd, _, src_rows, rows = tables(name)
    r = np.random.default_rng(len(name) * 1000 + cin + cout)
    x = r.integers(-3, 4, (src_rows, cin)).astype(np.float32)
    w = r.integers(-2, 3, (fwd.shape[1], cin, cout)).astype(np.float32)
    bias = r.integers(-3, 4, (cout,)).astype(np.float32)
    g = r.integers(-3, 4, (rows, cout)).astype(np.float32)
    for a in (x, w, bias, g):
        a.setflags(write=False)
    return x, w, bias, g


def randoms(name, seed=0):
    """random data away from the half types' subnormal range: magnitudes in [1/4, 4), either sign -> (x, w, bias, g) float64"""
    _, _, _, _, cin, cout = BY_NAME[name]
    fwd, _, src_rows, rows = tables(name)
    r = np.random.default_rng(seed + 7 * len(name))

    def draw(shape, scale=1.0):
        return np.exp2(r.uniform(-2, 2, shape)) * r.choice((-1.0, 1.0), shape) * scale
    return draw((src_rows, cin)), draw((fwd.shape[1], cin, cout), 0.25), draw((cout,)), draw((rows, cout))
