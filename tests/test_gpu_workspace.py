"""GPU: every entry whose workspace is one carve function runs inside exactly what its size query returns.

Each case calls the raw C ABI (not d3d_amd._lib.workspace, which over-allocates by a quarter) on one uint8 buffer of query + 64 KiB
bytes, filled with 0xA5, and passes (buffer, query): the 64 KiB behind the query must come back untouched -- an overrun lands in
memory the test owns -- and the outputs must equal those of the same call on a workspace of twice the query: bit for bit, except
where the kernels accumulate with float atomics (the IoU and loss backward: the tolerances of tests/test_gpu_box.py and
tests/test_gpu_boxloss.py, 1e-9 in fp64 and 1e-3 in fp32).

With query - 256 bytes an entry refuses (D3D_ERR_WORKSPACE) and leaves its outputs alone, apart from what it clears before it
looks at the workspace (the status word and dst_match of the score matchers, both outputs of d3d_nn_match).  Every entry that
refuses compares the size with its QUERY (or carves the one layout the query is), so the shape does not matter for queries that
are a maximum over routes; the cases are fp64 hard NMS at 5000 boxes (nms_carve<double> sets d3d_nms2d_workspace_bytes) and the
300 x 300 matrices (the GRBOX forward's carve sets d3d_iou2d_workspace_bytes there).  The entries that take another route
instead of refusing -- GRBOX / DRBOX, d3d_iou3d_forward, d3d_match_distance -- must return the same result then."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TAIL = 65536
POISON = 0x77
F32, F64, F64_M32 = 0, 1, 2
RBOX, GRBOX = 2, 4
HARD, LINEAR = 0, 1
ERR_WORKSPACE = -3


def _header_enum(name):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d3d_hip.h")).read()
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, src).group(1))


NMS_BROAD_SWEEP = _header_enum("D3D_NMS_BROAD_SWEEP")
NMS_SOFT_NO_LDS = _header_enum("D3D_NMS_SOFT_NO_LDS")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def out(shape, dtype):
    """an output buffer filled with the poison byte"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(POISON)
    return t


def boxes2d(n, seed, dtype):
    """[n, 5] rotated boxes spread so that a box meets a handful of others, and their scores"""
    rng = np.random.default_rng(seed)
    ext = 3.0 * np.sqrt(n)
    b = np.stack([rng.random(n) * ext, rng.random(n) * ext, rng.random(n) * 4 + 1, rng.random(n) * 4 + 1, (rng.random(n) - 0.5) * 6], 1)
    return b.astype(dtype), rng.random(n).astype(dtype)


def boxes3d(n, seed, cols):
    rng = np.random.default_rng(seed)
    b = np.stack([rng.random(n) * 60, rng.random(n) * 60, rng.random(n) * 2 - 2, rng.random(n) * 1.5 + 3.5, rng.random(n) * 0.5 + 1.6,
                  rng.random(n) * 0.5 + 1.4, rng.random(n) * 2 * np.pi - np.pi], 1).astype(np.float32)
    if cols == 9:                                           # (label, score, x, y, z, lx, ly, lz, yaw)
        b = np.concatenate([np.zeros((n, 1), np.float32), rng.random((n, 1)).astype(np.float32), b], 1)
    return b


class Case:
    """query: bytes; call(ws, ws_bytes) -> (status, [outputs]) on fresh poisoned outputs; tol: None = bit-equal;
    short: what query - 256 bytes must do -- 'refuse' (+ cleared: indices of outputs the entry clears first) or 'same'"""

    def __init__(self, name, query, call, tol=None, short="refuse", cleared=(), short_tol=None):
        self.name, self.query, self.call, self.tol, self.short, self.cleared, self.short_tol = name, query, call, tol, short, cleared, short_tol


def nms_case(lib, name, n, dtype, sup=HARD, flags=0, own_order=False):
    np_t = np.float64 if dtype == F64 else np.float32
    b, s = boxes2d(n, 100 + n, np_t)
    tb, ts = T(b), T(s)
    order = None if own_order else torch.argsort(ts, descending=True, stable=True)

    def call(ws, nbytes):
        sup_out = out((n,), torch.uint8)
        rc = lib.d3d_nms2d(P(tb), P(ts), P(order), n, RBOX, sup, dtype, 0.3, 0.05, 0.5, P(sup_out), P(ws), nbytes, None, flags)
        return rc, [sup_out]
    return Case(name, lib.d3d_nms2d_workspace_bytes(n), call)


def iou2d_case(lib, name, kind, dtype, backward, n=300, m=300):
    box_t = np.float32 if dtype == F32 else np.float64
    mat_t = torch.float64 if dtype == F64 else torch.float32
    b1, _ = boxes2d(n, 7, box_t)
    b2, _ = boxes2d(m, 8, box_t)
    t1, t2 = T(b1), T(b2)
    grad = T(np.random.default_rng(9).random((n, m)).astype(np.float64)).to(mat_t)
    box_torch = torch.float32 if dtype == F32 else torch.float64
    tol = None
    if backward:
        tol = 1e-3 if dtype == F32 else 1e-9

    def call(ws, nbytes):
        if backward:
            g1, g2 = out((n, 5), box_torch), out((m, 5), box_torch)
            rc = lib.d3d_iou2d_backward(P(t1), n, P(t2), m, P(grad), kind, dtype, P(g1), P(g2), P(ws), nbytes, None)
            return rc, [g1, g2]
        ious = out((n, m), mat_t)
        rc = lib.d3d_iou2d_forward(P(t1), n, P(t2), m, kind, dtype, P(ious), P(ws), nbytes, None, 0)
        return rc, [ious]
    # GRBOX falls back to its single kernel (forward: the same values bit for bit, tests/test_gpu_boxloss.py); RBOX fp64 forward
    # falls back to the kernel without a list (not asserted here: D3D_F64_M32, which has no such kernel, refuses)
    short = "same" if kind == GRBOX else None if (dtype == F64 and not backward) else "refuse"
    return Case(name, lib.d3d_iou2d_workspace_bytes(n, m, dtype), call, tol=tol, short=short, short_tol=tol)


def iou3d_case(lib, name, distance, n=300, m=300):
    cols = 9 if distance else 7
    t1, t2 = T(boxes3d(n, 11, cols)), T(boxes3d(m, 12, cols))

    def call(ws, nbytes):
        res = out((n, m), torch.float32)
        if distance:
            rc = lib.d3d_match_distance(P(t1), n, P(t2), m, 1, P(res), P(ws), nbytes, None)
        else:
            rc = lib.d3d_iou3d_forward(P(t1), n, P(t2), m, 1, P(res), P(ws), nbytes, None)
        return rc, [res]
    # a short workspace: the kernel without a list, whose fp32 clip adds up in another order (1e-3: the bound of smoke())
    return Case(name, lib.d3d_iou3d_workspace_bytes(n, m), call, short="same", short_tol=1e-3)


def argsort_case(lib, name, n, dtype, radix):
    keys = T(np.random.default_rng(21).random(n).astype(np.float64 if dtype == F64 else np.float32))
    if radix:
        lib.d3d_internal_argsort_desc_radix.restype = ctypes.c_int
        lib.d3d_internal_argsort_desc_radix.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_size_t, ctypes.c_void_p]

    def call(ws, nbytes):
        order = out((n,), torch.int64)
        f = lib.d3d_internal_argsort_desc_radix if radix else lib.d3d_argsort_desc
        return f(P(keys), n, dtype, P(order), P(ws), nbytes, None), [order]
    # The radix entry of the tests has no query of its own.  At 5000 keys the public query is the larger of the bucket and the radix
    # carve, so that case shows the route only; at 2000 keys the bucket path takes no part in the query (it starts at 2049), the
    # query IS the radix carve, and the radix entry -- which sorts any size on the radix path -- must fit it and refuse below it.
    exact = not radix or n <= 2048
    return Case(name, lib.d3d_argsort_desc_workspace_bytes(n, dtype), call, short="refuse" if exact else None)


def grid_case(lib, name, ncells=100000, nkeys=5000):
    rng = np.random.default_rng(31)
    keys = T(rng.integers(0, ncells, nkeys).astype(np.int64))
    probe = T(rng.integers(0, ncells, nkeys).astype(np.int64))
    nslots = len(np.unique(keys.cpu().numpy()))

    def call(ws, nbytes):
        counts, key_of_slot, slot = out((4,), torch.int64), out((nslots,), torch.int64), out((nkeys,), torch.int64)
        rc = lib.d3d_grid_compact_index(P(keys), nkeys, ncells, P(counts), P(ws), nbytes, None)
        if rc == 0:
            rc = lib.d3d_grid_compact_keys(ncells, P(ws), nbytes, P(key_of_slot), None)
        if rc == 0:
            rc = lib.d3d_grid_compact_lookup(P(probe), nkeys, ncells, P(ws), nbytes, -1, P(slot), None)
        return rc, [counts[:1], key_of_slot, slot]
    return Case(name, lib.d3d_grid_compact_workspace_bytes(ncells), call)


def score_match_case(lib, name, batches, rows, m):
    n = batches * rows
    rng = np.random.default_rng(41)
    dist = T(rng.random((n, m)).astype(np.float32))
    src_tag, dst_tag = T(rng.integers(0, 3, n).astype(np.int32)), T(rng.integers(0, 3, m).astype(np.int32))
    thr = T(np.full(m, 0.2, np.float32))
    order = T(np.concatenate([rng.permutation(rows) for _ in range(batches)]).astype(np.int64))
    row_off = T(np.arange(batches + 1, dtype=np.int64) * rows)

    def call(ws, nbytes):
        src_match, dst_match, status = out((n,), torch.int32), out((batches, m), torch.int32), out((1,), torch.int32)
        if batches == 1:
            rc = lib.d3d_score_match(P(dist), n, m, P(src_tag), P(dst_tag), P(thr), P(order), P(src_match), P(dst_match), P(status), P(ws),
                                     nbytes, None)
        else:
            rc = lib.d3d_score_match_batched(P(dist), None, None, None, P(row_off), batches, n, m, P(src_tag), P(dst_tag), P(thr), P(order),
                                             P(src_match), P(dst_match), P(status), P(ws), nbytes, None)
        return rc, [src_match, dst_match, status]
    if batches == 1:
        return Case(name, lib.d3d_score_match_workspace_bytes(n, m), call, cleared=(2,))
    return Case(name, lib.d3d_score_match_batched_workspace_bytes(n, m, batches), call, cleared=(1, 2))


def nn_match_case(lib, name, ns=200, nd=300):
    rng = np.random.default_rng(51)
    dist = T(rng.random((ns, nd)).astype(np.float32))
    src_idx, dst_idx = T(np.arange(ns, dtype=np.int64)), T(np.arange(nd, dtype=np.int64))
    src_tag, dst_tag = T(rng.integers(0, 3, ns).astype(np.int32)), T(rng.integers(0, 3, nd).astype(np.int32))
    thr = T(np.full(nd, 0.3, np.float32))

    def call(ws, nbytes):
        src_match, dst_match = out((ns,), torch.int32), out((nd,), torch.int32)
        rc = lib.d3d_nn_match(P(dist), nd, P(src_idx), ns, P(dst_idx), nd, P(src_tag), P(dst_tag), P(thr), None, None, P(src_match),
                              P(dst_match), P(ws), nbytes, None)
        return rc, [src_match, dst_match]
    return Case(name, lib.d3d_nn_match_workspace_bytes(ns, nd), call, cleared=(0, 1))


def owner_pack_case(lib, name, n=5000, world=4, c=4):
    rng = np.random.default_rng(61)
    keys = T(np.concatenate([rng.permutation(1 << 20)[:n], [-1]]).astype(np.int64))       # keys[n] = -1 - status
    cnt, agg = T(rng.integers(1, 9, n).astype(np.int32)), T(rng.random((n, c)).astype(np.float32))
    first = T(rng.permutation(4 * n)[:n].astype(np.int64))
    counts = T(np.array([n, 0, 0, 0], np.int64))
    words = lib.d3d_owner_record_words(c)

    def call(ws, nbytes):
        send, perm, pos, sc = out((n, words), torch.int32), out((n,), torch.int32), out((n,), torch.int32), out((2 * world + 1,), torch.int64)
        rc = lib.d3d_owner_pack(P(keys), P(cnt), P(agg), P(first), P(counts), n, c, world, 0, None, None, P(send), P(perm), P(pos), None, P(sc),
                                P(ws), nbytes, None, None, 0)
        return rc, [send, perm, pos, sc]
    return Case(name, lib.d3d_owner_pack_workspace_bytes(n, world), call)


def owner_number_case(lib, name, n_total=5000, owned=700):
    rng = np.random.default_rng(71)
    marked = np.sort(rng.permutation(n_total)[:2 * owned])                  # the frame's first points; every other one is this owner's
    words = np.zeros((n_total + 63) // 64 + 1, np.uint64)
    for f in marked:
        words[f >> 6] |= np.uint64(1) << np.uint64(f & 63)
    gbits, first_o = T(words.view(np.int64)), T(marked[::2].astype(np.int64))
    counts_o = T(np.array([owned, 0, 0, 0], np.int64))

    def call(ws, nbytes):
        vids, counts = out((owned,), torch.int64), out((4,), torch.int64)
        rc = lib.d3d_owner_number(P(gbits), n_total, P(first_o), P(counts_o), owned, P(vids), P(counts), P(ws), nbytes, None)
        return rc, [vids, counts[:1]]
    return Case(name, lib.d3d_owner_number_workspace_bytes(n_total), call)


def build_cases(lib):
    cases = []
    for dtype, tag in ((F32, "f32"), (F64, "f64")):
        for n in (200, 2000, 5000):         # one-workgroup resolve; small set, general resolve; grid broad phase
            cases.append(nms_case(lib, "nms_rbox_%s_%d" % (tag, n), n, dtype))
    cases.append(nms_case(lib, "nms_sweep_5000", 5000, F64, flags=NMS_BROAD_SWEEP))          # the argsort and fbx arrays
    cases.append(nms_case(lib, "nms_own_order_5000", 5000, F64, own_order=True))             # order_ws and the fp64 argsort scratch
    cases.append(nms_case(lib, "softnms_lds_300", 300, F64, sup=LINEAR))
    cases.append(nms_case(lib, "softnms_global_300", 300, F64, sup=LINEAR, flags=NMS_SOFT_NO_LDS))
    cases.append(iou2d_case(lib, "iou2d_forward_rbox_f64", RBOX, F64, False))
    cases.append(iou2d_case(lib, "iou2d_forward_rbox_f64_m32", RBOX, F64_M32, False))
    cases.append(iou2d_case(lib, "iou2d_backward_rbox_f64", RBOX, F64, True))
    for dtype, tag in ((F32, "f32"), (F64, "f64")):
        cases.append(iou2d_case(lib, "grbox_forward_%s" % tag, GRBOX, dtype, False))
        cases.append(iou2d_case(lib, "grbox_backward_%s" % tag, GRBOX, dtype, True))
    cases.append(iou3d_case(lib, "iou3d_forward_rotated", False))
    cases.append(iou3d_case(lib, "match_distance", True))
    cases.append(argsort_case(lib, "argsort_f32_5000", 5000, F32, False))                    # bucket route
    cases.append(argsort_case(lib, "argsort_f64_5000", 5000, F64, False))
    cases.append(argsort_case(lib, "argsort_radix_5000", 5000, F32, True))
    cases.append(argsort_case(lib, "argsort_radix_f32_2000", 2000, F32, True))               # the radix carve alone sets the query
    cases.append(argsort_case(lib, "argsort_radix_f64_2000", 2000, F64, True))
    cases.append(grid_case(lib, "grid_compact_index_keys_lookup"))
    cases.append(score_match_case(lib, "score_match_200x300", 1, 200, 300))
    cases.append(score_match_case(lib, "score_match_batched_4x50x300", 4, 50, 300))
    cases.append(nn_match_case(lib, "nn_match_200x300"))
    cases.append(owner_pack_case(lib, "owner_pack_5000_w4"))
    cases.append(owner_number_case(lib, "owner_number_5000"))
    return cases


CASE_NAMES = ["nms_rbox_f32_200", "nms_rbox_f32_2000", "nms_rbox_f32_5000", "nms_rbox_f64_200", "nms_rbox_f64_2000", "nms_rbox_f64_5000",
              "nms_sweep_5000", "nms_own_order_5000", "softnms_lds_300", "softnms_global_300", "iou2d_forward_rbox_f64",
              "iou2d_forward_rbox_f64_m32", "iou2d_backward_rbox_f64", "grbox_forward_f32", "grbox_backward_f32", "grbox_forward_f64",
              "grbox_backward_f64", "iou3d_forward_rotated", "match_distance", "argsort_f32_5000", "argsort_f64_5000", "argsort_radix_5000",
              "argsort_radix_f32_2000", "argsort_radix_f64_2000",
              "grid_compact_index_keys_lookup", "score_match_200x300", "score_match_batched_4x50x300", "nn_match_200x300",
              "owner_pack_5000_w4", "owner_number_5000"]


@pytest.fixture(scope="module")
def cases():
    from d3d_amd import _lib
    return {c.name: c for c in build_cases(_lib.load())}


def same(a, b, tol):
    if tol is None:
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return torch.allclose(a.double(), b.double(), rtol=tol, atol=tol)


def poisoned(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def test_case_list_is_complete(cases):
    assert sorted(cases) == sorted(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_entry_stays_inside_its_query(cases, name):
    c = cases[name]
    q = int(c.query)
    assert q > 0 and q % 256 == 0
    buf = torch.full((q + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, got = c.call(buf, q)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[q:] == 0xA5).all()), "%s wrote behind the %d bytes its query returns" % (name, q)
    assert not any(poisoned(t) for t in got if t.numel() > 8)
    big = torch.full((2 * q,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, exp = c.call(big, 2 * q)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for a, b in zip(got, exp):
        assert same(a, b, c.tol), name
    if c.short is None:
        return
    rc, short = c.call(buf, q - 256)
    torch.cuda.synchronize()
    if c.short == "refuse":
        assert rc == ERR_WORKSPACE, rc
        for k, t in enumerate(short):
            assert k in c.cleared or poisoned(t), "%s: output %d written by a refused call" % (name, k)
    else:
        assert rc == 0, rc
        for a, b in zip(short, got):
            assert same(a, b, c.short_tol), name
