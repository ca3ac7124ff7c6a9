"""GPU: box2d_nms_batched / d3d_nms2d_grouped against the loop of per-group box2d_nms calls -- exact equality of the bool
masks, every case; a subset also against the oracle's nms2d per group."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from d3d_amd import _lib, synth

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)         # around the chunk of 64 ranks, the 256-thread form and the cap
MODES = {"f32": (np.float32, False), "wide": (np.float32, True), "f64": (np.float64, True)}


def clustered(n, seed, dtype=np.float64):
    """n boxes at detector density: the objects of synth.boxes2d_sparse, each seen 5-20 times with jitter -> (boxes, scores)"""
    rng = np.random.default_rng(seed)
    objects, _ = synth.boxes2d_sparse(n // 5 + 1, seed + 1000)
    objects = objects[np.repeat(np.arange(len(objects)), rng.integers(5, 21, len(objects)))[:n]]
    b = objects.copy()
    b[:, :2] += rng.normal(0, 2.0, (n, 2))
    b[:, 2:4] *= rng.uniform(0.85, 1.15, (n, 2))
    b[:, 4] += rng.normal(0, 0.1, n)
    o = rng.permutation(n)
    return b[o].astype(dtype), rng.random(n).astype(dtype)


def batch(sizes, seed, dtype=np.float64, ids=None):
    """one clustered set per group, the rows of all groups shuffled together -> (boxes, scores, group ids)"""
    rng = np.random.default_rng(seed)
    if ids is None:
        ids = rng.choice(1 << 20, len(sizes), replace=False) - (1 << 19)
    parts = [clustered(m, seed + 7 * k, dtype) for k, m in enumerate(sizes)]
    b, s = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    g = np.repeat(np.asarray(ids, np.int64), sizes)
    o = rng.permutation(len(g))
    return b[o], s[o], g[o]


def segments(g):
    """[(group value, rows in ascending order)]"""
    g = np.asarray(g)
    o = np.argsort(g, kind="stable")
    cuts = np.flatnonzero(np.diff(g[o])) + 1
    return [(g[i[0]], i) for i in np.split(o, cuts)]


def loop_reference(b, s, g, **kw):
    """what the contract names: box2d_nms on every group's rows, in ascending row order"""
    from d3d_amd.box import box2d_nms
    keep = torch.zeros((len(b),), dtype=torch.bool, device=b.device)
    for _, idx in segments(g.cpu().numpy() if torch.is_tensor(g) else g):
        idx = torch.from_numpy(idx).to(b.device)
        keep[idx] = box2d_nms(b[idx], s[idx], **kw)
    return keep


def cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("method", ["box", "rbox"])
def test_group_sizes_in_one_call(method, mode):
    from d3d_amd.box import box2d_nms_batched
    dtype, precise = MODES[mode]
    ids = [-7, 0, (1 << 40) + 5, 3, 1 << 31, -(1 << 35), 11, 12, 2, 1]
    bn, sn, gn = batch(SIZES, 11, dtype, ids)
    b, s, g = cuda(bn, sn, gn)
    kw = dict(iou_method=method, iou_threshold=0.3, precise=precise)
    got = box2d_nms_batched(b, s, g, **kw)
    assert got.dtype == torch.bool and got.device == b.device and got.shape == (len(bn),)
    exp = loop_reference(b, s, g, **kw)
    assert torch.equal(got, exp)
    kept = got.cpu().numpy()
    for value, idx in segments(gn):
        assert kept[idx].any()
        if len(idx) >= 63:
            assert 0 < kept[idx].sum() < len(idx), "the boxes of a group neither all survive nor all vanish"
        if precise and len(idx) <= 257:                            # (fp64 arithmetic: the oracle's mask is the same)
            assert np.array_equal(kept[idx], oracle.box2d_nms(bn[idx], sn[idx], iou_method=method, iou_threshold=0.3)), value


def test_groups_are_isolated():
    from d3d_amd.box import box2d_nms, box2d_nms_batched
    bn, sn = clustered(200, 5)
    b1, s1 = cuda(bn, sn)
    single = box2d_nms(b1, s1, iou_method="box", iou_threshold=0.1)
    ids = np.array([4, -1, 9, 1 << 33, 0, 77, 5], np.int64)
    g = torch.from_numpy(np.tile(ids, 200)).cuda()                  # row r of copy k: position 7 r + k
    b, s = b1.repeat_interleave(7, 0), s1.repeat_interleave(7, 0)
    got = box2d_nms_batched(b, s, g, iou_method="box", iou_threshold=0.1)
    for k in range(7):
        assert torch.equal(got[k::7], single), ids[k]
    together = box2d_nms(b, s, iou_method="box", iou_threshold=0.1)
    assert not torch.equal(got, together)                           # (ungrouped, the copies suppress each other)


@pytest.mark.parametrize("score_threshold", [0, -10.0])
def test_ties_and_special_scores(score_threshold):
    from d3d_amd.box import box2d_nms_batched
    sizes = (130, 130, 70, 70, 9)
    bn, sn, gn = batch(sizes, 21, np.float32, ids=[5, 6, 7, 8, 9])
    sn[gn == 5] = 0.5                                               # all equal inside a group: stable by row
    sn[gn == 6] = 0.5                                               # ... and equal to another group's
    rng = np.random.default_rng(3)
    r7 = np.flatnonzero(gn == 7)
    sn[r7] = rng.choice(np.array([np.nan, 0.0, -0.0, -1.5, 0.25, 0.25, 0.75], np.float32), len(r7))
    r8 = np.flatnonzero(gn == 8)
    sn[r8] = rng.choice(np.array([-0.0, 0.0, -3.0, np.nan], np.float32), len(r8))      # nothing above the default threshold
    sn[gn == 9] = np.nan
    b, s, g = cuda(bn, sn, gn)
    for method in ("box", "rbox"):
        for precise in (False, True):
            kw = dict(iou_method=method, iou_threshold=0.2, score_threshold=score_threshold, precise=precise)
            assert torch.equal(box2d_nms_batched(b, s, g, **kw), loop_reference(b, s, g, **kw)), (method, precise)
    kw = dict(iou_method="rbox", iou_threshold=0.2, score_threshold=score_threshold)
    kept = box2d_nms_batched(b, s, g, **kw).cpu().numpy()
    rows5 = np.flatnonzero(gn == 5)
    assert kept[rows5[0]], "all scores equal: the first row of the group ranks first"
    exp5 = oracle.box2d_nms(bn[rows5].astype(np.float64), np.linspace(1, 0.5, len(rows5)), iou_method="rbox", iou_threshold=0.2)
    assert np.array_equal(kept[rows5], exp5)                        # (strictly descending scores spell the row order out)


def test_score_threshold_acts_per_group():
    from d3d_amd.box import box2d_nms_batched
    bn, sn, gn = batch((90, 90, 90), 31, np.float64, ids=[1, 2, 3])
    sn[gn == 1] = 0.05 + 0.4 * sn[gn == 1]                           # entirely below the threshold
    sn[gn == 2] = 0.55 + 0.4 * sn[gn == 2]                           # entirely above
    b, s, g = cuda(bn, sn, gn)                                       # group 3: straddles it
    kw = dict(iou_method="rbox", iou_threshold=0.3, score_threshold=0.5)
    got = box2d_nms_batched(b, s, g, **kw)
    assert torch.equal(got, loop_reference(b, s, g, **kw))
    kept = got.cpu().numpy()
    r1 = np.flatnonzero(gn == 1)
    assert kept[r1].sum() == 1 and kept[r1[np.argmax(sn[r1])]], "the group's own top box survives the tail, and only it"
    assert kept[gn == 2].sum() > 1
    r3 = np.flatnonzero(gn == 3)
    assert not kept[r3[sn[r3] <= 0.5]].any() and kept[r3[sn[r3] > 0.5]].any()


def test_many_tiny_groups():
    from d3d_amd.box import box2d_nms_batched
    rng = np.random.default_rng(41)
    sizes = rng.integers(1, 9, 3000)
    n = int(sizes.sum())
    bn, sn = clustered(n, 42, np.float32)
    gn = rng.permutation(np.repeat(rng.choice(1 << 40, 3000, replace=False), sizes))
    b, s, g = cuda(bn, sn, gn)
    kw = dict(iou_method="rbox", iou_threshold=0.3, precise=True)
    got = box2d_nms_batched(b, s, g, **kw)
    assert torch.equal(got, loop_reference(b, s, g, **kw))
    assert 0 < int(got.sum()) < n


def test_single_group_and_class_scores():
    from d3d_amd.box import box2d_nms, box2d_nms_batched
    bn, sn = clustered(700, 51, np.float32)
    b, s = cuda(bn, sn)
    g = torch.full((700,), -3, dtype=torch.int16, device="cuda")
    for method in ("box", "rbox"):
        assert torch.equal(box2d_nms_batched(b, s, g, iou_method=method, iou_threshold=0.4),
                           box2d_nms(b, s, iou_method=method, iou_threshold=0.4))
    # [N,3] scores: the class maximum ranks the boxes
    s3 = torch.from_numpy(np.random.default_rng(52).random((700, 3)).astype(np.float32)).cuda()
    g = torch.from_numpy(np.random.default_rng(53).integers(0, 6, 700).astype(np.uint8)).cuda()
    got = box2d_nms_batched(b, s3, g, iou_method="rbox", iou_threshold=0.3)
    assert torch.equal(got, loop_reference(b, s3, g, iou_method="rbox", iou_threshold=0.3))
    assert torch.equal(got, box2d_nms_batched(b, s3.max(axis=1).values, g, iou_method="rbox", iou_threshold=0.3))


def test_routing_by_group_size(monkeypatch):
    import d3d_amd.box as box
    kw = dict(iou_method="rbox", iou_threshold=0.3)
    b, s, g = cuda(*batch((1024, 300, 17), 61, np.float32))
    exp = loop_reference(b, s, g, **kw)
    real = box.nms2d

    def refuse(*a, **k):
        raise AssertionError("nms2d called although every group is within the cap")
    monkeypatch.setattr(box, "nms2d", refuse)
    assert torch.equal(box.box2d_nms_batched(b, s, g, **kw), exp)
    # one group above the cap: that one, and only that one, goes through nms2d
    monkeypatch.setattr(box, "nms2d", real)
    b, s, g = cuda(*batch((40, 1025, 3, 260), 62, np.float32))
    exp = loop_reference(b, s, g, **kw)
    calls = []

    def counted(boxes, *a, **k):
        calls.append(len(boxes))
        return real(boxes, *a, **k)
    monkeypatch.setattr(box, "nms2d", counted)
    got = box.box2d_nms_batched(b, s, g, **kw)
    assert calls == [1025]
    assert torch.equal(got, exp)


def raw_grouped(b, s, perm, seg, max_group, keep, iou_type=2, dtype=_lib.F32, iou_threshold=0.3, score_threshold=0.0):
    lib = _lib.load()
    ngroups = seg.numel() - 1 if seg is not None else 0
    nbytes = lib.d3d_nms2d_grouped_workspace_bytes(len(b), ngroups)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    return lib.d3d_nms2d_grouped(_lib.ptr(b), _lib.ptr(s), _lib.ptr(perm) if perm is not None else None,
                                 _lib.ptr(seg) if seg is not None else None, len(b), ngroups, max_group, iou_type, dtype,
                                 iou_threshold, score_threshold, _lib.ptr(keep), _lib.ptr(ws), nbytes, _lib.stream_ptr(), 0)


def test_raw_entry_point():
    kw = dict(iou_method="rbox", iou_threshold=0.3, precise=False)
    sizes = (300, 1030, 5, 64)
    bn, sn, gn = batch(sizes, 71, np.float32, ids=[1, 2, 3, 4])
    # rows already grouped: perm = NULL
    o = np.argsort(gn, kind="stable")
    b, s, g = cuda(bn[o], sn[o], gn[o])
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    exp = loop_reference(b, s, g, **kw).view(torch.uint8)
    over = (g == 2)
    for hint in (300, 0):                                           # (the hint only chooses the workgroup size: 1024 threads both times)
        keep = torch.full((len(b),), 0xAA, dtype=torch.uint8, device="cuda")
        assert raw_grouped(b, s, None, seg, hint, keep) == 0
        assert bool((keep[over] == 0xAA).all()), "a segment above the cap is skipped: its keep bytes are not written"
        assert torch.equal(keep[~over], exp[~over])
    # groups of at most 256 boxes: the 256-thread form and the 1024-thread form agree
    small = torch.tensor([0, 5, 5, 69, 300], dtype=torch.int64, device="cuda")       # (one empty segment)
    rows = torch.cat([torch.arange(1330, 1399), torch.arange(0, 231)]).cuda()
    exp_small = loop_reference(b[rows], s[rows], torch.repeat_interleave(torch.arange(4).cuda(), small.diff()), **kw).view(torch.uint8)
    for hint in (231, 0):
        keep = torch.full((300,), 0xAA, dtype=torch.uint8, device="cuda")
        assert raw_grouped(b[rows].contiguous(), s[rows].contiguous(), None, small, hint, keep) == 0
        assert torch.equal(keep, exp_small)
    # shuffled rows through perm (stable: ascending rows inside a segment)
    b, s, g = cuda(bn, sn, gn)
    perm = torch.from_numpy(o).cuda()
    exp = loop_reference(b, s, g, **kw).view(torch.uint8)
    keep = torch.full((len(b),), 0xAA, dtype=torch.uint8, device="cuda")
    assert raw_grouped(b, s, perm, seg, 300, keep) == 0
    over = (g == 2)
    assert bool((keep[over] == 0xAA).all()) and torch.equal(keep[~over], exp[~over])
    # nothing to do
    assert raw_grouped(b, s, perm, seg[:1], 0, keep) == 0
    assert raw_grouped(b[:0], s[:0], None, None, 0, keep[:0]) == 0
    torch.cuda.synchronize()


def test_raw_entry_point_in_a_graph():
    kw = dict(iou_method="rbox", iou_threshold=0.3, precise=True)
    sizes = (200, 500, 33, 1000)
    bn, sn, gn = batch(sizes, 81, np.float64, ids=[1, 2, 3, 4])
    b, s, g = cuda(bn, sn, gn)
    perm = torch.from_numpy(np.argsort(gn, kind="stable")).cuda()
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    keep = torch.zeros((len(b),), dtype=torch.uint8, device="cuda")
    first = loop_reference(b, s, g, **kw).view(torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the capture stream
        assert raw_grouped(b, s, perm, seg, 1000, keep, dtype=_lib.F64) == 0
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(keep, first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert raw_grouped(b, s, perm, seg, 1000, keep, dtype=_lib.F64) == 0
    s.copy_(torch.from_numpy(sn[::-1].copy()).cuda())                # new scores, same buffers
    keep.fill_(0xAA)
    graph.replay()
    torch.cuda.synchronize()
    second = loop_reference(b, s, g, **kw).view(torch.uint8)
    assert torch.equal(keep, second) and not torch.equal(first, second)


def test_inputs_come_back_as_box2d_nms_returns_them():
    from d3d_amd.box import box2d_nms, box2d_nms_batched
    bn, sn, gn = batch((150, 80, 300), 91, np.float32)
    kw = dict(iou_method="rbox", iou_threshold=0.3)
    exp = loop_reference(*cuda(bn, sn, gn), **kw).cpu()
    got = box2d_nms_batched(bn, sn, gn.astype(np.int32), **kw)       # numpy in, numpy out
    like = box2d_nms(bn[:10], sn[:10], **kw)
    assert type(got) is type(like) is np.ndarray and got.dtype == like.dtype == np.bool_
    assert np.array_equal(got, exp.numpy())
    got = box2d_nms_batched(torch.from_numpy(bn), torch.from_numpy(sn), torch.from_numpy(gn), **kw)      # CPU tensors
    like = box2d_nms(torch.from_numpy(bn[:10]), torch.from_numpy(sn[:10]), **kw)
    assert got.device == like.device == torch.device("cpu") and got.dtype == like.dtype and torch.equal(got, exp)
    got = box2d_nms_batched(torch.from_numpy(bn), torch.from_numpy(sn), gn, **kw)                        # ids may be numpy beside tensors
    assert torch.equal(got, exp)
    wide = torch.zeros((len(bn), 10), dtype=torch.float32, device="cuda")
    wide[:, ::2] = torch.from_numpy(bn).cuda()
    strided_s = torch.zeros((len(bn), 2), dtype=torch.float32, device="cuda")
    strided_s[:, 1] = torch.from_numpy(sn).cuda()
    strided_g = torch.zeros((len(bn), 3), dtype=torch.int64, device="cuda")
    strided_g[:, 2] = torch.from_numpy(gn).cuda()
    got = box2d_nms_batched(wide[:, ::2], strided_s[:, 1], strided_g[:, 2], **kw)                        # any strides
    assert got.is_cuda and torch.equal(got.cpu(), exp)
