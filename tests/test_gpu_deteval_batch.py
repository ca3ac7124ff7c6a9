"""GPU: DetectionEvaluator.calc_stats_batch and d3d_deteval_batched -- a whole split in one call equals the loop of calc_stats
over its frames, element by element and bit for bit (tests/deteval_cases.py's scenes; tests/test_deteval_cases.py holds the scenes
themselves against the oracle on the CPU)."""
import functools

import numpy as np
import pytest
import torch

import oracle
import deteval_cases as cases

pytestmark = pytest.mark.gpu

COUNTS = ("ndt", "tp", "fp", "fn")
FLOATS = ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var")
KEYS = ["ngt", "ndt", "tp", "fp", "fn", "acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var"]


def _bound():
    from d3d_amd import _lib
    return int(_lib.load().d3d_deteval_frame_max())


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "d":
        return cases.scene_d(_bound())
    if name == "c-nan":             # (NaN scores: only the reference's own behaviour is specified)
        return cases.without_frame(scene("c"), scene("c")["names"]["nan"])
    return getattr(cases, "scene_" + name)()


def evaluator(s, compat):
    from d3d_amd.benchmarks import DetectionEvaluator
    return DetectionEvaluator(s["classes"], s["min_overlaps"], reference_compat=compat, **s["kwargs"])


@functools.lru_cache(maxsize=None)
def loop(name, compat):
    """the baseline, computed once per (scene, mode): calc_stats frame by frame"""
    s = scene(name)
    ev = evaluator(s, compat)
    return tuple(ev.calc_stats(g, d) for g, d in cases.frames_of(s))


def batch(s, ev, **kw):
    return ev.calc_stats_batch(kw.get("gt", s["gt"]), kw.get("dt", s["dt"]), kw.get("go", s["go"]), kw.get("do", s["do"]))


def assert_same(got, exp, T, classes, ctx):
    assert len(got) == len(exp), ctx
    for f, (a, b) in enumerate(zip(got, exp)):
        assert list(a.keys()) == KEYS == list(b.keys()), (ctx, f)
        for c in classes:
            assert type(a.ngt[c]) is int and a.ngt[c] == b.ngt[c], (ctx, f, c)
            for k in COUNTS:
                assert type(a[k][c]) is list and len(a[k][c]) == T and all(type(v) is int for v in a[k][c]), (ctx, f, k, c)
                assert a[k][c] == b[k][c], (ctx, f, k, c, a[k][c], b[k][c])
            for k in FLOATS:
                assert type(a[k][c]) is list and len(a[k][c]) == T and all(type(v) is float for v in a[k][c]), (ctx, f, k, c)
                assert np.array_equal(np.asarray(a[k][c], np.float32), np.asarray(b[k][c], np.float32), equal_nan=True), \
                    (ctx, f, k, c, a[k][c], b[k][c])
        assert set(a.ngt) == set(classes)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_batch_equals_the_loop_of_calc_stats(name, compat, monkeypatch):
    if name == "c" and not compat:
        name = "c-nan"
    s = scene(name)
    ev = evaluator(s, compat)
    own, calls = ev.calc_stats, []
    monkeypatch.setattr(ev, "calc_stats", lambda g, d: (calls.append((len(g), len(d))), own(g, d))[1])
    got = batch(s, ev)
    assert_same(got, loop(name, compat), len(ev.score_thresholds), s["classes"], (name, compat))
    # the frames went through the batched kernels: only the tie and NaN frames of (c) take calc_stats, and only in compat mode
    fr = cases.frames_of(s)
    expect = [(len(fr[s["names"][k]][0]), len(fr[s["names"][k]][1])) for k in ("ties", "nan")] if name == "c" else []
    assert calls == expect
    st = ev.get_stats()                       # nothing was added to the totals
    assert all(st.ngt[c] == 0 and sum(st.tp[c]) == 0 for c in s["classes"])
    if name == "a":
        assert ev._pr_nsamples == 40
    if name.startswith("c"):
        assert s["kwargs"]["pr_sample_scale"] == "lin"


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_against_the_oracle(name, compat):
    """counts exact, acc_* at rtol=1e-4 / atol=1e-5 against oracle.calc_stats per frame.  The oracle computes its IoU in fp32
    as the reference does; tests/test_deteval_cases.py holds its own rounding on these scenes inside half this tolerance (against
    an fp64 evaluation), which leaves the device the other half.  Every figure out of tolerance is printed before the assert."""
    s = scene(name)
    ev = evaluator(s, compat)
    got = batch(s, ev)
    off = []
    for f, (g, d) in enumerate(cases.frames_of(s)):
        exp = oracle.calc_stats(g, d, s["classes"], cases.max_distance(s), ev.score_thresholds, literal=compat)
        for c in s["classes"]:
            assert got[f].ngt[c] == exp.ngt[c]
            for k in COUNTS:
                assert got[f][k][c] == exp[k][c], (name, compat, f, k, c)
            for k in FLOATS[:-1]:
                if not np.allclose(got[f][k][c], exp[k][c], rtol=1e-4, atol=1e-5, equal_nan=True):
                    a, b = np.asarray(got[f][k][c]), np.asarray(exp[k][c])
                    print("off", name, compat, f, k, c, "max |got - exp| = %.3g" % np.nanmax(np.abs(a - b)), "tp", got[f].tp[c],
                          "\n got", a.tolist(), "\n exp", b.tolist())
                    off.append((f, k, c))
    assert not off, off


@pytest.mark.parametrize("compat", [True, False])
def test_chunks_equal_one_call(compat, monkeypatch):
    from d3d_amd import benchmarks
    s = scene("e")
    ev = evaluator(s, compat)
    whole = batch(s, ev)
    T = len(ev.score_thresholds)
    lib = benchmarks._lib.load()
    own = lib.d3d_deteval_batched
    for frames_cap, bytes_cap in ((7, None), (1, None), (None, 4096)):
        calls = []
        with monkeypatch.context() as mp:
            if frames_cap is not None:
                mp.setattr(benchmarks, "_DET_MAX_FRAMES", frames_cap)
            if bytes_cap is not None:
                mp.setattr(benchmarks, "_DET_MAX_CACHE_BYTES", bytes_cap)
            mp.setattr(lib, "d3d_deteval_batched", lambda *a: (calls.append(a[5]), own(*a))[1])      # (a[5]: the call's frames)
            assert_same(batch(s, ev), whole, T, s["classes"], (compat, frames_cap, bytes_cap))
        if frames_cap is not None:
            assert calls == [frames_cap] * (300 // frames_cap) + ([300 % frames_cap] if 300 % frames_cap else [])
        else:
            assert len(calls) > 3 and sum(calls) == 300


@pytest.mark.parametrize("compat", [True, False])
def test_a_frame_above_the_bound_falls_back(compat, monkeypatch):
    s = scene("d")
    ev = evaluator(s, compat)
    own, calls = ev.calc_stats, []
    monkeypatch.setattr(ev, "calc_stats", lambda g, d: (calls.append((len(g), len(d))), own(g, d))[1])
    got = batch(s, ev)
    assert calls == [(_bound() + 1, _bound() + 1)]          # the frame AT the bound went through the kernels
    assert_same(got, loop("d", compat), len(ev.score_thresholds), s["classes"], ("d", compat))
    assert sum(got[s["names"]["at"]].tp[1]) > 0 and sum(got[s["names"]["above"]].tp[1]) > 0


def test_device_tensors_equal_numpy():
    s = scene("a")
    for compat in (True, False):
        ev = evaluator(s, compat)
        T = lambda a: torch.from_numpy(a).cuda()
        got = batch(s, ev, gt=T(s["gt"]), dt=T(s["dt"]), go=T(s["go"]), do=torch.from_numpy(s["do"]))
        assert_same(got, loop("a", compat), len(ev.score_thresholds), s["classes"], ("tensors", compat))


def test_bad_offsets_and_empty_split():
    s = scene("b")
    ev = evaluator(s, True)
    go, do = s["go"], s["do"]
    for bad_go, bad_do in ((go[1:], do[1:]), (go[:-1], do[:-1]), (go, do[:-1]), (go[:-1], do), (np.zeros((0,), np.int64), do),
                           (np.concatenate([go[:2], go[1:2] - 1, go[2:]]), np.concatenate([do[:2], do[1:2], do[2:]])),
                           (np.concatenate([go, go[-1:]]), do)):
        with pytest.raises(ValueError):
            ev.calc_stats_batch(s["gt"], s["dt"], bad_go, bad_do)
    assert ev.calc_stats_batch(np.zeros((0, 9), np.float32), np.zeros((0, 9), np.float32), [0], [0]) == []


def test_tracking_evaluator_refuses():
    from d3d_amd.benchmarks import TrackingEvaluator
    s = scene("b")
    with pytest.raises(TypeError, match="calc_stats_sequence"):
        TrackingEvaluator([1, 2], [0.5, 0.5]).calc_stats_batch(s["gt"], s["dt"], s["go"], s["do"])


def test_c_entry_cache_association_refusal_and_workspace():
    """d3d_deteval_batched on three small frames: the ragged cache against prepare_boxes, the literal association against
    ReferenceAssociation.match_many, the own-row association against score_match, a frame above the bound refused with nothing
    written, and the workspace query against what the call accepts"""
    from d3d_amd import _lib
    from d3d_amd.tracking.matcher import DistanceTypes, ReferenceAssociation, prepare_boxes, score_match
    lib = _lib.load()
    s = scene("a")
    fr = cases.frames_of(s)[:3] + [(np.zeros((0, 9), np.float32), cases.frames_of(s)[3][1])]
    classes, maxd = s["classes"], cases.max_distance(s)
    thr = evaluator(s, True).score_thresholds
    Tn, C, F = len(thr), len(classes), len(fr)
    gt, dt = np.concatenate([g for g, _ in fr]), np.concatenate([d for _, d in fr])
    go = np.concatenate([[0], np.cumsum([len(g) for g, _ in fr])]).astype(np.int64)
    do = np.concatenate([[0], np.cumsum([len(d) for _, d in fr])]).astype(np.int64)
    co = np.concatenate([[0], np.cumsum([len(g) * len(d) for g, d in fr])]).astype(np.int64)
    slot = lambda tags: np.array([classes.index(int(t)) if int(t) in classes else -1 for t in tags], np.int32)
    gslot, dslot = slot(gt[:, 0]), slot(dt[:, 0])
    perm, rank = np.zeros((len(dt),), np.int32), np.full((len(dt),), -1, np.int32)
    slots_lit, slots_own = np.zeros((F, Tn), np.int32), np.zeros((F,), np.int32)
    for f, (g, d) in enumerate(fr):
        inc = np.nonzero(dslot[do[f]:do[f + 1]] >= 0)[0]
        order = inc[np.argsort(-d[inc, 1], kind="stable")]
        perm[do[f]:do[f] + len(order)] = order
        rank[do[f] + order] = np.arange(len(order))
        slots_own[f] = len(order)
        slots_lit[f] = [(~(d[inc, 1] < t)).sum() for t in thr]
    dev = torch.device("cuda", torch.cuda.current_device())
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(dt=cu(dt), gt=cu(gt), do=cu(do), go=cu(go), co=cu(co), dslot=cu(dslot), gslot=cu(gslot), perm=cu(perm), rank=cu(rank),
             maxd=cu(np.array([maxd[c] for c in classes], np.float32)))
    pairs, M, N = int(co[-1]), len(gt), len(dt)
    P = lambda x: _lib.ptr(x) if x is not None else None

    def call(literal, cache, gm, gi, dm, ws=None, max_n=None, max_m=None):
        sl = cu(slots_lit if literal else slots_own)
        rc = lib.d3d_deteval_batched(P(t["dt"]), P(t["gt"]), P(t["do"]), P(t["go"]), P(t["co"]), F, pairs,
                                     int(np.diff(do).max()) if max_n is None else max_n, int(np.diff(go).max()) if max_m is None else max_m,
                                     P(t["dslot"]), P(t["gslot"]), P(t["perm"]), P(t["rank"]), P(sl), Tn, P(t["maxd"]), C, int(literal),
                                     P(cache), P(gm), P(gi), P(dm), P(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    fresh = lambda n, dtype, v: torch.full((n,), v, dtype=dtype, device=dev)
    cache = fresh(pairs, torch.float32, -7.0)
    gm, gi = fresh(Tn * M, torch.int32, -7), fresh(Tn * M, torch.float32, -7.0)
    assert call(True, cache, gm, gi, None) == 0
    cache_h, gm_h, gi_h = cache.cpu().numpy(), gm.cpu().numpy(), gi.cpu().numpy()
    for f, (g, d) in enumerate(fr):
        n, m = len(d), len(g)
        if n == 0 or m == 0:
            continue
        exp_cache = prepare_boxes(d, g, DistanceTypes.RIoU)
        got_cache = cache_h[co[f]:co[f + 1]].reshape(n, m)
        assert np.array_equal(got_cache.view(np.uint32), exp_cache.cpu().numpy().view(np.uint32)), f
        gtag, dtag = g[:, 0].astype(np.int64), d[:, 0].astype(np.int64)
        gt_idx = np.nonzero(np.isin(gtag, classes))[0]
        assoc = ReferenceAssociation(exp_cache, d[:, 1], dtag, gtag, maxd, gt_idx)
        subsets = [np.nonzero(np.isin(dtag, classes) & ~(d[:, 1] < tv))[0] for tv in thr]
        _, dm_exp = assoc.match_many(subsets)
        dm_exp = dm_exp.cpu().numpy()
        got_dm = gm_h[Tn * go[f]:Tn * go[f + 1]].reshape(Tn, m)
        assert np.array_equal(got_dm, dm_exp), f
        got_iou = gi_h[Tn * go[f]:Tn * go[f + 1]].reshape(Tn, m)
        exp_iou = np.where(dm_exp >= 0, np.float32(1) - got_cache[np.maximum(dm_exp, 0), np.arange(m)[None, :]], np.float32(0))
        assert np.array_equal(got_iou, exp_iou), f
        assert (dm_exp >= 0).sum() > 0
    # the own-row association, with the cache in the workspace
    need = lib.d3d_deteval_batched_workspace_bytes(pairs, 0)
    assert need == (4 * pairs + 255) // 256 * 256 and lib.d3d_deteval_batched_workspace_bytes(pairs, 1) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    gm1, gi1, dm1 = fresh(M, torch.int32, -7), fresh(M, torch.float32, -7.0), fresh(N, torch.int32, -7)
    assert call(False, None, gm1, gi1, dm1, ws=ws) == 0
    assert np.array_equal(ws[:4 * pairs].view(torch.float32).cpu().numpy().view(np.uint32), cache_h.view(np.uint32))
    for f, (g, d) in enumerate(fr):
        if len(g) == 0:
            assert np.all(dm1[do[f]:do[f + 1]].cpu().numpy() == -1)
            continue
        sm_exp, dm_exp = score_match(cache[co[f]:co[f + 1]].view(len(d), len(g)), d[:, 1], d[:, 0].astype(np.int64),
                                     g[:, 0].astype(np.int64), maxd)
        assert np.array_equal(dm1[do[f]:do[f + 1]].cpu().numpy(), sm_exp.cpu().numpy()), f
        assert np.array_equal(gm1[go[f]:go[f + 1]].cpu().numpy(), dm_exp.cpu().numpy()), f
    # too small a workspace, and a batch with a frame above the bound: refused, nothing written
    gm2, gi2, dm2 = fresh(M, torch.int32, -7), fresh(M, torch.float32, -7.0), fresh(N, torch.int32, -7)
    assert call(False, None, gm2, gi2, dm2, ws=ws[:need - 256]) == _lib.ERR_WORKSPACE
    cache2 = fresh(pairs, torch.float32, -7.0)
    for kw in (dict(max_n=_bound() + 1), dict(max_m=_bound() + 1)):
        assert call(False, cache2, gm2, gi2, dm2, **kw) == _lib.ERR_UNSUPPORTED
        assert call(True, cache2, gm, gi, None, **kw) == _lib.ERR_UNSUPPORTED
    assert call(False, cache2, gm2, gi2, dm2, max_n=_bound(), max_m=_bound()) == 0      # the bound itself is taken
    gm3, dm3 = fresh(M, torch.int32, -7), fresh(N, torch.int32, -7)
    cache3 = fresh(pairs, torch.float32, -7.0)
    assert call(False, cache3, gm3, gi2, dm3, max_n=_bound() + 1) == _lib.ERR_UNSUPPORTED
    assert torch.all(cache3 == -7.0) and torch.all(gm3 == -7) and torch.all(dm3 == -7)
    assert np.array_equal(gm.cpu().numpy(), gm_h)
