"""GPU: TransformSet.project_points_to_camera / project_points_to_cameras / transform_points (d3d_project_points,
d3d_transform_points) against the reference's recorded results and, at 1 M points, against the tests' own fp64 model.  The
comparison rule is camera_reference.check_projection everywhere: mask, dmask, K and Kd equal; only points within 1e-6 px of a
bound (or with |d| < 1e-6) stay out, at most 10 per case, asserted; uv in view within 1e-9 px, out of view rtol 1e-9."""
import json

import numpy as np
import pytest
import torch

import camera_reference as cr
from camera_cases import DIST_BARREL, DIST_REAL, GOLDEN, KITTI, case_expected, case_inputs, case_model, names, rigid

pytestmark = pytest.mark.gpu

KINDS = ("kitti", "kitti_dist", "barrel")


def rig(name):
    from d3d_amd.abstraction import TransformSet
    return cr.replay(TransformSet, str(GOLDEN["rig/%s/json" % name]))


def to_np(res):
    return tuple(r.cpu().numpy() if torch.is_tensor(r) else r for r in res)


def gpu_full_form(ts, pts, frame_to, frame_from=None):
    n = len(pts)
    return cr.full_form(n, lambda ro, rd: to_np(ts.project_points_to_camera(pts, frame_to, frame_from, remove_outlier=ro, return_dmask=rd)))


def model_of(ts, pts, frame_to, frame_from=None):
    """the tests' model on the matrices the class holds (checked against the reference's by tests/test_camera.py)"""
    meta = ts.intrinsics_meta[frame_to]
    pts = pts.cpu().numpy() if torch.is_tensor(pts) else pts
    return cr.project(pts, ts.get_extrinsic(frame_to, frame_from), ts.intrinsics[frame_to], meta.width, meta.height,
                      np.asarray(meta.distort_coeffs, np.float64), meta.intri_matrix)


@pytest.mark.parametrize("name", names("case"))
def test_golden_cases(name):
    spec, pts = case_inputs(name)
    ts = rig(spec["rig"])
    near = cr.near_points(case_model(name, pts))
    got = gpu_full_form(ts, pts, spec["frame_to"], spec["frame_from"])
    assert all(isinstance(v, np.ndarray) for v in got.values())                  # numpy in -> numpy out
    n_near = cr.check_projection(case_expected(name), got, near, name)
    print("%s: N=%d K=%d Kd=%d near=%d" % (name, len(pts), len(got["mask"]), len(got["dmask"]), n_near))


@pytest.mark.parametrize("kind", KINDS)
def test_million_points_against_the_model(kind):
    from d3d_amd import synth
    cloud = synth.lidar_like(1_000_000, 1)
    ts = rig(kind)
    model = model_of(ts, cloud, "cam")
    near = cr.near_points(model)
    dev = torch.from_numpy(cloud).cuda()
    got = gpu_full_form(ts, dev, "cam")
    n_near = cr.check_projection(cr.expected(model), got, near, kind)
    print("%s: K=%d Kd=%d near=%d" % (kind, len(got["mask"]), len(got["dmask"]), n_near))
    res = ts.project_points_to_camera(dev, "cam", return_dmask=True)
    assert all(r.is_cuda and r.device == dev.device for r in res)               # torch in -> torch out on the same device
    assert res[0].dtype == torch.float64 and res[1].dtype == torch.int64 and res[2].dtype == torch.int64


@pytest.mark.parametrize("n", [1, 63, 64, 1023, 1024, 1025, 4097, 120_001])
def test_tile_edges(n):
    """clouds that end inside a wavefront row, a wavefront and a workgroup's tile"""
    from d3d_amd import synth
    cloud = synth.lidar_like(n, 3)[:, :3].astype(np.float64)
    ts = rig("kitti_dist")
    model = model_of(ts, cloud, "cam")
    cr.check_projection(cr.expected(model), gpu_full_form(ts, cloud, "cam"), cr.near_points(model), "n=%d" % n)


def test_inputs_numpy_torch_dtypes_and_layouts():
    from d3d_amd import synth
    base = synth.lidar_like(50_000, 5)
    ts = rig("kitti_dist")
    exp32 = cr.expected(model_of(ts, base, "cam"))
    near = cr.near_points(model_of(ts, base, "cam"))
    wide = np.zeros((len(base), 8), np.float32)
    wide[:, ::2] = base
    variants = {
        "numpy f32": base,
        "torch cpu f32": torch.from_numpy(base),
        "torch cuda f32": torch.from_numpy(base).cuda(),
        "numpy every other column": wide[:, ::2],
        "torch cuda every other column": torch.from_numpy(wide).cuda()[:, ::2],
        "numpy reversed twice": np.ascontiguousarray(base[::-1])[::-1],
        "torch cuda transposed storage": torch.from_numpy(np.ascontiguousarray(base.T)).cuda().T,
        "torch cuda rows 1.. of [N,4]": torch.from_numpy(np.concatenate([base[:1], base])).cuda()[1:],
        "torch cuda [N,3] off a 12-byte offset": torch.from_numpy(np.concatenate([base[:1, :3], base[:, :3]])).cuda()[1:],
    }
    for what, pts in variants.items():
        got = gpu_full_form(ts, pts, "cam")
        cr.check_projection(exp32, got, near, what)
        res = ts.project_points_to_camera(pts, "cam")
        if isinstance(pts, np.ndarray):
            assert all(isinstance(r, np.ndarray) for r in res), what
        else:
            assert all(torch.is_tensor(r) and r.device == pts.device for r in res), what
    # fp64 rows are read as fp64 ...
    rng = np.random.default_rng(6)
    b64 = base.astype(np.float64) + rng.normal(0, 1e-7, base.shape)
    m64 = model_of(ts, b64, "cam")
    for pts in (b64, torch.from_numpy(b64).cuda(), torch.from_numpy(b64[:, :3].copy()).cuda()):
        cr.check_projection(cr.expected(m64), gpu_full_form(ts, pts, "cam"), cr.near_points(m64), "f64")
    assert np.abs(cr.expected(m64)["uv_all"] - exp32["uv_all"])[exp32["mask"]].max() > 1e-6       # (the two clouds do differ)
    # ... and any other dtype goes through fp32
    h = base.astype(np.float16)
    m16 = model_of(ts, h.astype(np.float32), "cam")
    cr.check_projection(cr.expected(m16), gpu_full_form(ts, torch.from_numpy(h).cuda(), "cam"), cr.near_points(m16), "f16")
    ints = np.round(base * 4).astype(np.int32)
    mi = model_of(ts, ints.astype(np.float32), "cam")
    cr.check_projection(cr.expected(mi), gpu_full_form(ts, ints, "cam"), cr.near_points(mi), "int32")


def six_camera_rig():
    from d3d_amd.abstraction import TransformSet
    ts = TransformSet("lidar")
    frames = []
    for k in range(9):
        name = "cam%d" % k
        dist = [[], DIST_REAL, DIST_BARREL][k % 3]
        ts.set_intrinsic_pinhole(name, KITTI["size"] if k % 2 else (1920, 1280), KITTI["cx"] + 3 * k, KITTI["cy"], KITTI["fx"], KITTI["fy"] + k,
                                 s=0.5 * (k % 2), distort_coeffs=dist)
        ts.set_extrinsic(rigid(2 * np.pi * k / 6, 0.01 * k, -0.005 * k, [0.1 * k, -0.2, 0.3]), frame_to=name)
        frames.append(name)
    return ts, frames


@pytest.mark.parametrize("ncam", [6, 9])
def test_rig_in_one_call_equals_single_calls_bit_for_bit(ncam):
    """6 cameras: one launch set; 9: more records than one launch carries"""
    from d3d_amd import synth
    ts, frames = six_camera_rig()
    frames = frames[:ncam]
    cloud = torch.from_numpy(synth.lidar_like(300_000, 9)).cuda()
    seen = set()
    for ro in (True, False):
        for rd in (True, False):
            batched = ts.project_points_to_cameras(cloud, frames, remove_outlier=ro, return_dmask=rd)
            assert len(batched) == ncam
            for frame, res in zip(frames, batched):
                single = ts.project_points_to_camera(cloud, frame, remove_outlier=ro, return_dmask=rd)
                assert len(res) == len(single) == (3 if rd else 2)
                for a, b in zip(res, single):
                    assert a.shape == b.shape and a.dtype == b.dtype
                    assert np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))      # the bits, NaN included
                seen.add(len(res[1]))
    assert len(seen) >= 3                                  # the cameras do see different parts of the cloud
    # and a single call is right
    model = model_of(ts, cloud, frames[-1])
    cr.check_projection(cr.expected(model), gpu_full_form(ts, cloud, frames[-1]), cr.near_points(model), frames[-1])


def test_two_cameras_over_more_than_4096_tiles():
    """4098 tile sums per camera: the workgroup that scans a camera's sums takes a second step of 4096 with two live sums, and
    camera 1's workgroup is not workgroup 0.  K, Kd, the compacted mask with its uv rows and dmask against the model."""
    from d3d_amd import synth
    n = 4096 * 1024 + 1025
    cloud = synth.lidar_like(n, 11)
    assert cloud.dtype == np.float32
    ts, frames = six_camera_rig()
    frames = frames[:2]
    got = ts.project_points_to_cameras(torch.from_numpy(cloud).cuda(), frames, remove_outlier=True, return_dmask=True)
    assert len(got) == 2
    counts = []
    for frame, res in zip(frames, got):
        model = model_of(ts, cloud, frame)
        near = cr.near_points(model)
        assert int(near.sum()) <= cr.MAX_NEAR
        exp = cr.expected(model)
        uv, mask, dmask = to_np(res)
        assert uv.shape == (len(mask), 2) and uv.dtype == np.float64 and mask.dtype == np.int64 and dmask.dtype == np.int64
        for key, g_idx in (("mask", mask), ("dmask", dmask)):
            assert g_idx.size == 0 or (g_idx[0] >= 0 and g_idx[-1] < n and np.all(np.diff(g_idx) > 0)), "%s: %s is not ascending" % (frame, key)
            e, g = np.zeros(n, bool), np.zeros(n, bool)
            e[exp[key]] = True
            g[g_idx] = True
            bad = np.nonzero((e != g) & ~near)[0]
            assert bad.size == 0, "%s: %s differs at points %s" % (frame, key, bad[:10])
            if not near.any():
                assert np.array_equal(exp[key], g_idx), "%s: %s" % (frame, key)       # K / Kd and every index
        kept = ~near[mask] & model["mask"][mask]
        assert np.abs(uv[kept] - exp["uv_all"][mask[kept]]).max() <= cr.UV_ATOL, frame     # row j = the j-th point in view
        counts.append((len(mask), len(dmask)))
    assert counts[0] != counts[1] and all(k > 4096 * 1024 // 8 for c in counts for k in c)     # (live sums in both steps)


def test_non_default_stream():
    from d3d_amd import synth
    cloud = torch.from_numpy(synth.lidar_like(200_000, 4)).cuda()
    ts = rig("barrel")
    exp = to_np(ts.project_points_to_camera(cloud, "cam", return_dmask=True))
    expt = ts.transform_points(cloud, "cam").cpu().numpy()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        later = torch.from_numpy(synth.lidar_like(200_000, 4)).cuda(non_blocking=True)     # produced on the side stream
        got = ts.project_points_to_camera(later, "cam", return_dmask=True)
        gott = ts.transform_points(later, "cam")
    stream.synchronize()
    for a, b in zip(to_np(got), exp):
        assert np.array_equal(a, b)
    assert np.array_equal(gott.cpu().numpy(), expt)


@pytest.mark.parametrize("name", names("transform"))
def test_transform_points_golden(name):
    spec, pts = case_inputs(name, "transform")
    ts = rig(spec["rig"])
    exp = GOLDEN["transform/%s/out" % name]
    for p in (pts, torch.from_numpy(pts).cuda()):
        got = ts.transform_points(p, spec["frame_to"], spec["frame_from"])
        assert isinstance(got, np.ndarray) if isinstance(p, np.ndarray) else got.is_cuda
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == exp.shape
        assert np.allclose(got, exp, rtol=cr.XYZ_TOL, atol=cr.XYZ_TOL)


@pytest.mark.parametrize("cols,dtype", [(3, np.float32), (4, np.float32), (6, np.float64), (4, np.float16)])
def test_transform_points_million(cols, dtype):
    from d3d_amd import synth
    rng = np.random.default_rng(8)
    cloud = np.concatenate([synth.lidar_like(1_000_000, 2), rng.random((1_000_000, 2), np.float32)], 1)[:, :cols].astype(dtype)
    ts = rig("chain")
    got = ts.transform_points(torch.from_numpy(cloud).cuda(), "cam_b", "lidar").cpu().numpy()
    exp = cr.transform(cloud.astype(np.float32) if dtype == np.float16 else cloud, ts.get_extrinsic("cam_b", "lidar"))
    assert got.dtype == np.float64 and got.shape == (len(cloud), cols)
    assert np.allclose(got, exp, rtol=cr.XYZ_TOL, atol=cr.XYZ_TOL)
    assert np.array_equal(got[:, 3:], cloud[:, 3:].astype(np.float64))
    empty = ts.transform_points(cloud[:0], "cam_b", "lidar")
    assert empty.shape == (0, cols) and empty.dtype == np.float64


def test_chain_into_the_fusion_operators():
    """project -> sample a semantic image at uv -> paint_label: the chain stays on the device"""
    from d3d_amd import synth
    from d3d_amd.abstraction import paint_label
    cloud = torch.from_numpy(synth.lidar_like(100_000, 11)).cuda()
    ts = rig("kitti")
    uv, mask = ts.project_points_to_camera(cloud, "cam")
    assert uv.is_cuda and mask.is_cuda and uv.shape == (len(mask), 2)
    image = torch.arange(375 * 1242, device="cuda").reshape(375, 1242) % 4
    sem = torch.zeros(len(cloud), dtype=torch.uint8, device="cuda")
    sem[mask] = image[uv[:, 1].long(), uv[:, 0].long()].to(torch.uint8)          # in view: 0 <= floor(v) < 375, 0 <= floor(u) < 1242
    boxes = torch.tensor([[20.0, 0.0, -1.0, 40.0, 40.0, 4.0, 0.1]], device="cuda")
    ids = paint_label(boxes, cloud, sem, labels=torch.tensor([1], dtype=torch.uint8))
    assert ids.shape == (len(cloud),) and int(ids.max()) == 1
    assert json.loads(str(GOLDEN["rig/kitti/frames"])) == ts.frames
