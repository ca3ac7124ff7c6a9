"""CPU: the camera tests' own fp64 model (tests/camera_reference.py) against the reference's recorded results
(tests/golden/camera_ref_cases.npz, written by tests/golden/make_camera_golden.py), the host side of d3d_amd.abstraction's
TransformSet against the recorded extrinsics, its argument validation, and the D3DCamera record against the header.
No GPU: the device path is tests/test_gpu_camera.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import camera_reference as cr

from camera_cases import GOLDEN, ROOT, case_expected, case_inputs, case_model, names


def test_golden_file_holds_the_cases_it_should():
    cases = names("case")
    assert len(cases) >= 16 and len(names("rig")) >= 7 and len(names("transform")) >= 4 and len(names("rejected")) >= 10
    specs = [json.loads(str(GOLDEN["case/%s/spec" % c])) for c in cases]
    assert {(s["cols"], s["dtype"]) for s in specs} >= {(c, d) for c in (3, 4, 6) for d in ("float32", "float64")}
    assert {s["cloud"] for s in specs} == {"lidar", "wide", "special", "empty"}
    special = GOLDEN["cloud/special"]
    assert np.isnan(special).any() and np.isinf(special).any() and (special[:, 0] == 0).sum() >= 4
    assert all(2000 <= len(GOLDEN["cloud/" + c]) <= 4096 for c in ("lidar", "wide", "special")) and len(GOLDEN["cloud/empty"]) == 0
    assert all(float(GOLDEN["time/%s_1M_s" % k][0]) > 0 for k in ("kitti", "kitti_dist", "barrel"))


@pytest.mark.parametrize("name", names("case"))
def test_model_matches_the_reference(name):
    spec, pts = case_inputs(name)
    model = case_model(name, pts)
    near = cr.near_points(model)
    assert int(near.sum()) == int(GOLDEN["case/%s/near" % name])
    n_near = cr.check_projection(case_expected(name), cr.expected(model), near, name)
    print("%s: N=%d K=%d Kd=%d near=%d" % (name, len(pts), model["mask"].sum(), model["dmask"].sum(), n_near))


def test_barrel_distortion_folds_points_back_and_the_pre_mask_drops_them():
    """what the +-20 px mask ahead of the distortion is for: far-out points land inside the image after a strong barrel
    distortion; the recorded mask leaves them out"""
    spec, pts = case_inputs("barrel_wide")
    model = case_model("barrel_wide", pts)
    w, h = model["width"], model["height"]
    folded = (0 < model["u"]) & (model["u"] < w) & (0 < model["v"]) & (model["v"] < h) & model["dmask"] & ~model["pre"]
    assert folded.sum() > 20
    assert not np.isin(np.nonzero(folded)[0], GOLDEN["case/barrel_wide/mask"]).any()


@pytest.mark.parametrize("name", names("transform"))
def test_model_transform_matches_the_reference(name):
    from d3d_amd.abstraction import TransformSet
    spec, pts = case_inputs(name, "transform")
    ts = cr.replay(TransformSet, str(GOLDEN["rig/%s/json" % spec["rig"]]))
    got = cr.transform(pts, ts.get_extrinsic(spec["frame_to"], spec["frame_from"]))
    exp = GOLDEN["transform/%s/out" % name]
    assert got.dtype == np.float64 and got.shape == exp.shape
    assert np.allclose(got, exp, rtol=cr.XYZ_TOL, atol=cr.XYZ_TOL)


@pytest.mark.parametrize("rig", names("rig"))
def test_host_bookkeeping_matches_the_reference(rig):
    """frames, repr and every get_extrinsic pair: np.linalg.inv and dot on both sides"""
    from d3d_amd.abstraction import TransformSet
    ts = cr.replay(TransformSet, str(GOLDEN["rig/%s/json" % rig]))
    assert ts.frames == json.loads(str(GOLDEN["rig/%s/frames" % rig]))
    assert repr(ts) == str(GOLDEN["rig/%s/repr" % rig])
    keys = [k for k in GOLDEN.files if k.startswith("rig/%s/ext/" % rig)]
    assert len(keys) >= 4
    for k in keys:
        fto, ffrom = (None if f == "None" else f for f in k.split("/")[-1].split("|"))
        got = ts.get_extrinsic(fto, ffrom)
        assert got.shape == (4, 4) and got.dtype == np.float64
        assert np.allclose(got, GOLDEN[k]), k
        assert np.allclose(ts.get_extrinsic(frame_to=fto, frame_from=ffrom), GOLDEN[k])


def test_camera_records_match_the_reference_inputs():
    """the D3DCamera record the device gets = the matrices the reference projected with"""
    from d3d_amd.abstraction import TransformSet, _D3DCamera
    for name in names("case"):
        spec, _ = case_inputs(name)
        ts = cr.replay(TransformSet, str(GOLDEN["rig/%s/json" % spec["rig"]]))
        rec = _D3DCamera()
        ts._camera_record(rec, spec["frame_to"], spec["frame_from"])
        p = "case/%s/" % name
        assert np.allclose(np.array(rec.rt[:]).reshape(3, 4), GOLDEN[p + "rt"][:3])
        assert np.array_equal(np.array(rec.P[:]).reshape(3, 3), GOLDEN[p + "P"])            # the fp32 pinhole parameters included
        assert [rec.width, rec.height] == GOLDEN[p + "size"].tolist()
        dist = GOLDEN[p + "dist"]
        assert rec.has_dist == (1 if dist.size else 0)
        if dist.size:
            intri = GOLDEN[p + "intri"]
            assert np.array_equal(rec.dist[:], dist)
            assert [rec.fx, rec.fy, rec.cx, rec.cy] == [intri[0, 0], intri[1, 1], intri[0, 2], intri[1, 2]]


@pytest.mark.parametrize("name", names("rejected"))
def test_rejected_calls_raise_value_error(name):
    """what the reference rejects (the recorded exception type), the class rejects with ValueError -- before any device is touched"""
    from d3d_amd.abstraction import TransformSet
    rec = json.loads(str(GOLDEN["rejected/%s/json" % name]))
    assert str(GOLDEN["rejected/%s/raised" % name]) in ("ValueError", "TypeError")
    with pytest.raises(ValueError):
        ts = cr.replay(TransformSet, rec["rig"])
        method, args, kwargs = rec["call"]
        getattr(ts, method)(*cr.decode(args), **cr.decode(kwargs))


def test_argument_validation_without_gpu():
    import torch
    from d3d_amd.abstraction import TransformSet
    ts = cr.replay(TransformSet, str(GOLDEN["rig/kitti/json"]))
    for bad in (np.zeros((4, 2), np.float32), np.zeros((4,), np.float32), np.zeros((2, 3, 3)), [[0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError):
            ts.project_points_to_camera(bad, "cam")
        with pytest.raises(ValueError):
            ts.transform_points(bad, "cam")
    with pytest.raises(ValueError):
        ts.project_points_to_cameras(np.zeros((4, 3)), [])
    with pytest.raises(ValueError):                                  # the base frame is no camera
        ts.project_points_to_camera(np.zeros((4, 3)), None)
    lidar = TransformSet("base")
    lidar.set_intrinsic_lidar("lidar")
    lidar.set_extrinsic(np.eye(4), frame_to="lidar")
    with pytest.raises(ValueError):                                  # nor is a lidar
        lidar.project_points_to_camera(np.zeros((4, 3)), "lidar")
    # a frame against itself: the identity is accepted and changes nothing (the reference's check cannot pass)
    before = {k: v.copy() for k, v in ts.extrinsics.items()}
    ts.set_extrinsic(np.eye(4), frame_to="cam", frame_from="cam")
    ts.set_extrinsic(np.eye(4)[:3])
    ts.set_extrinsic(np.eye(4), frame_to="velo", frame_from=None)
    assert before.keys() == ts.extrinsics.keys() and all(np.array_equal(before[k], ts.extrinsics[k]) for k in before)
    with pytest.raises(ValueError):
        ts.set_extrinsic(np.eye(4) * 2, frame_to=None, frame_from="velo")
    # the pinhole parameters are kept as fp32, like the reference's C float arguments; mirror_coeff is stored and unused
    p = TransformSet("b")
    p.set_intrinsic_pinhole("c", (640, 480), 320.1, 240.1, 500.3, 500.7, s=0.1)
    assert p.intrinsics_meta["c"].intri_matrix[0, 0] == float(np.float32(500.3)) and p.intrinsics_meta["c"].width == 640
    assert np.array_equal(p.intrinsics["c"][2], [1.0, 0.0, 0.0])       # depth = the front axis
    p.set_intrinsic_camera("m", np.eye(3), (10, 10), mirror_coeff=0.5)
    assert p.intrinsics_meta["m"].mirror_coeff == 0.5 and p.frames == ["c", "m"]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):      # no silent CPU fallback
            ts.project_points_to_camera(np.zeros((4, 3), np.float32), "cam")
        with pytest.raises(RuntimeError, match="HIP device"):
            ts.transform_points(np.zeros((4, 3), np.float32), "cam")


def test_camera_record_layout_matches_the_header(tmp_path):
    """D3DCamera: the ctypes Structure the Python layer fills (d3d_amd.abstraction._D3DCamera) against the struct of
    include/d3d_hip.h as gcc lays it out -- size and the offset of every field; a multiple of 8 bytes"""
    from d3d_amd import _lib
    from d3d_amd.abstraction import _D3DCamera
    fields = [f[0] for f in _D3DCamera._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "d3d_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(D3DCamera));\n' +
                   "".join('    printf("%%zu\\n", offsetof(D3DCamera, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", str(src), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_D3DCamera) == 256 and got[0] % 8 == 0
    assert got[1:] == [getattr(_D3DCamera, f).offset for f in fields]
    lib = _lib.load()
    assert lib.d3d_project_points_workspace_bytes(0, 1) >= 0
    assert lib.d3d_project_points_workspace_bytes(1000000, 6) >= 6 * 977 * 8
    assert lib.d3d_project_points_workspace_bytes(-1, 1) == 0 and lib.d3d_project_points_workspace_bytes(10, 0) == 0
