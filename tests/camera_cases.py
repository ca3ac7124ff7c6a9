"""What the camera tests share: the rigs' constants (also used by tests/golden/make_camera_golden.py) and the access to the
recorded cases of tests/golden/camera_ref_cases.npz."""
import json
import os

import numpy as np

import camera_reference as cr


def rigid(yaw, pitch, roll, t):
    cy, sy, cp, sp, cr_, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rx = np.array([[1, 0, 0], [0, cr_, -sr], [0, sr, cr_]])
    m = np.eye(4)
    m[:3, :3] = rz.dot(ry).dot(rx)
    m[:3, 3] = t
    return m


KITTI = dict(size=[1242, 375], cx=609.5593, cy=172.854, fx=721.5377, fy=721.5377)
T_CAM = rigid(0.012, -0.007, 0.004, [-0.27, 0.06, -0.08])           # lidar -> camera, both front-left-up
DIST_REAL = [-0.3691, 0.1968, 0.0013, -0.0006, -0.0745]
DIST_BARREL = [-0.85, 0.12, 0.002, -0.001, 0.0]


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "camera_ref_cases.npz")
GOLDEN = np.load(GOLDEN_PATH) if os.path.exists(GOLDEN_PATH) else None      # (absent only while the generator writes it)


def names(prefix):
    return sorted({k.split("/")[1] for k in GOLDEN.files if k.startswith(prefix + "/")})


def case_inputs(name, kind="case"):
    """-> (spec, the case's points as the reference got them)"""
    spec = json.loads(str(GOLDEN["%s/%s/spec" % (kind, name)]))
    cloud = GOLDEN["cloud/" + spec["cloud"]]
    if kind == "transform":
        cloud = cloud[:512]
    with np.errstate(over="ignore"):            # (the special cloud's 1e300 becomes inf in fp32, as it did for the reference)
        return spec, np.ascontiguousarray(cloud[:, :spec["cols"]]).astype(spec["dtype"])


def case_expected(name):
    p = "case/%s/" % name
    exp = dict(uv_all=GOLDEN[p + "uv_all"], mask=GOLDEN[p + "mask"], dmask=GOLDEN[p + "dmask"])
    exp["uv_kept"] = exp["uv_all"][exp["mask"]]
    return exp


def case_model(name, pts):
    p = "case/%s/" % name
    w, h = GOLDEN[p + "size"].tolist()
    return cr.project(pts, GOLDEN[p + "rt"], GOLDEN[p + "P"], w, h, GOLDEN[p + "dist"], GOLDEN[p + "intri"])
