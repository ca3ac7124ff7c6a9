"""Seeded fuzzing of TransformSet.project_points_to_camera / project_points_to_cameras / transform_points on the GPU against
tests/camera_reference.py, beyond the seeds of the suite: random pinhole and general cameras, with and without distortion,
random extrinsics, clouds of random size, row length and dtype with non-finite rows mixed in.  The comparison rule is the
suite's (camera_reference.check_projection).  A script, not collected by pytest.
usage: python tests/camera_fuzz.py [rounds] [first seed]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import camera_reference as cr                                # noqa: E402
from camera_cases import rigid                               # noqa: E402
from d3d_amd.abstraction import TransformSet                 # noqa: E402


def random_rig(rng, ncam):
    ts = TransformSet("base")
    frames = []
    for k in range(ncam):
        name = "cam%d" % k
        w, h = int(rng.integers(64, 2048)), int(rng.integers(64, 1536))
        f = rng.uniform(0.3, 2.0) * w
        dist = []
        if rng.random() < 0.6:
            dist = (rng.normal(0, 1, 5) * [0.4, 0.2, 0.005, 0.005, 0.1]).tolist()
        if rng.random() < 0.7:
            ts.set_intrinsic_pinhole(name, (w, h), w / 2 + rng.normal(0, 10), h / 2 + rng.normal(0, 10), f, f * rng.uniform(0.9, 1.1),
                                     s=rng.normal(0, 1) if rng.random() < 0.3 else 0, distort_coeffs=dist)
        else:
            P = np.array([[w / 2, -f, 0], [h / 2, 0, -f], [1, 0, 0]]) + rng.normal(0, 0.01, (3, 3))
            ts.set_intrinsic_camera(name, P, (w, h), rotate=False, distort_coeffs=dist,
                                    intri_matrix=np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]]) if dist else None)
        ts.set_extrinsic(rigid(rng.uniform(-np.pi, np.pi), rng.normal(0, 0.1), rng.normal(0, 0.1), rng.normal(0, 1, 3)), frame_to=name)
        frames.append(name)
    return ts, frames


def random_cloud(rng):
    n = int(rng.choice([0, 1, 63, 1000, 1024, 5000, 70000, 300000]))
    cols = int(rng.choice([3, 4, 6]))
    dtype = rng.choice([np.float32, np.float64])
    pts = np.concatenate([rng.uniform(-80, 80, (n, 2)), rng.uniform(-5, 8, (n, 1)), rng.random((n, cols - 3))], 1)
    if n > 10:
        bad = rng.integers(0, n, 6)
        pts[bad[0], 0] = np.nan
        pts[bad[1], 1] = np.inf
        pts[bad[2], 2] = -np.inf
        pts[bad[3], :3] = 0.0
    return pts.astype(dtype)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    for seed in range(seed0, seed0 + rounds):
        rng = np.random.default_rng(seed)
        ncam = int(rng.integers(1, 11))
        ts, frames = random_rig(rng, ncam)
        pts = random_cloud(rng)
        dev = torch.from_numpy(pts).cuda()
        n_near = 0
        for k, frame in enumerate(frames):
            meta = ts.intrinsics_meta[frame]
            model = cr.project(pts, ts.get_extrinsic(frame), ts.intrinsics[frame], meta.width, meta.height,
                               np.asarray(meta.distort_coeffs, np.float64), meta.intri_matrix)

            def call(ro, rd):
                res = ts.project_points_to_cameras(dev, frames, remove_outlier=ro, return_dmask=rd)[k]
                return tuple(r.cpu().numpy() for r in res)
            n_near += cr.check_projection(cr.expected(model), cr.full_form(len(pts), call), cr.near_points(model), "seed %d %s" % (seed, frame))
        got = ts.transform_points(dev, frames[0]).cpu().numpy()
        with np.errstate(all="ignore"):
            exp = cr.transform(pts, ts.get_extrinsic(frames[0]))
        assert np.allclose(got, exp, rtol=cr.XYZ_TOL, atol=cr.XYZ_TOL, equal_nan=True), "seed %d transform_points" % seed
        print("seed %d: %d cameras, %s %s, near %d: ok" % (seed, ncam, pts.shape, pts.dtype, n_near), flush=True)


if __name__ == "__main__":
    main()
