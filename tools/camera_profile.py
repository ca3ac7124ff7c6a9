"""TransformSet.project_points_to_camera / project_points_to_cameras / transform_points on the GPU (d3d_project_points,
d3d_transform_points): time per call and per kernel, one process, after warm-up, many repetitions.
  * clouds: synth.lidar_like, 120 k and 1 M points, fp32 [N,4], resident on the device;
  * one camera without and with distortion, remove_outlier on and off, with and without dmask;
  * a 6-camera rig in one call against six single calls;
  * transform_points.
Per configuration: the wall time of a call (launches, the one wait for the result sizes and the copies of the results to their
final size included; median and minimum), the time between HIP events around the call on its stream, the kernels' own times
from the library's event profiler (a run of its own: the events serialise the launches), and the bytes the operator has to
move against the kernel time:
    read   2 x N x row bytes               (the count pass and the emit pass each read the cloud once, whatever the cameras)
    write  per camera K x (16 + 8) bytes   (uv and mask of the points in view), + Kd x 8 with dmask,
           or N x 16 + K x 8 with remove_outlier off
Beside them the reference's single-core time for 1 M points per camera kind, as tests/golden/make_camera_golden.py recorded it
(time/*_1M_s in tests/golden/camera_ref_cases.npz).
usage: python tools/camera_profile.py [out.json]   (writes profiles/camera_profile.{json,txt} by default)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from d3d_amd import _lib, synth                                                       # noqa: E402
from d3d_amd.abstraction import TransformSet                                          # noqa: E402

WARMUP, REPS = 10, 100


def timed(fn):
    """-> wall median / min (ms), event median (ms) over REPS calls after WARMUP"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return dict(wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), event_ms_median=float(np.median(dev)))


def kernels(fn, reps=20):
    """-> {kernel: ms per call} from the library's event profiler"""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.d3d_profile_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split(",")
        out[name] = float(ms) / reps
    return out


def rig():
    import camera_cases as cc
    ts = TransformSet("lidar")
    frames = []
    for k in range(6):                      # six cameras around the vehicle, every second one with distortion
        name = "cam%d" % k
        ts.set_intrinsic_pinhole(name, cc.KITTI["size"], cc.KITTI["cx"], cc.KITTI["cy"], cc.KITTI["fx"], cc.KITTI["fy"],
                                 distort_coeffs=cc.DIST_REAL if k % 2 else [])
        ts.set_extrinsic(cc.rigid(2 * np.pi * k / 6, 0.0, 0.0, [0.1 * k, -0.2, 0.3]), frame_to=name)
        frames.append(name)
    return ts, frames


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "camera_profile.json")
    torch.cuda.set_device(0)
    ts, frames = rig()
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, configs=[])
    for n in (120_000, 1_000_000):
        cloud = torch.from_numpy(synth.lidar_like(n, 1)).cuda()
        row = cloud.shape[1] * cloud.element_size()
        for what, frame_list, batched in (("1 camera", ["cam0"], True), ("1 camera, distortion", ["cam1"], True),
                                          ("6 cameras, one call", frames, True), ("6 cameras, six calls", frames, False)):
            for remove_outlier, return_dmask in ((True, False), (True, True), (False, False)):
                if len(frame_list) > 1 and return_dmask:
                    continue
                if batched:
                    def fn():
                        return ts.project_points_to_cameras(cloud, frame_list, remove_outlier=remove_outlier, return_dmask=return_dmask)
                else:
                    def fn():
                        return [ts.project_points_to_camera(cloud, f, remove_outlier=remove_outlier, return_dmask=return_dmask)
                                for f in frame_list]
                sizes = [(len(r[1]), len(r[2]) if return_dmask else 0) for r in ts.project_points_to_cameras(cloud, frame_list, return_dmask=return_dmask)]
                passes = 1 if batched else len(frame_list)
                nbytes = 2 * n * row * passes
                for k, kd in sizes:
                    nbytes += (n * 16 + k * 8) if not remove_outlier else k * 24
                    nbytes += kd * 8
                cfg = dict(points=n, what=what, remove_outlier=remove_outlier, return_dmask=return_dmask, in_view=[s[0] for s in sizes],
                           bytes_to_move=nbytes)
                cfg.update(timed(fn))
                cfg["kernel_ms"] = kernels(fn)
                ksum = sum(cfg["kernel_ms"].values())
                cfg["kernel_ms_sum"] = ksum
                cfg["achieved_GBps_over_kernel_time"] = nbytes / (ksum * 1e-3) / 1e9 if ksum > 0 else None
                res["configs"].append(cfg)
                print(json.dumps(cfg), flush=True)
        cfg = dict(points=n, what="transform_points", bytes_to_move=n * row + n * cloud.shape[1] * 8)
        cfg.update(timed(lambda: ts.transform_points(cloud, "cam0")))
        cfg["kernel_ms"] = kernels(lambda: ts.transform_points(cloud, "cam0"))
        cfg["kernel_ms_sum"] = sum(cfg["kernel_ms"].values())
        cfg["achieved_GBps_over_kernel_time"] = cfg["bytes_to_move"] / (cfg["kernel_ms_sum"] * 1e-3) / 1e9
        res["configs"].append(cfg)
        print(json.dumps(cfg), flush=True)
    golden = os.path.join(ROOT, "tests", "golden", "camera_ref_cases.npz")
    if os.path.exists(golden):
        g = np.load(golden)
        res["reference_cpu_1M_points_s"] = {k: float(g["time/%s_1M_s" % k][0]) for k in ("kitti", "kitti_dist", "barrel")}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out)[0] + ".txt", "w") as f:
        f.write("%s; %d warm-up calls, %d timed calls per line; times in ms\n" % (res["device"], WARMUP, REPS))
        f.write("%9s  %-24s %-7s %-5s %9s %9s %9s %9s %12s %9s\n" % ("points", "what", "remove", "dmask", "wall med", "wall min", "event med",
                                                                      "kernels", "bytes", "GB/s"))
        for c in res["configs"]:
            f.write("%9d  %-24s %-7s %-5s %9.4f %9.4f %9.4f %9.4f %12d %9.1f\n" % (
                c["points"], c["what"], c.get("remove_outlier", "-"), c.get("return_dmask", "-"), c["wall_ms_median"], c["wall_ms_min"],
                c["event_ms_median"], c["kernel_ms_sum"], c["bytes_to_move"], c["achieved_GBps_over_kernel_time"]))
            f.write("           " + ", ".join("%s %.4f" % kv for kv in c["kernel_ms"].items()) + "\n")
        for k, v in res.get("reference_cpu_1M_points_s", {}).items():
            f.write("reference, one CPU core, 1 M points, %s: %.1f ms\n" % (k, v * 1e3))


if __name__ == "__main__":
    main()
