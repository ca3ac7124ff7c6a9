"""SegmentationEvaluator on the GPU (d3d_segeval): per-call times on a 120 k-point frame (semantic / panoptic), a batch of 100
such frames in one call (calc_stats_batch), an 8 M-point frame; per-kernel times from the library's event profiler; the
roofline fraction with bytes = 2 B/point semantic, 6 B/point panoptic + frame_off + the [F, 256] outputs, against a measured
read-copy bandwidth; beside each, the reference's single-core CPU time that tests/golden/make_seg_golden.py recorded.
usage: python tools/segeval_profile.py [out.json]"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3d_amd import _lib, synth                         # noqa: E402
from d3d_amd.benchmarks import SegmentationEvaluator    # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "seg_ref_cases.npz")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def kernels(fn):
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 14)
    lib.d3d_profile_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split(",")
        out[name] = round(float(ms) * 1e3 / int(calls), 2)
    return out


def copy_bandwidth():
    """GB/s of a 1 GiB device-to-device copy (read + write bytes)"""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    med, best = timed(lambda: b.copy_(a), 10)
    return 2 * a.numel() / (best * 1e-6) / 1e9


def main():
    torch.cuda.set_device(0)
    ref = np.load(GOLD)
    ev = SegmentationEvaluator(list(range(1, 20)))
    lib = _lib.load()
    bw = copy_bandwidth()
    res = dict(copy_GBps=round(bw, 1), cases={})
    shapes = (("frame120k", 120000, 1), ("batch100", 120000, 100), ("frame8m", 8000000, 1))
    for tag, n, frames in shapes:
        frs = [synth.segmentation_frame(n, seed=s) for s in range(min(frames, 10))]
        cat = [torch.from_numpy(np.concatenate([frs[f % len(frs)][k] for f in range(frames)])).cuda() for k in range(4)]
        off = np.arange(frames + 1, dtype=np.int64) * n
        for pano in (False, True):
            ids = (cat[2], cat[3]) if pano else (None, None)
            if frames == 1:
                fn = lambda: ev.calc_stats(cat[0], cat[1], *ids)                       # noqa: E731
            else:
                fn = lambda: ev.calc_stats_batch(cat[0], cat[1], *ids, off)             # noqa: E731
            # the C call alone (what the kernels cost, no Python, no result copy)
            dev = cat[0].device
            out = torch.empty((7, frames, 256), dtype=torch.int32, device=dev)
            foff = torch.from_numpy(off).to(dev)
            wsb = lib.d3d_segeval_workspace_bytes(n * frames, frames)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
            mask = (ctypes.c_uint32 * 8)(*ev._mask)
            rows = [_lib.ptr(out[k]) for k in range(7)]
            args = [_lib.ptr(cat[0]), _lib.ptr(cat[1]), _lib.ptr(ids[0]) if pano else None, _lib.ptr(ids[1]) if pano else None,
                    _lib.ptr(foff), n * frames, frames, mask, 0, 0] + rows + [_lib.ptr(ws), wsb, _lib.stream_ptr()]
            ccall = lambda: _lib.check(lib.d3d_segeval(*args), "d3d_segeval")            # noqa: E731
            c_med, c_min = timed(ccall, 20)
            t0 = time.perf_counter()
            reps = 20
            for _ in range(reps):
                fn()
            py_us = (time.perf_counter() - t0) / reps * 1e6
            nbytes = n * frames * (6 if pano else 2) + (frames + 1) * 8 + frames * 256 * 4 * 7
            key = "%s_%s" % (tag, "pano" if pano else "sem")
            cpu_ms = float(ref["time/" + key][0]) * 1e3 if ("time/" + key) in ref.files else None
            r = dict(points=n * frames, frames=frames, gpu_call_us_median=round(c_med, 1), gpu_call_us_min=round(c_min, 1),
                     python_call_us=round(py_us, 1), kernels_us=kernels(ccall), bytes=nbytes,
                     roofline_fraction=round(nbytes / (c_min * 1e-6) / 1e9 / bw, 4),
                     workspace_bytes=int(wsb), reference_cpu_ms=cpu_ms,
                     speedup_vs_reference=round(cpu_ms * 1e3 / c_med, 1) if cpu_ms else None)
            res["cases"][key] = r
            print("%-16s gpu %8.1f us (min %8.1f)  python %8.1f us  ref cpu %9.2f ms  x%-8s roofline %.3f  %s" % (
                key, c_med, c_min, py_us, cpu_ms or float("nan"), r["speedup_vs_reference"], r["roofline_fraction"],
                r["kernels_us"]))
            del ws
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
