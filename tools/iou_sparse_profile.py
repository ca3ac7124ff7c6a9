"""box2d_iou_sparse / iou3d_sparse (boxsparse.hip) against the only route a caller had before them, one process, HIP events:
  (a) matrix  D = box2d_iou(b1, b2, 'rbox', precise=True) (resp. iou3d), pairs = (D > 0).nonzero(), values = D[pairs[:,0], pairs[:,1]]
  (b) sparse  pairs, values = box2d_iou_sparse(b1, b2, 'rbox', 0.0, precise=True) (resp. iou3d_sparse)
Workloads: boxes at config 3's density (synth.boxes2d_sparse) at 5 k x 5 k and 20 k x 20 k, fp32 boxes with precise=True and fp64
boxes -- the matrix fits, both answers are asserted equal (indices equal, values bit for bit) before anything is timed; 100 k x
100 k with the sparse operator alone (the line says how large the matrix would be); config 4's 20 k x 5 k 7-column boxes
(synth.boxes3d_eval).  The variants alternate inside every round; WARMUP rounds are dropped, then the median, minimum and maximum
over the timed rounds, each variant between its own pair of events per round (the sparse operator's one host read is inside its
pair).  Then the sparse operator's kernels one by one (the library's per-kernel timing, which serialises the launches) and the
host read, as shares of their sum.
usage: python tools/iou_sparse_profile.py [out.txt]   (writes profiles/iou_sparse_profile.txt by default)"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib, synth                                                       # noqa: E402
from d3d_amd.box import box2d_iou, box2d_iou_sparse, iou3d, iou3d_sparse              # noqa: E402

WARMUP = 3
MATRIX_MAX = 20000
# (name, dims, rows, columns, numpy dtype, timed rounds)
WORKLOADS = (("2D rbox fp32 precise", 2, 5000, 5000, np.float32, 30), ("2D rbox fp64", 2, 5000, 5000, np.float64, 30),
             ("2D rbox fp32 precise", 2, 20000, 20000, np.float32, 15), ("2D rbox fp64", 2, 20000, 20000, np.float64, 15),
             ("2D rbox fp32 precise", 2, 100000, 100000, np.float32, 10), ("2D rbox fp64", 2, 100000, 100000, np.float64, 10),
             ("3D rbox fp32", 3, 20000, 5000, np.float32, 20))


def boxes(dims, n, m, dtype):
    if dims == 3:
        pred, gt = synth.boxes3d_eval(m, n // m)
        return torch.from_numpy(np.ascontiguousarray(pred[:, :7], dtype)).cuda(), torch.from_numpy(np.ascontiguousarray(gt[:, :7], dtype)).cuda()
    b1, b2 = synth.boxes2d_sparse(n, 11)[0], synth.boxes2d_sparse(m, 12)[0]
    return torch.from_numpy(b1.astype(dtype)).cuda(), torch.from_numpy(b2.astype(dtype)).cuda()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_shares(fn, reps=5):
    lib = _lib.load()
    fn()
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
        if name.startswith("k_sp_") or name == "k_scan_tile_sums":        # (the scan over the tile sums is the shared kernel)
            out[name] = float(ms) / reps
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iou_sparse_profile.txt")
    assert torch.cuda.is_available(), "iou_sparse_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; boxes at config 3's density (7 columns: config 4's); %d warm-up rounds, then per variant the median [min .. max] of the "
             "timed rounds in ms, variants alternating inside a round, HIP events around each; threshold 0" % (torch.cuda.get_device_name(0), WARMUP),
             "%-22s %15s %9s %6s %-28s %-28s %8s" % ("workload", "N x M", "K", "rounds", "(a) matrix + nonzero + gather", "(b) sparse", "a / b")]
    print("\n".join(lines), flush=True)
    notes = []
    for name, dims, n, m, dtype, rounds in WORKLOADS:
        b1, b2 = boxes(dims, n, m, dtype)

        def sparse():
            if dims == 2:
                return box2d_iou_sparse(b1, b2, method="rbox", threshold=0.0, precise=True)
            return iou3d_sparse(b1, b2, method="rbox", threshold=0.0)

        def matrix():
            d = box2d_iou(b1, b2, method="rbox", precise=True) if dims == 2 else iou3d(b1, b2, "rbox")
            pairs = (d > 0).nonzero()
            return pairs, d[pairs[:, 0], pairs[:, 1]]

        variants = [sparse] + ([matrix] if max(n, m) <= MATRIX_MAX else [])
        ps, vs = sparse()
        if matrix in variants:
            pm, vm = matrix()
            assert torch.equal(ps, pm), "the sparse pairs are not the matrix's"
            assert torch.equal(vs.view(torch.int64 if vs.dtype == torch.float64 else torch.int32),
                               vm.view(torch.int64 if vm.dtype == torch.float64 else torch.int32)), "the sparse values are not the matrix's"
            del pm, vm
        ms = {f: [] for f in variants}
        for r in range(WARMUP + rounds):
            for f in variants:
                t = event_ms(f)
                if r >= WARMUP:
                    ms[f].append(t)
        med = {f: float(np.median(ms[f])) for f in variants}
        cell = lambda f: "%.4f [%.4f .. %.4f]" % (med[f], min(ms[f]), max(ms[f])) if f in ms else "-"      # noqa: E731
        lines.append("%-22s %15s %9d %6d %-28s %-28s %8s" % (name, "%d x %d" % (n, m), len(ps), rounds, cell(matrix), cell(sparse),
                                                           "%.2fx" % (med[matrix] / med[sparse]) if matrix in ms else "-"))
        if matrix not in ms:
            lines[-1] += "   (a) not run: the [N,M] matrix alone is %.1f GB" % (n * m * b1.element_size() / 1e9)
        print(lines[-1], flush=True)
        shares = kernel_shares(sparse)
        off = torch.zeros(8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            int(off[7])
        shares["host read of offsets[n]"] = (time.perf_counter() - t0) / 20 * 1e3
        total = sum(shares.values())
        notes.append("%-22s %15s  " % (name, "%d x %d" % (n, m)) + "  ".join("%s %.4f ms (%.0f %%)" % (k, v, 100 * v / total) for k, v in shares.items()))
    lines.append("the sparse operator's launches one by one (serialised) and its host read on an idle stream, ms per call and share of their sum:")
    lines += notes
    print("\n".join(lines[-len(notes) - 1:]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
