"""d3d_bessel_e (i0e / i1e, bessel.hip) on the GPU: time per call and bytes per second, one process, HIP events after warm-up.
  * both functions, fp32 and fp64, n = 2^24 and 2^28, input and output resident on the device, the raw C entry (no allocation
    inside the timed window);
  * inputs uniform in +-5 (every wavefront on the series for |x| <= 8), in 9 .. 20 (every wavefront on the series for |x| > 8)
    and in +-20 (nearly every wavefront holds both sides: both series run and a select picks);
  * bytes: one read and one write per element, 8 B per fp32 element and 16 B per fp64 element, over the event time; the share
    of the 8 TB/s HBM peak beside it;
  * for information, torch.special.i0e / i1e on the same tensor, timed the same way (another algorithm with other roundings:
    no yardstick for the bits, only for what an elementwise Bessel pass costs on this device).
Each row is the median over REPS calls timed one by one; d3d_i0e_backward (two reads, one write per element) closes the table.
usage: python tools/math_profile.py [out.txt]   (writes profiles/math_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib                                                              # noqa: E402

PEAK_GBPS = 8000.0
WARMUP = 5
RANGES = (("+-5 (small series)", -5.0, 5.0), ("9..20 (large series)", 9.0, 20.0), ("+-20 (mixed wavefronts)", -20.0, 20.0))


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "math_profile.txt")
    assert torch.cuda.is_available(), "math_profile needs a GPU"
    torch.cuda.set_device(0)
    lib = _lib.load()
    lines = ["%s; %d warm-up calls, then the median (and minimum) of the timed calls, each between its own pair of HIP events; "
             "GB/s = (read + written bytes) / median; peak = 8000 GB/s" % (torch.cuda.get_device_name(0), WARMUP),
             "%-5s %-5s %10s %-24s %10s %10s %9s %7s %14s" % ("fn", "dtype", "n", "input", "median ms", "min ms", "GB/s", "of peak",
                                                              "torch.special ms")]
    print("\n".join(lines), flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for dtype, code, esize in ((torch.float32, _lib.F32, 4), (torch.float64, _lib.F64, 8)):
        for n in (1 << 24, 1 << 28):
            reps = 50 if n == 1 << 24 else 12
            x = torch.empty(n, dtype=dtype, device="cuda")
            out = torch.empty_like(x)
            for label, lo, hi in RANGES:
                x.uniform_(lo, hi, generator=g)
                for order, tfn in ((0, torch.special.i0e), (1, torch.special.i1e)):
                    def fn():
                        rc = lib.d3d_bessel_e(order, _lib.ptr(x), n, code, _lib.ptr(out), _lib.stream_ptr())
                        assert rc == _lib.OK
                    med, mn = timed(fn, reps)
                    tmed, _ = timed(lambda: tfn(x, out=out), reps)
                    gbps = 2.0 * n * esize / (med * 1e-3) / 1e9
                    line = "%-5s %-5s %10d %-24s %10.4f %10.4f %9.1f %7.3f %14.4f" % (
                        "i%de" % order, "fp32" if esize == 4 else "fp64", n, label, med, mn, gbps, gbps / PEAK_GBPS, tmed)
                    lines.append(line)
                    print(line, flush=True)
            if n == 1 << 28:                                  # the backward: x and grad read, grad_x written
                x.uniform_(-20.0, 20.0, generator=g)
                grad = torch.empty_like(x).uniform_(-1.0, 1.0, generator=g)

                def bwd():
                    rc = lib.d3d_i0e_backward(_lib.ptr(x), _lib.ptr(grad), n, code, _lib.ptr(out), _lib.stream_ptr())
                    assert rc == _lib.OK
                med, mn = timed(bwd, reps)
                gbps = 3.0 * n * esize / (med * 1e-3) / 1e9
                line = "%-5s %-5s %10d %-24s %10.4f %10.4f %9.1f %7.3f %14s" % (
                    "bwd", "fp32" if esize == 4 else "fp64", n, RANGES[2][0], med, mn, gbps, gbps / PEAK_GBPS, "-")
                lines.append(line)
                print(line, flush=True)
                del grad
            del x, out
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
