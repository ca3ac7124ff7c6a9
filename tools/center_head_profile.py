"""The centre-head operators (csrc/center.hip) against the torch-only routes a detector had before them, one process, HIP events:
  peaks    heatmap_peaks  vs  max_pool2d + `==` + multiply + OpenPCDet's two-stage topk (kernel 1: the two topk's alone);
           4 x 10 x 180 x 180 (nuScenes) and 1 x 3 x 468 x 468 (Waymo), k = 500, kernel 1 and 3, fp32 and bf16
  circle   circle_nms     vs  (a) a cdist-style d2 matrix on the GPU + the sequential sweep over its rows (one host read per row),
                              (b) det3d's loop on the host, copies to and from the GPU included;
           500 and 4096 rows per segment, 1 and 24 segments, fp32, scattered centres (about half survive)
  draw     gaussian_heatmap vs OpenPCDet's per-box Python loop of slice kernels on the GPU; 50 and 500 boxes per sample, batch 4,
           3 classes, 180 x 180
Per workload the variants alternate inside every round; WARMUP rounds are dropped, then the median [min .. max] of the timed rounds.
The results are compared before anything is timed (peaks: values and cells on a tie-free map; circle: the mask; draw: 1 ulp).
Peak memory: torch's allocator high-water mark over one call, above what was allocated before it.  A leg that loses says LOSES.
usage: python tools/center_head_profile.py [out.txt]   (writes profiles/center_head_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd.box import circle_nms, gaussian_heatmap, heatmap_peaks                   # noqa: E402

WARMUP, ROUNDS, SLOW_ROUNDS = 3, 30, 5


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def race(variants, rounds):
    """variants: [(name, fn)] -> {name: (median, min, max)} in ms, alternating inside every round"""
    times = {name: [] for name, _ in variants}
    for r in range(WARMUP + rounds):
        for name, fn in variants:
            t = event_ms(fn)
            if r >= WARMUP:
                times[name].append(t)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in times.items()}


def cell(t):
    return "%8.3f [%7.3f .. %7.3f]" % t


def verdict(ours, theirs):
    ratio = theirs[0] / ours[0]
    return "%6.2fx%s" % (ratio, "" if ratio >= 1 else " LOSES")


# ---------------------------------------------------------------- the torch-only routes
def torch_peaks(heat, k, kernel):
    """CenterNet's _nms, then OpenPCDet's centernet_utils._topk"""
    b, c, h, w = heat.shape
    if kernel > 1:
        hmax = torch.nn.functional.max_pool2d(heat, kernel, 1, kernel // 2)
        heat = heat * (hmax == heat).to(heat.dtype)
    scores, inds = torch.topk(heat.flatten(2, 3), k)
    ys, xs = torch.div(inds, w, rounding_mode="floor"), inds % w
    score, ind = torch.topk(scores.view(b, -1), k)
    classes = torch.div(ind, k, rounding_mode="floor")
    ys, xs = ys.view(b, -1).gather(1, ind), xs.view(b, -1).gather(1, ind)
    return score, classes, ys, xs


def torch_circle_matrix(xy, scores, t, offsets):
    keep = torch.zeros(len(xy), dtype=torch.bool, device=xy.device)
    for lo, hi in zip(offsets, offsets[1:]):
        order = torch.argsort(scores[lo:hi], descending=True, stable=True)
        p = xy[lo:hi][order]
        d = p[:, None, :] - p[None, :, :]
        hit = ((d * d).sum(-1) <= t).triu(1)
        alive = torch.ones(hi - lo, dtype=torch.bool, device=xy.device)
        for a in range(hi - lo):
            if bool(alive[a]):                                                         # (the sweep is sequential: one read per row)
                alive &= ~hit[a]
        keep[lo:hi][order] = alive
    return keep


def host_circle_loop(xy, scores, t, offsets):
    """det3d's loop (numba there; numpy's vector form of the inner loop here), on the host: copies in, mask back"""
    p, s = xy.cpu().numpy(), scores.cpu().numpy()
    keep = np.zeros(len(p), bool)
    for lo, hi in zip(offsets, offsets[1:]):
        order = lo + np.argsort(-s[lo:hi], kind="stable")
        sup = np.zeros(len(p), bool)
        for a, i in enumerate(order):
            if sup[i]:
                continue
            keep[i] = True
            later = order[a + 1:]
            d = p[i] - p[later]
            sup[later[(d * d).sum(1) <= t]] = True
    return torch.from_numpy(keep).to(xy.device)


def torch_draw(centers, radii, classes, shape, offsets):
    """OpenPCDet's draw_gaussian_to_heatmap once per box"""
    b, c, h, w = shape
    out = torch.zeros(shape, device="cuda")
    cs, rs, cl = centers.tolist(), radii.tolist(), classes.tolist()
    for s in range(b):
        for i in range(offsets[s], offsets[s + 1]):
            (x, y), r = cs[i], rs[i]
            d = 2 * r + 1
            ax = torch.arange(-r, r + 1, device="cuda", dtype=torch.float32)
            g = torch.exp(-(ax[None, :] * ax[None, :] + ax[:, None] * ax[:, None]) / (2 * (d / 6) ** 2))
            left, right, top, bottom = min(x, r), min(w - x, r + 1), min(y, r), min(h - y, r + 1)
            view = out[s, cl[i], y - top:y + bottom, x - left:x + right]
            torch.max(view, g[r - top:r + bottom, r - left:r + right], out=view)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "center_head_profile.txt")
    assert torch.cuda.is_available(), "center_head_profile needs a GPU"
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(5)
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of the timed rounds in ms, variants alternating inside a "
             "round, HIP events around each; ratio = baseline / ours" % (torch.cuda.get_device_name(0), WARMUP)]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("heatmap_peaks, k = 500 vs max_pool2d + == + two-stage topk; peak memory of one call in MB")
    say("%-16s %-5s %-6s %-28s %-28s %-14s %9s %9s" % ("shape", "dtype", "kernel", "heatmap_peaks", "torch", "ratio", "ours MB", "torch MB"))
    for shape in ((4, 10, 180, 180), (1, 3, 468, 468)):
        for dtype in (torch.float32, torch.bfloat16):
            n = int(np.prod(shape))
            # fp32: distinct values, so both routes must agree cell for cell; bf16: ties, the values must agree
            base = torch.randperm(n, generator=gen).float().reshape(shape)
            heat = (base / n if dtype == torch.float32 else (base % 30000) / 60000 + 0.25).to(dtype).cuda()
            for kernel in (1, 3):
                ours = heatmap_peaks(heat, 500, kernel)
                theirs = torch_peaks(heat, 500, kernel)
                if dtype == torch.float32:
                    assert torch.equal(ours.scores, theirs[0]) and torch.equal(ours.classes.long(), theirs[1])
                    assert torch.equal(ours.ys.long(), theirs[2]) and torch.equal(ours.xs.long(), theirs[3])
                else:
                    assert torch.equal(ours.scores, theirs[0])                          # (ties in bf16: the values agree, the cells may not)
                res = race([("ours", lambda: heatmap_peaks(heat, 500, kernel)), ("torch", lambda: torch_peaks(heat, 500, kernel))], ROUNDS)
                mem = [peak_bytes(lambda: heatmap_peaks(heat, 500, kernel)) / 2 ** 20, peak_bytes(lambda: torch_peaks(heat, 500, kernel)) / 2 ** 20]
                say("%-16s %-5s %-6d %-28s %-28s %-14s %9.2f %9.2f" % ("x".join(map(str, shape)), str(dtype)[6:].replace("float", "fp").replace("bfp", "bf"),
                                                                        kernel, cell(res["ours"]), cell(res["torch"]), verdict(res["ours"], res["torch"]),
                                                                        mem[0], mem[1]))

    say("circle_nms, fp32 vs (a) d2 matrix + sequential sweep on the GPU, (b) det3d's loop on the host with the copies")
    say("%-14s %-28s %-28s %-28s %-14s %-14s %9s %9s" % ("rows x segs", "circle_nms", "(a) matrix", "(b) host loop", "(a) ratio", "(b) ratio",
                                                        "ours MB", "(a) MB"))
    for per, segs in ((500, 1), (500, 24), (4096, 1), (4096, 24)):
        n = per * segs
        side = float(np.sqrt(per)) * 2.0
        xy = (torch.rand((n, 2), generator=gen) * side).cuda()
        sc = torch.rand((n,), generator=gen).cuda()
        offsets = list(range(0, n + 1, per))
        t = 4.0
        ours = circle_nms(xy, sc, t, offsets=offsets)
        assert torch.equal(ours, host_circle_loop(xy, sc, t, offsets))
        slow = n > 20000
        if not slow:
            assert torch.equal(ours, torch_circle_matrix(xy, sc, t, offsets))
        variants = [("ours", lambda: circle_nms(xy, sc, t, offsets=offsets)), ("host", lambda: host_circle_loop(xy, sc, t, offsets))]
        if not slow:
            variants.append(("matrix", lambda: torch_circle_matrix(xy, sc, t, offsets)))
        res = race(variants, SLOW_ROUNDS if n > 4096 else ROUNDS)
        mem = [peak_bytes(lambda: circle_nms(xy, sc, t, offsets=offsets)) / 2 ** 20,
               float("nan") if slow else peak_bytes(lambda: torch_circle_matrix(xy, sc, t, offsets)) / 2 ** 20]
        say("%-14s %-28s %-28s %-28s %-14s %-14s %9.2f %9.2f  kept %d" % (
            "%d x %d" % (per, segs), cell(res["ours"]), cell(res["matrix"]) if not slow else "not run (minutes)", cell(res["host"]),
            verdict(res["ours"], res["matrix"]) if not slow else "-", verdict(res["ours"], res["host"]), mem[0], mem[1], int(ours.sum())))

    say("gaussian_heatmap, batch 4, 3 classes, 180 x 180 vs the per-box Python loop of slice kernels")
    say("%-14s %-28s %-28s %-14s %9s %9s" % ("boxes/sample", "gaussian_heatmap", "per-box loop", "ratio", "ours MB", "loop MB"))
    shape = (4, 3, 180, 180)
    for per in (50, 500):
        m = 4 * per
        centers = torch.stack([torch.randint(0, 180, (m,), generator=gen), torch.randint(0, 180, (m,), generator=gen)], 1)
        radii, classes = torch.randint(2, 7, (m,), generator=gen), torch.randint(0, 3, (m,), generator=gen)
        offsets = list(range(0, m + 1, per))
        dc, dr, dl = centers.cuda(), radii.cuda(), classes.cuda()
        ours, theirs = gaussian_heatmap(dc, dr, dl, shape, offsets), torch_draw(centers, radii, classes, shape, offsets)
        assert torch.equal(ours == 0, theirs == 0) and float((ours - theirs).abs().max()) < 1e-6      # (the loop's exp is fp32)
        res = race([("ours", lambda: gaussian_heatmap(dc, dr, dl, shape, offsets)),
                    ("loop", lambda: torch_draw(centers, radii, classes, shape, offsets))], SLOW_ROUNDS)
        mem = [peak_bytes(lambda: gaussian_heatmap(dc, dr, dl, shape, offsets)) / 2 ** 20,
               peak_bytes(lambda: torch_draw(centers, radii, classes, shape, offsets)) / 2 ** 20]
        say("%-14d %-28s %-28s %-14s %9.2f %9.2f" % (per, cell(res["ours"]), cell(res["loop"]), verdict(res["ours"], res["loop"]), mem[0], mem[1]))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
