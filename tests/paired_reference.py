"""CPU reference of the paired box operators (box2d_iou_paired, box3d_iou_paired), numpy fp64 on top of the C oracle; the
seeded inputs their tests share.  No GPU, no torch.

value of pair i   2D 'box' / 'rbox': oracle.iou2d_pairs; 'grbox' / 'drbox': oracle.loss_iou2dr on the 1 x 1 matrix;
                  3D: the BEV value of columns (x, y, lx, ly, rz) times max(min(zmax) - max(zmin), 0) / max(max(zmax) - min(zmin), 1e-6),
                  0 where the BEV value is 0 (the definition of oracle.iou3d, here in fp64)
gradient          central differences, one parameter of ALL pairs moved at once (the pairs are independent)"""
import functools

import numpy as np

import oracle

N = 40
H = 1e-6
METHODS_2D = ("box", "rbox", "grbox", "drbox")
METHODS_3D = ("box", "rbox")
BEV = [0, 1, 3, 4, 6]


def rand_boxes(n, seed, spread=8.0):
    """the generator of tests/test_gpu_boxloss.py (_rand_boxes), restated: that module needs torch and a GPU mark"""
    rng = np.random.default_rng(seed)
    return np.stack([(rng.random(n) - .5) * spread, (rng.random(n) - .5) * spread, rng.random(n) * 5 + .1, rng.random(n) * 5 + .1,
                     (rng.random(n) - .5) * 10], 1)


def with_z(b1, b2, seed):
    """[n,5] x 2 -> [n,7] x 2 (x, y, z, lx, ly, lz, rz): centre (u - .5) * 2, height u * 2 + .5, drawn for boxes 1 then boxes 2"""
    rng = np.random.default_rng(seed)
    out = []
    for b in (b1, b2):
        zc, lz = (rng.random(len(b)) - .5) * 2, rng.random(len(b)) * 2 + .5
        out.append(np.stack([b[:, 0], b[:, 1], zc, b[:, 2], b[:, 3], lz, b[:, 4]], 1))
    return out


def seeded_pairs():
    """(b1[40,5], b2[40,5], b1_3d[40,7], b2_3d[40,7], w[40]) -- fresh copies"""
    b1, b2 = rand_boxes(N, 21, 6.0), rand_boxes(N, 22, 6.0)
    c1, c2 = with_z(b1, b2, 24)
    return b1, b2, c1, c2, np.random.default_rng(23).random(N)


def iou2d(b1, b2, method):
    b1, b2 = np.ascontiguousarray(b1, np.float64), np.ascontiguousarray(b2, np.float64)
    if method in ("box", "rbox"):
        idx = np.arange(len(b1))
        return oracle.iou2d_pairs(b1, b2, idx, idx, method)
    return np.array([oracle.loss_iou2dr(b1[i:i + 1], b2[i:i + 1], method)[0, 0] for i in range(len(b1))])


def iou3d(b1, b2, method):
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    bev = iou2d(b1[:, BEV], b2[:, BEV], method)
    top1, bot1, top2, bot2 = b1[:, 2] + b1[:, 5] / 2, b1[:, 2] - b1[:, 5] / 2, b2[:, 2] + b2[:, 5] / 2, b2[:, 2] - b2[:, 5] / 2
    zi = np.maximum(np.minimum(top1, top2) - np.maximum(bot1, bot2), 0)
    zu = np.maximum(np.maximum(top1, top2) - np.minimum(bot1, bot2), 1e-6)
    return np.where(bev != 0, bev * (zi / zu), 0.0)


def central_gradients(fn, b1, b2, w, h=H):
    """gradients of (fn(b1, b2) * w).sum() by every parameter of b1 and of b2"""
    g1, g2 = np.zeros_like(b1), np.zeros_like(b2)
    for k in range(b1.shape[1]):
        p, m = b1.copy(), b1.copy()
        p[:, k] += h
        m[:, k] -= h
        g1[:, k] = w * (fn(p, b2) - fn(m, b2)) / (2 * h)
        p, m = b2.copy(), b2.copy()
        p[:, k] += h
        m[:, k] -= h
        g2[:, k] = w * (fn(b1, p) - fn(b1, m)) / (2 * h)
    return g1, g2


@functools.lru_cache(maxsize=None)
def reference(dims, method):
    """(values[40], g1, g2) of the seeded pairs, computed once per (dims, method); callers must not write into them"""
    b1, b2, c1, c2, w = seeded_pairs()
    fn = functools.partial(iou2d if dims == 2 else iou3d, method=method)
    x1, x2 = (b1, b2) if dims == 2 else (c1, c2)
    out = (fn(x1, x2),) + central_gradients(fn, x1, x2, w)
    for a in out:
        a.setflags(write=False)
    return out
