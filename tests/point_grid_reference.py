"""The numpy model of PointGrid (the rules of include/d3d_hip.h): bounds, plan, mapping, order / offsets / packed, and the cells a
query walks -- the ball box and the kNN rings with their stop bound -- as plain Python over fp64, for the superset checks."""
import math

import numpy as np

SLACK = 2.0 ** -20
OUT = 2.0 ** -50
ROW_MAX = 2 ** 31 - 1


def _segments(offsets, total):
    offs = [0, total] if offsets is None else [int(v) for v in offsets]
    return list(zip(offs[:-1], offs[1:]))


def bounds_model(points, offsets=None):
    """-> (bounds [S, 6] float64, finite_rows [S] int64)"""
    points = np.asarray(points)
    segs = _segments(offsets, points.shape[0])
    bounds, rows = np.zeros((len(segs), 6), np.float64), np.zeros(len(segs), np.int64)
    for s, (a, b) in enumerate(segs):
        x = points[a:b, :3].astype(np.float64)
        x = x[np.isfinite(x).all(axis=1)]
        rows[s] = len(x)
        if len(x):
            bounds[s, :3], bounds[s, 3:] = x.min(0), x.max(0)
    return bounds, rows


def plan_model(bounds, finite_rows, cell_size, max_cells_per_point=2.0):
    """-> ([dict(lo, h, inv_h, dims, base)], total_cells); ValueError above 2^31 - 1 cells"""
    out, base = [], 0
    for b, rows in zip(np.asarray(bounds, np.float64).reshape(-1, 6), np.asarray(finite_rows).reshape(-1)):
        lo = tuple(float(v) for v in b[:3]) if rows > 0 else (0.0, 0.0, 0.0)
        ext = [float(b[3 + a]) - float(b[a]) if rows > 0 else 0.0 for a in range(3)]
        cap = max(64.0, float(math.ceil(max_cells_per_point * float(rows))))
        h = float(cell_size)
        while not (math.floor(ext[0] / h) + 1.0) * (math.floor(ext[1] / h) + 1.0) * (math.floor(ext[2] / h) + 1.0) <= cap:
            h = h * 2.0
        inv_h = 1.0 / h
        dims = tuple(int(math.floor(e * inv_h) + 1.0) for e in ext)
        cells = dims[0] * dims[1] * dims[2]
        if cells > ROW_MAX:
            raise ValueError("too many cells")
        out.append(dict(lo=lo, h=h, inv_h=inv_h, dims=dims, base=base))
        base += cells + 1
        if base > ROW_MAX:
            raise ValueError("too many cells")
    return out, base


def cell_rel(t, inv_h, dim):
    """clamp(floor(t * inv_h), 0, dim - 1) while still a double; NaN -> 0"""
    f = np.floor(np.float64(t) * np.float64(inv_h))
    if not f > 0.0:
        return 0
    return int(min(f, float(dim - 1)))


def mapping_model(points, plan, offsets=None):
    """-> mapping [N] int64: the cell of every row, -1 for a NaN row, the overflow cell for an infinite one"""
    points = np.asarray(points)
    out = np.full(points.shape[0], -1, np.int64)
    for g, (a, b) in zip(plan, _segments(offsets, points.shape[0])):
        dx, dy, dz = g["dims"]
        for i in range(a, b):
            x = points[i, :3].astype(np.float64)
            if np.isnan(x).any():
                continue
            if np.isinf(x).any():
                out[i] = g["base"] + dx * dy * dz
                continue
            c = [cell_rel(x[k] - np.float64(g["lo"][k]), g["inv_h"], g["dims"][k]) for k in range(3)]
            out[i] = g["base"] + (c[2] * dy + c[1]) * dx + c[0]
    return out


def index_model(mapping, total_cells, points):
    """-> (order int32 [K'], offsets int64 [total_cells + 1], packed [K', 3] in the dtype of the points)"""
    rows = np.nonzero(mapping >= 0)[0]
    order = rows[np.argsort(mapping[rows], kind="stable")].astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(mapping[rows], minlength=total_cells))]).astype(np.int64)
    return order, offsets, np.asarray(points)[order.astype(np.int64), :3]


def grid_model(points, cell_size, offsets=None, max_cells_per_point=2.0):
    """everything at once -> dict(plan, total, mapping, order, offsets, packed)"""
    bounds, rows = bounds_model(points, offsets)
    plan, total = plan_model(bounds, rows, cell_size, max_cells_per_point)
    mapping = mapping_model(points, plan, offsets)
    order, offs, packed = index_model(mapping, total, points)
    return dict(plan=plan, total=total, mapping=mapping, order=order, offsets=offs, packed=packed, bounds=bounds, rows=rows)


def _cells_rows(grid, g, box):
    """the rows of the cells of box = ((x0, x1), (y0, y1), (z0, z1)) of segment g, through order / offsets"""
    dx, dy, _ = g["dims"]
    out = []
    for z in range(box[2][0], box[2][1] + 1):
        for y in range(box[1][0], box[1][1] + 1):
            a = g["base"] + (z * dy + y) * dx
            out.append(grid["order"][grid["offsets"][a + box[0][0]]:grid["offsets"][a + box[0][1] + 1]])
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def ball_box(g, centre, radius, dtype):
    """the box of cells d3d_ball_query_grid walks for one centre, or None: (x0, x1), (y0, y1), (z0, z1)"""
    centre = np.asarray(centre, dtype)[:3]
    if not np.isfinite(centre).all():
        return None
    big_r = np.float64(dtype(radius)) * (1.0 + SLACK)
    box = []
    with np.errstate(over="ignore"):
        for a in range(3):
            u = np.float64(centre[a]) - np.float64(g["lo"][a])
            e0, e1 = u - big_r, u + big_r
            e0, e1 = e0 - abs(e0) * OUT, e1 + abs(e1) * OUT
            if e1 * g["inv_h"] < 0.0 or np.floor(e0 * g["inv_h"]) > float(g["dims"][a] - 1):
                return None
            box.append((cell_rel(e0, g["inv_h"], g["dims"][a]), cell_rel(e1, g["inv_h"], g["dims"][a])))
    return tuple(box)


def ball_candidates(grid, s, centre, radius, dtype):
    """the rows the grid route judges for one centre of segment s, ascending"""
    box = ball_box(grid["plan"][s], centre, radius, dtype)
    return np.zeros(0, np.int32) if box is None else np.sort(_cells_rows(grid, grid["plan"][s], box))


def knn_candidates(grid, s, centre, k, points, dtype):
    """the walk of d3d_knn_query_grid for one centre of segment s, with the model's own q and keys -> (the rows it judged, ascending;
    the number of rings).  A NaN centre judges nothing."""
    g = grid["plan"][s]
    centre = np.asarray(centre, dtype)[:3]
    if np.isnan(centre).any():
        return np.zeros(0, np.int32), 0
    pts = np.asarray(points, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        u = [np.float64(centre[a]) - np.float64(g["lo"][a]) for a in range(3)]
    dims = g["dims"]
    cc = [cell_rel(u[a], g["inv_h"], dims[a]) for a in range(3)]
    least = 4.0 * float(np.finfo(dtype).tiny)
    seen, keys, rho, overflow = [], [], 0, True

    def judge(rows):
        with np.errstate(over="ignore", invalid="ignore"):
            d = pts[rows.astype(np.int64), :3] - centre
            q = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        seen.append(rows)
        keys.extend((float(v), int(r)) for v, r in zip(q, rows) if not np.isnan(v))
        keys.sort()
        del keys[k:]

    while True:
        box = [(max(cc[a] - rho, 0), min(cc[a] + rho, dims[a] - 1)) for a in range(3)]
        rows = _cells_rows(grid, g, box)
        judge(np.setdiff1d(rows, np.concatenate(seen) if seen else np.zeros(0, np.int32)))       # ring rho = its box minus what was walked
        d, is_open = math.inf, False
        with np.errstate(over="ignore", invalid="ignore"):
            for a in range(3):
                if cc[a] - rho > 0:
                    is_open, d = True, min(d, float(u[a] - np.float64(cc[a] - rho) * np.float64(g["h"])))
                if cc[a] + rho < dims[a] - 1:
                    is_open, d = True, min(d, float(np.float64(cc[a] + rho + 1) * np.float64(g["h"]) - u[a]))
        if not is_open:
            break
        dd = d * (1.0 - SLACK) - SLACK * g["h"]
        if dd > 0.0 and len(keys) == k:
            bound = dd * dd * (1.0 - SLACK)
            if keys[-1][0] < bound and bound >= least:
                overflow = False
                break
        rho += 1
    if overflow and (len(keys) < k or not keys[-1][0] < math.inf):
        cell = g["base"] + dims[0] * dims[1] * dims[2]
        judge(grid["order"][grid["offsets"][cell]:grid["offsets"][cell + 1]])
    return np.sort(np.concatenate(seen)), rho + 1
