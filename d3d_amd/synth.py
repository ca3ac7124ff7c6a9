"""Synthetic workloads of BASELINE.json's configs; numpy, seeded, host side."""
import numpy as np

KITTI_BOUNDS = [0, 70.4, -40, 40, -3, 1]
KITTI_SHAPE = [704, 800, 40]          # 0.1 m voxels
WAYMO_BOUNDS = [-75.2, 75.2, -75.2, 75.2, -2, 4]
WAYMO_SHAPE = [3008, 3008, 120]       # 0.05 m voxels


def lidar_like(n, seed=0, bounds=KITTI_BOUNDS):
    """LiDAR-like cloud [n,4] f32: r = rmax*u^2 + 2, uniform azimuth, 70 % ground z = -1.73 + 0.03 N(0,1),
    30 % uniform z, uniform intensity; rejection-filtered to `bounds`, first n kept."""
    xr, yr, zr = bounds[0:2], bounds[2:4], bounds[4:6]
    rng = np.random.default_rng(seed)
    rmax = np.hypot(max(abs(xr[0]), abs(xr[1])), max(abs(yr[0]), abs(yr[1])))
    chunks, have = [], 0
    while have < n:
        m = max(2 * (n - have), 1024)
        r = rmax * rng.random(m) ** 2 + 2
        az = rng.random(m) * 2 * np.pi
        x, y = r * np.cos(az), r * np.sin(az)
        ground = rng.random(m) < 0.7
        z = np.where(ground, -1.73 + 0.03 * rng.standard_normal(m), zr[0] + (zr[1] - zr[0]) * rng.random(m))
        pts = np.stack([x, y, z, rng.random(m)], 1).astype(np.float32)
        ok = (pts[:, 0] >= xr[0]) & (pts[:, 0] < xr[1]) & (pts[:, 1] >= yr[0]) & (pts[:, 1] < yr[1]) & \
             (pts[:, 2] >= zr[0]) & (pts[:, 2] < zr[1])
        chunks.append(pts[ok])
        have += int(ok.sum())
    return np.ascontiguousarray(np.concatenate(chunks)[:n])


def uniform_cloud(n, seed=0, bounds=KITTI_BOUNDS):
    rng = np.random.default_rng(seed)
    lo = np.array([bounds[0], bounds[2], bounds[4], 0], np.float64)
    hi = np.array([bounds[1], bounds[3], bounds[5], 1], np.float64)
    return (lo + (hi - lo) * rng.random((n, 4))).astype(np.float32)


def boxes2d_sparse(n, seed=1, dtype=np.float64):
    """cfg3: same density as reference test/test_box.py:126-131 (500 boxes in 200 x 400)."""
    rng = np.random.default_rng(seed)
    side = np.sqrt(n / 500.0)
    b = np.stack([rng.random(n) * 200 * side, rng.random(n) * 400 * side, rng.random(n) * 20 + 10,
                  rng.random(n) * 30 + 5, rng.random(n) * 2 - 1], 1)
    scores = rng.random(n)
    return b.astype(dtype), scores.astype(dtype)


def boxes2d_dense(n, seed=1, dtype=np.float64):
    """the reference's own benchmark boxes (test/compare/benchmark_riou.py:70-74)"""
    rng = np.random.default_rng(seed)
    b = np.stack([(rng.random(n) - 0.5) * 10, (rng.random(n) - 0.5) * 10, rng.random(n) * 5, rng.random(n) * 5,
                  (rng.random(n) - 0.5) * 10], 1)
    return b.astype(dtype), rng.random(n).astype(dtype)


def boxes3d_eval(n_gt=5000, rep=4, seed=2):
    """cfg4: GT [n_gt,7] car-like boxes over 150 x 150 m; preds = each GT repeated `rep` times with noise."""
    rng = np.random.default_rng(seed)
    gt = np.stack([rng.random(n_gt) * 150, rng.random(n_gt) * 150, rng.random(n_gt) * 2 - 2,
                   rng.random(n_gt) * 1.5 + 3.5, rng.random(n_gt) * 0.5 + 1.6, rng.random(n_gt) * 0.5 + 1.4,
                   rng.random(n_gt) * 2 * np.pi - np.pi], 1)
    pred = np.repeat(gt, rep, axis=0)
    pred[:, 0:3] += 0.3 * rng.standard_normal((len(pred), 3))
    pred[:, 3:6] += 0.1 * rng.standard_normal((len(pred), 3))
    pred[:, 6] += 0.1 * rng.standard_normal(len(pred))
    return pred.astype(np.float32), gt.astype(np.float32)


def segmentation_frame(n, num_classes=19, inst_per_class=30, noise=0.05, seed=0):
    """A panoptic LiDAR frame for SegmentationEvaluator: labels 0 (unlabelled) .. num_classes, each class with inst_per_class
    instances (ids 1 ..), every instance a contiguous run of points (segments in random order, Dirichlet sizes); the
    prediction relabels a `noise` fraction of the points and renumbers the ids.  -> gt_labels, pred_labels (u8),
    gt_ids, pred_ids (u16)."""
    rng = np.random.default_rng(seed)
    k = num_classes * inst_per_class
    seg_label = np.concatenate([1 + np.arange(k) // inst_per_class, [0]]).astype(np.uint8)
    seg_id = np.concatenate([1 + np.arange(k) % inst_per_class, [0]]).astype(np.uint16)
    sizes = rng.multinomial(n, rng.dirichlet(np.ones(k + 1)))
    order = rng.permutation(k + 1)
    gt_labels = np.repeat(seg_label[order], sizes[order])
    gt_ids = np.repeat(seg_id[order], sizes[order])
    pred_labels = gt_labels.copy()
    pred_ids = ((gt_ids.astype(np.int64) * 7 + 3) % 1000).astype(np.uint16)
    flip = rng.random(n) < noise
    pred_labels[flip] = rng.integers(0, num_classes + 1, int(flip.sum()))
    pred_ids[flip] = rng.integers(0, 1000, int(flip.sum()))
    return gt_labels, pred_labels, gt_ids, pred_ids


def tracking_sequence(frames=20, n_tracks=30, classes=(1, 2), seed=0, dropout=0.1, swap=0.05, false_tracks=5, jitter=0.3):
    """A seeded tracking sequence: n_tracks objects moving in straight lines, detected with jitter; a detection drops out with
    probability `dropout`, two detections of a frame swap their ids with probability `swap`, `false_tracks` spurious tracks
    per frame.  -> (gt [G,9] f32, dt [D,9] f32, gt_tids u64[G], dt_tids u64[D], gt_offsets [F+1], dt_offsets [F+1]).
    Scores are distinct (uniform), tids are unique per frame and > 0."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-40, 40, (n_tracks, 3)).astype(np.float32)
    pos[:, 2] = rng.uniform(-1, 1, n_tracks)
    vel = rng.normal(0, 0.6, (n_tracks, 3)).astype(np.float32)
    vel[:, 2] = 0
    dims = rng.uniform(1.5, 4.5, (n_tracks, 3)).astype(np.float32)
    yaw = rng.uniform(-np.pi, np.pi, n_tracks).astype(np.float32)
    cls = rng.choice(np.asarray(classes), n_tracks)
    gts, dts, gtids, dtids, go, do = [], [], [], [], [0], [0]
    next_false = 100000
    for f in range(frames):
        p = pos + f * vel
        g = np.concatenate([cls[:, None], np.ones((n_tracks, 1)), p, dims, yaw[:, None]], 1).astype(np.float32)
        keep = rng.random(n_tracks) > dropout * 0.5
        gts.append(g[keep])
        gtids.append(np.arange(1, n_tracks + 1, dtype=np.uint64)[keep])
        det = rng.random(n_tracks) > dropout
        d = g[det].copy()
        d[:, 2:5] += rng.normal(0, jitter, (len(d), 3)).astype(np.float32)
        d[:, 5:8] *= rng.uniform(0.9, 1.1, (len(d), 3)).astype(np.float32)
        d[:, 8] += rng.normal(0, 0.1, len(d)).astype(np.float32)
        dtid = np.arange(1001, 1001 + n_tracks, dtype=np.uint64)[det]
        if len(dtid) >= 2 and rng.random() < swap * len(dtid):
            i, j = rng.choice(len(dtid), 2, replace=False)
            dtid[i], dtid[j] = dtid[j], dtid[i]
        fk = np.concatenate([rng.choice(np.asarray(classes), (false_tracks, 1)), np.zeros((false_tracks, 1)),
                             rng.uniform(-40, 40, (false_tracks, 3)), rng.uniform(1.5, 4.5, (false_tracks, 3)),
                             rng.uniform(-np.pi, np.pi, (false_tracks, 1))], 1).astype(np.float32)
        fk[:, 4] = rng.uniform(-1, 1, false_tracks)
        d = np.concatenate([d, fk])
        d[:, 1] = rng.random(len(d)).astype(np.float32)
        dtid = np.concatenate([dtid, np.arange(next_false, next_false + false_tracks, dtype=np.uint64)])
        next_false += false_tracks
        o = rng.permutation(len(d))
        dts.append(d[o])
        dtids.append(dtid[o])
        go.append(go[-1] + len(gts[-1]))
        do.append(do[-1] + len(d))
    return (np.concatenate(gts), np.concatenate(dts), np.concatenate(gtids), np.concatenate(dtids),
            np.asarray(go, np.int64), np.asarray(do, np.int64))
