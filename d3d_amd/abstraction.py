"""d3d_amd.abstraction -- the point-in-box batch operators of the reference's d3d.abstraction containers on MI355X, at the
ARRAY level (the containers themselves -- ObjectTarget3D, Target3DArray -- are out of scope):

  crop_points(boxes, cloud)              Target3DArray.crop_points   (abstraction.pyx:684-687; one box: :321-324)
  paint_label(boxes, cloud, semantics)   Target3DArray.paint_label   (abstraction.pyx:662-682)

`boxes` is either [M,7] rows (x, y, z, lx, ly, lz, rz) or the [n,9] rows of Target3DArray.to_numpy (label, score, x, y, z,
lx, ly, lz, yaw; abstraction.pyx:263-272), read in place.  Per pair the test is box3dr_contains (dgal_wrap.h:6-19): closed z
interval, fp32.  numpy in -> numpy out; torch in -> torch out on the same device.  There is no CPU path: CPU inputs are
staged through the current HIP device.

And the sensor bookkeeping of the reference's TransformSet (abstraction.pyx:777-1035), again on arrays:

  TransformSet.transform_points(points, frame_to, frame_from)                (abstraction.pyx:971-977)
  TransformSet.project_points_to_camera(points, frame_to, frame_from, ...)   (abstraction.pyx:979-1035)
  TransformSet.project_points_to_cameras(points, frames_to, frame_from, ...) the same for a rig in one pass over the cloud

The frames, intrinsics and extrinsics live on the host in fp64 numpy, as there; the per-point work runs on the device in fp64
(d3d_transform_points, d3d_project_points).  transform_objects, dump and load need the containers and are not here.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._rows import back_to_caller, device_of


def _ingress(boxes, cloud):
    # (not _rows.as_tensor: what is neither array nor tensor goes on to the shape checks and fails there, as it always has)
    convert = isinstance(cloud, np.ndarray)
    bx = torch.from_numpy(boxes) if isinstance(boxes, np.ndarray) else boxes
    pts = torch.from_numpy(cloud) if isinstance(cloud, np.ndarray) else cloud
    if bx.dim() != 2 or bx.shape[1] not in (7, 9):
        raise ValueError("boxes should be [M,7] (x,y,z,lx,ly,lz,rz) or [M,9] (label,score,x,y,z,lx,ly,lz,yaw)")
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("cloud should be [N,>=3] (x, y, z first)")
    dev = device_of(pts, bx)
    odev = pts.device
    bx = bx.to(dev, torch.float32).contiguous()       # the reference's memoryviews are float32 (abstraction.pyx:310)
    pts = pts.to(dev, torch.float32).contiguous()
    return bx, pts, dev, odev, convert


def crop_points(boxes, cloud):
    """bool[M,N]: [i, j] = box i contains point j (Target3DArray.crop_points; a single box: pass one row)."""
    lib = _lib.load()
    bx, pts, dev, odev, convert = _ingress(boxes, cloud)
    m, n = bx.shape[0], pts.shape[0]
    with torch.cuda.device(dev):
        out = torch.empty((m, n), dtype=torch.uint8, device=dev)
        rc = lib.d3d_crop_3dr(_lib.ptr(pts), n, pts.shape[1], _lib.ptr(bx), m, bx.shape[1], 0 if bx.shape[1] == 7 else 2,
                              _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "crop_3dr")
    return _egress(out.view(torch.bool), odev, dev, convert, False)


def paint_label(boxes, cloud, semantics, labels=None):
    """uint16[N]: 1 + index of the first box (the best score of a descendingly sorted array) that contains the point and
    whose class equals the point's semantic label, 0 where there is none (Target3DArray.paint_label).  `labels`: class per
    box; defaults to column 0 of [n,9] rows (tag.labels[0], abstraction.pyx:667)."""
    lib = _lib.load()
    bx, pts, dev, odev, convert = _ingress(boxes, cloud)
    def as_u8(t, what):
        # class ids travel as uint8 (abstraction.pyx:662-682 compares uint8 label arrays): a value outside [0, 255] would
        # wrap silently in the cast -- refuse it
        t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        if t.numel() and t.dtype != torch.uint8:
            lo, hi = float(t.min()), float(t.max())
            if lo < 0 or hi > 255 or (t.is_floating_point() and bool((t != t.round()).any())):
                raise ValueError("%s must be integers in [0, 255]" % what)
        return t.to(dev, torch.uint8).contiguous()
    if labels is None:
        if bx.shape[1] != 9:
            raise ValueError("labels are needed with [M,7] boxes")
        lab = as_u8(bx[:, 0], "labels")
    else:
        lab = as_u8(labels, "labels")
    sem = as_u8(semantics, "semantics")
    m, n = bx.shape[0], pts.shape[0]
    if sem.numel() != n or lab.numel() != m:
        raise ValueError("semantics needs one entry per point, labels one per box")
    with torch.cuda.device(dev):
        idarr = torch.empty((n,), dtype=torch.int16, device=dev)      # uint16 bits (torch has no uint16 arithmetic type)
        rc = lib.d3d_paint_label(_lib.ptr(pts), n, pts.shape[1], _lib.ptr(sem), _lib.ptr(bx), m, bx.shape[1],
                                 0 if bx.shape[1] == 7 else 2, _lib.ptr(lab), _lib.ptr(idarr), _lib.stream_ptr())
    _lib.check(rc, "paint_label")
    if convert or odev != dev:
        out = idarr.cpu().numpy().view(np.uint16)
        return out if convert else torch.from_numpy(out.astype(np.int32))
    return idarr.to(torch.int32) & 0xffff


class CameraMetadata:
    """intrinsic parameters of a camera (abstraction.pyx:733-749)"""
    def __init__(self, width, height, distort_coeffs, intri_matrix, mirror_coeff):
        self.width = int(width)
        self.height = int(height)
        self.distort_coeffs = distort_coeffs
        self.intri_matrix = intri_matrix
        self.mirror_coeff = mirror_coeff


class LidarMetadata:
    pass


class RadarMetadata:
    pass


class PinMetadata:
    """a ground-fixed coordinate (abstraction.pyx:765-775)"""
    def __init__(self, lon, lat):
        self.lon = lon
        self.lat = lat


class _D3DCamera(ctypes.Structure):
    """D3DCamera of include/d3d_hip.h"""
    _fields_ = [("rt", ctypes.c_double * 12), ("P", ctypes.c_double * 9),
                ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("dist", ctypes.c_double * 5),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("has_dist", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_FLU_TO_RDF = np.array([[0., -1., 0.], [0., 0., -1.], [1., 0., 0.]])      # front-left-up axes -> right-down-front


def _c_float(x):
    # the reference declares these arguments as C floats: the value it keeps is the nearest fp32
    return float(np.float32(x))


def _ingress_points(points):
    """-> (points on the device: fp32 or fp64, contiguous [N, >=3]; device; the caller's device; numpy in?)"""
    convert = isinstance(points, np.ndarray)
    if convert and any(st < 0 for st in points.strides):
        points = np.ascontiguousarray(points)
    pts = torch.from_numpy(points) if convert else points      # (not _rows.as_tensor: no tensor is this front's ValueError below)
    if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("points should be [N,>=3] (x, y, z first)")
    odev = pts.device
    dev = device_of(pts)
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.to(torch.float32)
    return pts.to(dev).contiguous(), dev, odev, convert


def _egress(t, odev, dev, convert, sliced):
    """a result on the caller's side; `sliced`: t is the head of an upper-bound buffer, which a copy lets go"""
    if sliced and odev == dev:      # (this front's own: _lib.to_caller copies nothing for a caller on the GPU itself)
        t = t.clone()
    return back_to_caller(_lib.to_caller(t, odev, dev), convert)


class TransformSet:
    """The reference's collection of intrinsic and extrinsic sensor parameters (abstraction.pyx:777-1035) with its method names
    and argument order.  Extrinsics are stored as the 4x4 transform from the base frame to the frame; every frame, camera
    frames included, is front-left-up.  Differences, all on cases where the reference cannot succeed:
      * set_extrinsic between a frame and itself: the reference's check calls np.allclose with one argument and always
        raises; here an identity matrix is accepted (and changes nothing), anything else is a ValueError;
      * a camera with distortion coefficients needs exactly five of them (k1, k2, p1, p2, k3) and an intri_matrix: anything
        else is a ValueError when points are projected (the reference fails on the tuple unpacking);
      * projecting to a frame that has no camera intrinsics is a ValueError.
    transform_objects, dump and load are not here (they need the containers)."""

    def __init__(self, base_frame):
        self.base_frame = base_frame
        self.intrinsics = {}            # frame -> the 3x3 projection matrix (cameras) or None
        self.intrinsics_meta = {}       # frame -> sensor metadata
        self.extrinsics = {}            # frame -> 4x4 transform from the base frame

    # ------------------------------------------------------------ frames
    def _is_base(self, frame):
        return frame is None or frame == self.base_frame

    def _is_same(self, frame1, frame2):
        return frame1 == frame2 or (self._is_base(frame1) and self._is_base(frame2))

    def _assert_exist(self, frame_id, extrinsic=False):
        if self._is_base(frame_id):
            return
        if frame_id not in self.intrinsics:
            raise ValueError("Frame {0} has no intrinsic parameters: add intrinsics for {0} first".format(frame_id))
        if extrinsic and frame_id not in self.extrinsics:
            raise ValueError("Frame {0} has no extrinsic parameters: add an extrinsic for {0} first".format(frame_id))

    @property
    def frames(self):
        """the registered frame names (without the base frame)"""
        return list(self.intrinsics.keys())

    def __repr__(self):
        return "<TransformSet with frames: *%s>" % ", ".join([self.base_frame] + self.frames)

    # ------------------------------------------------------------ intrinsics
    def set_intrinsic_general(self, frame_id, metadata=None):
        """marks that a frame exists"""
        self.intrinsics[frame_id] = None
        self.intrinsics_meta[frame_id] = metadata

    def set_intrinsic_camera(self, frame_id, transform, size, rotate=True, distort_coeffs=[], intri_matrix=None,
                             mirror_coeff=float("nan")):
        """transform: the 3x3 projection matrix; size: (width, height); rotate: append the axis rotation from front-left-up to
        right-down-front; distort_coeffs: (k1, k2, p1, p2, k3) of the OpenCV model or empty; intri_matrix: the matrix of the
        general camera model the distortion works in; mirror_coeff: stored, unused (as in the reference)"""
        width, height = size
        transform = np.asarray(transform, dtype=np.float64)
        if rotate:
            transform = transform.dot(_FLU_TO_RDF)
        self.intrinsics[frame_id] = transform
        self.intrinsics_meta[frame_id] = CameraMetadata(
            width, height, np.asarray(distort_coeffs),
            None if intri_matrix is None else np.asarray(intri_matrix, dtype=np.float64), _c_float(mirror_coeff))

    def set_intrinsic_lidar(self, frame_id):
        self.intrinsics[frame_id] = None
        self.intrinsics_meta[frame_id] = LidarMetadata()

    def set_intrinsic_radar(self, frame_id):
        self.intrinsics[frame_id] = None
        self.intrinsics_meta[frame_id] = RadarMetadata()

    def set_intrinsic_pinhole(self, frame_id, size, cx, cy, fx, fy, s=0, distort_coeffs=[]):
        """pinhole parameters (s: skew); each is kept as the nearest fp32, as the reference's C float arguments are"""
        cx, cy, fx, fy, s = (_c_float(v) for v in (cx, cy, fx, fy, s))
        P = np.array([[fx, s, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
        self.set_intrinsic_camera(frame_id, P, size, rotate=True, distort_coeffs=distort_coeffs, intri_matrix=P)

    def set_intrinsic_map_pin(self, frame_id, lon=float("nan"), lat=float("nan")):
        self.intrinsics[frame_id] = None
        self.intrinsics_meta[frame_id] = PinMetadata(_c_float(lon), _c_float(lat))

    # ------------------------------------------------------------ extrinsics
    def set_extrinsic(self, transform, frame_to=None, frame_from=None):
        """transform takes a point from `frame_from` to `frame_to` (None: the base frame), 3x4 or 4x4.  One of the two frames
        must be the base frame or already have an extrinsic; the other one gets its extrinsic from the chain.  Between a frame
        and itself only an identity is accepted (the reference's check there cannot pass; see the class docstring)."""
        transform = np.asarray(transform, dtype=np.float64)
        if transform.shape == (3, 4):
            transform = np.vstack([transform, [0., 0., 0., 1.]])
        elif transform.shape != (4, 4):
            raise ValueError("an extrinsic is a 3x4 or 4x4 matrix")
        if self._is_same(frame_to, frame_from):
            if not np.array_equal(transform, np.eye(4)):
                raise ValueError("the transform between a frame and itself is the identity")
            return

        if self._is_base(frame_to):
            self._assert_exist(frame_from)
            self.extrinsics[frame_from] = np.linalg.inv(transform)
            return
        self._assert_exist(frame_to)
        if self._is_base(frame_from):
            self.extrinsics[frame_to] = transform
            return
        self._assert_exist(frame_from)

        known_from, known_to = frame_from in self.extrinsics, frame_to in self.extrinsics
        if known_from and known_to:
            raise ValueError("Frames %s and %s both have an extrinsic already: update one of them at a time" % (frame_to, frame_from))
        if known_from:
            self.extrinsics[frame_to] = np.dot(transform, self.extrinsics[frame_from])
        elif known_to:
            self.extrinsics[frame_from] = np.dot(np.linalg.inv(transform), self.extrinsics[frame_to])
        else:
            raise ValueError("Neither %s nor %s has an extrinsic: add one of them first" % (frame_to, frame_from))

    def get_extrinsic(self, frame_to=None, frame_from=None):
        """the 4x4 transform from `frame_from` to `frame_to` (None: the base frame)"""
        if self._is_same(frame_to, frame_from):
            return np.eye(4)
        if self._is_base(frame_from):
            self._assert_exist(frame_to, extrinsic=True)
            return self.extrinsics[frame_to]
        self._assert_exist(frame_from, extrinsic=True)
        back = np.linalg.inv(self.extrinsics[frame_from])
        if self._is_base(frame_to):
            return back
        self._assert_exist(frame_to, extrinsic=True)
        return np.dot(self.extrinsics[frame_to], back)

    # ------------------------------------------------------------ points
    def transform_points(self, points, frame_to, frame_from=None):
        """the cloud [N,>=3] in `frame_to`: fp64 [N, cols], columns 0..2 = R . p + t, the others as they are
        (abstraction.pyx:971-977).  numpy in -> numpy out; torch in -> torch out on the same device."""
        rt = np.ascontiguousarray(np.asarray(self.get_extrinsic(frame_to, frame_from), dtype=np.float64)[:3, :4])
        pts, dev, odev, convert = _ingress_points(points)
        lib = _lib.load()
        n, cols = pts.shape
        with torch.cuda.device(dev):
            out = torch.empty((n, cols), dtype=torch.float64, device=dev)
            rc = lib.d3d_transform_points(_lib.ptr(pts), n, cols, _lib.F32 if pts.dtype == torch.float32 else _lib.F64,
                                          rt.ctypes.data_as(ctypes.c_void_p), _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "transform_points")
        return _egress(out, odev, dev, convert, False)

    def _camera_record(self, rec, frame_to, frame_from):
        """fills one D3DCamera; every check of the call that needs no device"""
        self._assert_exist(frame_to)
        P = None if self._is_base(frame_to) else self.intrinsics[frame_to]
        meta = self.intrinsics_meta.get(frame_to)
        if P is None or not isinstance(meta, CameraMetadata):
            raise ValueError("Frame %s has no camera intrinsics" % frame_to)
        if P.ndim != 2 or P.shape[0] < 3 or P.shape[1] != 3:
            raise ValueError("the projection matrix of frame %s is not 3x3" % frame_to)
        rt = np.asarray(self.get_extrinsic(frame_to=frame_to, frame_from=frame_from), dtype=np.float64)
        rec.rt[:] = rt[:3, :4].reshape(-1).tolist()
        rec.P[:] = P[:3].reshape(-1).tolist()
        rec.width, rec.height = meta.width, meta.height
        distorts = np.asarray(meta.distort_coeffs if meta.distort_coeffs is not None else [], dtype=np.float64).reshape(-1)
        rec.has_dist = 1 if distorts.size > 0 else 0
        if rec.has_dist:
            im = meta.intri_matrix
            if distorts.size != 5 or im is None or im.ndim != 2 or im.shape[0] < 2 or im.shape[1] < 3:
                raise ValueError("distortion needs five coefficients (k1, k2, p1, p2, k3) and an intri_matrix (frame %s)" % frame_to)
            rec.fx, rec.fy, rec.cx, rec.cy = float(im[0, 0]), float(im[1, 1]), float(im[0, 2]), float(im[1, 2])
            rec.dist[:] = distorts.tolist()

    def project_points_to_cameras(self, points, frames_to, frame_from=None, remove_outlier=True, return_dmask=False):
        """project_points_to_camera for every frame of `frames_to` in one pass over the cloud and one wait for the result sizes:
        a list of the per-camera tuples, each identical to the single call's."""
        frames_to = list(frames_to)
        if not frames_to:
            raise ValueError("frames_to is empty")
        self._assert_exist(frame_from)
        ncam = len(frames_to)
        recs = (_D3DCamera * ncam)()
        for k, frame in enumerate(frames_to):
            self._camera_record(recs[k], frame, frame_from)
        pts, dev, odev, convert = _ingress_points(points)
        lib = _lib.load()
        n, cols = pts.shape
        flags = (0 if remove_outlier else _lib.PROJECT_ALL_UV) | (_lib.PROJECT_DMASK if return_dmask else 0)
        with torch.cuda.device(dev):
            uv = torch.empty((ncam, n, 2), dtype=torch.float64, device=dev)
            mask = torch.empty((ncam, n), dtype=torch.int64, device=dev)
            dmask = torch.empty((ncam, n), dtype=torch.int64, device=dev) if return_dmask else None
            counts = torch.empty((ncam, 2), dtype=torch.int64, device=dev)
            nbytes = lib.d3d_project_points_workspace_bytes(n, ncam)
            ws = _lib.workspace(nbytes, dev)
            rc = lib.d3d_project_points(_lib.ptr(pts), n, cols, _lib.F32 if pts.dtype == torch.float32 else _lib.F64,
                                        ctypes.cast(recs, ctypes.c_void_p), ncam, flags, _lib.ptr(uv), _lib.ptr(mask),
                                        _lib.ptr(dmask), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "project_points")
            sizes = counts.cpu().tolist()                 # the call's one synchronisation
            out = []
            for c, (k, kd) in enumerate(sizes):
                res = (_egress(uv[c, :k], odev, dev, convert, True) if remove_outlier else _egress(uv[c], odev, dev, convert, ncam > 1),
                       _egress(mask[c, :k], odev, dev, convert, True))
                if return_dmask:
                    res += (_egress(dmask[c, :kd], odev, dev, convert, True),)
                out.append(res)
        return out

    def project_points_to_camera(self, points, frame_to, frame_from=None, remove_outlier=True, return_dmask=False):
        """(uv, mask) or (uv, mask, dmask) of abstraction.pyx:979-1035.  uv: fp64 [K,2] image coordinates of the points in view,
        in point order, or with remove_outlier=False fp64 [N,2] for every point; mask: int64 [K], the ascending indices of the
        points in view; dmask: int64 [Kd], those of the points in front of the camera (d > 0).  points [N,>=3]: fp32 or fp64
        are read in place when contiguous on the device, other dtypes are converted to fp32.  numpy in -> numpy out; torch in
        -> torch out on the same device."""
        return self.project_points_to_cameras(points, [frame_to], frame_from, remove_outlier, return_dmask)[0]


__all__ = ["crop_points", "paint_label", "TransformSet"]
