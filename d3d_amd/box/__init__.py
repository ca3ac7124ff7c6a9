"""d3d_amd.box -- drop-in for d3d.box on MI355X.

Mirrors reference d3d/box/__init__.py: `box2d_iou` (:180, methods box / rbox / grbox / drbox), `box2d_nms` (:226),
`box2dr_crop` / `box3dp_crop` (:278-315), `box2dr_pdist` / `box3dr_pdist` (:333-381), the autograd functions `Iou2D`,
`Iou2DR`, `GIou2DR`, `DIou2DR`, `PDist2DR` (:41-150) and the enums `IouType`, `SupressionType` (box/common.h:5-10).
The compiled module's own names (box/impl.cpp:8-54) live in `d3d_amd.box.box_impl`.  north_star's names `iou2d`, `iou3d`,
`nms` are thin aliases (the reference reaches "iou3d" only through Cython: d3d/dgal_wrap.h:45-91,
d3d/tracking/matcher.pyx:57-80).  All compute runs in HIP kernels behind include/d3d_hip.h.
"""
import ctypes
import enum

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib, options
from .._rows import device_of, group_ids


class IouType(enum.IntEnum):            # box/common.h:5-9
    NA = 0
    BOX = 1
    RBOX = 2
    GBOX = 3
    GRBOX = 4
    DBOX = 5
    DRBOX = 6


class SupressionType(enum.IntEnum):     # box/common.h:10  (sic: the reference spells it this way)
    HARD = 0
    LINEAR = 1
    GAUSSIAN = 2


cuda_available = True   # box/impl.cpp:9-13: this build always has its device path

# (per-call options -- flags=, poison= -- or the calling context's: d3d_amd.options)


def _dtype_code(t, wide32=False):
    """the library's code of t's dtype; wide32 (`_wide32`): D3D_F32_WIDE for the fp32 tensors it stands for"""
    if t.dtype == torch.float64:
        return _lib.F64
    if t.dtype == torch.float32:
        return _lib.F32_WIDE if wide32 else _lib.F32
    raise RuntimeError("boxes must be float32 or float64")   # AT_DISPATCH_FLOATING_TYPES (iou.cpp:132)


class _Staged:
    """The frame of every call into the library: `with _Staged(x, y) as call:` has the inputs contiguous on one GPU in `call.inputs`
    -- `call.dev`: that of the first CUDA tensor among them, else the current GPU -- and that GPU current inside the block;
    `call.back(results)` brings a tensor, tuple or dict of results to the device the first input came from (`_lib.to_caller`)."""
    __slots__ = ("odev", "dev", "inputs", "_previous")

    def __init__(self, *ts):
        self.odev = ts[0].device
        self.dev = dev = device_of(*ts)
        self.inputs = [t.to(dev).contiguous() for t in ts]

    def __enter__(self):        # (the two calls `with torch.cuda.device(dev)` makes, without building that object per call)
        self._previous = torch.cuda._exchange_device(self.dev.index)
        return self

    def __exit__(self, *exc):
        torch.cuda._maybe_exchange_device(self._previous)
        return False

    def back(self, results):
        return _lib.to_caller(results, self.odev, self.dev)


_NX2 = "Input of rbox_2d_iou should be Nx2 tensors!"       # (sic: reference box/__init__.py:206-207)
_FIELDS = {5: "Input boxes should have 5 fields: x, y, w, h, r", 7: "Input boxes should have 7 fields: x, y, z, lx, ly, lz, rz"}


def _check_fields(cols, *boxes, flat=None):
    """every tensor of `boxes` is [*, cols]: ValueError with the reference's message for that width (box/__init__.py:208-209).  A
    tensor that is not 2-D answers with `flat` first where the front has such a message of its own, else with the width's."""
    for b in boxes:
        if len(b.shape) != 2:
            raise ValueError(flat or _FIELDS[cols])
    for b in boxes:
        if b.shape[1] != cols:
            raise ValueError(_FIELDS[cols])


def _wide32(precise, a, b):
    """precise on two fp32 tensors: they go in as they are and the kernels widen them where they load them -- fp64 arithmetic
    without .double() copies; `_dtype_code(a, True)` is the code for it (D3D_F32_WIDE)"""
    return precise and a.dtype == torch.float32 and b.dtype == torch.float32


def _promote(precise, a, b):
    """The `precise` rule of box2d_iou (reference box/__init__.py:204-205, 224) for the two tensors of a front -> (a, b, wide32):
    fp32 pairs as they are (`_wide32`), anything else as .double() copies; the result is cast back to the dtype that came in."""
    wide32 = _wide32(precise, a, b)
    if precise and not wide32:
        a, b = a.double(), b.double()
    return a, b, wide32


def _mixed_code(boxes, iou_type, matrix32, wide32):
    """the dtype code d3d_iou2d_forward / _backward take: the boxes' own, or a mixed form for the box / rbox methods"""
    code = _dtype_code(boxes)
    if matrix32 or wide32:
        if code != (_lib.F32 if wide32 else _lib.F64) or int(iou_type) not in (IouType.BOX, IouType.RBOX):
            raise ValueError("matrix32 takes fp64 boxes, wide32 fp32 boxes, both the box / rbox methods")
        code = _lib.F32_WIDE if wide32 else _lib.F64_M32
    return code


_MAX_ROWS = 65535 * 64      # rows of boxes1 per d3d_iou2d_forward launch (grid.y limit x 64-row tiles)


def _iou_forward(boxes1, boxes2, iou_type, flags=None, matrix32=False, wide32=False):
    """matrix32 (fp64 boxes, BOX / RBOX): the arithmetic in fp64, `ious` stored as fp32 (D3D_F64_M32);
    wide32 (fp32 boxes, BOX / RBOX): the same with the boxes widened where the kernels load them (D3D_F32_WIDE)"""
    lib = _lib.load()
    if boxes1.dtype != boxes2.dtype:
        raise RuntimeError("boxes1 and boxes2 must have the same dtype")
    fl = options.current().iou_flags if flags is None else int(flags)
    with _Staged(boxes1, boxes2) as call:
        (b1, b2), dev = call.inputs, call.dev
        n, m = b1.shape[0], b2.shape[0]
        ious = torch.empty((n, m), dtype=torch.float32 if matrix32 else b1.dtype, device=dev)
        if options.current().poison:
            ious.fill_(float("nan"))
        code = _mixed_code(b1, iou_type, matrix32, wide32)
        # one launch covers 65535 tiles of 64 rows; taller inputs go in row blocks into the same output
        for r0 in range(0, max(n, 1), _MAX_ROWS):
            r1 = min(n, r0 + _MAX_ROWS)
            ws = _lib.workspace(lib.d3d_iou2d_workspace_bytes(r1 - r0, m, code), dev)
            rc = lib.d3d_iou2d_forward(_lib.ptr(b1[r0:r1]), r1 - r0, _lib.ptr(b2), m, int(iou_type), code, _lib.ptr(ious[r0:r1]),
                                       _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr(), fl)
            _lib.check(rc, "iou2d_forward")
    return call.back(ious)


def iou2d_forward(boxes1, boxes2):
    """iou2d_forward / iou2d_forward_cuda (iou.h:7-13; iou.cpp:35-46): AABB-of-rotated-box IoU [N,M]."""
    return _iou_forward(boxes1, boxes2, IouType.BOX)


def iou2dr_forward(boxes1, boxes2):
    """`ious` of iou2dr_forward / iou2dr_forward_cuda (iou.h:25-31; iou.cpp:125-141).  The reference's 3-tuple form
    (ious, nx, xflags) is `d3d_amd.box.box_impl.iou2dr_forward`; the flags alone: `iou2dr_flags`."""
    return _iou_forward(boxes1, boxes2, IouType.RBOX)


def giou2dr_forward(boxes1, boxes2):
    """`ious` of giou2dr_forward[_cuda] (iou.h:41-47; iou.cpp:243-258): GIoU = IoU - (hull - union) / hull"""
    return _iou_forward(boxes1, boxes2, IouType.GRBOX)


def diou2dr_forward(boxes1, boxes2):
    """`ious` of diou2dr_forward[_cuda] (iou.h:56-62; iou.cpp:352-367): DIoU = IoU - centre distance^2 / hull diameter^2"""
    return _iou_forward(boxes1, boxes2, IouType.DRBOX)


def iou2dr_flags(boxes1, boxes2, which=("nx", "xflags")):
    """the autograd bookkeeping of the rotated IoU family (include/d3d_hip.h: d3d_iou2dr_flags) -> dict of uint8 tensors:
    nx[N,M], xflags[N,M,8] (iou.cpp:125-141), nm[N,M], mflags[N,M,8] (giou, iou.cpp:243-258), far[N,M,2] (diou, :352-367)"""
    lib = _lib.load()
    if boxes1.dtype != boxes2.dtype:
        raise RuntimeError("boxes1 and boxes2 must have the same dtype")
    with _Staged(boxes1.detach(), boxes2.detach()) as call:
        b1, b2 = call.inputs
        n, m = b1.shape[0], b2.shape[0]
        shapes = dict(nx=(n, m), xflags=(n, m, 8), nm=(n, m), mflags=(n, m, 8), far=(n, m, 2))
        out = {k: torch.empty(shapes[k], dtype=torch.uint8, device=call.dev) for k in which}
        rc = lib.d3d_iou2dr_flags(_lib.ptr(b1), n, _lib.ptr(b2), m, _dtype_code(b1), _lib.ptr(out.get("nx")),
                                  _lib.ptr(out.get("xflags")), _lib.ptr(out.get("nm")), _lib.ptr(out.get("mflags")),
                                  _lib.ptr(out.get("far")), _lib.stream_ptr())
    _lib.check(rc, "iou2dr_flags")
    return call.back(out)


def _iou_backward(boxes1, boxes2, grad, iou_type, matrix32=False, wide32=False):
    """matrix32 (fp64 boxes, BOX / RBOX): `grad` is read as fp32 and widened in the kernels (D3D_F64_M32);
    wide32 (fp32 boxes, BOX / RBOX): the boxes too (D3D_F32_WIDE) -- the sums are kept in fp64 and come back rounded to fp32"""
    lib = _lib.load()
    with _Staged(boxes1.detach(), boxes2.detach(), grad.to(torch.float32 if matrix32 or wide32 else boxes1.dtype)) as call:
        (b1, b2, g), dev = call.inputs, call.dev
        n, m = b1.shape[0], b2.shape[0]
        code = _mixed_code(b1, iou_type, matrix32, wide32)
        # both results in ONE buffer: the library then clears them with one launch, and the wide form rounds them with one
        gg = torch.empty((n + m, 5), dtype=torch.float64 if wide32 else b1.dtype, device=dev)
        ws = _lib.workspace(lib.d3d_iou2d_workspace_bytes(n, m, code), dev)
        rc = lib.d3d_iou2d_backward(_lib.ptr(b1), n, _lib.ptr(b2), m, _lib.ptr(g), int(iou_type), code, _lib.ptr(gg[:n]),
                                    _lib.ptr(gg[n:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "iou2d_backward")
        if wide32:
            gg = gg.to(torch.float32)
    return call.back((gg[:n], gg[n:]))


def iou2d_backward(boxes1, boxes2, grad):
    """iou2d_backward[_cuda] (iou.h:14-24; iou.cpp:75-93): (grad_boxes1[N,5], grad_boxes2[M,5])"""
    return _iou_backward(boxes1, boxes2, grad, IouType.BOX)


def iou2dr_backward(boxes1, boxes2, grad, nx=None, xflags=None):
    """iou2dr_backward[_cuda] (iou.h:32-40; iou.cpp:191-211).  `nx` / `xflags` (the reference's saved clip flags)
    are accepted for signature compatibility and ignored: the clip is recomputed."""
    return _iou_backward(boxes1, boxes2, grad, IouType.RBOX)


def giou2dr_backward(boxes1, boxes2, grad, nxm=None, xmflags=None):
    """giou2dr_backward[_cuda] (iou.h:48-55; iou.cpp:303-320); the saved flags are ignored (analytic gradients)"""
    return _iou_backward(boxes1, boxes2, grad, IouType.GRBOX)


def diou2dr_backward(boxes1, boxes2, grad, nxd=None, xflags=None):
    """diou2dr_backward[_cuda] (iou.h:63-69; iou.cpp:402-419); the saved flags are ignored (analytic gradients)"""
    return _iou_backward(boxes1, boxes2, grad, IouType.DRBOX)


def _iou_function(iou_type):
    """the autograd function of one method of the IoU family: forward saves the boxes, backward recomputes from them"""
    class IouFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, boxes1, boxes2):
            ctx.save_for_backward(boxes1, boxes2)
            return _iou_forward(boxes1, boxes2, iou_type)

        @staticmethod
        def backward(ctx, grad):
            boxes1, boxes2 = ctx.saved_tensors
            return _iou_backward(boxes1, boxes2, grad.contiguous(), iou_type)

    return IouFunction


class Iou2D(_iou_function(IouType.BOX)):
    """Differentiable axis aligned IoU function for 2D boxes -- reference box/__init__.py:41-61"""


class Iou2DR(_iou_function(IouType.RBOX)):
    """Differentiable rotated IoU function for 2D boxes -- reference box/__init__.py:63-84"""


class GIou2DR(_iou_function(IouType.GRBOX)):
    """Differentiable rotated GIoU function for 2D boxes -- reference box/__init__.py:86-107"""


class DIou2DR(_iou_function(IouType.DRBOX)):
    """Differentiable rotated DIoU function for 2D boxes -- reference box/__init__.py:109-130"""


class _IouPrecise32(torch.autograd.Function):
    """box2d_iou(precise=True) on fp32 boxes, 'box' / 'rbox': the reference widens the boxes, computes in fp64 and casts the matrix
    back (box/__init__.py:204-205, 224).  Same numbers -- fp64 arithmetic on the widened boxes, every value rounded once -- with
    the widening where the boxes are loaded, the rounding where the matrix is stored, and in backward the widening where the
    incoming gradient is read: no fp64 copy of an [N,M] matrix in either direction, no cast launches in front of the forward."""

    @staticmethod
    def forward(ctx, boxes1, boxes2, iou_type):
        ctx.save_for_backward(boxes1, boxes2)
        ctx.iou_type = iou_type
        return _iou_forward(boxes1, boxes2, iou_type, wide32=True)

    @staticmethod
    def backward(ctx, grad):
        boxes1, boxes2 = ctx.saved_tensors
        g1, g2 = _iou_backward(boxes1, boxes2, grad.contiguous(), ctx.iou_type, wide32=True)
        return g1, g2, None


_IOU_FUNCTIONS = {IouType.BOX: Iou2D, IouType.RBOX: Iou2DR, IouType.GRBOX: GIou2DR, IouType.DRBOX: DIou2DR}


def _ingress(first, *rest):
    """numpy arrays in, numpy arrays out: -> (tensors, was_numpy).  A mix of the two is refused with the reference's message
    (box/__init__.py:191-192, 237-238)."""
    if not isinstance(first, np.ndarray):
        return (first,) + rest, False
    assert all(isinstance(a, np.ndarray) for a in rest), "Input should be both numpy tensor or pytorch tensor!"
    return tuple(torch.from_numpy(a) for a in (first,) + rest), True


def _egress(t, was_numpy):
    return t.numpy() if was_numpy else t


def box2d_iou(boxes1, boxes2, method="box", precise=True):
    """Differentiable IoU on axis-aligned ('box') or rotated ('rbox') 2D boxes, and the loss variants 'grbox' / 'drbox' --
    signature, validation order, messages and dtype handling of reference box/__init__.py:180-224.

    :param boxes1: N x 5 (x,y,w,h,r), torch tensor or numpy array
    :param boxes2: M x 5
    :param precise: compute in float64 and cast back to the input dtype
    """
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    # fp32 boxes, precise: the fp64 arithmetic with an fp32 matrix (_IouPrecise32) instead of .double() ... .to(float32) around it
    dtype_in = boxes1.dtype
    boxes1, boxes2, fused32 = _promote(precise, boxes1, boxes2)
    _check_fields(5, boxes1, boxes2, flat=_NX2)
    iou_type = getattr(IouType, method.upper())                   # AttributeError for unknown names, like the reference
    fn = _IOU_FUNCTIONS.get(iou_type)
    if fn is None:
        raise ValueError("Unrecognized iou type!")
    if fused32 and iou_type in (IouType.BOX, IouType.RBOX):
        return _egress(_IouPrecise32.apply(boxes1, boxes2, iou_type), was_numpy)
    if fused32:
        boxes1, boxes2 = boxes1.double(), boxes2.double()
    ious = fn.apply(boxes1, boxes2)
    return _egress(ious.to(dtype_in) if precise else ious, was_numpy)


def argsort_desc(scores):
    """stable descending argsort on the device (nms.cpp:103 uses torch's unstable argsort)."""
    lib = _lib.load()
    n = scores.numel()
    code = _dtype_code(scores)
    with _Staged(scores) as call:
        order = torch.empty((n,), dtype=torch.int64, device=call.dev)
        ws = _lib.workspace(lib.d3d_argsort_desc_workspace_bytes(n, code), call.dev)
        rc = lib.d3d_argsort_desc(_lib.ptr(call.inputs[0]), n, code, _lib.ptr(order), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr())
    _lib.check(rc, "argsort_desc")
    return call.back(order)


NMS_STATUS_DENSE_PATH, NMS_STATUS_SCAN_GAVE_UP = 1, 2


def nms2d(boxes, scores, iou_type, supression_type, iou_threshold, score_threshold, supression_param, sort_keys=None,
          flags=None, return_status=False, keep_mask=False, wide32=False):
    """nms2d / nms2d_cuda (nms.h:6-18; nms.cpp:98-119): returns the SUPPRESSED mask (bool[N]).
    Follows the CPU control flow of the reference (nms.cpp:23-59).  sort_keys: optional fp32 tensor that orders like
    `scores` (the scores before their promotion to fp64): half the radix passes of the argsort, same order.
    return_status: (mask, status) with d3d_nms2d_status's bits -- which route decided the mask (waits for the stream).
    keep_mask: the kernels write the KEEP mask instead (D3D_NMS_KEEP_MASK): box2d_nms's `~suppressed` without the extra pass.
    wide32 (fp32 boxes and scores): the arithmetic in fp64, the values widened where the kernels load them (D3D_F32_WIDE): what
    box2d_nms(precise=True) computes for fp32 tensors, without the .double() copies."""
    lib = _lib.load()
    iou_type, supression_type = int(iou_type), int(supression_type)
    if iou_type not in (IouType.BOX, IouType.RBOX):
        raise ValueError("Unsupported iou type!")                   # common.h:25
    if supression_type not in (0, 1, 2):
        raise ValueError("Unsupported supression type!")            # common.h:40
    if boxes.dtype != scores.dtype:
        raise RuntimeError("boxes and scores must have the same dtype")
    with _Staged(boxes, scores) as call:
        (b, s), dev = call.inputs, call.dev
        n = b.shape[0]
        code = _dtype_code(b, wide32)
        if wide32 and code != _lib.F32_WIDE:
            raise ValueError("wide32 takes fp32 boxes and scores")
        # order = None: the library sorts the scores itself (inside the first kernel for up to 4096 boxes)
        order = None
        if sort_keys is not None and sort_keys.dtype == torch.float32 and sort_keys.numel() == n and s.dtype != torch.float32 and n > 4096:
            order = argsort_desc(sort_keys.to(dev).contiguous())
        sup = torch.empty((n,), dtype=torch.uint8, device=dev)
        # both workspaces are carved from one arena; the sort finished with it (same stream)
        ws = _lib.workspace(lib.d3d_nms2d_workspace_bytes(n), dev)
        # (the per-thread host word: the call decides from ITS OWN grid whether the level kernels are worth launching)
        rc = lib.d3d_nms2d_notify(_lib.ptr(b), _lib.ptr(s), _lib.ptr(order) if order is not None else None, n, iou_type, supression_type,
                                  code, float(iou_threshold), float(score_threshold), float(supression_param), _lib.ptr(sup),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
                                  (options.current().nms_flags if flags is None else int(flags)) | (_lib.NMS_KEEP_MASK if keep_mask else 0),
                                  _lib.HostWord.get().ptr)
        _lib.check(rc, "nms2d")
        status = ctypes.c_uint32(0)
        if return_status and n > 0:
            _lib.check(lib.d3d_nms2d_status(_lib.ptr(ws), supression_type, _lib.stream_ptr(), ctypes.byref(status)), "nms2d_status")
    sup = call.back(sup.view(torch.bool))
    return (sup, int(status.value)) if return_status else sup


nms2d_cuda = nms2d


def box2d_nms(boxes, scores, iou_method="box", supression_method="hard",
              iou_threshold=0, score_threshold=0, supression_param=0, precise=True):
    """NMS on axis-aligned or rotated 2D boxes; returns the KEEP mask -- signature, validation order and messages of reference
    box/__init__.py:226-276 (fp64 promotion of boxes AND scores, class-max of [N,K] scores, the empty case's CPU tensor)."""
    (boxes, scores), was_numpy = _ingress(boxes, scores)
    # (the order of fp32 scores survives the promotion -- fp32 -> fp64 is monotone and injective -- so the sort may use the narrow keys)
    keys = scores if scores.dtype == torch.float32 else None
    # fp32 boxes AND scores, precise: fp64 arithmetic on values widened inside the kernels (D3D_F32_WIDE) instead of .double() copies
    boxes, scores, wide32 = _promote(precise, boxes, scores)
    if len(boxes) != len(scores):
        raise ValueError("Numbers of boxes and scores are inconsistent!")
    if scores.dim() == 2:
        scores = scores.max(axis=1).values
        keys = None if keys is None else keys.max(axis=1).values
    if boxes.numel() == 0:
        return torch.tensor([], dtype=torch.bool)
    # (the reference returns ~suppressed, box/__init__.py:272: here the kernels that decide the mask write it inverted)
    keep = nms2d(boxes, scores, getattr(IouType, iou_method.upper()), getattr(SupressionType, supression_method.upper()),
                 iou_threshold, score_threshold, supression_param, sort_keys=None if wide32 else keys, keep_mask=True, wide32=wide32)
    return _egress(keep, was_numpy)


_group_ids = group_ids               # (shared with circle_nms: d3d_amd._rows)


def box2d_nms_batched(boxes, scores, groups, iou_method="box", supression_method="hard",
                      iou_threshold=0, score_threshold=0, supression_param=0, precise=True):
    """Hard NMS inside every group of a batch -- the (sample, class) groups of a detector's output -- and never across groups;
    returns the KEEP mask bool[N].  The reference has no counterpart (its nms2d is one loop over one set).

    boxes [N,5], scores [N] or [N,K] and the keywords are box2d_nms's (torch or numpy, CPU or GPU, any strides; the same fp64
    promotion for `precise`, class-max of 2-D scores, messages, empty result and egress).  groups [N]: any integer dtype, any
    values (negative, above 2^31, unsorted, with gaps); rows with equal values form a group.  For every group value g, with
    idx = (groups == g).nonzero() in ascending row order,

        keep[idx] == box2d_nms(boxes[idx], scores[idx], <same keywords>)      bit for bit

    -- ties in score keep ascending row order, and the score-threshold tail never suppresses the top-ranked box of its own
    group.  One workgroup per group in one launch (d3d_nms2d_grouped); a group above d3d_nms2d_group_max() boxes (1024) goes
    through nms2d on its own.  Only supression_method="hard": soft-NMS is sequential per set and stays with box2d_nms.
    """
    (boxes, scores), was_numpy = _ingress(boxes, scores)
    boxes, scores, wide32 = _promote(precise, boxes, scores)
    if len(boxes) != len(scores):
        raise ValueError("Numbers of boxes and scores are inconsistent!")
    groups = _group_ids(groups)
    if groups.dim() != 1 or len(groups) != len(boxes):
        raise ValueError("Numbers of boxes and groups are inconsistent!")
    if scores.dim() == 2:
        scores = scores.max(axis=1).values
    if boxes.numel() == 0:
        return torch.tensor([], dtype=torch.bool)
    iou_type = getattr(IouType, iou_method.upper())
    if getattr(SupressionType, supression_method.upper()) != SupressionType.HARD:
        raise ValueError("box2d_nms_batched does hard NMS only: soft-NMS is sequential per set, use box2d_nms on each group")
    if iou_type not in (IouType.BOX, IouType.RBOX):
        raise ValueError("Unsupported iou type!")                   # common.h:25
    if boxes.dtype != scores.dtype:
        raise RuntimeError("boxes and scores must have the same dtype")
    code = _dtype_code(boxes, wide32)
    # everything above is host-side: nothing has touched the library or a device
    lib = _lib.load()
    with _Staged(boxes, scores) as call:
        (b, s), dev = call.inputs, call.dev
        n = b.shape[0]
        # stable: the rows of a segment stay in ascending row order, the order ties in score keep
        ids, perm = torch.sort(groups.to(dev), stable=True)
        counts = torch.unique_consecutive(ids, return_counts=True)[1]
        ngroups = counts.numel()
        seg = torch.zeros((ngroups + 1,), dtype=torch.int64, device=dev)
        seg[1:] = counts.cumsum(0)
        largest = int(counts.max())                                  # (the one host read besides the number of groups)
        cap = int(lib.d3d_nms2d_group_max())
        keep = torch.empty((n,), dtype=torch.uint8, device=dev)
        if largest > cap:
            # the grouped entry skips these segments (their keep bytes stay untouched): each is one set for nms2d
            sizes, starts = counts.tolist(), seg.tolist()
            for g, size in enumerate(sizes):
                if size > cap:
                    idx = perm[starts[g]:starts[g + 1]]
                    keep[idx] = nms2d(b[idx], s[idx], iou_type, SupressionType.HARD, iou_threshold, score_threshold,
                                      supression_param, keep_mask=True, wide32=wide32).view(torch.uint8)
            largest = max([size for size in sizes if size <= cap], default=0)
        ws = _lib.workspace(lib.d3d_nms2d_grouped_workspace_bytes(n, ngroups), dev)
        rc = lib.d3d_nms2d_grouped(_lib.ptr(b), _lib.ptr(s), _lib.ptr(perm), _lib.ptr(seg), n, ngroups, largest, int(iou_type), code,
                                   float(iou_threshold), float(score_threshold), _lib.ptr(keep), _lib.ptr(ws), ws.numel(),
                                   _lib.stream_ptr(), _lib.NMS_KEEP_MASK)
        _lib.check(rc, "nms2d_grouped")
    return _egress(call.back(keep.view(torch.bool)), was_numpy)


def iou3d(boxes1, boxes2, method="rbox"):
    """Pairwise "3D IoU" of [N,7] x [M,7] boxes (x,y,z,lx,ly,lz,rz) -> f32[N,M]: BEV IoU (rotated for
    'rbox' = box3dr_iou, AABB for 'box' = box3d_iou) times the 1-D z-interval IoU, all in fp32
    (reference d3d/dgal_wrap.h:45-91; the pair loop of BaseMatcher.prepare_boxes,
    d3d/tracking/matcher.pyx:57-80, stores 1 - this value)."""
    lib = _lib.load()
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    key = method.upper()
    if key not in ("RBOX", "BOX"):
        raise ValueError("Unrecognized iou type!")
    _check_fields(7, boxes1, boxes2)
    with _Staged(boxes1.to(torch.float32), boxes2.to(torch.float32)) as call:
        (b1, b2), dev = call.inputs, call.dev
        n, m = b1.shape[0], b2.shape[0]
        out = torch.empty((n, m), dtype=torch.float32, device=dev)
        if options.current().poison:
            out.fill_(float("nan"))
        ws = _lib.workspace(lib.d3d_iou3d_workspace_bytes(n, m), dev)
        rc = lib.d3d_iou3d_forward(_lib.ptr(b1), n, _lib.ptr(b2), m, 1 if key == "RBOX" else 0, _lib.ptr(out),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "iou3d_forward")
    return _egress(call.back(out), was_numpy)


def _iou_paired(boxes1, boxes2, cols, kind, code, need_jac):
    """one launch of d3d_iou2d_paired (cols 5) / d3d_iou3d_paired (cols 7) -> (ious[N] on the caller's device, jac[N, 2 cols] on the GPU
    or None).  jac is in the arithmetic's dtype: fp64 unless `code` is D3D_F32."""
    lib = _lib.load()
    with _Staged(boxes1.detach(), boxes2.detach()) as call:
        (b1, b2), dev = call.inputs, call.dev
        n = b1.shape[0]
        ious = torch.empty((n,), dtype=b1.dtype, device=dev)
        jac = torch.empty((n, 2 * cols), dtype=torch.float32 if code == _lib.F32 else torch.float64, device=dev) if need_jac else None
        if options.current().poison:
            ious.fill_(float("nan"))
            if need_jac:
                jac.fill_(float("nan"))
        fn = lib.d3d_iou2d_paired if cols == 5 else lib.d3d_iou3d_paired
        rc = fn(_lib.ptr(b1), _lib.ptr(b2), n, int(kind), code, _lib.ptr(ious), _lib.ptr(jac), _lib.stream_ptr())
    _lib.check(rc, "iou2d_paired" if cols == 5 else "iou3d_paired")
    return call.back(ious), jac


def _paired_forward(ctx, cols, boxes1, boxes2, kind, code):
    need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    ious, jac = _iou_paired(boxes1, boxes2, cols, kind, code, need)
    if need:                                                       # (otherwise jac is not even allocated: the GRAD = false kernel ran)
        ctx.save_for_backward(jac)
        ctx.origin = (boxes1.device, boxes1.dtype)
    return ious


def _paired_backward(ctx, cols, grad):
    jac, = ctx.saved_tensors
    odev, dtype = ctx.origin
    g = (grad.to(device=jac.device, dtype=jac.dtype)[:, None] * jac).to(device=odev, dtype=dtype)
    return g[:, :cols] if ctx.needs_input_grad[0] else None, g[:, cols:] if ctx.needs_input_grad[1] else None, None, None


class IouPaired2D(torch.autograd.Function):
    """box2d_iou_paired: (boxes1[N,5], boxes2[N,5], IouType, dtype code) -> [N].  forward is one launch; when an input needs a
    gradient the same launch writes the pairs' partial derivatives jac[N,10] (80 bytes per pair in fp64) and backward is
    grad[:, None] * jac -- every pair owns its rows: no atomics, no kernel, no second pass over the boxes.  Differentiable once."""

    @staticmethod
    def forward(ctx, boxes1, boxes2, iou_type, code):
        return _paired_forward(ctx, 5, boxes1, boxes2, iou_type, code)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _paired_backward(ctx, 5, grad)


class IouPaired3D(torch.autograd.Function):
    """box3d_iou_paired: (boxes1[N,7], boxes2[N,7], rotated, dtype code) -> [N]; as IouPaired2D with jac[N,14] (112 bytes per pair)"""

    @staticmethod
    def forward(ctx, boxes1, boxes2, rotated, code):
        return _paired_forward(ctx, 7, boxes1, boxes2, rotated, code)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _paired_backward(ctx, 7, grad)


def _paired(fn, boxes1, boxes2, kind, precise, was_numpy):
    """dtype handling of box2d_iou for the paired operators: precise = fp64 arithmetic, the result cast back; on fp32 boxes the
    widening happens where the kernel loads them (D3D_F32_WIDE) -- no .double() copies, no cast launch"""
    dtype_in = boxes1.dtype
    boxes1, boxes2, wide32 = _promote(precise, boxes1, boxes2)
    if boxes1.dtype != boxes2.dtype:
        raise RuntimeError("boxes1 and boxes2 must have the same dtype")
    code = _dtype_code(boxes1, wide32)
    if len(boxes1) == 0:                                            # nothing to launch (and nothing to differentiate)
        return _egress(boxes1[:, 0].to(dtype_in), was_numpy)
    ious = fn.apply(boxes1, boxes2, kind, code)
    return _egress(ious.to(dtype_in) if precise else ious, was_numpy)


def box2d_iou_paired(boxes1, boxes2, method="rbox", precise=True):
    """IoU of box i of `boxes1` with box i of `boxes2` -- the diagonal of box2d_iou(boxes1, boxes2, method, precise) without its
    matrix: what a detector's regression loss takes for its N matched (prediction, target) pairs.  Differentiable in both inputs
    (once); the reference has no counterpart.

    :param boxes1: N x 5 (x,y,w,h,r), torch tensor or numpy array
    :param boxes2: N x 5
    :param method: 'box', 'rbox', or the loss variants 'grbox' (GIoU) / 'drbox' (DIoU); resolved like box2d_iou's
    :param precise: compute in float64 and cast back to the input dtype
    :return: [N]; 0 (and a zero gradient) for a rectangle without area ('rbox', 'grbox', 'drbox') and for pairs apart ('box', 'rbox')
    """
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    _check_fields(5, boxes1, boxes2, flat=_NX2)
    if len(boxes1) != len(boxes2):
        raise ValueError("Paired boxes should come in equal numbers: %d and %d" % (len(boxes1), len(boxes2)))
    iou_type = getattr(IouType, method.upper())                   # AttributeError for unknown names, like box2d_iou
    if iou_type not in _IOU_FUNCTIONS:
        raise ValueError("Unrecognized iou type!")
    return _paired(IouPaired2D, boxes1, boxes2, int(iou_type), precise, was_numpy)


def box3d_iou_paired(boxes1, boxes2, method="rbox", precise=True):
    """"3D IoU" of box i of `boxes1` with box i of `boxes2`, the measure of iou3d (the evaluator's and the matcher's): the BEV IoU
    of (x, y, lx, ly, rz) -- rotated for 'rbox', of the bounding boxes for 'box' -- times the IoU of the z intervals,
    max(min(zmax) - max(zmin), 0) / max(max(zmax) - min(zmin), 1e-6); 0 where the BEV IoU is 0.  Differentiable in both inputs
    (once), fp32 and fp64.  The dimensions are not clipped (that is the matcher's guard).  This is NOT the volumetric IoU
    (intersection volume over union volume), which is a different function and not offered here.

    :param boxes1: N x 7 (x,y,z,lx,ly,lz,rz), torch tensor or numpy array
    :param boxes2: N x 7
    :param precise: compute in float64 and cast back to the input dtype
    """
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    key = method.upper()
    if key not in ("RBOX", "BOX"):
        raise ValueError("Unrecognized iou type!")
    _check_fields(7, boxes1, boxes2)
    if len(boxes1) != len(boxes2):
        raise ValueError("Paired boxes should come in equal numbers: %d and %d" % (len(boxes1), len(boxes2)))
    return _paired(IouPaired3D, boxes1, boxes2, 1 if key == "RBOX" else 0, precise, was_numpy)


def _sparse_threshold(threshold):
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("threshold should be a finite number >= 0, got %r" % (threshold,))
    if not (0 <= t < float("inf")):                                 # (NaN fails the comparison too)
        raise ValueError("threshold should be a finite number >= 0, got %r" % (threshold,))
    return t


def _iou_sparse(boxes1, boxes2, cols, iou_type, code, threshold, return_offsets, was_numpy):
    """d3d_iou_sparse_count, ONE host read (offsets[n] = K), d3d_iou_sparse_emit -> (pairs[K,2] i64, values[K], offsets[n+1] i64)
    on the caller's device; values in the dtype of `boxes1`"""
    odev = boxes1.device
    n, m = boxes1.shape[0], boxes2.shape[0]
    if n == 0 or m == 0:                                            # no pair: nothing to launch, nothing to load
        res = (torch.zeros((0, 2), dtype=torch.int64, device=odev), torch.zeros((0,), dtype=boxes1.dtype, device=odev),
               torch.zeros((n + 1,), dtype=torch.int64, device=odev))
    else:
        lib = _lib.load()
        with _Staged(boxes1.detach(), boxes2.detach()) as call:
            (b1, b2), dev = call.inputs, call.dev
            offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
            ws = _lib.workspace(lib.d3d_iou_sparse_workspace_bytes(n, m), dev)
            inputs = (_lib.ptr(b1), n, _lib.ptr(b2), m, cols, int(iou_type), code, threshold)
            _lib.check(lib.d3d_iou_sparse_count(*inputs, _lib.ptr(offsets), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "iou_sparse_count")
            k = int(offsets[n])                                      # the one host synchronisation of the call
            pairs = torch.empty((k, 2), dtype=torch.int64, device=dev)
            values = torch.empty((k,), dtype=b1.dtype, device=dev)
            if k > 0:
                _lib.check(lib.d3d_iou_sparse_emit(*inputs, _lib.ptr(offsets), k, _lib.ptr(pairs), _lib.ptr(values), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr()), "iou_sparse_emit")
        res = call.back((pairs, values, offsets))
    res = tuple(_egress(t, was_numpy) for t in res)
    return res if return_offsets else res[:2]


def box2d_iou_sparse(boxes1, boxes2, method="rbox", threshold=0.0, precise=True, return_offsets=False):
    """The entries of D = box2d_iou(boxes1, boxes2, method, precise) that are above `threshold`, as a list -- without the [N,M]
    matrix, which for two large sets is almost all zeros (and at 200 k x 200 k boxes does not fit on the card): what matching
    detections to ground truth, a graph for box fusion or cluster NMS, and an evaluator's association take.  The reference has no
    counterpart.

    :param boxes1: N x 5 (x,y,w,h,r), torch tensor or numpy array (numpy in, numpy out; CPU or GPU, any strides)
    :param boxes2: M x 5
    :param method: 'box' or 'rbox' (the loss variants are nonzero almost everywhere: ValueError)
    :param threshold: finite, >= 0; the comparison is strict and made on the stored value, the threshold rounded to D's dtype
    :param precise: compute in float64 and cast back to the input dtype, as box2d_iou does
    :param return_offsets: also return offsets int64 [N+1] (CSR): pairs[offsets[i]:offsets[i+1]] are row i's pairs
    :return: pairs int64 [K,2] == (D > threshold).nonzero(), ascending by row and then by column, and
        values [K] == D[pairs[:,0], pairs[:,1]] bit for bit, in D's dtype.  With threshold 0: exactly the overlapping pairs -- a
        touching pair (IoU 0), a NaN entry, a rectangle without area ('rbox') have none.

    boxes1 and boxes2 must be both float32 or both float64.  The values carry no gradient:
    box2d_iou_paired(boxes1[pairs[:,0]], boxes2[pairs[:,1]], method, precise) gives the same bits with autograd.
    """
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    threshold = _sparse_threshold(threshold)
    _check_fields(5, boxes1, boxes2, flat=_NX2)
    iou_type = getattr(IouType, method.upper())                   # AttributeError for unknown names, like box2d_iou
    if iou_type not in (IouType.BOX, IouType.RBOX):
        raise ValueError("Unsupported iou type!")
    if boxes1.dtype != boxes2.dtype:
        raise RuntimeError("boxes1 and boxes2 must have the same dtype")
    # box2d_iou's promotion: fp32 boxes, precise -- fp64 arithmetic on rows widened inside the kernels, the value rounded to fp32;
    # the values stay in the boxes' dtype, so nothing is copied to fp64 and another dtype is refused
    return _iou_sparse(boxes1, boxes2, 5, iou_type, _dtype_code(boxes1, _wide32(precise, boxes1, boxes2)), threshold, return_offsets, was_numpy)


def iou3d_sparse(boxes1, boxes2, method="rbox", threshold=0.0, return_offsets=False):
    """The entries of D = iou3d(boxes1, boxes2, method) above `threshold` as a list, without the matrix: box2d_iou_sparse for
    [N,7] x [M,7] rows (x,y,z,lx,ly,lz,rz), in fp32 as iou3d.  A pair whose BEV footprints overlap while the z ranges are apart or
    only touch has value 0 and is left out.  box3d_iou_paired(boxes1[pairs[:,0]], boxes2[pairs[:,1]], method, precise=False) on
    fp32 rows gives the same bits with autograd."""
    (boxes1, boxes2), was_numpy = _ingress(boxes1, boxes2)
    threshold = _sparse_threshold(threshold)
    key = method.upper()
    if key not in ("RBOX", "BOX"):
        raise ValueError("Unsupported iou type!" if hasattr(IouType, key) else "Unrecognized iou type!")
    _check_fields(7, boxes1, boxes2)
    return _iou_sparse(boxes1.to(torch.float32), boxes2.to(torch.float32), 7, getattr(IouType, key), _lib.F32, threshold, return_offsets,
                       was_numpy)


def _check_points_boxes(points, boxes):
    if len(points.shape) != 2 or points.shape[1] != 2 or len(boxes.shape) != 2 or boxes.shape[1] != 5:
        raise ValueError("points should be Nx2 and boxes Mx5")
    if points.dtype != boxes.dtype:
        raise RuntimeError("points and boxes must have the same dtype")


def crop_2dr(points, boxes):
    """crop_2dr of the reference (utils.cpp:38-47; box_impl.crop_2dr): bool[M,N] indicators, [i,j] = point j is
    inside rotated box i.  points [N,2], boxes [M,5], same floating dtype."""
    lib = _lib.load()
    _check_points_boxes(points, boxes)
    with _Staged(points, boxes) as call:
        p, b = call.inputs
        n, m = p.shape[0], b.shape[0]
        out = torch.empty((m, n), dtype=torch.uint8, device=call.dev)
        rc = lib.d3d_crop_2dr(_lib.ptr(p), n, _lib.ptr(b), m, _dtype_code(p), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "crop_2dr")
    return call.back(out.view(torch.bool))


def box2dr_crop(points, boxes):
    """Crop points by rotated boxes -- reference box/__init__.py:278-287 (returns the [M,N] indicator matrix,
    as the reference's code does)."""
    return crop_2dr(points, boxes)


def _project(points, boxes, axis):
    """[N,3] points and [M,7] boxes seen along `axis` -> (points [N,2], boxes [M,5]: x, y, w, h, r in the plane of the two other axes)"""
    if axis not in (0, 1, 2):
        raise ValueError("The projection axis can only be 0-x, 1-y and 2-z!")
    u, v = (a for a in (0, 1, 2) if a != axis)
    return points[:, [u, v]], boxes[:, [u, v, 3 + u, 3 + v, 6]]


def box3dp_crop(points, boxes, project_axis=2):
    """Crop points [N,3] by boxes [M,7] projected along `project_axis` -- reference box/__init__.py:289-315.  fp32, along z, a cloud
    of 4096 points and more against up to 4096 boxes: ONE launch (d3d_crop_3dp: the same tests on the same float expressions);
    anything else: the reference's composition around crop_2dr."""
    if (project_axis == 2 and torch.is_tensor(points) and torch.is_tensor(boxes) and points.dtype == torch.float32 and
            boxes.dtype == torch.float32 and points.dim() == 2 and boxes.dim() == 2 and points.shape[1] >= 3 and boxes.shape[1] == 7
            and points.shape[0] >= 4096 and 0 < boxes.shape[0] <= 4096):
        lib = _lib.load()
        with _Staged(points.detach(), boxes.detach()) as call:
            p, b = call.inputs
            n, m = p.shape[0], b.shape[0]
            out = torch.empty((m, n), dtype=torch.uint8, device=call.dev)
            rc = lib.d3d_crop_3dp(_lib.ptr(p), n, p.shape[1], _lib.ptr(b), m, 7, 2, _lib.ptr(out), _lib.stream_ptr())
        if rc != _lib.ERR_UNSUPPORTED:
            _lib.check(rc, "crop_3dp")
            return call.back(out.view(torch.bool))
    mask_2d = crop_2dr(*_project(points, boxes, project_axis))
    points_p = points[:, [project_axis]].t()
    boxes_p = boxes[:, [project_axis]]
    boxes_pd = boxes[:, [3 + project_axis]] / 2
    mask_p = (points_p - boxes_pd < boxes_p) & (boxes_p < points_p + boxes_pd)
    return mask_2d & mask_p


def pdist2dr_forward(points, boxes):
    """pdist2dr_forward[_cuda] (dist.h:7-9; dist.cpp:36-52): (distance[M,N], iedge[M,N] uint8) for points[N,2], boxes[M,5];
    signed distance to the box boundary, positive inside"""
    lib = _lib.load()
    _check_points_boxes(points, boxes)
    with _Staged(points.detach(), boxes.detach()) as call:
        p, b = call.inputs
        n, m = p.shape[0], b.shape[0]
        dist = torch.empty((m, n), dtype=p.dtype, device=call.dev)
        iedge = torch.empty((m, n), dtype=torch.uint8, device=call.dev)
        rc = lib.d3d_pdist2dr_forward(_lib.ptr(p), n, _lib.ptr(b), m, _dtype_code(p), _lib.ptr(dist), _lib.ptr(iedge),
                                      _lib.stream_ptr())
    _lib.check(rc, "pdist2dr_forward")
    return call.back((dist, iedge))


def pdist2dr_backward(points, boxes, grad, iedge=None):
    """pdist2dr_backward[_cuda] (dist.h:10-13; dist.cpp:90-110): (grad_boxes[M,5], grad_points[N,2]); `iedge` is accepted
    for signature compatibility and ignored (the nearest feature is recomputed)"""
    lib = _lib.load()
    with _Staged(points.detach(), boxes.detach(), grad.to(points.dtype)) as call:
        p, b, g = call.inputs
        n, m = p.shape[0], b.shape[0]
        gb = torch.empty((m, 5), dtype=p.dtype, device=call.dev)
        gp = torch.empty((n, 2), dtype=p.dtype, device=call.dev)
        rc = lib.d3d_pdist2dr_backward(_lib.ptr(p), n, _lib.ptr(b), m, _lib.ptr(g), _dtype_code(p), _lib.ptr(gb), _lib.ptr(gp),
                                       _lib.stream_ptr())
    _lib.check(rc, "pdist2dr_backward")
    return call.back((gb, gp))


class PDist2DR(torch.autograd.Function):
    """reference box/__init__.py:132-150 -- with its argument mix-up fixed: the compiled functions take (points, boxes)
    (dist.h:7-13) while the reference passes (boxes, points) and returns the two gradients in the wrong order"""

    @staticmethod
    def forward(ctx, points, boxes):
        dist, iedge = pdist2dr_forward(points, boxes)
        ctx.save_for_backward(points, boxes)
        return dist

    @staticmethod
    def backward(ctx, grad):
        points, boxes = ctx.saved_tensors
        grad_boxes, grad_points = pdist2dr_backward(points, boxes, grad.contiguous())
        return grad_points, grad_boxes


def seg1d_iou(seg1, seg2, reference_compat=True):
    """IoU of 1-D segments, row by row: seg1, seg2 [N,2] = (centre, width) -> [N] -- reference box/__init__.py:152-178 (plain
    tensor arithmetic there too).  The default reproduces the reference's values bit for bit, INCLUDING its slip: the half-width
    of seg2 is taken from seg1 (:164).  `reference_compat=False` uses seg2's own width -- INTEGRATION.md section 5"""
    assert torch.all(seg1[:, 1] > 0)
    assert torch.all(seg2[:, 1] > 0)
    d1, d2 = seg1[:, 1] / 2, (seg1 if reference_compat else seg2)[:, 1] / 2
    s1max, s1min, s2max, s2min = seg1[:, 0] + d1, seg1[:, 0] - d1, seg2[:, 0] + d2, seg2[:, 0] - d2
    i = torch.clamp_min(torch.minimum(s1max, s2max) - torch.maximum(s1min, s2min), 0)
    u = torch.clamp_min(torch.maximum(s1max, s2max) - torch.minimum(s1min, s2min), 1e-6)
    return i / u


def seg1d_pdist(points, segs):
    """distance from points [N,1] to 1-D segments [M,2] = (centre, width) -- reference box/__init__.py:317-331
    (positive inside; broadcasts to the [N,M] / [M] shapes the reference's callers use)"""
    assert torch.all(segs[:, 1] > 0)
    dsegs = segs[:, 1] / 2
    smax, smin = segs[:, 0] + dsegs, segs[:, 0] - dsegs
    return torch.where(points > segs[:, 0], smax - points, points - smin)


def box2dr_pdist(points, boxes, method="rbox"):
    """Signed distance from points [N,2] to rotated 2D boxes [M,5] -> [M,N] -- reference box/__init__.py:333-349"""
    _check_fields(5, boxes, flat="Input boxes should be Nx2 tensors!")
    if method != "rbox":
        raise ValueError("Only supported rotated boxes by now!")
    return PDist2DR.apply(points, boxes)


def box3dr_pdist(points, boxes, project_axis=2):
    """Signed distance from points [N,3] to 3D boxes [M,7] (surfaces) -> [M,N] -- reference box/__init__.py:351-381.
    (The reference combines a [M,N] planar distance with a [N,M] axial one, which only broadcasts for N == M; here the
    axial distance is laid out [M,N] as well.)"""
    points_2d, boxes_2d = _project(points, boxes, project_axis)
    dist_2d = box2dr_pdist(points_2d.contiguous(), boxes_2d.contiguous())
    dist_p = seg1d_pdist(points[:, [project_axis]], boxes[:, [project_axis, 3 + project_axis]]).t()
    return torch.where(
        dist_p > 0,
        torch.where(dist_2d > 0, torch.min(dist_p, dist_2d), dist_2d),
        torch.where(dist_2d > 0, dist_p, -torch.sqrt(dist_2d.square() + dist_p.square())))


# north_star operator names
iou2d = box2d_iou
nms = box2d_nms

from .center import (HeatmapPeaks, circle_nms, circle_nms_max, gather_at_peaks, gaussian_heatmap, gaussian_radius,  # noqa: E402
                     heatmap_peaks, heatmap_peaks_max)

__all__ = ["HeatmapPeaks", "heatmap_peaks", "heatmap_peaks_max", "gather_at_peaks", "circle_nms", "circle_nms_max", "gaussian_heatmap",
           "gaussian_radius",
           "Iou2D", "Iou2DR", "GIou2DR", "DIou2DR", "PDist2DR", "iou2d_backward", "iou2dr_backward", "giou2dr_forward",
           "giou2dr_backward", "diou2dr_forward", "diou2dr_backward", "iou2dr_flags", "pdist2dr_forward", "pdist2dr_backward",
           "box2dr_crop", "box3dp_crop", "box2dr_pdist", "box3dr_pdist", "seg1d_pdist", "seg1d_iou", "crop_2dr", "box2d_iou", "box2d_nms",
           "box2d_nms_batched", "box2d_iou_paired", "box3d_iou_paired", "IouPaired2D", "IouPaired3D", "box2d_iou_sparse", "iou3d_sparse",
           "iou2d", "iou3d", "nms", "iou2d_forward", "iou2dr_forward", "nms2d", "nms2d_cuda", "argsort_desc", "IouType",
           "SupressionType", "cuda_available"]
