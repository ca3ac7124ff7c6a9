"""CPU: the numpy model of the voxel interpolation (voxel_interp_reference.py) against a brute force over a coordinate dictionary and
against torch's dense grid_sample and its autograd in fp64, voxel_positions against the voxelizer's own coordinates, and the argument
checks of d3d_amd.voxel.interp and of the C entries that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_interp_cases as cases
import voxel_interp_reference as ref


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("name", cases.SCENES)
def test_model_is_the_brute_force_over_a_coordinate_dictionary(name, dtype):
    c, b, _, pb = cases.scene(name)
    p = cases.positions(name, dtype)
    for mode in ref.MODES:
        for normalize in (False, True):
            t, w = ref.corners(c, p, b, pb, mode, normalize)
            bt, bw = ref.corners_brute(c, p, b, pb, mode, normalize)
            assert t.dtype == np.int32 and w.dtype == p.dtype and t.shape == (len(p), ref.MODES[mode])
            assert np.array_equal(t, bt), (mode, normalize)
            assert np.array_equal(w.view(np.uint8), bw.view(np.uint8)), (mode, normalize)
            assert np.all(w[t < 0] == 0) and np.all((t >= -1) & (t < max(len(c), 1)))


def test_scenes_are_what_they_claim():
    """conditions on the inputs the GPU tests rely on"""
    t, w = cases.table("integers", "f32")
    assert np.all(w[t >= 0] == (np.nonzero(t >= 0)[1] == 0)) and (t[:, 0] >= 0).sum() > 20       # f = 0: corner 0 carries it all
    for dtype in ("f32", "f64"):
        _, _, f = ref.base(cases.positions("tiny_negative", dtype), "linear")
        assert (f == 1).sum() > 20 and f.max() == 1                                              # f rounds to exactly 1
        t, w = cases.table("nonfinite", dtype)
        assert np.all(t[:36] == -1) and np.all(w[:36] == 0) and (t[40:] >= 0).any()              # out of range, or far outside the box
    n = ref.entries_per_voxel(cases.table("crowded", "f32")[0], 27)
    assert n.max() == cases.CROWD + 1 and cases.CROWD in n and cases.CROWD % 4 == 0 and (cases.CROWD + 1) % 4 != 0
    assert (ref.entries_per_voxel(cases.table("untouched", "f32")[0], 65) == 0).sum() > 30
    t, _ = cases.table("outside", "f32")
    assert (t < 0).all(1).sum() > 10 and ((t >= 0).any(1) & (t < 0).any(1)).sum() > 10
    t, _ = cases.table("batches", "f64")
    pb = cases.scene("batches")[3]
    assert np.all(t[(pb != 0) & (pb != 2)] == -1) and (t[pb == 2] >= 0).any() and (t[pb == 0] >= 0).any()
    t, _ = cases.table("wrap", "f32")
    assert (t >= 0).sum() > 100 and np.all(t[110:, 4:] == -1)          # the absent coordinate: x + 1 corners of floor(x) = absent - 1


def _dense(name):
    """a scene moved to the origin of a dense grid with one cell of margin -> (local coords, local positions, the grid's (X, Y, Z))"""
    c, _, p, _ = cases.scene(name)
    lo = c.min(0) - 1
    return c - lo, p - lo, tuple(int(a) for a in (c - lo).max(0) + 2)


@pytest.mark.parametrize("name", ("random", "negative", "quarters", "outside", "untouched", "crowded"))
def test_model_is_dense_grid_sample_and_its_autograd(name):
    """fp64: the voxels written into a zero grid [1, C, X, Y, Z], sampled with mode="bilinear", align_corners=True,
    padding_mode="zeros" at the positions (the grid's last dimension is (z, y, x): its first entry walks the LAST dense axis).  An
    inactive cell is a zero, which adds what an absent corner adds: nothing.

    The bound.  grid_sample takes the position as xn = 2 p / (S - 1) - 1 and turns it back into ((xn + 1) / 2) (S - 1): four roundings
    of numbers of magnitude up to S, the grid's extent, so the position it interpolates at is off by at most d = 4 eps S per axis.
    Trilinear interpolation is continuous and each corner's weight moves by at most d per axis: the value moves by at most 3 d times
    the largest |x| of the (at most 8) cells around each of the two positions, bounded here by 8 max|x|.  On top of that both sides
    round their own sum of 8 products: 16 eps sum_j |w_j| |x_j| covers the two.  The transpose sums, per voxel, n such terms w g:
    (n + 16) eps sum |w| |g|, plus 3 d times the sum of |g| over all points (every point may hand a voxel up to 3 d of weight)."""
    c, p, shape = _dense(name)
    v, k, ch = len(c), len(p), 3
    eps = 2.0 ** -52
    x = cases.randoms(v, ch, 1)
    g = cases.randoms(k, ch, 2)
    table, w = ref.corners(c, p)
    out = ref.forward(x, table, w, "f64")
    gf = ref.transpose(g, table, w, v, "f64")

    xt = torch.from_numpy(x).requires_grad_()
    at = tuple(torch.from_numpy(c[:, a]) for a in range(3))
    dense = torch.zeros(shape + (ch,), dtype=torch.float64).index_put(at, xt).permute(3, 0, 1, 2)[None]
    size = torch.tensor(shape, dtype=torch.float64)
    norm = (2 * torch.from_numpy(p) / (size - 1) - 1).flip(1)                        # (z, y, x)
    y = torch.nn.functional.grid_sample(dense, norm[None, :, None, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)
    y = y[0, :, :, 0, 0].t()
    y.backward(torch.from_numpy(g))

    d = 4 * eps * max(shape)
    tol = 16 * eps * ref.forward(np.abs(x), table, np.abs(w), "f64") + 3 * d * 8 * np.abs(x).max()
    assert tol.max() < 1e-11                                                         # the bound is worth something
    assert np.all(np.abs(out - y.detach().numpy()) <= tol)
    n = ref.entries_per_voxel(table, v)[:, None]
    tol = (n + 16) * eps * ref.transpose(np.abs(g), table, np.abs(w), v, "f64") + 3 * d * np.abs(g).sum(0)[None, :]
    assert tol.max() < 1e-9
    assert np.all(np.abs(gf - xt.grad.numpy()) <= tol)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_transpose_is_the_adjoint_of_forward(kind):
    """<forward(x), g> == <x, transpose(g)> up to the order of the sums (exact on integer data with quarter-step positions)"""
    c = cases.scene("quarters")[0]
    table, w = cases.table("quarters", "f32")
    x = cases.small_integers(len(c), 4, 3).astype(ref.fold_type(kind))
    g = cases.small_integers(len(table), 4, 4).astype(ref.fold_type(kind))
    lhs = (ref.forward(x, table, w, kind).astype(np.float64) * g).sum()
    rhs = (x * ref.transpose(g, table, w, len(c), kind).astype(np.float64)).sum()
    assert lhs == rhs and lhs != 0


def test_voxel_positions_round_to_the_voxelizers_coordinates():
    """points kept at least 1e-3 of a cell away from every face: floor(position + 0.5) is the coordinate the reference voxelizer gives
    the point's voxel, and the position's fraction is the point's place between the centres"""
    import oracle
    from d3d_amd import synth
    from d3d_amd.voxel import voxel_positions
    gen = oracle.VoxelGenerator(synth.KITTI_BOUNDS, [176, 200, 8], max_points=1000, max_voxels=100000)
    r = np.random.default_rng(5)
    cell = r.integers(0, [176, 200, 8], (4000, 3))
    frac = r.uniform(1e-3, 1 - 1e-3, (4000, 3))
    lo = np.array(synth.KITTI_BOUNDS, np.float64).reshape(3, 2)[:, 0]
    pts = np.concatenate([lo + (cell + frac) * gen._size.astype(np.float64), r.random((4000, 1))], 1).astype(np.float32)
    sp = gen(pts)
    assert len(sp.points) == 4000 and np.array_equal(sp.points, pts)
    want = sp.coords[sp.points_mapping]
    for dtype in (None, torch.float64):
        pos = voxel_positions(torch.from_numpy(pts), torch.from_numpy(gen._size), torch.from_numpy(gen._offset), dtype=dtype)
        assert pos.shape == (4000, 3) and pos.dtype == (dtype or torch.float32)
        assert np.array_equal(torch.floor(pos + 0.5).long().numpy(), want)
        assert np.abs(pos.double().numpy() - (want + frac - 0.5)).max() < 1e-3
    got = voxel_positions(pts, gen._size.tolist(), gen._offset.tolist())
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(np.floor(got + 0.5).astype(np.int64), want)
    assert voxel_positions(pts[:, :3], 0.4).shape == (4000, 3)
    with pytest.raises(ValueError):
        voxel_positions(pts[:, :2], 0.4)
    with pytest.raises(ValueError):
        voxel_positions(pts, 0.4, dtype=torch.float16)


# ---------------------------------------------------------------- the library's host side

def _fake_interp(v=6, k=9, j=8):
    """a VoxelInterp that was never built (building one needs a GPU): what the argument checks read of it"""
    from d3d_amd.voxel import VoxelInterp
    itp = VoxelInterp.__new__(VoxelInterp)
    itp.device, itp.num_voxels, itp.num_points, itp.num_corners, itp.num_entries = torch.device("cuda", 0), v, k, j, 0
    return itp


def test_voxel_interp_refuses_bad_arguments_without_a_gpu():
    from d3d_amd.voxel import VoxelInterp
    c, p = np.zeros((6, 3), np.int64), np.zeros((9, 3), np.float32)
    for bad in (np.zeros((6, 2), np.int64), np.zeros(6, np.int64), np.zeros((6, 3), np.float32)):
        with pytest.raises(ValueError, match="coords"):
            VoxelInterp(bad, p)
    for bad in (np.zeros((9, 2), np.float32), np.zeros(9, np.float32), np.zeros((9, 3, 1))):
        with pytest.raises(ValueError, match=r"\[K, 3\]"):
            VoxelInterp(c, bad)
    for bad in (np.zeros((9, 3), np.float16), np.zeros((9, 3), np.int64), torch.zeros((9, 3), dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float32 or float64"):
            VoxelInterp(c, bad)
    with pytest.raises(TypeError):
        VoxelInterp(c, [[0.0, 0.0, 0.0]])
    b, pb = np.zeros(6, np.int64), np.zeros(9, np.int64)
    for kw in (dict(batch_index=b), dict(position_batch=pb)):
        with pytest.raises(ValueError, match="exactly when"):
            VoxelInterp(c, p, **kw)
    with pytest.raises(ValueError, match="batch_index"):
        VoxelInterp(c, p, batch_index=np.zeros(5, np.int64), position_batch=pb)
    for bad in (np.zeros(8, np.int64), np.zeros((9, 1), np.int64), np.zeros(9, np.float32)):
        with pytest.raises(ValueError, match="position_batch"):
            VoxelInterp(c, p, batch_index=b, position_batch=bad)
    for mode in ("cubic", "LINEAR", None, 8):
        with pytest.raises(ValueError, match="mode"):
            VoxelInterp(c, p, mode=mode)
    wide = np.array([[0, 0, 0], [2 ** 31, 2 ** 31, 2 ** 31]], np.int64)
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelInterp(wide, p)
    with pytest.raises(ValueError, match="2\\^62"):
        VoxelInterp(np.array([[0, 0, 0], [2 ** 21, 2 ** 21, 2 ** 20]], np.int64), p, batch_index=np.array([0, 2 ** 10], np.int64), position_batch=pb)


def test_operators_refuse_bad_arguments_without_a_gpu():
    from d3d_amd.voxel import voxel_interpolate, voxel_splat
    itp = _fake_interp()
    for fn, rows in ((voxel_interpolate, 6), (voxel_splat, 9)):
        for owner in (torch.zeros((9, 8), dtype=torch.int32), None, "interp"):
            with pytest.raises(TypeError):
                fn(torch.zeros((rows, 4)), owner)
        with pytest.raises(TypeError):
            fn([[0.0] * 4] * rows, itp)
        for bad in (torch.zeros((rows, 4), dtype=torch.int32), np.zeros((rows, 4), np.int64), torch.zeros((rows, 4), dtype=torch.complex64)):
            with pytest.raises(ValueError, match="float32, float64, float16 or bfloat16"):
                fn(bad, itp)
        for bad in (torch.zeros(rows), torch.zeros((rows, 4, 1)), torch.zeros(())):
            with pytest.raises(ValueError, match="2-D"):
                fn(bad, itp)
        for bad in (torch.zeros((rows + 1, 4)), torch.zeros((rows - 1, 4), dtype=torch.bfloat16), np.zeros((0, 4), np.float16)):
            with pytest.raises(ValueError, match="rows"):
                fn(bad, itp)


def test_refusals_without_launching():
    """every refusal of the three entries returns before any HIP call: they answer on a machine without a GPU, with pointers that are
    never followed"""
    from d3d_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    big = lib.d3d_voxel_corners_workspace_bytes(10)
    assert big == lib.d3d_voxel_neighbors_workspace_bytes(10) > 0
    cor = lambda co=p, b=None, v=10, pos=p, pb=None, k=5, dtype=0, j=8, t=p, w=p, n=p, ws=p, wsb=big: \
        lib.d3d_voxel_corners(co, b, v, pos, pb, k, dtype, j, 0, t, w, n, ws, wsb, None)
    fwd = lambda feat=p, v=10, c=4, dtype=0, t=p, w=p, rows=5, j=8, out=p: lib.d3d_table_interp_forward(feat, v, c, dtype, t, w, rows, j, out, None)
    bwd = lambda g=p, rows=5, c=4, dtype=0, o=p, off=p, w=p, j=8, v=10, out=p: lib.d3d_table_interp_backward(g, rows, c, dtype, o, off, w, j, v, out, None)
    bad, uns = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    assert [cor(v=-1), cor(k=-1), cor(n=None), cor(j=2), cor(j=0), cor(co=None), cor(pos=None), cor(t=None), cor(w=None), cor(b=p), cor(pb=p)] == [bad] * 11
    assert [cor(dtype=4), cor(dtype=5), cor(dtype=2), cor(v=2 ** 31), cor(k=2 ** 28), cor(k=2 ** 31, j=1)] == [uns] * 6
    assert [cor(ws=None), cor(wsb=big - 1)] == [_lib.ERR_WORKSPACE] * 2
    assert [fwd(v=-1), fwd(rows=-1), fwd(c=0), fwd(j=2), fwd(j=27), fwd(feat=None), fwd(t=None), fwd(w=None), fwd(out=None)] == [bad] * 9
    assert [fwd(dtype=2), fwd(dtype=3), fwd(dtype=6), fwd(v=2 ** 31), fwd(rows=2 ** 28), fwd(rows=2 ** 31, j=1)] == [uns] * 6
    assert [bwd(v=-1), bwd(rows=-1), bwd(c=0), bwd(j=3), bwd(g=None), bwd(o=None), bwd(off=None), bwd(w=None), bwd(out=None)] == [bad] * 9
    assert [bwd(dtype=2), bwd(dtype=-1), bwd(v=2 ** 31), bwd(rows=2 ** 28), bwd(rows=2 ** 31, j=1)] == [uns] * 5
    for dtype in (0, 1, 4, 5):
        assert fwd(dtype=dtype, rows=0, feat=None, t=None, w=None, out=None) == _lib.OK
        assert bwd(dtype=dtype, v=0, g=None, o=None, off=None, w=None, out=None) == _lib.OK
