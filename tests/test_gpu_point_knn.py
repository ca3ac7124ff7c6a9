"""GPU: knn_query, the kNN weights and point_interpolate (csrc/psample.hip, csrc/vinterp.hip) against the numpy models of
point_knn_reference.py, bit for bit: tables with array_equal, floats by their bits.  The one exception is gradcheck (fp64, torch's
defaults)."""
import numpy as np
import pytest
import torch

import point_knn_cases as cases
import point_knn_reference as ref
from d3d_amd import _lib
from d3d_amd.point import PointInterp, ball_query, furthest_point_sample, knn_query, point_interpolate

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
CODE = {np.float32: _lib.F32, np.float64: _lib.F64}
FOLD_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """two torch tensors of one dtype and shape hold the same bits"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_OF[a.element_size()]),
                                                                     b.contiguous().view(INT_OF[b.element_size()]))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_knn(pts, ctr, k, poffs=None, coffs=None, what=None):
    want_table, want_dist2 = ref.knn_model(pts, ctr, k, poffs, coffs)
    table, dist2 = knn_query(cuda(pts), cuda(ctr), k, poffs, coffs)
    assert table.is_cuda and dist2.is_cuda and table.dtype == torch.int32 and table.shape == dist2.shape == (len(ctr), k)
    assert np.array_equal(table.cpu().numpy(), want_table), what
    assert dist2.cpu().numpy().dtype == pts.dtype and np.array_equal(bits(dist2.cpu().numpy()), bits(want_dist2)), what
    return want_table, want_dist2


@pytest.fixture(scope="module")
def cloud():
    """one LiDAR-like cloud on a 1/64 grid the tests slice rows from (float64; a test casts it)"""
    rng = np.random.default_rng(41)
    pts = rng.uniform(-1.0, 1.0, (6000, 4)) * np.array([50.0, 50.0, 2.0, 1.0])
    return np.round(pts * 64) / 64


# ---------------------------------------------------------------- the query
@pytest.mark.parametrize("k", (1, 3, 16, 63, 64))
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_sizes(cloud, dtype, k):
    """rows around k, the tile (64) and the round (256) of a wavefront's walk; centres around the wavefronts of a workgroup (4)"""
    for n in sorted({1, 2, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 1025} - {0}):
        for m in (1, 3, 4, 5, 67):
            assert_knn(cloud[:n].astype(dtype), cloud[2000:2000 + m, :3].astype(dtype), k, what=(n, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_scenes(dtype):
    """equal q on a lattice, duplicates, the two sorted clouds, rows and centres that are not finite, q = +inf, short and empty
    segments, a ragged batch"""
    for name, pts, ctr, poffs, coffs in cases.scenes():
        for k in (1, 3, 16, 64):
            assert_knn(pts.astype(dtype), ctr.astype(dtype), k, poffs, coffs, what=(name, k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_strides_and_views(cloud, dtype):
    rng = np.random.default_rng(42)
    for d in (3, 4, 5):
        for dc in (3, 4, 5):
            pts = np.concatenate([cloud[:300, :3], rng.normal(size=(300, d - 3))], 1).astype(dtype)
            ctr = np.concatenate([cloud[300:320, :3], rng.normal(size=(20, dc - 3))], 1).astype(dtype)
            assert_knn(pts, ctr, 5, what=(d, dc))
    want = ref.knn_model(cloud[:300, :3].astype(dtype), cloud[:7, :3].astype(dtype), 5)
    wide = cuda(cloud[:300].astype(dtype))                                       # a column slice of [N, 4] rows: read as it lies
    table, dist2 = knn_query(wide[:, :3], wide[:7, :3], 5)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(bits(dist2.cpu().numpy()), bits(want[1]))
    full = cuda(np.concatenate([np.zeros((1, 3), dtype), cloud[:300, :3].astype(dtype)]))
    view = full[1:]                                                              # one row into an allocation: element alignment only
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    table, dist2 = knn_query(view, view[:7], 5)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(bits(dist2.cpu().numpy()), bits(want[1]))


def test_knn_host_numpy_raw_and_repeat(cloud):
    pts, ctr = cloud[:700].astype(np.float32), cloud[700:740, :3].astype(np.float32)
    poffs, coffs = [0, 300, 700], [0, 10, 40]
    want_table, want_dist2 = ref.knn_model(pts, ctr, 6, poffs, coffs)
    table, dist2 = knn_query(pts, ctr, 6, np.array(poffs), np.array(coffs))
    assert isinstance(table, np.ndarray) and isinstance(dist2, np.ndarray) and table.dtype == np.int32 and dist2.dtype == np.float32
    assert np.array_equal(table, want_table) and np.array_equal(bits(dist2), bits(want_dist2))
    table = knn_query(torch.from_numpy(pts), torch.from_numpy(ctr), 6, torch.tensor(poffs), torch.tensor(coffs), return_distances=False)
    assert torch.is_tensor(table) and not table.is_cuda and np.array_equal(table.numpy(), want_table)
    first = knn_query(cuda(pts), cuda(ctr), 6, torch.tensor(poffs).cuda(), torch.tensor(coffs).cuda())      # (offsets read back)
    second = knn_query(cuda(pts), cuda(ctr), 6, poffs, coffs)
    assert first[0].is_cuda and np.array_equal(first[0].cpu().numpy(), want_table)
    assert torch.equal(first[0], second[0]) and same_bits(first[1], second[1])                                # the same call twice
    # the raw entry without distances
    lib = _lib.load()
    p, c = cuda(pts), cuda(ctr)
    raw = torch.full((40, 6), -9, dtype=torch.int32, device="cuda")
    rc = lib.d3d_knn_query(_lib.ptr(p), 700, 4, _lib.ptr(c), 40, 3, _lib.F32, None, None, 0, 6, _lib.ptr(raw), None, _lib.stream_ptr())
    assert rc == _lib.OK and np.array_equal(raw.cpu().numpy(), ref.knn_model(pts, ctr, 6)[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_consistent_with_ball_query(cloud, dtype):
    """with fewer than nsample rows inside r, the ball's rows are the kNN rows with dist2 < r * r, in ascending row"""
    pts, ctr, r, k = cuda(cloud[:3000].astype(dtype)), cuda(cloud[3000:3100, :3].astype(dtype)), 6.0, 64
    ball, counts = ball_query(pts, ctr, r, k)
    assert 0 < int(counts.min()) and int(counts.max()) < k
    table, dist2 = knn_query(pts, ctr, k)
    r2 = dtype(r) * dtype(r)
    for c in range(100):
        inside = table[c][dist2[c] < float(r2)].cpu().numpy()
        assert np.array_equal(np.sort(inside), ball[c, :int(counts[c])].cpu().numpy()), c


# ---------------------------------------------------------------- the weights
def gpu_weights(table, dist2, power, eps):
    m, k = table.shape
    t, q = cuda(table), cuda(dist2)
    w = torch.full((m, k), -7, dtype=q.dtype, device="cuda")
    rc = _lib.load().d3d_knn_weights(_lib.ptr(t), _lib.ptr(q), m, k, CODE[dist2.dtype.type], power, eps, _lib.ptr(w), _lib.stream_ptr())
    assert rc == _lib.OK
    return w.cpu().numpy()


@pytest.mark.parametrize("power", (1, 2))
@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_on_the_scenes(dtype, power):
    for name, pts, ctr, poffs, coffs in cases.scenes():
        pts, ctr = pts.astype(dtype), ctr.astype(dtype)
        for k, eps in ((3, 1e-8), (16, 0.0)):
            table, dist2 = ref.knn_model(pts, ctr, k, poffs, coffs)
            want = ref.knn_weights_model(table, dist2, power, eps)
            assert np.array_equal(bits(gpu_weights(table, dist2, power, eps)), bits(want)), (name, k)
            itp = PointInterp(cuda(pts), cuda(ctr), k, poffs, coffs, power=power, eps=eps)
            assert (itp.num_known, itp.num_points, itp.k) == (len(pts), len(ctr), k)
            assert np.array_equal(itp.table.cpu().numpy(), table) and np.array_equal(bits(itp.dist2.cpu().numpy()), bits(dist2)), (name, k)
            assert np.array_equal(bits(itp.weights.cpu().numpy()), bits(want)), (name, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_sqrt_and_division_are_correctly_rounded(dtype):
    """2^16 random q over the normal range, in pairs of similar size so that both weights carry bits: u = 1 / (sqrt(q) + eps) and
    w = u / s against numpy's correctly rounded sqrt and division, by bits.  This decides how the kernel takes its square root."""
    rng = np.random.default_rng(43)
    span = 60 if dtype == np.float32 else 400
    q0 = np.exp2(rng.uniform(-span, span, 2 ** 15))
    dist2 = np.stack([q0, q0 * rng.uniform(0.25, 4.0, 2 ** 15)], 1).astype(dtype)
    assert np.all(dist2 >= np.finfo(dtype).tiny) and np.all(np.isfinite(dist2)) and dist2.size == 2 ** 16
    table = np.zeros(dist2.shape, np.int32)
    one = dtype(1)
    for power in (1, 2):
        for eps in (0.0, 1e-8):
            root = np.sqrt(dist2) if power == 1 else dist2
            u = one / (root + dtype(eps))
            s = (dtype(0) + u[:, 0]) + u[:, 1]
            want = u / s[:, None]
            got = gpu_weights(table, dist2, power, eps)
            wrong = int((bits(got) != bits(want)).sum())
            print("knn weights %s power %d eps %g: %d of %d weights differ from numpy" % (dtype.__name__, power, eps, wrong, want.size))
            assert wrong == 0
    assert np.array_equal(bits(want[:64]), bits(ref.knn_weights_model(table[:64], dist2[:64], 2, 1e-8)))       # (the model, vectorised)


# ---------------------------------------------------------------- the fold
def acc_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def widen(t):
    """a tensor's values in the accumulation dtype, exactly"""
    return t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()


def rounded(a, dtype):
    return torch.from_numpy(a).to(dtype)                 # (to nearest even)


def random_table(rng, rows, j, v, absent=0.2):
    table = rng.integers(0, v, (rows, j)).astype(np.int32)
    table[rng.random((rows, j)) < absent] = -1
    table[0] = -1                                        # a row without entries
    return table


@pytest.mark.parametrize("j", (1, 3, 5, 16, 64))
@pytest.mark.parametrize("dtype", FOLD_DTYPES)
def test_point_interpolate_forward_and_gradient(dtype, j):
    """vector rows (C a multiple of 16 bytes), scalar rows and rows that start off 16 bytes (C = 1, 3, 130 elements)"""
    rng = np.random.default_rng(44)
    v, rows = 37, 70
    table = random_table(rng, rows, j, v)
    w = rng.uniform(0.0, 1.0, (rows, j)).astype(acc_dtype(dtype))
    itp = PointInterp.from_table(cuda(table), cuda(w), v)
    for c in (1, 3, 4, 8, 130, 260):
        feat = torch.from_numpy(rng.normal(size=(v, c))).to(dtype).cuda().requires_grad_()
        grad = torch.from_numpy(rng.normal(size=(rows, c))).to(dtype).cuda()
        out = point_interpolate(feat, itp)
        assert out.is_cuda and out.dtype == dtype and out.shape == (rows, c)
        assert same_bits(out.detach().cpu(), rounded(ref.wfold_model(widen(feat), table, w), dtype)), c
        out.backward(grad)
        assert same_bits(feat.grad.cpu(), rounded(ref.wfold_transpose_model(widen(grad), table, w, v), dtype)), c
    feat = torch.zeros((v, 0), dtype=dtype, device="cuda")
    assert point_interpolate(feat, itp).shape == (rows, 0)
    host = torch.from_numpy(rng.normal(size=(v, 4))).to(dtype)                   # host in, host out; numpy likewise
    out = point_interpolate(host, itp)
    assert not out.is_cuda and same_bits(out, rounded(ref.wfold_model(widen(host), table, w), dtype))
    if dtype in (torch.float32, torch.float64):
        assert isinstance(point_interpolate(host.numpy(), itp), np.ndarray)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_half_types_round_the_exact_value_once(dtype):
    """small integers: every product and fp32 sum is exact, so the result is the exact value rounded once, to nearest even"""
    rng = np.random.default_rng(45)
    v, rows, j, c = 50, 90, 16, 24
    table = random_table(rng, rows, j, v, absent=0.1)
    w = rng.integers(-8, 9, (rows, j)).astype(np.float32)
    feat = rng.integers(-64, 65, (v, c)).astype(np.float64)
    dense = np.zeros((rows, v))
    for r in range(rows):
        for jj in range(j):
            if table[r, jj] >= 0:
                dense[r, table[r, jj]] += w[r, jj]
    exact = dense @ feat
    assert np.abs(exact).max() > 2048                    # beyond the integers either half type holds
    out = point_interpolate(torch.from_numpy(feat).to(dtype).cuda(), PointInterp.from_table(cuda(table), cuda(w), v))
    assert same_bits(out.cpu(), torch.from_numpy(exact).to(dtype))


def test_from_table_with_a_ball_query_table(cloud):
    """a ball-query table (with -1) and weights of the caller's: the table pooling operators' table, folded"""
    rng = np.random.default_rng(46)
    pts, ctr = cloud[:1500].astype(np.float32), cloud[1500:1560, :3].astype(np.float32)
    table, counts = ball_query(cuda(pts), cuda(ctr), 6.0, 24)
    assert int(counts.min()) < 24 and bool((table == -1).any()) and int(counts.max()) == 24
    w = rng.uniform(-1.0, 1.0, (60, 24)).astype(np.float32)
    itp = PointInterp.from_table(table, cuda(w), 1500)
    assert itp.dist2 is None and itp.k == 24 and itp.num_known == 1500 and itp.num_points == 60
    feat = torch.from_numpy(rng.normal(size=(1500, 20)).astype(np.float32)).cuda().requires_grad_()
    out = point_interpolate(feat, itp)
    assert same_bits(out.detach().cpu(), torch.from_numpy(ref.wfold_model(widen(feat), table.cpu().numpy(), w)))
    grad = torch.from_numpy(rng.normal(size=(60, 20)).astype(np.float32)).cuda()
    out.backward(grad)
    assert same_bits(feat.grad.cpu(), torch.from_numpy(ref.wfold_transpose_model(widen(grad), table.cpu().numpy(), w, 1500)))
    with pytest.raises(ValueError):                      # a GPU table is checked as well
        PointInterp.from_table(table, cuda(w), int(table.max()))


def test_permuting_the_query_rows_permutes_the_output(cloud):
    rng = np.random.default_rng(47)
    known, unknown = cuda(cloud[:500].astype(np.float32)), cuda(cloud[500:1700].astype(np.float32))
    feat = torch.from_numpy(rng.normal(size=(500, 36)).astype(np.float32)).cuda()
    perm = torch.from_numpy(rng.permutation(1200)).cuda()
    for k in (3, 7):
        a = point_interpolate(feat, PointInterp(known, unknown, k))
        b = point_interpolate(feat, PointInterp(known, unknown[perm], k))
        assert same_bits(a[perm], b)
        assert same_bits(a, point_interpolate(feat, PointInterp(known, unknown, k)))                          # and every run the same bits


@pytest.mark.parametrize("dtype", FOLD_DTYPES)
def test_width_8_gives_the_bits_of_the_fixed_width_entries(dtype):
    rng = np.random.default_rng(48)
    lib = _lib.load()
    v, rows, j = 60, 130, 8
    table = cuda(random_table(rng, rows, j, v))
    w = cuda(rng.uniform(0.0, 1.0, (rows, j)).astype(acc_dtype(dtype)))
    from d3d_amd.voxel import VoxelIndex
    from d3d_amd._rows import FEATURE_CODES as _CODES
    idx = VoxelIndex(table.view(-1), v, keep_mapping=False)
    for c in (5, 16):
        feat = torch.from_numpy(rng.normal(size=(v, c))).to(dtype).cuda()
        grad = torch.from_numpy(rng.normal(size=(rows, c))).to(dtype).cuda()
        outs, backs = [], []
        for name in ("d3d_table_interp", "d3d_knn_interp"):
            out, back = torch.empty((rows, c), dtype=dtype, device="cuda"), torch.empty((v, c), dtype=dtype, device="cuda")
            assert getattr(lib, name + "_forward")(_lib.ptr(feat), v, c, _CODES[dtype], _lib.ptr(table), _lib.ptr(w), rows, j, _lib.ptr(out),
                                                   _lib.stream_ptr()) == _lib.OK
            assert getattr(lib, name + "_backward")(_lib.ptr(grad), rows, c, _CODES[dtype], _lib.ptr(idx.order), _lib.ptr(idx.offsets), _lib.ptr(w),
                                                    j, v, _lib.ptr(back), _lib.stream_ptr()) == _lib.OK
            outs.append(out), backs.append(back)
        assert same_bits(outs[0], outs[1]) and same_bits(backs[0], backs[1]), c


def test_gradcheck_fp64(cloud):
    known, unknown = cuda(cloud[:40, :3]), cuda(cloud[40:75, :3])
    for k, power in ((3, 1), (5, 2)):
        itp = PointInterp(known, unknown, k, power=power)
        feat = torch.randn((40, 6), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(k)).requires_grad_()
        assert torch.autograd.gradcheck(lambda f: point_interpolate(f, itp), (feat,))


# ---------------------------------------------------------------- the chain of a feature-propagation layer
def test_sample_then_propagate_back(cloud):
    """FPS -> the three nearest samples of every row -> interpolation in bf16, against the models; a sampled row's nearest sample is a
    row with its own coordinates at q = 0, which takes (nearly) all the weight: eps keeps it short of 1, so compare to the model"""
    rng = np.random.default_rng(49)
    pts_np = cloud[:4000].astype(np.float32)
    pts = cuda(pts_np)
    idx = furthest_point_sample(pts, 256)
    known_np = pts_np[idx.cpu().numpy()]
    itp = PointInterp(pts[idx], pts, k=3)
    table, dist2 = ref.knn_model(known_np, pts_np, 3)
    w = ref.knn_weights_model(table, dist2, 1, 1e-8)
    assert np.array_equal(itp.table.cpu().numpy(), table) and np.array_equal(bits(itp.weights.cpu().numpy()), bits(w))
    feat = torch.from_numpy(rng.normal(size=(256, 32))).to(torch.bfloat16).cuda()
    out = point_interpolate(feat, itp)
    assert same_bits(out.cpu(), rounded(ref.wfold_model(widen(feat), table, w), torch.bfloat16))
    own = itp.table[idx.long(), 0].long()                                        # the sample a sampled row finds first ...
    assert bool((itp.dist2[idx.long(), 0] == 0).all()) and torch.equal(pts[idx][own, :3], pts[idx, :3])       # ... lies where it lies
    assert bool((itp.weights[idx.long(), 0] > 0.999).all())
    assert same_bits(out[idx.long()].cpu(), rounded(ref.wfold_model(widen(feat), table[idx.cpu().numpy()], w[idx.cpu().numpy()]), torch.bfloat16))
