"""CPU: the numpy model of voxel_pool (voxel_pool_reference.py) against numpy's and torch's own CPU scatter operators, the
host-side validation of d3d_amd.voxel.pool, and the index's workspace query -- nothing here touches a GPU."""
import numpy as np
import pytest
import torch

import voxel_pool_cases as cases
import voxel_pool_reference as ref

DRAWS = [cases.mixed(), cases.random_mapping(5000, 300, 11, unmapped=0.1), cases.from_counts(cases.FAN_IN, 12),
         cases.random_mapping(700, 2000, 13)]


@pytest.mark.parametrize("draw", range(len(DRAWS)))
def test_model_sum_is_np_add_at(draw):
    m, v = DRAWS[draw]
    for dtype in (np.float32, np.float64):
        f = cases.features(len(m), 5, dtype, draw)
        want = np.zeros((v, 5), dtype)
        np.add.at(want, m[m >= 0], f[m >= 0])
        got, arg = ref.pool(f, m, v, "sum")
        assert arg is None and got.dtype == dtype and ref.same_bits(got, want)
        cnt = np.bincount(m[m >= 0], minlength=v)
        mean = ref.pool(f, m, v, "mean")[0]
        assert ref.same_bits(mean[cnt > 0], (want[cnt > 0] / cnt[cnt > 0].astype(dtype)[:, None]).astype(dtype)) and np.all(mean[cnt == 0] == 0)


@pytest.mark.parametrize("draw", range(len(DRAWS)))
def test_model_extremes_are_torch_scatter_reduce(draw):
    """continuous values: no NaN, no tie -- where torch's operator and the model must name the same element"""
    m, v = DRAWS[draw]
    f = np.random.default_rng(draw).standard_normal((len(m), 4)).astype(np.float32)
    kept = torch.from_numpy(m[m >= 0])
    for red, name in (("max", "amax"), ("min", "amin")):
        want = torch.zeros(v, 4).scatter_reduce_(0, kept[:, None].expand(-1, 4), torch.from_numpy(f[m >= 0]), name, include_self=False)
        got, arg = ref.pool(f, m, v, red)
        assert ref.same_bits(got, want.numpy())
        has = arg[:, 0] >= 0
        assert np.array_equal(has, np.bincount(m[m >= 0], minlength=v) > 0)
        assert np.array_equal(np.take_along_axis(f, arg[has].astype(np.int64), 0), got[has]) and np.all(m[arg[has]] == np.nonzero(has)[0][:, None])


@pytest.mark.parametrize("draw", range(len(DRAWS)))
def test_model_backward_is_torch_autograd(draw):
    m, v = DRAWS[draw]
    f = torch.from_numpy(cases.features(len(m), 3, np.float64, draw)).requires_grad_()
    g = np.random.default_rng(draw + 50).standard_normal((v, 3))
    kept = torch.from_numpy(np.nonzero(m >= 0)[0])
    out = torch.zeros(v, 3, dtype=torch.float64).index_add_(0, torch.from_numpy(m[m >= 0]), f[kept])
    out.backward(torch.from_numpy(g))
    assert ref.same_bits(ref.backward(g, m, v, "sum"), f.grad.numpy())
    assert ref.same_bits(ref.unpool(g, m), f.grad.numpy())
    cnt = np.maximum(np.bincount(m[m >= 0], minlength=v), 1).astype(np.float64)
    assert ref.same_bits(ref.backward(g, m, v, "mean"), ref.backward(g / cnt[:, None], m, v, "sum"))
    # max: the gradient lands on the winner alone (continuous values: torch's amax agrees)
    x = torch.randn(len(m), 3, dtype=torch.float64, generator=torch.Generator().manual_seed(draw)).requires_grad_()
    o = torch.zeros(v, 3, dtype=torch.float64).scatter_reduce(0, torch.from_numpy(m[m >= 0])[:, None].expand(-1, 3), x[kept], "amax", include_self=False)
    o.backward(torch.from_numpy(g))
    arg = ref.pool(x.detach().numpy(), m, v, "max")[1]
    assert ref.same_bits(ref.backward(g, m, v, "max", arg), x.grad.numpy())


def test_index_definition():
    m = np.array([2, -1, 0, 2, 2, -1, 0, 4], np.int64)
    order, offsets = ref.index(m, 6)
    assert order.tolist() == [2, 6, 0, 3, 4, 7] and offsets.tolist() == [0, 2, 2, 5, 5, 6, 6] and order.dtype == np.int32


def test_special_values_in_the_model():
    f, m, v = cases.special_values(np.float32)
    mx, amx = ref.pool(f, m, v, "max")
    mn, _ = ref.pool(f, m, v, "min")
    first = [np.nonzero(m == j)[0] for j in range(v)]
    assert np.isnan(mx[:4, 0]).all() and np.isnan(mn[:4, 0]).all()
    assert amx[0, 0] == first[0][0] and amx[1, 0] == first[1][2] and amx[3, 0] == first[3][0]          # the FIRST NaN
    assert not np.signbit(mx[4, 0]) and np.signbit(mx[5, 0]) and amx[4, 0] == first[4][0]              # the earlier zero stays
    assert mx[6, 0] == np.inf and mn[6, 0] == -np.inf and amx[7, 0] == first[7][0] and mx[8, 0] == -np.inf
    assert mx[9, 0] == 0 and amx[9, 0] == -1


def test_host_side_validation_without_gpu():
    from d3d_amd.voxel import VoxelIndex, voxel_pool, voxel_unpool
    m = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6), m, 2)                               # not [K, C]
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6, 2, 2), m, 2)
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(5, 3), m, 2)                            # 5 rows, 6 ids
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6, 3, dtype=torch.int32), m, 2)         # integer features
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6, 3, dtype=torch.float16), m, 2)       # half precision is out of scope
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6, 3), m, 2, reduction="median")
    with pytest.raises(ValueError):
        voxel_pool(torch.zeros(6, 3), m)                               # a bare mapping needs num_voxels
    with pytest.raises(ValueError):
        voxel_unpool(torch.zeros(2), m)
    with pytest.raises(ValueError):
        VoxelIndex(torch.zeros(6, 1, dtype=torch.int64), 2)
    with pytest.raises(ValueError):
        VoxelIndex(torch.zeros(6), 2)                                  # float ids
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):          # no silent CPU fallback
            voxel_pool(torch.zeros(6, 3), m, 2, reduction="MAX")
        with pytest.raises(RuntimeError, match="HIP device"):
            voxel_unpool(np.zeros((2, 3), np.float32), m.numpy())
        with pytest.raises(RuntimeError, match="HIP device"):
            VoxelIndex(m, 2)


def test_index_workspace_query():
    from d3d_amd import _lib
    lib = _lib.load()
    sizes = (1, 1000, 10 ** 6, 2 * 10 ** 7)
    b = [[lib.d3d_voxel_index_workspace_bytes(k, v) for v in sizes] for k in sizes]
    for i in range(4):
        for j in range(4):
            assert b[i][j] > 0 and b[i][j] % 256 == 0
            assert (i == 0 or b[i][j] >= b[i - 1][j]) and (j == 0 or b[i][j] >= b[i][j - 1])
    assert b[3][0] > b[0][0] and b[0][3] > b[0][0]
    assert b[2][2] >= 10 ** 6 * (4 + 4)                                # at least the histogram and the keys
