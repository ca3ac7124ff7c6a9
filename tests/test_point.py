"""aligned_scatter ("next" row): CPU -- the C oracle against outputs of the REAL reference, and the fp64 model of
tests/point_reference.py against those outputs and against the oracle on every case of its grid; GPU -- the HIP kernels
against the goldens, the oracle and the reference's own test expectations (test/test_point.py).  The kernels' launch routes
at size are walked by tests/test_gpu_point.py."""
import os

import numpy as np
import pytest
import torch

import oracle
import point_reference as pr
from golden_io import GOLDEN

Z = np.load(os.path.join(GOLDEN, "point_ref_cases.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files if k.startswith("c")}, key=lambda s: int(s[1:]))


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference(name):
    coord, img, grad, at = Z[name + "/coord"], Z[name + "/img"], Z[name + "/grad"], int(Z[name + "/atype"][0])
    fwd = oracle.aligned_scatter_forward(coord, img, at)
    assert fwd.dtype == img.dtype and np.array_equal(fwd, Z[name + "/fwd"])
    # Backward: the reference's CPU wrapper builds its dispatch lambda but never calls it (scatter.cpp:196-206:
    # `_SCATTER_DISPATCH_DIM(...)` inside the AT_DISPATCH body is an unused expression), so the real reference
    # returns image_grad untouched -- recorded in the golden file.  The oracle restates the intended
    # aligned_scatter_backward_templated (scatter.cpp:143-180); it is pinned by the adjoint identity
    # <forward(img), g> == <img, backward(g)> (both maps are linear in img) and by the reference's own test
    # expectations (test_reference_test_expectations below).
    assert not np.any(Z[name + "/bwd"])
    bwd = oracle.aligned_scatter_backward(coord, grad, at, img.shape)
    lhs = float(np.sum(fwd.astype(np.float64) * grad.astype(np.float64)))
    rhs = float(np.sum(img.astype(np.float64) * bwd.astype(np.float64)))
    assert abs(lhs - rhs) <= (1e-4 if img.dtype == np.float32 else 1e-10) * abs(lhs)


def test_oracle_rejects_unsupported():
    img = np.zeros((1, 2, 3, 3), np.float32)
    with pytest.raises(ValueError):
        oracle.aligned_scatter_forward(np.zeros((1, 3), np.float32), img, "max")
    with pytest.raises(ValueError):
        oracle.aligned_scatter_forward(np.zeros((1, 5), np.float32), np.zeros((1, 2, 2, 2, 2, 2), np.float32), "mean")


@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference_forward(name):
    """The model against what the real reference recorded: 2^(dim+2) roundings of the map's dtype on sum |term| -- plus the
    absolute part of the weights' error (point_reference's docstring: 1 + x rounds to the spacing of 1 + x, not of the
    weight).  Without that part the reference's own outputs miss the count: c1 by 5.7 x (14 elements), c3 by 1.8 x,
    c11 (fp64) by 1.6 x; with it the worst case stands at 0.72 of the bound."""
    coord, img, at = Z[name + "/coord"], Z[name + "/img"], int(Z[name + "/atype"][0])
    dim, u = coord.shape[1] - 1, pr.unit(img.dtype)
    out, S, E = pr.forward_terms(coord, img, at, u)
    err = np.abs(Z[name + "/fwd"].astype(np.float64) - out)
    bound = (1 << (dim + 2)) * u * S + E
    print(name, "worst error / bound %.3f" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert out.shape == Z[name + "/fwd"].shape and np.all(err <= bound)


GRID = pr.grid()


def test_grid_covers_what_it_claims():
    assert {c.C for c in GRID} == set(pr.CHANNELS) and {c.dims for c in GRID} == set(pr.MAPS)
    assert {(c.atype, c.dtype.name) for c in GRID} == {(a, d) for a in (1, 2) for d in ("float32", "float64")}
    for C in pr.CHANNELS:
        assert {c.dims for c in GRID if c.C == C} == set(pr.MAPS)
    assert {c.B for c in GRID} == {1, 2, 3} and {0, 1, 70001, 200000} <= {c.n for c in GRID}
    assert {255, 256, 257} <= {c.n * c.C for c in GRID}
    assert {c.dims for c in GRID if c.n == 200000} == {(40, 50), (7, 11, 13)}
    for route in (lambda c: c.C < 8, lambda c: c.C >= 8):            # each route: methods x dtypes, started and zero image_grad
        assert len({(c.atype, c.dtype.name, c.init) for c in GRID if route(c)}) == 8
        assert any(c.hot for c in GRID if route(c))


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_model_matches_oracle(case):
    """What makes the model fit to judge a kernel: on every case of the GPU grid it agrees with the C oracle (one particular
    order of the sums) within the bounds the kernels are held to, and an fp32 case keeps K <= K_CAP, so that
    (K + 3 dim + 4) u < 2^-12 and an error of 2^-10 of an element's mass cannot pass."""
    coord, image, grad, _ = case.make()
    if case.n >= case.B:
        assert set(coord[:, 0].astype(int)) == set(range(case.B))
    out, S, E = pr.forward_terms(coord, image, case.atype, case.u)
    got = oracle.aligned_scatter_forward(coord, image, case.atype)
    assert got.dtype == case.dtype and np.all(np.abs(got - out) <= pr.forward_bound(S, case.dim, case.u, E))
    exact, K, A, E = pr.backward_terms(coord, grad, case.atype, case.shape, None, case.u)
    if case.dtype == np.float32:
        assert K.max() <= pr.K_CAP
    if case.hot:
        assert K.max() >= case.hot << case.dim
    got = oracle.aligned_scatter_backward(coord, grad, case.atype, case.shape)
    assert got.dtype == case.dtype and np.all(np.abs(got - exact) <= pr.backward_bound(K, A, case.dim, case.u, E))


def test_model_definition_by_hand():
    """the quirks the model must keep, on values one can check by hand"""
    img = np.arange(2 * 1 * 4, dtype=np.float64).reshape(2, 1, 4)               # map b: 4 b + cell
    coord = np.array([[0, 1.25], [1, 2.0], [0, 0.0], [0, -0.0], [1, 3.0], [0, 3.5], [1, -7.0], [0, 1e9]])
    lin = pr.forward(coord, img, pr.LINEAR)[:, 0]
    assert np.array_equal(lin, [1.25, 2 * 6.0, 0.0, 0.0, 2 * 7.0, 0.5 * 3 + 0.5 * 3, 0.5 * 4 + 0.5 * 4, 3.0])
    mean = pr.forward(coord, img, pr.MEAN)[:, 0]
    assert np.array_equal(mean, [1.5, 6.0, 0.0, 0.0, 7.0, 3.0, 4.0, 3.0])
    g = np.array([[1.0], [-2.0], [4.0], [8.0], [16.0], [32.0], [64.0], [128.0]])
    init = np.full((2, 1, 4), 0.5)
    exact, K, A = pr.backward(coord, g, pr.LINEAR, img.shape, init)
    assert np.array_equal(exact[0, 0], [0.5 + 2 * 4 + 2 * 8, 0.5 + 0.75, 0.5 + 0.25, 0.5 + 32 + 128])
    assert np.array_equal(exact[1, 0], [0.5 + 64, 0.5, 0.5 - 4, 0.5 + 32])
    assert np.array_equal(K[0, 0], [4, 1, 1, 4]) and np.array_equal(K[1, 0], [2, 0, 2, 2])
    assert np.array_equal(A[1, 0], [0.5 + 64, 0.5, 0.5 + 4, 0.5 + 32])
    flat, tot, Ks, As, _ = pr.backward_sparse(coord, g, pr.LINEAR, img.shape)
    dense = np.zeros(8)
    dense[flat] = tot
    assert np.array_equal(dense.reshape(2, 1, 4), exact - init) and np.array_equal(Ks, K.ravel()[flat])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_matches_reference(name):
    from d3d_amd.point import AlignType, aligned_scatter_backward, aligned_scatter_forward
    coord, img, grad, at = Z[name + "/coord"], Z[name + "/img"], Z[name + "/grad"], int(Z[name + "/atype"][0])
    c, f, g = torch.from_numpy(coord).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(grad).cuda()
    fwd = aligned_scatter_forward(c, f, AlignType(at)).cpu().numpy()
    assert np.array_equal(fwd, Z[name + "/fwd"])          # same accumulation order -> bit-exact
    ig = torch.zeros_like(f)
    aligned_scatter_backward(c, g, AlignType(at), ig)
    tol = 1e-5 if img.dtype == np.float32 else 1e-12       # atomic accumulation order
    np.testing.assert_allclose(ig.cpu().numpy(), oracle.aligned_scatter_backward(coord, grad, at, img.shape),
                               rtol=tol, atol=tol)


@pytest.mark.gpu
@pytest.mark.parametrize("cuda", [True, False])
def test_reference_test_expectations(cuda):
    """reference test/test_point.py:10-60 (drop / mean / linear forward values and gradients)"""
    from d3d_amd.point import aligned_scatter
    coord = torch.tensor([[0, 0.25, 0.25, 0.25], [0, 1.25, 1.25, 1.25], [1, 2.25, 2.25, 2.25]])
    image_feat = torch.rand(2, 10, 3, 3, 3)
    if cuda:
        coord, image_feat = coord.cuda(), image_feat.cuda()
    image_feat.requires_grad = True
    indexing = lambda ic: (ic[:, 0], slice(None)) + tuple(ic[:, i] for i in range(1, coord.shape[1]))  # noqa: E731
    lcoords = torch.tensor(np.array(np.meshgrid([0, 1], [0, 1], [0, 1])).T.reshape(-1, 3)).to(coord.device)
    full = lambda v: torch.full([10], float(v), device=coord.device)  # noqa: E731
    pfeat = aligned_scatter(coord, image_feat, "drop")
    assert torch.allclose(pfeat, image_feat[indexing(coord.long())])
    pfeat = aligned_scatter(coord, image_feat, "mean")
    ic = torch.cat([torch.zeros((8, 1), dtype=torch.long, device=coord.device), lcoords], 1)
    assert torch.allclose(pfeat[0], torch.mean(image_feat[indexing(ic)], 0))
    ic = torch.cat([torch.zeros((8, 1), dtype=torch.long, device=coord.device), lcoords + 1], 1)
    assert torch.allclose(pfeat[1], torch.mean(image_feat[indexing(ic)], 0))
    assert torch.allclose(pfeat[2], image_feat[1, :, 2, 2, 2])
    pfeat.sum().backward()
    assert torch.allclose(image_feat.grad[0, :, 0, 0, 0], full(1 / 8))
    assert torch.allclose(image_feat.grad[0, :, 1, 1, 1], full(1 / 4))
    assert torch.allclose(image_feat.grad[1, :, 2, 2, 2], full(1))
    image_feat.grad.zero_()
    pfeat = aligned_scatter(coord, image_feat, "linear")
    wmap = torch.tensor([0.25 ** i * 0.75 ** (3 - i) for i in range(4)], device=coord.device)
    lweight = wmap[torch.sum(lcoords, 1).long()]
    ic = torch.cat([torch.zeros((8, 1), dtype=torch.long, device=coord.device), lcoords], 1)
    assert torch.allclose(pfeat[0], torch.sum(image_feat[indexing(ic)] * lweight.unsqueeze(1), 0))
    assert torch.allclose(pfeat[2], image_feat[1, :, 2, 2, 2])
    pfeat.sum().backward()
    assert torch.allclose(image_feat.grad[0, :, 0, 0, 0], full(.75 ** 3))
    assert torch.allclose(image_feat.grad[0, :, 1, 1, 1], full(.75 ** 3 + .25 ** 3))
    assert torch.allclose(image_feat.grad[1, :, 2, 2, 2], full(1))
    with pytest.raises(ValueError):
        aligned_scatter(coord, image_feat, "max")


@pytest.mark.gpu
def test_large_vs_oracle():
    from d3d_amd.point import AlignType, aligned_scatter_forward
    rng = np.random.default_rng(5)
    img = rng.random((2, 64, 40, 50)).astype(np.float32)
    coord = np.concatenate([rng.integers(0, 2, (200000, 1)), rng.random((200000, 2)) * [41, 51] - 0.5], 1).astype(np.float32)
    got = aligned_scatter_forward(torch.from_numpy(coord).cuda(), torch.from_numpy(img).cuda(), AlignType.LINEAR).cpu().numpy()
    assert np.array_equal(got, oracle.aligned_scatter_forward(coord, img, "linear"))
