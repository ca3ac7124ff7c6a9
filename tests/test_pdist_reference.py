"""The fp64 model of the point-to-box distance (tests/pdist_reference.py) and the compiled oracle (oracle.pdist2dr) guard
each other, without a GPU: the closed form in the box frame against the reference's per-edge loop, on the inputs that
tests/test_gpu_pdist.py gives the kernels."""
import numpy as np
import pytest

import oracle
import pdist_reference as ref


@pytest.mark.parametrize("offset", ref.OFFSETS)
def test_model_agrees_with_the_oracle(offset):
    shares = []
    for n, m in ref.FORWARD_SHAPES:
        pts, boxes = ref.scene(n, m, ref.seed_of(n, m), offset)
        dref, eref = oracle.pdist2dr(pts, boxes)
        err = np.abs(ref.signed_distance(pts, boxes) - dref)
        assert err.max() <= 1e-12, (n, m, err.max())
        feat, decided, accept = ref.features(pts, boxes)
        assert np.array_equal(feat[decided], eref[decided]), (n, m)
        assert ref.feature_ok(eref, feat, decided, accept).all(), (n, m)
        assert np.array_equal((dref > 0)[decided], (ref.signed_distance(pts, boxes) > 0)[decided])
        shares.append(1 - decided.mean())
        assert shares[-1] <= 0.01, (n, m, shares[-1])
    n, m = ref.FORWARD_SHAPES[-1]
    inside = (ref.signed_distance(*ref.scene(n, m, ref.seed_of(n, m), offset)) > 0).any(0).mean()
    assert inside > 0.5                                         # points inside some box: the planted third, and of the others


def test_scene_uses_the_box_generator_of_the_loss_tests():
    from test_gpu_boxloss import _rand_boxes
    pts, boxes = ref.scene(301, 40, 5)
    assert np.array_equal(boxes, _rand_boxes(40, 5, 8.0))
    assert pts.shape == (301, 2) and np.abs(pts).max() <= 6 + 0.55 * 5.1 * 2


@pytest.mark.parametrize("offset", ref.OFFSETS)
def test_grad_reference_against_central_differences_of_the_oracle(offset):
    n, m = 257, 65
    pts, boxes, g, share = ref.backward_case(n, m, offset, "dense", np.float64)
    assert share <= 0.01
    gp, gb, sp, sb = ref.grad_reference(pts, boxes, g)
    assert sp.shape == (n, 1) and (sp >= np.abs(gp)).all() and (sb >= np.abs(gb)).all()
    h = 1e-6

    def loss(p, b):
        return float((oracle.pdist2dr(p, b)[0] * g).sum())
    for i in range(0, m, 9):
        for k in range(5):
            a, c = boxes.copy(), boxes.copy()
            a[i, k] += h
            c[i, k] -= h
            fd = (loss(pts, a) - loss(pts, c)) / (2 * h)
            assert abs(fd - gb[i, k]) < 1e-6 * max(1.0, sb[i, k]), (i, k, fd, gb[i, k])
    for j in range(0, n, 37):
        for k in range(2):
            a, c = pts.copy(), pts.copy()
            a[j, k] += h
            c[j, k] -= h
            fd = (loss(a, boxes) - loss(c, boxes)) / (2 * h)
            assert abs(fd - gp[j, k]) < 1e-6 * max(1.0, sp[j, 0]), (j, k, fd, gp[j, k])


def test_weights_and_exclusions():
    for n, m in ref.BACKWARD_SHAPES:
        for offset in ref.OFFSETS:
            for dtype in (np.float32, np.float64):
                shares = [ref.backward_case(n, m, offset, kind, dtype)[3] for kind in ref.WEIGHT_KINDS]
                assert max(shares) <= 0.01, (n, m, offset, shares)
    _, _, g, _ = ref.backward_case(700, 90, 0.0, "zero_row_col", np.float64)
    assert not g[45].any() and not g[:, 233].any() and np.count_nonzero(g) > 0.9 * g.size
    _, _, g, _ = ref.backward_case(700, 90, 0.0, "sparse", np.float64)
    assert 0.005 < np.count_nonzero(g) / g.size < 0.015
    assert not ref.backward_case(700, 90, 0.0, "zero", np.float64)[2].any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_3d_model_on_hand_made_points(axis):
    # the box of test_pdist_forward_backward, its axes permuted: inside the smallest gap to the six faces
    p3 = np.array([[0.5, 0.2, 0.1], [1.9, 0, 0], [3.0, 0, 0], [0, 0, 2.0], [3, 0, 3]])
    pts = np.empty_like(p3)
    dims = np.empty(3)
    ctr = np.zeros(3)
    src_dims = np.array([4.0, 2.0, 2.0])
    planar = [k for k in range(3) if k != axis]
    pts[:, planar[0]], pts[:, planar[1]], pts[:, axis] = p3[:, 0], p3[:, 1], p3[:, 2]
    dims[planar[0]], dims[planar[1]], dims[axis] = src_dims
    box = np.concatenate([ctr, dims, [0.0]])[None]
    got = ref.signed_distance3(pts, box, axis)[0]
    assert np.allclose(got, [0.8, 0.1, -1.0, -1.0, -np.sqrt(1 + 4)], atol=1e-12)
