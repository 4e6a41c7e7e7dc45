"""CPU tests of the Poisson blending restatement (tests/poisson_ref.py): hand-worked equation systems, the quantiser
against torch's save_image arithmetic, and convergence of the Jacobi sweeps to the direct solution."""
import numpy as np
import torch

from tests import poisson_ref as R


def test_setup_3x3_region_in_5x5():
    s = np.zeros((1, 5, 5), np.uint8)
    s[0, 2, 2] = 8
    t = np.full((1, 5, 5), 10, np.uint8)
    mask = np.zeros((5, 5), np.uint8)
    mask[1:4, 1:4] = 255
    b, x0 = R.setup(s, t, mask)
    # centre: four source gradients 8 - 0; corners: no gradient, two target pixels outside the region (2 x 10);
    # edge centres: the gradient towards the centre (0 - 8) and one target pixel outside (10)
    want = np.array([[20, 2, 20], [2, 32, 2], [20, 2, 20]], np.float32)
    assert np.array_equal(b[0, 1:4, 1:4], want)
    assert np.count_nonzero(b) == 9 and np.array_equal(x0[0, 1:4, 1:4], np.full((3, 3), 10, np.float32))
    assert np.count_nonzero(x0) == 9


def test_gradient_tie_keeps_source():
    s = np.zeros((1, 3, 3), np.uint8)
    s[0, 1, 1] = 3                               # source gradient +3 towards every neighbour
    t = np.full((1, 3, 3), 3, np.uint8)
    t[0, 1, 1] = 0                               # target gradient -3: same magnitude
    b, _ = R.setup(s, t, np.full((3, 3), 255, np.uint8))
    assert b[0, 1, 1] == 4 * 3 + 4 * 3           # source gradients + the four target pixels outside the region
    t2 = t.copy()
    t2[0, 1, 1] = 7                              # target gradient +4, larger than the source's +3: the target's wins
    b2, _ = R.setup(s, t2, np.full((3, 3), 255, np.uint8))
    assert b2[0, 1, 1] == 4 * 4 + 4 * 3


def test_border_pixels_excluded():
    mask = np.full((4, 5), 255, np.uint8)
    om = R.omega(mask)
    assert om.sum() == 2 * 3 and om[1:3, 1:4].all()
    assert not R.omega(np.full((4, 5), 127, np.uint8)).any()
    assert R.omega(np.full((4, 5), 128, np.uint8)).sum() == 6
    rng = np.random.default_rng(0)
    s, t = rng.integers(0, 256, (2, 3, 4, 5), dtype=np.uint8)
    out, _ = R.solve(s, t, mask, 50)
    assert np.array_equal(out[:, 0], t[:, 0]) and np.array_equal(out[:, :, 0], t[:, :, 0])
    assert np.array_equal(out[:, -1], t[:, -1]) and np.array_equal(out[:, :, -1], t[:, :, -1])


def test_zero_sweeps_and_empty_region_return_target():
    rng = np.random.default_rng(1)
    s, t = rng.integers(0, 256, (2, 3, 9, 11), dtype=np.uint8)
    mask = np.zeros((9, 11), np.uint8)
    mask[2:7, 3:9] = 255
    out, x = R.solve(s, t, mask, 0)
    assert np.array_equal(out, t)
    out, x = R.solve(s, t, np.zeros((9, 11), np.uint8), 40)
    assert np.array_equal(out, t) and not x.any()


def test_quantize_matches_save_image_arithmetic():
    k = np.arange(256, dtype=np.float32)
    x = np.concatenate([k / 255, (k + 0.5) / 255, np.nextafter(k / 255, 2), np.nextafter((k + 0.5) / 255, -2),
                        np.array([-1.0, -1e-7, 0.0, 1.0, 1.0 + 1e-6, 3.0], np.float32),
                        np.random.default_rng(2).random(10000, dtype=np.float32) * 1.2 - 0.1]).astype(np.float32)
    want = torch.from_numpy(x).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()   # torchvision.utils.save_image
    assert np.array_equal(R.quantize(x), want)


def test_jacobi_converges_to_direct_solve():
    from scipy.sparse import lil_matrix
    from scipy.sparse.linalg import spsolve

    rng = np.random.default_rng(3)
    H, W = 24, 20
    s, t = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    mask = np.where((yy - 11) ** 2 / 64 + (xx - 9) ** 2 / 40 <= 1, 255, 0).astype(np.uint8)
    mask[0, :] = 255                             # touches the border: those pixels stay outside Omega
    b, x0 = R.setup(s, t, mask)
    x = R.jacobi(b, x0, mask, 20000)
    om = R.omega(mask)
    pts = list(zip(*np.nonzero(om)))
    index = {p: i for i, p in enumerate(pts)}
    A = lil_matrix((len(pts), len(pts)))
    for i, (y, x_) in enumerate(pts):
        A[i, i] = 4.0
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            j = index.get((y + dy, x_ + dx))
            if j is not None:
                A[i, j] = -1.0
    A = A.tocsr()
    for c in range(3):
        direct = spsolve(A, b[c][om].astype(np.float64))
        assert np.abs(x[c][om] - direct).max() <= 1e-3
    assert not x[:, ~om].any()
