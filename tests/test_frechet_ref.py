"""CPU tests of the Frechet-distance restatements (tests/frechet_ref.py) themselves: the sequential statistics against
numpy's own, the two fp64 routes of the distance against each other and against 60-digit arithmetic, and the measured
errors that the thresholds of tests/frechet_checks.py are derived from - a figure recorded there must still be an upper
bound of what numpy does here."""
import numpy as np
import pytest

from tests import frechet_checks as K
from tests import frechet_ref as R


def test_stats_are_mean_and_covariance():
    f1, _ = R.features(24, 67, 130)
    mu, cov = R.gaussian(f1)
    f64 = f1.astype(np.float64)
    assert np.allclose(mu, f64.mean(0), rtol=0, atol=1e-14)
    assert np.allclose(cov, np.cov(f64, rowvar=False), rtol=0, atol=1e-13)
    assert np.array_equal(cov, cov.T)
    total, cov_sum = R.stats(f1)
    again = R.accumulate(*R.accumulate(np.zeros(24), np.zeros((24, 24)), f1[:30]), f1[30:])
    assert np.array_equal(again[0], total) and np.array_equal(again[1], cov_sum)


def test_truth_of_known_spectra():
    assert np.array_equal(R.eigh_truth(np.diag([3.0, -1.0, 2.0])), [-1.0, 2.0, 3.0])
    assert np.allclose(R.eigh_truth(np.array([[2.0, 1.0], [1.0, 2.0]])), [1.0, 3.0], rtol=0, atol=1e-15)
    # two Gaussians with commuting covariances: sum_i (sqrt(a_i) - sqrt(b_i))^2 + |mu1 - mu2|^2
    a, b = np.array([4.0, 9.0, 0.0]), np.array([1.0, 16.0, 25.0])
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + 3.0
    args = (np.zeros(3), np.diag(a), np.ones(3), np.diag(b))
    for fn in (R.fid_truth, R.fid_symmetric, R.fid_eigvals):
        assert abs(fn(*args) - want) <= 1e-13, fn.__name__


@pytest.mark.parametrize("family", R.EIG_FAMILIES)
def test_eigvalsh_error_is_within_the_recorded_figure(family):
    worst = 0.0
    for d in K.EIG_SIZES:
        a = R.eig_matrix(family, d)
        assert np.array_equal(a, a.T)
        if d > R.MP_MAX_D:
            continue
        truth = K.eig_truth(family, d)
        worst = max(worst, float(np.abs(np.linalg.eigvalsh(a) - truth).max()) / (float(np.abs(truth).max()) or 1.0))
    print(f"{family}: numpy eigvalsh within {worst:.3e} of the truth (recorded {K.EIG_MEASURED[family]:.3e})")
    assert worst <= K.EIG_MEASURED[family]
    assert 8.0 * K.EIG_MEASURED[family] <= 1e-11
    spectrum = K.eig_truth("spread", 37)
    assert 0.99e6 < spectrum[-1] / spectrum[0] < 1.01e6  # the spread is what the family's name says
    assert np.sum(np.abs(K.eig_truth("rank_deficient", 37)) < 1e-12) == 37 - 17  # 18 samples: rank 17
    assert np.ptp(K.eig_truth("cluster", 37)) < 1e-9


@pytest.mark.parametrize("case", list(K.DIST_CASES) + [K.DIST_CASE_GPU[0]])
def test_routes_agree_within_the_recorded_figure(case):
    """The error of both fp64 routes against the truth (d <= 40), their disagreement above."""
    family = {**K.DIST_CASES, K.DIST_CASE_GPU[0]: K.DIST_CASE_GPU[1]}[case]
    d, n1, n2 = case
    assert (family == "deficient") == (min(n1, n2) - 1 < d)
    worst = 0.0
    for pair in ("ab", "ba") if d <= R.MP_MAX_D else ("ab",):
        truth, sym, eigvals = K.dist_reference(d, n1, n2, pair)
        if truth is not None:
            worst = max(worst, abs(sym - truth) / max(1.0, abs(truth)), abs(eigvals - truth) / max(1.0, abs(truth)))
        else:
            worst = max(worst, abs(sym - eigvals) / max(1.0, abs(sym)))
    print(f"{case} {family}: fp64 routes within {worst:.3e} (recorded {K.DIST_MEASURED[family]:.3e})")
    assert worst <= K.DIST_MEASURED[family]
    assert K.dist_threshold(family, d) <= K.DIST_CAP[family]


def test_front_end_refusals_need_no_device():
    from hairfastgan_amd import metrics as MT

    with pytest.raises(NotImplementedError, match="Inception"):
        MT.FrechetDistance(2048)
    with pytest.raises(TypeError):
        MT.FrechetDistance("clip")
    fid = MT.FrechetDistance(lambda x: x, reset_real_features=False, normalize=True)
    assert fid.to("cuda").eval() is fid and fid.state(True) is None
    with pytest.raises(RuntimeError, match="More than one sample"):
        fid.compute()
