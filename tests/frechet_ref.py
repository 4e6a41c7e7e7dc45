"""TEST INFRASTRUCTURE - numpy and mpmath restatements of the Frechet distance (hairfastgan_amd.metrics, csrc/frechet.h):
the streaming statistics as the sequential fp64 loops the kernel must reproduce bit for bit, the distance by the
reference's formula (torchmetrics' _compute_fid as scripts/fid_metric.py uses it: eigvals of the non-symmetric product) and
by the symmetric route the device takes, and both in 60-digit arithmetic (mpmath) as the truth for d <= 40."""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MP_DIGITS = 60
MP_MAX_D = 40


# ---- inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def features(d, n1, n2, seed=0):
    """Two fp32 feature sets of a seeded generator: f1 [n1,d] correlated, f2 [n2,d] with a scale ramp over the features."""
    rng = np.random.default_rng(7000 + 131 * d + 17 * n1 + n2 + seed)
    w = rng.standard_normal((d, d)) / np.sqrt(d)
    f1 = rng.standard_normal((n1, d)) @ w + 0.3
    f2 = rng.standard_normal((n2, d)) * np.linspace(0.2, 2.0, d) + 0.1 * rng.standard_normal(d)
    f1, f2 = f1.astype(np.float32), f2.astype(np.float32)
    f1.setflags(write=False)
    f2.setflags(write=False)
    return f1, f2


EIG_FAMILIES = ("diagonal", "spread", "rank_deficient", "cluster", "zero_row")


@functools.lru_cache(maxsize=None)
def eig_matrix(family, d):
    """A symmetric fp64 test matrix [d,d] (read-only)."""
    rng = np.random.default_rng(9000 + 31 * d + EIG_FAMILIES.index(family))
    q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    if family == "diagonal":  # no rotation is taken
        a = np.diag(rng.uniform(0.5, 2.0, d))
    elif family in ("spread", "zero_row"):  # Q diag(lambda) Q^T, lambda over six decades
        a = (q * np.logspace(-3.0, 3.0, d)) @ q.T
        if family == "zero_row":
            a[d // 2, :] = 0.0
            a[:, d // 2] = 0.0
    elif family == "rank_deficient":  # a covariance of fewer samples than features (d >= 2)
        f = rng.standard_normal((max(2, d // 2), d))
        a = np.cov(f, rowvar=False).reshape(d, d)
    elif family == "cluster":  # c I plus eigenvalues 1e-9 apart
        a = (q * (3.0 + 1e-9 * rng.uniform(0.0, 1.0, d))) @ q.T
    else:
        raise KeyError(family)
    a = 0.5 * (a + a.T)
    a.setflags(write=False)
    return a


# ---- statistics ---------------------------------------------------------------------------------------------------
def accumulate(total, cov_sum, f):
    """total += sum_n f[n], cov_sum += sum_n outer(f[n], f[n]): fp64, one sample after the other (in place)."""
    f64 = f.astype(np.float64)
    for row in f64:
        total += row
        cov_sum += np.outer(row, row)
    return total, cov_sum


def stats(f):
    """-> (sum [d], cov_sum [d,d]) of the sequential fp64 loops."""
    d = f.shape[1]
    return accumulate(np.zeros(d), np.zeros((d, d)), f)


def moments(total, cov_sum, n):
    """-> (mu, cov) = (sum / n, (cov_sum - n (mu_i mu_j)) / (n - 1)), every operation rounded once."""
    mu = total / n
    return mu, (cov_sum - n * np.outer(mu, mu)) / (n - 1.0)


def gaussian(f):
    return moments(*stats(f), f.shape[0])


# ---- the distance in fp64 -----------------------------------------------------------------------------------------
def _head(mu1, s1, mu2, s2):
    return float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2))


def fid_eigvals(mu1, s1, mu2, s2):
    """The reference's route: a + b - 2 c with c = eigvals(s1 @ s2).sqrt().real.sum()."""
    ev = np.linalg.eigvals(s1 @ s2).astype(np.complex128)
    return _head(mu1, s1, mu2, s2) - 2.0 * float(np.sqrt(ev).real.sum())


def fid_symmetric(mu1, s1, mu2, s2):
    """The device's route: eigh, congruence, eigvalsh."""
    w, v = np.linalg.eigh(s1)
    b = np.sqrt(np.maximum(w, 0.0))[:, None] * v.T
    m = b @ s2 @ b.T
    ev = np.linalg.eigvalsh(0.5 * (m + m.T))
    return _head(mu1, s1, mu2, s2) - 2.0 * float(np.sqrt(np.maximum(ev, 0.0)).sum())


# ---- the truth (mpmath) -------------------------------------------------------------------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = MP_DIGITS
    return mpmath


def eigh_truth(a):
    """Ascending eigenvalues of the symmetric fp64 matrix `a` taken as exact, in 60-digit arithmetic, rounded to fp64."""
    mp = _mp()
    d = a.shape[0]
    assert d <= MP_MAX_D
    e = mp.eigsy(mp.matrix(a.tolist()), eigvals_only=True)
    return np.array(sorted(float(e[i]) for i in range(d)))


def fid_truth(mu1, s1, mu2, s2):
    """The distance of the fp64 statistics taken as exact, in 60-digit arithmetic (the symmetric route: there every
    eigenvalue is real)."""
    mp = _mp()
    d = len(mu1)
    assert d <= MP_MAX_D
    m1, m2 = mp.matrix(s1.tolist()), mp.matrix(s2.tolist())
    w, v = mp.eigsy(m1)
    b = mp.matrix(d, d)
    for i in range(d):
        r = mp.sqrt(w[i]) if w[i] > 0 else mp.mpf(0)
        for k in range(d):
            b[i, k] = r * v[k, i]
    m = b * m2 * b.T
    ev = mp.eigsy((m + m.T) / 2, eigvals_only=True)
    roots = mp.fsum(mp.sqrt(ev[i]) for i in range(d) if ev[i] > 0)
    head = mp.fsum((mp.mpf(float(x)) - mp.mpf(float(y))) ** 2 for x, y in zip(mu1, mu2))
    head += mp.fsum(m1[i, i] + m2[i, i] for i in range(d))
    return float(head - 2 * roots)
