"""TEST INFRASTRUCTURE - two independent fp64 restatements of SSIM (csrc/ssim.h, hairfastgan_amd.ssim), written from the
formulas of the metric (Wang et al. 2004; skimage.metrics.structural_similarity, which is not installed here):

  scipy form    skimage's own steps: scipy.ndimage filters over the WHOLE image (uniform_filter(size=7), gaussian_filter(sigma=
                1.5, truncate=3.5, mode="reflect"); any other window: correlate1d along both axes), the formula, then the crop
                by (win - 1) // 2 - what skimage averages
  conv form     a separable torch.conv2d over the valid region only, in the dtype asked for: float64 is the truth, float32 the
                evaluation the device must beat.  It also gives the map, cs, the masked mean and MS-SSIM (F.avg_pool2d(., 2)
                between the scales)

Both use the expression order of include/hairfast_hip.h.  `ssim_floor`: the first-order rounding bound of the formula in fp64.
"""
import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

U64 = 2.0 ** -53  # unit roundoff of fp64
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(kind, win=None, sigma=1.5):
    """-> (taps float64 numpy, cn): "uniform" (7, sample covariance), "gaussian" (11, population covariance) or a sequence of taps (cn 1)."""
    if isinstance(kind, str) and kind == "uniform":
        win = 7 if win is None else win
        return np.full(win, 1.0 / win), win * win / (win * win - 1.0)
    if isinstance(kind, str) and kind == "gaussian":
        r = int(3.5 * sigma + 0.5) if win is None else win // 2
        g = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
        return g / g.sum(), 1.0
    return np.asarray(kind, dtype=np.float64), 1.0


def constants(data_range, K1=0.01, K2=0.03):
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


def _formula(ux, uy, uxx, uyy, uxy, c1, c2, cn):
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
    b1, b2 = ux * ux + uy * uy + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2), a2 / b2


# ---- scipy form ---------------------------------------------------------------------------------------------------
def scipy_maps(x, y, kind, data_range, cn=None):
    """x, y [P,H,W] numpy (any real dtype) -> (S, cs) float64 [P,oh,ow]: filters over the whole plane, then the crop."""
    taps, cn0 = window(kind)
    cn = cn0 if cn is None else cn
    win = len(taps)
    if isinstance(kind, str) and kind == "uniform":
        f = lambda z: ndimage.uniform_filter(z, size=win)  # noqa: E731
    elif isinstance(kind, str) and kind == "gaussian":
        f = lambda z: ndimage.gaussian_filter(z, sigma=1.5, truncate=3.5, mode="reflect")  # noqa: E731
    else:
        f = lambda z: ndimage.correlate1d(ndimage.correlate1d(z, taps, axis=1, mode="reflect"), taps, axis=0, mode="reflect")  # noqa: E731
    c1, c2 = constants(data_range)
    p = (win - 1) // 2
    s_out, cs_out = [], []
    for a, b in zip(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)):
        s, cs = _formula(f(a), f(b), f(a * a), f(b * b), f(a * b), c1, c2, cn)
        h, w = a.shape
        s_out.append(s[p:h - p, p:w - p])
        cs_out.append(cs[p:h - p, p:w - p])
    return np.stack(s_out), np.stack(cs_out)


# ---- conv form ----------------------------------------------------------------------------------------------------
def moments(x, y, taps, dtype=torch.float64):
    """x, y [P,H,W] tensors -> the five window moments [P,oh,ow] in `dtype` (row pass, then column pass; a correlation)."""
    w = torch.as_tensor(np.asarray(taps), dtype=dtype)
    x, y = x.to(dtype)[:, None], y.to(dtype)[:, None]
    f = lambda z: F.conv2d(F.conv2d(z, w.view(1, 1, 1, -1)), w.view(1, 1, -1, 1))[:, 0]  # noqa: E731
    return f(x), f(y), f(x * x), f(y * y), f(x * y)


def conv_maps(x, y, kind, data_range, cn=None, dtype=torch.float64):
    """-> (S, cs) [P,oh,ow] in `dtype`."""
    taps, cn0 = window(kind)
    c1, c2 = constants(data_range)
    return _formula(*moments(x, y, taps, dtype), c1, c2, cn0 if cn is None else cn)


def ssim_floor(x, y, kind, data_range, cn=None):
    """(floor of S, floor of cs) float64 [P,oh,ow]: a first-order bound of the rounding error of ANY fp64 evaluation of the
    formula whose window sums run over win x win terms in two passes, from the operation count, on the fp64 values of the
    case.  With u = 2^-53:
      a window moment f(z) is two passes of win products and win - 1 additions, and z = x x is a product itself: |df(z)| <=
      g f(|z|), g = (2 win + 2) u.  With ax = f(|x|): ax^2 <= uxx (the taps are non-negative and sum to 1), |ux| <= ax, and
      f(|x y|) <= (uxx + uyy) / 2.
      vx = cn (uxx - ux ux): |dvx| <= cn (g uxx + 2 |ux| g ax + u ux^2 + u |uxx - ux^2|) + u |vx| <= cn (3 g + 3 u) uxx; vy alike;
      |dvxy| <= cn (3 g + 3 u) (uxx + uyy) / 2.  With E = cn (3 g + 3 u) (uxx + uyy):
      a2 = 2 vxy + C2 and b2 = vx + vy + C2 carry E + 2 u b2 at most (|a2| <= b2), so cs = a2 / b2 carries 2 E / b2 + 4 u;
      a1 = 2 ux uy + C1 and b1 = ux^2 + uy^2 + C1 carry 2 g (uxx + uyy) + 3 u b1, so l = a1 / b1 (|l| <= 1) carries
      4 g (uxx + uyy) / b1 + 7 u;  S = l cs (three more roundings): |dS| <= 2 E / b2 + 4 g (uxx + uyy) / b1 + 14 u.
    The bound scales with (uxx + uyy) / (vx + vy + C2): with uxx + uyy up to 1.3e5 over b2 of 1e2 to 1e4 it is 2e-14 to 1e-12 on
    the plane means of 8-bit images (8e-12 on constant planes, where b2 = C2), and 1e-7 where the mean is a thousand times the
    spread.  Sums over pixels are not included (the factor on the restatements' disagreement covers them)."""
    taps, cn0 = window(kind)
    cn = cn0 if cn is None else cn
    c1, c2 = constants(data_range)
    ux, uy, uxx, uyy, uxy = moments(x, y, taps)
    g = (2 * len(taps) + 2) * U64
    e = cn * (3 * g + 3 * U64) * (uxx + uyy)
    b1 = ux * ux + uy * uy + c1
    b2 = cn * (uxx - ux * ux) + cn * (uyy - uy * uy) + c2
    cs_floor = 2 * e / b2 + 4 * U64
    return cs_floor + 4 * g * (uxx + uyy) / b1 + 10 * U64, cs_floor


def masked_mean(s_map, mask):
    """s_map [N,C,oh,ow], mask [N,oh,ow] -> [N]: sum(m S) / sum(m) per channel, then the mean over channels."""
    m = mask.double()[:, None]
    return ((s_map * m).sum((2, 3)) / m.sum((2, 3))).mean(1)


def ssim(x, y, kind, data_range, cn=None, dtype=torch.float64):
    """x, y [N,C,H,W] -> [N] float64: the mean of S per channel, then over channels."""
    n, c, h, w = x.shape
    s, _ = conv_maps(x.reshape(n * c, h, w), y.reshape(n * c, h, w), kind, data_range, cn, dtype)
    return s.double().mean((1, 2)).reshape(n, c).mean(1)


def ms_ssim(x, y, kind, data_range, weights=MS_WEIGHTS, dtype=torch.float64):
    """x, y [N,C,H,W] -> [N] float64: prod_j max(cs_j, 0)^w_j max(ssim_M, 0)^w_M per channel, the mean over channels."""
    n, c, h, w = x.shape
    x, y = x.reshape(n * c, 1, h, w).to(dtype), y.reshape(n * c, 1, h, w).to(dtype)
    vals = []
    for j, wt in enumerate(weights):
        s, cs = conv_maps(x[:, 0], y[:, 0], kind, data_range, None, dtype)
        v = s if j == len(weights) - 1 else cs
        vals.append(v.double().mean((1, 2)).clamp_min(0) ** wt)
        x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return torch.stack(vals).prod(0).reshape(n, c).mean(1)
