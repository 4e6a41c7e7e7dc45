"""SSIM and MS-SSIM on the device: structural similarity of a result and a target image (losses/lpips/__init__.py:52-53
`dssim`, losses/lpips/networks_basic.py:167 `DSSIM`, selected by dist_model.py:80 model='SSIM'; the same code in
losses/masked_lpips and models/FeatureStyleEncoder/lpips).  There it is scikit-image on the host, one image at a time after a
device -> host copy; here one fused fp64 launch per call (hf_ssim_planes_f64, csrc/ssim.h) over the whole batch.

    python -m hairfastgan_amd.lpips --mode ssim|ms_ssim [--ssim_window gaussian|uniform] --data_path DIR --gt_path DIR

Conventions (INTEGRATION.md names the library call each corresponds to):
  window="gaussian"   taps exp(-(k / sigma)^2 / 2), normalised; win_size 2 int(3.5 sigma + 0.5) + 1 = 11; population
                      covariance (cn = 1): Wang et al. 2004, skimage's gaussian_weights=True, use_sample_covariance=False
  window="uniform"    win_size 7, sample covariance (cn = win^2 / (win^2 - 1)): skimage's default, what `dssim` calls
The window is applied over the valid region only (no padding): an image [H,W] gives a map [H - win + 1, W - win + 1], which
is skimage's map cropped by (win - 1) / 2 on each side - the region skimage averages.
The window moments, the formula and every sum are fp64: the variances are E[x^2] - E[x]^2 next to C2 = (0.03 R)^2, and an
fp32 evaluation is off by up to 1.6e-6 on the image mean and by more on flat regions.  Gradients, windows above 11, the Lab
colour-space branch of `DSSIM` and a mask for MS-SSIM are not part of this backend.

`lib=None`: the loaded HIP library on torch's current stream.  Tests hand in the CPU interpreter build of the same kernel
sources and CPU tensors.
"""
import functools
import math

import torch

from . import _marshal as M
from .metrics import _backend

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_WIN, MAX_WIN = 3, 11


def window_taps(window, win_size=None, sigma=1.5):
    """-> (taps: list of float, cn): the 1-D window and the covariance normalisation of a convention."""
    if window == "gaussian":
        win = 2 * int(3.5 * sigma + 0.5) + 1 if win_size is None else int(win_size)
    elif window == "uniform":
        win = 7 if win_size is None else int(win_size)
    else:
        raise ValueError(f"window must be 'gaussian' or 'uniform'; got {window!r}")
    if win % 2 == 0 or not MIN_WIN <= win <= MAX_WIN:
        raise ValueError(f"win_size must be odd and in {MIN_WIN}..{MAX_WIN}; got {win}")
    if window == "uniform":
        return [1.0 / win] * win, win * win / (win * win - 1.0)
    g = [math.exp(-0.5 * (k / sigma) ** 2) for k in range(-(win // 2), win // 2 + 1)]
    total = math.fsum(g)
    return [v / total for v in g], 1.0


@functools.lru_cache(maxsize=32)
def _cached_taps(taps, device):
    return torch.tensor(taps, dtype=torch.float64).to(device)


def _device_taps(taps, device):
    """The window on the device, copied once per (window, device): at most 32 tensors of at most 88 bytes are kept."""
    return _cached_taps(tuple(taps), torch.device(device))


def _check_pair(x, y, data_range):
    if x.ndim != 4 or x.shape != y.shape:
        raise ValueError(f"two image batches [N,C,H,W] of one shape; got {tuple(x.shape)}, {tuple(y.shape)}")
    if x.dtype != y.dtype or x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"both images uint8 or both fp32; got {x.dtype}, {y.dtype}")
    if data_range is None:
        if x.dtype != torch.uint8:
            raise ValueError("float images need an explicit data_range")
        data_range = 255.0
    return float(data_range)


def _channel_mean(v):
    """[N,C] -> [N]: the columns added in ascending order (elementwise, so a sample's bits do not depend on the batch)."""
    acc = v[:, 0]
    for c in range(1, v.shape[1]):
        acc = acc + v[:, c]
    return acc / v.shape[1]


@torch.inference_mode()
def ssim(x, y, data_range=None, window="gaussian", win_size=None, sigma=1.5, use_sample_covariance=None, K1=0.01, K2=0.03,
         mask=None, full=False, lib=None):
    """[N] float64 on the device: per channel the mean of S over the valid region, then the mean over channels.  x, y
    [N,C,H,W], both uint8 (data_range 255) or both fp32 (data_range required).
    use_sample_covariance: overrides the window's convention (True: cn = win^2 / (win^2 - 1), False: 1).
    mask: non-negative weights [N,1,H,W] or [N,H,W] at image resolution, on the images' device (any dtype; e.g. everything a
        segmentation does not label hair), cropped by (win - 1) / 2 like S; the result is sum(m S) / sum(m) per channel, nan
        for an all-zero mask.
    full=True: -> (scores, the map S [N,C,H-win+1,W-win+1] float64)."""
    data_range = _check_pair(x, y, data_range)
    taps, cn = window_taps(window, win_size, sigma)
    win = len(taps)
    if use_sample_covariance is not None:
        cn = win * win / (win * win - 1.0) if use_sample_covariance else 1.0
    n, _, h, w = x.shape
    if h < win or w < win:
        raise ValueError(f"images of {h} x {w} are smaller than the {win} x {win} window")
    if mask is not None:
        if tuple(mask.shape) not in ((n, 1, h, w), (n, h, w)):
            raise ValueError(f"mask must be [N,1,H,W] or [N,H,W] = {(n, 1, h, w)}; got {tuple(mask.shape)}")
        if mask.device != x.device:  # its pointer goes to the kernel like the images'
            raise ValueError(f"mask is on {mask.device}, the images on {x.device}")
        p = (win - 1) // 2
        mask = mask.reshape(n, h, w)[:, p:h - p, p:w - p].float().contiguous()
    L, st = _backend(lib, x, y, *(() if mask is None else (mask,)))
    out = M.ssim_planes(L, st, x, y, _device_taps(taps, x.device), (K1 * data_range) ** 2, (K2 * data_range) ** 2, cn, mask=mask,
                        want_map=full)
    per_channel = out["s"] / out["m"] if mask is not None else out["s"] / ((h - win + 1) * (w - win + 1))
    score = _channel_mean(per_channel)
    return (score, out["map"]) if full else score


@torch.inference_mode()
def dssim(x, y, data_range=None, lib=None):
    """[N] float64: (1 - ssim) / 2 with skimage's default window (uniform 7, sample covariance) - the reference's `dssim`."""
    return (1.0 - ssim(x, y, data_range, window="uniform", lib=lib)) / 2.0


@torch.inference_mode()
def ms_ssim(x, y, data_range=None, weights=MS_SSIM_WEIGHTS, window="gaussian", win_size=None, sigma=1.5, K1=0.01, K2=0.03, lib=None,
            mask=None):
    """[N] float64: multi-scale SSIM (Wang, Simoncelli, Bovik 2003) in the `pytorch_msssim` convention.  M = len(weights)
    scales, one launch each; every launch but the last also writes the next level, the 2x2 means in fp64 (every level of an
    8-bit image is then exact).  Per image and channel prod_{j<M} max(cs_j, 0)^w_j max(ssim_M, 0)^w_M, then the mean over
    channels.  ValueError unless min(H, W) // 2^(M-1) >= win_size (176 with the defaults), and for a mask (not supported)."""
    if mask is not None:
        raise ValueError("ms_ssim takes no mask (the scales would each need their own)")
    data_range = _check_pair(x, y, data_range)
    taps, cn = window_taps(window, win_size, sigma)
    win, levels = len(taps), len(weights)
    if levels < 1:
        raise ValueError("weights must name at least one scale")
    _, _, h, w = x.shape
    if min(h, w) // 2 ** (levels - 1) < win:
        raise ValueError(f"images of {h} x {w} are too small for {levels} scales of a {win} x {win} window: "
                         f"min(H, W) must be at least {win * 2 ** (levels - 1)}")
    L, st = _backend(lib, x, y)
    t = _device_taps(taps, x.device)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    values = []
    for j in range(levels):
        last = j == levels - 1
        out = M.ssim_planes(L, st, x, y, t, c1, c2, cn, want_cs=not last, want_next=not last)
        values.append((out["s"] if last else out["cs"]) / ((x.shape[2] - win + 1) * (x.shape[3] - win + 1)))
        if not last:
            x, y = out["next"]
    prod = None  # elementwise in ascending scale order: a sample's bits do not depend on the batch
    for v, wt in zip(values, weights):
        term = v.clamp_min(0.0) ** float(wt)
        prod = term if prod is None else prod * term
    return _channel_mean(prod)
