"""TEST INFRASTRUCTURE - torch / numpy restatements of the LPIPS and L2 / PSNR path (csrc/lpips.h, hairfastgan_amd.lpips),
written from the formulas of the metric; every function takes the dtype to evaluate in: float64 is the truth, float32 on the
CPU is the yardstick the device's error is compared with.

  direct conv   y = act(conv_{k x k, stride, pad}(in_scale x + in_shift) + bias), the affine on real pixels only (padding 0)
  max pool      torch's own F.max_pool2d
  LPIPS layer   (1 / HW) sum_pixels sum_c w_c (fx_c / (|fx| + 1e-10) - fy_c / (|fy| + 1e-10))^2, |.| the channel norm of a pixel
  towers        the AlexNet / VGG16 `features` layer tables with a ReLU after every convolution; z-score (x - mean) / std
  LPIPS         sum over the tapped layers of the layer distance; `forward` = sum over the batch / N
  L2 / PSNR     numpy
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24  # unit roundoff of fp32
MEAN = (-0.030, -0.088, -0.188)
STD = (0.458, 0.448, 0.450)
# (features index, cin, cout, k, stride, pad); a max pool (k, 2) stands in front of the convolutions listed in POOLS
ALEX = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
VGG = tuple((i, ci, co, 3, 1, 1) for i, ci, co in (
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
    (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)))
NETS = {"alex": dict(convs=ALEX, pools=(3, 6), pool_k=3, taps=(0, 3, 6, 8, 10)),
        "vgg": dict(convs=VGG, pools=(5, 10, 17, 24), pool_k=2, taps=(2, 7, 14, 21, 28))}


def f32(a):
    """Inputs are rounded to fp32 before the truth sees them."""
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


# ---- direct conv --------------------------------------------------------------------------------------------------
def conv_direct(x, w, stride, pad, in_scale=None, in_shift=None, bias=None, relu=False):
    """fp64 -> (y, magnitude): magnitude = sum |w x^| + |b| per output, what the error bound of a K-term fp32 sum scales with."""
    x, w = x.double(), w.double()
    xh = x
    if in_scale is not None:
        xh = xh * in_scale.double()[None, :, None, None]
    if in_shift is not None:
        xh = xh + in_shift.double()[None, :, None, None]
    y = F.conv2d(xh, w, None if bias is None else bias.double(), stride, pad)
    mag = F.conv2d(xh.abs(), w.abs(), None if bias is None else bias.double().abs(), stride, pad)
    return (y.clamp_min(0.0) if relu else y), mag


# ---- LPIPS layer --------------------------------------------------------------------------------------------------
def lpips_layer(fx, fy, lin_w, dtype=torch.float64):
    """[N] of `dtype`: the layer distance by the formula, every step in `dtype` (sums across pixels included)."""
    fx, fy, w = fx.to(dtype), fy.to(dtype), lin_w.to(dtype).reshape(1, -1, 1, 1)
    nx = torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10
    ny = torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10
    d = (fx / nx - fy / ny) ** 2
    return (d * w).sum(1, keepdim=True).mean((2, 3)).reshape(-1)


def lpips_layer_floor(fx, fy, lin_w):
    """[N] float64: a first-order bound of the rounding error of ANY fp32 evaluation of the layer whose per-pixel arithmetic
    is fp32 (summation order free), from the operation count.  With u = 2^-24 and C channels:
      |fx|^2 is a sum of C non-negative terms: relative error <= C u, halved by the square root: the norm + eps carries
      (C / 2 + 2) u, the quotient x^_c = fx_c / norm (C / 2 + 3) u;
      d_c = x^_c - y^_c: absolute error <= (C / 2 + 3) u (|x^_c| + |y^_c|) + u |d_c|;
      d_c^2: 2 |d_c| times that, + u d_c^2;  w_c d_c^2 and its sum over C terms: (C + 2) u relative at most.
    Per pixel: u sum_c |w_c| ((C + 6) |d_c| (|x^_c| + |y^_c|) + (C + 6) d_c^2); the fp64 sum over pixels adds nothing."""
    fx, fy, w = fx.double(), fy.double(), lin_w.double().abs().reshape(1, -1, 1, 1)
    c = fx.shape[1]
    xh = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
    yh = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
    d = (xh - yh).abs()
    per_pixel = (w * ((c + 6) * d * (xh.abs() + yh.abs()) + (c + 6) * d * d)).sum(1, keepdim=True)
    return U32 * per_pixel.mean((2, 3)).reshape(-1)


# ---- towers -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_weights(net_type, seed=0):
    """Seeded stand-ins for the published weights, under the module's state-dict keys: He-scaled filters
    (std = sqrt(2 / fan_in)), biases 0.1 N(0,1), lin weights uniform in [0, 2 / C]."""
    g = torch.Generator().manual_seed(1000 + seed + (0 if net_type == "alex" else 500))
    net = NETS[net_type]
    sd = {"net.mean": torch.tensor(MEAN)[None, :, None, None], "net.std": torch.tensor(STD)[None, :, None, None]}
    j = 0
    for i, ci, co, k, _, _ in net["convs"]:
        sd[f"net.layers.{i}.weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f"net.layers.{i}.bias"] = 0.1 * torch.randn(co, generator=g)
        if i in net["taps"]:
            sd[f"lin.{j}.1.weight"] = torch.rand(1, co, 1, 1, generator=g) * (2.0 / co)
            j += 1
    return sd


def tower(sd, net_type, x, dtype=torch.float64):
    """The tapped activations (after the ReLU) of images x [N,3,H,W]."""
    net = NETS[net_type]
    x = (x.to(dtype) - sd["net.mean"].to(dtype)) / sd["net.std"].to(dtype)
    out = []
    for i, _, _, _, s, p in net["convs"]:
        if i in net["pools"]:
            x = F.max_pool2d(x, net["pool_k"], 2)
        x = F.relu(F.conv2d(x, sd[f"net.layers.{i}.weight"].to(dtype), sd[f"net.layers.{i}.bias"].to(dtype), s, p))
        if i in net["taps"]:
            out.append(x)
    return out


def lpips(sd, net_type, x, y, dtype=torch.float64):
    """[N] of `dtype`: the sum over the taps of the layer distances."""
    fx, fy = tower(sd, net_type, x, dtype), tower(sd, net_type, y, dtype)
    return sum(lpips_layer(a, b, sd[f"lin.{j}.1.weight"], dtype) for j, (a, b) in enumerate(zip(fx, fy)))


def lpips_floor(sd, net_type, x, y):
    """[N]: the layer floors summed over the taps, on the true (fp64) features - the error of the last stage alone."""
    fx, fy = tower(sd, net_type, x), tower(sd, net_type, y)
    return sum(lpips_layer_floor(a, b, sd[f"lin.{j}.1.weight"]) for j, (a, b) in enumerate(zip(fx, fy)))


# ---- L2 / PSNR ----------------------------------------------------------------------------------------------------
def sq_err_sum(a, b):
    """[N]: uint8 -> exact int64 sums; fp32 -> float64 sums of the exact differences' squares."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.uint8:
        d = a.astype(np.int64) - b.astype(np.int64)
        return (d * d).reshape(a.shape[0], -1).sum(1)
    d = a.astype(np.float64) - b.astype(np.float64)
    return (d * d).reshape(a.shape[0], -1).sum(1)


def psnr(a, b, data_range):
    n = np.asarray(a)[0].size
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(float(data_range) ** 2 / (sq_err_sum(a, b).astype(np.float64) / n))
