"""TEST INFRASTRUCTURE - torch / numpy restatements of the identity-similarity path (csrc/identity.h, hairfastgan_amd.identity),
written from the formulas of the reference (losses/pp_losses.py:50-53, 97-219, 267-296; encoder4editing/criteria/id_loss.py);
every function takes the dtype to evaluate in: float64 is the truth, float32 on the CPU is the yardstick the device's error is
compared with.

  crop and pool   out[i, j] = mean of x[y0 + floor(i ch / oh) : y0 + ceil((i + 1) ch / oh), x0 + ... ] (torch's adaptive
                  windows over the crop), optionally scale[c] mean + shift[c]; `crop_avgpool_ordered` is the kernel's stated
                  fp32 order: pixels added one by one in row-major order, divided by the count, one fused multiply-add
  normalise       x / sqrt(sum x^2) per row
  similarity      a . b per pair, or a b^T
  Backbone        plain torch modules under the reference's names (input_layer, body.<i>.shortcut_layer / res_layer,
                  output_layer), BatchNorms on their running statistics, Dropout the identity
  IDLoss          crop [35:223, 32:220], AdaptiveAvgPool2d to the network's input size, Backbone, dot products
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

U32 = 2.0 ** -24  # unit roundoff of fp32
CROP = (35, 32, 188, 188)
IR50 = ([(64, 64, 2)] + [(64, 64, 1)] * 2 + [(64, 128, 2)] + [(128, 128, 1)] * 3 + [(128, 256, 2)] + [(256, 256, 1)] * 13 +
        [(256, 512, 2)] + [(512, 512, 1)] * 2)  # get_blocks(50), pp_losses.py:60-73


# ---- kernels ------------------------------------------------------------------------------------------------------
def _windows(size, out):
    i = np.arange(out, dtype=np.int64)
    return (i * size) // out, ((i + 1) * size + out - 1) // out


def crop_avgpool(x, y0, x0, ch, cw, oh, ow, scale=None, shift=None):
    """fp64 -> (out, count [oh,ow], max |pixel| of each window [N,C,oh,ow])."""
    x = np.asarray(x, dtype=np.float64)
    ya, yb = _windows(ch, oh)
    xa, xb = _windows(cw, ow)
    out = np.empty(x.shape[:2] + (oh, ow))
    big = np.empty_like(out)
    for i in range(oh):
        for j in range(ow):
            win = x[:, :, y0 + ya[i]:y0 + yb[i], x0 + xa[j]:x0 + xb[j]]
            out[:, :, i, j] = win.sum((2, 3)) / (win.shape[2] * win.shape[3])
            big[:, :, i, j] = np.abs(win).max((2, 3))
    count = np.outer(yb - ya, xb - xa)
    if scale is not None:
        out = out * np.asarray(scale, dtype=np.float64)[None, :, None, None]
    if shift is not None:
        out = out + np.asarray(shift, dtype=np.float64)[None, :, None, None]
    return out, count, big


def crop_avgpool_ordered(x, y0, x0, ch, cw, oh, ow, scale=None, shift=None):
    """fp32, the kernel's order: every bin adds its pixels one by one (rows ascending, columns ascending inside a row) starting
    from 0, divides by the count, then one fused multiply-add (the exact product and sum in fp64, rounded to fp32: fp64 holds
    the product of two fp32 values exactly; the second rounding could differ from a true FMA only at an fp32 tie of a 53-bit
    sum)."""
    x = np.asarray(x, dtype=np.float32)
    ya, yb = _windows(ch, oh)
    xa, xb = _windows(cw, ow)
    acc = np.zeros(x.shape[:2] + (oh, ow), dtype=np.float32)
    for dy in range(int((yb - ya).max())):
        for dx in range(int((xb - xa).max())):
            yy, xx = ya + dy, xa + dx
            live = (yy < yb)[:, None] & (xx < xb)[None, :]
            yy, xx = np.minimum(yy, yb - 1), np.minimum(xx, xb - 1)
            v = x[:, :, (y0 + yy)[:, None], (x0 + xx)[None, :]]
            acc = np.where(live[None, None], (acc + v).astype(np.float32), acc)
    out = (acc / np.outer(yb - ya, xb - xa).astype(np.float32)[None, None]).astype(np.float32)
    if scale is not None or shift is not None:
        c = x.shape[1]
        sc = np.ones(c, np.float32) if scale is None else np.asarray(scale, dtype=np.float32)
        sh = np.zeros(c, np.float32) if shift is None else np.asarray(shift, dtype=np.float32)
        out = (sc.astype(np.float64)[None, :, None, None] * out.astype(np.float64) + sh.astype(np.float64)[None, :, None, None]).astype(np.float32)
    return out


def l2_normalize(x, dtype=torch.float64):
    x = x.to(dtype)
    return x / torch.sqrt(torch.sum(x * x, dim=1, keepdim=True))


def similarity(a, b, paired=True):
    """numpy fp64 of the fp32 rows."""
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    return (a * b).sum(1) if paired else a @ b.T


# ---- the network --------------------------------------------------------------------------------------------------
class _SE(nn.Module):
    def __init__(self, channels, reduction):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)

    def forward(self, x):
        return x * torch.sigmoid(self.fc2(F.relu(self.fc1(x.mean((2, 3), keepdim=True)))))


class _Unit(nn.Module):
    def __init__(self, in_channel, depth, stride):
        super().__init__()
        if in_channel == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        self.res_layer = nn.Sequential(nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth), _SE(depth, 16))

    def forward(self, x, shortcut_only=False):
        return self.shortcut_layer(x) if shortcut_only else self.res_layer(x) + self.shortcut_layer(x)


class Backbone(nn.Module):
    def __init__(self, input_size=112, units=None, affine=True):
        super().__init__()
        units = IR50 if units is None else units
        plane = input_size // int(np.prod([s for _, _, s in units]))
        depth = units[-1][1]
        self.input_size = input_size
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(depth), nn.Dropout(0.4), nn.Flatten(), nn.Linear(depth * plane * plane, 512),
                                          nn.BatchNorm1d(512, affine=affine))
        self.body = nn.Sequential(*[_Unit(*u) for u in units])

    def forward(self, x, shortcut_only=False, normalize=True):
        x = self.input_layer(x)
        for unit in self.body:
            x = unit(x, shortcut_only)
        x = self.output_layer(x)
        return l2_normalize(x, x.dtype) if normalize else x


def discriminating_state(units=None, input_size=112, seed=0, affine=True):
    """A state dict under which the network tells images apart and its residual branches matter: torch's default init;
    BatchNorm running variances uniform in [0.5, 1.5], weights in [0.75, 1.25], running means and biases 0.02 N(0,1); the last
    BatchNorm of every unit's residual branch has its weight multiplied by 4."""
    with torch.random.fork_rng():
        torch.manual_seed(4000 + seed)
        net = Backbone(input_size, units, affine)
        g = torch.Generator().manual_seed(5000 + seed)
        sd = net.state_dict()
        for k in sd:
            if k.endswith("running_var"):
                base = k[:-len("running_var")]
                sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
                sd[base + "running_mean"] = 0.02 * torch.randn(sd[k].shape, generator=g)
                if base + "weight" in sd:
                    sd[base + "weight"] = (0.75 + 0.5 * torch.rand(sd[k].shape, generator=g)) * (4.0 if base.endswith("res_layer.4.") else 1.0)
                    sd[base + "bias"] = 0.02 * torch.randn(sd[k].shape, generator=g)
        sd["output_layer.3.bias"] = 0.02 * torch.randn(512, generator=g)
    return {k: v.clone() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def discriminating_images(size=256, n=4, seed=0):
    """0.6 x a random 8^2 field + 0.4 x a 64^2 field, upsampled bicubically and clamped to [-1, 1]; image 1 is image 0 plus
    0.03 N(0,1) noise.  [n,3,size,size] fp32, read-only by agreement."""
    g = torch.Generator().manual_seed(6000 + seed)
    coarse = F.interpolate(torch.randn(n, 3, 8, 8, generator=g), size=(size, size), mode="bicubic", align_corners=False)
    fine = F.interpolate(torch.randn(n, 3, 64, 64, generator=g), size=(size, size), mode="bicubic", align_corners=False)
    x = (0.6 * coarse + 0.4 * fine).clamp(-1.0, 1.0)
    x[1] = (x[0] + 0.03 * torch.randn(3, size, size, generator=g)).clamp(-1.0, 1.0)
    return x.contiguous()


def network(sd, units=None, input_size=112, dtype=torch.float64, affine=True):
    net = Backbone(input_size, units, affine)
    net.load_state_dict(sd)
    return net.to(dtype).eval()


@torch.no_grad()
def extract_feats(net, x, crop=CROP, shortcut_only=False, normalize=True):
    """IDLoss.extract_feats in the network's dtype."""
    y0, x0, ch, cw = crop
    dtype = next(net.parameters()).dtype
    x = F.adaptive_avg_pool2d(x.to(dtype)[:, :, y0:y0 + ch, x0:x0 + cw], (net.input_size, net.input_size))
    return net(x, shortcut_only, normalize)


def id_loss(net, y_hat, y, x=None, crop=CROP):
    """The reference's two loops (pp_losses.py:284-296, id_loss.py:25-47) in the network's dtype."""
    f_hat, f_y = extract_feats(net, y_hat, crop), extract_feats(net, y, crop)
    n = y.shape[0]
    if x is None:
        return sum(1 - f_hat[i].dot(f_y[i]) for i in range(n)) / n
    f_x = extract_feats(net, x, crop)
    logs = [{"diff_target": float(f_hat[i].dot(f_y[i])), "diff_input": float(f_hat[i].dot(f_x[i])), "diff_views": float(f_y[i].dot(f_x[i]))}
            for i in range(n)]
    loss = sum(1 - f_hat[i].dot(f_y[i]) for i in range(n)) / n
    return loss, sum(d["diff_target"] - d["diff_views"] for d in logs) / n, logs
