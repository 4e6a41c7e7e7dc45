"""TEST INFRASTRUCTURE - the FID Inception-v3 (torch-fidelity's FeatureExtractorInceptionV3, `pt_inception-2015-12-05`, the
network of torchmetrics' FrechetInceptionDistance) restated in torch, dtype-generic: fp64 is the truth, fp32 on the CPU the
yardstick.  Written from the network's published definition and independent of hairfastgan_amd.inception: a functional walk
over a plain state dict, `torch.cat` where the product writes slices.

Switches for the three look-alike variants a port gets wrong: count_include_pad=True in the 3x3 average pools, an average
pool in Mixed_7c (torchvision's network; the FID one takes the maximum), a half-pixel bilinear resize (torch's
align_corners=False; the FID one is TF1's, without the offset)."""
import functools

import torch
import torch.nn.functional as F

TAPS = (64, 192, 768, 2048)


def cdiv(width, div):
    return -(-width // div)


def layer_table(channel_div=1):
    """[(name, cin, cout, (kh, kw), stride, (ph, pw))] of all 94 conv layers, in the network's order."""
    c = lambda v: cdiv(v, channel_div)  # noqa: E731
    t = [("Conv2d_1a_3x3", 3, c(32), (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", c(32), c(32), (3, 3), 1, (0, 0)),
         ("Conv2d_2b_3x3", c(32), c(64), (3, 3), 1, (1, 1)), ("Conv2d_3b_1x1", c(64), c(80), (1, 1), 1, (0, 0)),
         ("Conv2d_4a_3x3", c(80), c(192), (3, 3), 1, (0, 0))]

    def a(name, cin, pf):
        t.extend([(f"{name}.branch1x1", cin, c(64), (1, 1), 1, (0, 0)), (f"{name}.branch5x5_1", cin, c(48), (1, 1), 1, (0, 0)),
                  (f"{name}.branch5x5_2", c(48), c(64), (5, 5), 1, (2, 2)), (f"{name}.branch3x3dbl_1", cin, c(64), (1, 1), 1, (0, 0)),
                  (f"{name}.branch3x3dbl_2", c(64), c(96), (3, 3), 1, (1, 1)), (f"{name}.branch3x3dbl_3", c(96), c(96), (3, 3), 1, (1, 1)),
                  (f"{name}.branch_pool", cin, pf, (1, 1), 1, (0, 0))])
        return 2 * c(64) + c(96) + pf

    def cc(name, cin, c7):
        h, v = ((1, 7), (0, 3)), ((7, 1), (3, 0))
        t.extend([(f"{name}.branch1x1", cin, c(192), (1, 1), 1, (0, 0)), (f"{name}.branch7x7_1", cin, c7, (1, 1), 1, (0, 0)),
                  (f"{name}.branch7x7_2", c7, c7, h[0], 1, h[1]), (f"{name}.branch7x7_3", c7, c(192), v[0], 1, v[1]),
                  (f"{name}.branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (f"{name}.branch7x7dbl_2", c7, c7, v[0], 1, v[1]),
                  (f"{name}.branch7x7dbl_3", c7, c7, h[0], 1, h[1]), (f"{name}.branch7x7dbl_4", c7, c7, v[0], 1, v[1]),
                  (f"{name}.branch7x7dbl_5", c7, c(192), h[0], 1, h[1]), (f"{name}.branch_pool", cin, c(192), (1, 1), 1, (0, 0))])
        return 4 * c(192)

    def e(name, cin):
        t.extend([(f"{name}.branch1x1", cin, c(320), (1, 1), 1, (0, 0)), (f"{name}.branch3x3_1", cin, c(384), (1, 1), 1, (0, 0)),
                  (f"{name}.branch3x3_2a", c(384), c(384), (1, 3), 1, (0, 1)), (f"{name}.branch3x3_2b", c(384), c(384), (3, 1), 1, (1, 0)),
                  (f"{name}.branch3x3dbl_1", cin, c(448), (1, 1), 1, (0, 0)), (f"{name}.branch3x3dbl_2", c(448), c(384), (3, 3), 1, (1, 1)),
                  (f"{name}.branch3x3dbl_3a", c(384), c(384), (1, 3), 1, (0, 1)),
                  (f"{name}.branch3x3dbl_3b", c(384), c(384), (3, 1), 1, (1, 0)), (f"{name}.branch_pool", cin, c(192), (1, 1), 1, (0, 0))])
        return c(320) + 4 * c(384) + c(192)

    w = a("Mixed_5b", c(192), c(32))
    w = a("Mixed_5c", w, c(64))
    w = a("Mixed_5d", w, c(64))
    t.extend([("Mixed_6a.branch3x3", w, c(384), (3, 3), 2, (0, 0)), ("Mixed_6a.branch3x3dbl_1", w, c(64), (1, 1), 1, (0, 0)),
              ("Mixed_6a.branch3x3dbl_2", c(64), c(96), (3, 3), 1, (1, 1)), ("Mixed_6a.branch3x3dbl_3", c(96), c(96), (3, 3), 2, (0, 0))])
    w = c(384) + c(96) + w
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        w = cc(name, w, c(c7))
    t.extend([("Mixed_7a.branch3x3_1", w, c(192), (1, 1), 1, (0, 0)), ("Mixed_7a.branch3x3_2", c(192), c(320), (3, 3), 2, (0, 0)),
              ("Mixed_7a.branch7x7x3_1", w, c(192), (1, 1), 1, (0, 0)), ("Mixed_7a.branch7x7x3_2", c(192), c(192), (1, 7), 1, (0, 3)),
              ("Mixed_7a.branch7x7x3_3", c(192), c(192), (7, 1), 1, (3, 0)), ("Mixed_7a.branch7x7x3_4", c(192), c(192), (3, 3), 2, (0, 0))])
    w = c(320) + c(192) + w
    w = e("Mixed_7b", w)
    e("Mixed_7c", w)
    return t


def key_list(channel_div=1):
    """The reference class's state-dict keys without `fc.*`: 94 layers x 5 tensors."""
    return [f"{name}.{leaf}" for name, *_ in layer_table(channel_div)
            for leaf in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")]


@functools.lru_cache(maxsize=None)
def _state(channel_div, seed):
    g = torch.Generator().manual_seed(7000 + seed)
    sd = {}
    for name, cin, cout, (kh, kw), _, _ in layer_table(channel_div):
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5  # He-normal
        sd[f"{name}.bn.weight"] = 0.75 + 0.5 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.02 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.02 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
    return sd


def discriminating_state(channel_div=1, seed=0):
    """He-normal conv weights, BatchNorm variances in [0.5, 1.5], weights in [0.75, 1.25], means / biases 0.02 N(0,1)."""
    return {k: v.clone() for k, v in _state(channel_div, seed).items()}


@functools.lru_cache(maxsize=None)
def byte_images(size, n=3, seed=0):
    """Seeded byte images [n,3,size,size]: a smooth field plus texture; image 1 is image 0 +- 3 levels of noise.  Read-only
    by agreement."""
    g = torch.Generator().manual_seed(8000 + seed)
    coarse = F.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(size, size), mode="bicubic", align_corners=False)
    fine = torch.randn(n, 3, size, size, generator=g)
    x = (128 + 50 * coarse + 25 * fine).round().clamp(0, 255)
    x[1] = (x[0] + torch.randint(-3, 4, (3, size, size), generator=g)).clamp(0, 255)
    return x.to(torch.uint8).contiguous()


def resize_tf1(x, oh, ow, half_pixel=False, coord_dtype=torch.float32):
    """x [N,C,H,W] in any float dtype -> [N,C,oh,ow]: the definition.  The source coordinates (scale, src, t) are part of the
    definition in fp32 and are computed in coord_dtype = fp32 whatever x's dtype; the two lerps run in x's dtype (fp64: the
    truth of the six roundings the fp32 lerps make).  half_pixel: the look-alike - src = (o + 0.5) * scale - 0.5, clamped at 0
    (torch's align_corners=False)."""
    h, w = x.shape[2:]
    dt = coord_dtype

    def axis(n_in, n_out):
        scale = torch.tensor(n_in, dtype=dt) / torch.tensor(n_out, dtype=dt)
        o = torch.arange(n_out, dtype=dt)
        src = ((o + 0.5) * scale - 0.5).clamp_min(0) if half_pixel else o * scale
        i0 = src.floor().long().clamp_max(n_in - 1)
        return i0, (i0 + 1).clamp_max(n_in - 1), src - i0.to(dt)

    y0, y1, ty = axis(h, oh)
    x0, x1, tx = axis(w, ow)
    top_a, top_b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    bot_a, bot_b = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    tx, ty = tx.to(x.dtype), ty.to(x.dtype)
    top = top_a + (top_b - top_a) * tx
    bot = bot_a + (bot_b - bot_a) * tx
    return top + (bot - top) * ty[:, None]


def pool3x3(x, mode, stride, count_include_pad=False):
    if mode == "max":
        return F.max_pool2d(x, 3, stride, 1 if stride == 1 else 0)
    return F.avg_pool2d(x, 3, stride, 1 if stride == 1 else 0, count_include_pad=count_include_pad)


def forward(state, images, dtype=torch.float64, channel_div=1, resize=True, count_include_pad=False, avg_in_7c=False,
            half_pixel=False, upto=2048):
    """images uint8 [N,3,H,W] (or floats in [0,1]) -> {tap: [N,d]} in `dtype`."""
    sd = {k: v.to(dtype) for k, v in state.items()}
    table = {name: (stride, pad) for name, _, _, _, stride, pad in layer_table(channel_div)}
    if images.dtype != torch.uint8:
        images = (images * 255).to(torch.uint8)
    x = images.to(dtype)
    if resize:
        x = resize_tf1(x, 299, 299, half_pixel)
    x = (x - 128) / 128

    def bc(name, v):
        stride, pad = table[name]
        v = F.conv2d(v, sd[f"{name}.conv.weight"], None, stride, pad)
        v = F.batch_norm(v, sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"], sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"],
                         False, 0.0, 0.001)
        return F.relu(v)

    def avg(v):
        return pool3x3(v, "avg", 1, count_include_pad)

    out = {}
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = bc(name, x)
    x = F.max_pool2d(x, 3, 2)
    out[64] = x.mean((2, 3))
    if upto == 64:
        return out
    x = bc("Conv2d_4a_3x3", bc("Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, 3, 2)
    out[192] = x.mean((2, 3))
    if upto == 192:
        return out
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = torch.cat([bc(f"{n}.branch1x1", x), bc(f"{n}.branch5x5_2", bc(f"{n}.branch5x5_1", x)),
                       bc(f"{n}.branch3x3dbl_3", bc(f"{n}.branch3x3dbl_2", bc(f"{n}.branch3x3dbl_1", x))),
                       bc(f"{n}.branch_pool", avg(x))], 1)
    n = "Mixed_6a"
    x = torch.cat([bc(f"{n}.branch3x3", x), bc(f"{n}.branch3x3dbl_3", bc(f"{n}.branch3x3dbl_2", bc(f"{n}.branch3x3dbl_1", x))),
                   F.max_pool2d(x, 3, 2)], 1)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        b7 = bc(f"{n}.branch7x7_3", bc(f"{n}.branch7x7_2", bc(f"{n}.branch7x7_1", x)))
        bd = x
        for k in range(1, 6):
            bd = bc(f"{n}.branch7x7dbl_{k}", bd)
        x = torch.cat([bc(f"{n}.branch1x1", x), b7, bd, bc(f"{n}.branch_pool", avg(x))], 1)
    out[768] = x.mean((2, 3))
    if upto == 768:
        return out
    n = "Mixed_7a"
    b7 = x
    for k in range(1, 5):
        b7 = bc(f"{n}.branch7x7x3_{k}", b7)
    x = torch.cat([bc(f"{n}.branch3x3_2", bc(f"{n}.branch3x3_1", x)), b7, F.max_pool2d(x, 3, 2)], 1)
    for n in ("Mixed_7b", "Mixed_7c"):
        b3 = bc(f"{n}.branch3x3_1", x)
        bd = bc(f"{n}.branch3x3dbl_2", bc(f"{n}.branch3x3dbl_1", x))
        pooled = avg(x) if (n == "Mixed_7b" or avg_in_7c) else F.max_pool2d(x, 3, 1, 1)
        x = torch.cat([bc(f"{n}.branch1x1", x), bc(f"{n}.branch3x3_2a", b3), bc(f"{n}.branch3x3_2b", b3),
                       bc(f"{n}.branch3x3dbl_3a", bd), bc(f"{n}.branch3x3dbl_3b", bd), bc(f"{n}.branch_pool", pooled)], 1)
    out[2048] = x.mean((2, 3))
    return out
