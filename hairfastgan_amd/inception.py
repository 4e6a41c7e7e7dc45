"""The FID Inception-v3 on the device: the feature extractor behind the plain `FID` column of scripts/fid_metric.py, which
there is torchmetrics' FrechetInceptionDistance(normalize=False) with its built-in network - torch-fidelity's
`FeatureExtractorInceptionV3` with the weights `pt_inception-2015-12-05`.

    fid = FrechetDistance(InceptionV3(2048, weights=checkpoints.inception_fid()))

The network is restated here from its published definition; neither torchmetrics nor torch-fidelity is a dependency, and
agreement with the published weights on real images has NOT been verified (no weights file was available).

Pieces, all on the library's kernels:
  images -> 299^2 in [-1,1)   hf_resize_bilinear_tf1_f32: bytes (or trunc(255 x) of [0,1] floats) to fp32, the TF1-style
                              bilinear resize (no half-pixel offset), (x - 128) / 128 - one launch
  first layer                 hf_conv2d_direct_f32 (3 input channels; the BatchNorm scale folded into the weights once)
  the other 93 conv layers    hf_conv2d_rect_f16_f32: conv + folded BatchNorm + ReLU over a rectangle of taps, reading and
                              writing channel slices - a block's branches write the concatenated tensor directly, and the
                              1x1 heads that feed a block's deeper branches are ONE launch whose consumers read slices
  pools                       hf_pool3x3_f32 (max; average that does not count padding), into slices as well
  taps                        hf_plane_mean_f32: the spatial mean after the first / second max pool, Mixed_6e and Mixed_7c
The operand mode follows `_runtime.conv_precision()`: "f32" runs the exact-FMA form, every other mode the matrix cores with
f16x3 operands.  "f16" does NOT select fp16-rounded operands here: a metric's features must be comparable between runs and
machines, i.e. fp32-class in every mode, and operands rounded to fp16 move the first tap by 1e-4 where fp32 arithmetic moves
it by 1e-7 (the kernel's nterms = 1 form exists and is tested on its own; this network does not use it).  The first forward
pass under "f16" says so once in a warning.  "auto" is plain f16x3 here: the pass does not go through `_runtime.run_guarded`,
so there is no f32 re-run on a clamped fp16 operand - inputs lie in [-1, 1) and the layers are BatchNorm + ReLU, far from 65504.
Inference only: the BatchNorms use their running statistics.

`lib=None`: the loaded HIP library on torch's current stream.  Tests hand in the CPU interpreter build of the same kernel
sources and CPU tensors.
"""
import warnings

import torch
from torch import nn

from . import _marshal as M
from ._runtime import conv_precision
from .encoders._fused import FrozenPlanMixin
from .metrics import _backend

FEATURES = (64, 192, 768, 2048)
_NTERMS = {"f16x3": 3, "f16": 3, "f32": 0}  # fp32-class features in every mode: see the module docstring


class _BatchNorm2d(nn.BatchNorm2d):
    """BatchNorm2d(eps=0.001) whose state is the published file's four tensors: no batch counter, neither kept nor expected."""

    def __init__(self, channels):
        super().__init__(channels, eps=0.001)
        del self._buffers["num_batches_tracked"]
        self.register_buffer("num_batches_tracked", None)

    def _load_from_state_dict(self, *args):
        nn.Module._load_from_state_dict(self, *args)  # (nn.BatchNorm2d's own adds a counter to dicts that lack one)


class BasicConv2d(nn.Module):
    """Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU; keys `conv.weight`, `bn.{weight,bias,running_mean,running_var}`."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = _BatchNorm2d(cout)

    @property
    def cout(self):
        return self.conv.out_channels


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features, c):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, c(64), 1)
        self.branch5x5_1 = BasicConv2d(cin, c(48), 1)
        self.branch5x5_2 = BasicConv2d(c(48), c(64), 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, c(64), 1)
        self.branch3x3dbl_2 = BasicConv2d(c(64), c(96), 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(c(96), c(96), 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, 1)
        self.pool = "avg"
        # (direct branches, merged heads, chains behind the heads' slices, the pooled branch) - concatenation order = listed order
        self.order = [("branch1x1",), ("branch5x5_1", "branch5x5_2"), ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"),
                      ("pool", "branch_pool")]


class InceptionB(nn.Module):
    def __init__(self, cin, c):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, c(384), 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, c(64), 1)
        self.branch3x3dbl_2 = BasicConv2d(c(64), c(96), 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(c(96), c(96), 3, stride=2)
        self.pool = "max2"
        self.order = [("branch3x3",), ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ("pool",)]


class InceptionC(nn.Module):
    def __init__(self, cin, c7, c):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, c(192), 1)
        self.branch7x7_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, c(192), (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, c(192), (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, c(192), 1)
        self.pool = "avg"
        self.order = [("branch1x1",), ("branch7x7_1", "branch7x7_2", "branch7x7_3"),
                      ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), ("pool", "branch_pool")]


class InceptionD(nn.Module):
    def __init__(self, cin, c):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, c(192), 1)
        self.branch3x3_2 = BasicConv2d(c(192), c(320), 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, c(192), 1)
        self.branch7x7x3_2 = BasicConv2d(c(192), c(192), (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(c(192), c(192), (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(c(192), c(192), 3, stride=2)
        self.pool = "max2"
        self.order = [("branch3x3_1", "branch3x3_2"), ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), ("pool",)]


class InceptionE(nn.Module):
    def __init__(self, cin, pool, c):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, c(320), 1)
        self.branch3x3_1 = BasicConv2d(cin, c(384), 1)
        self.branch3x3_2a = BasicConv2d(c(384), c(384), (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(c(384), c(384), (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, c(448), 1)
        self.branch3x3dbl_2 = BasicConv2d(c(448), c(384), 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(c(384), c(384), (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(c(384), c(384), (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, c(192), 1)
        self.pool = pool  # "avg" (Mixed_7b) or "max" (Mixed_7c: the FID network's max pool 3, 1, 1)
        # a tuple as the last element of a chain: siblings that read the same tensor and are concatenated
        self.order = [("branch1x1",), ("branch3x3_1", ("branch3x3_2a", "branch3x3_2b")),
                      ("branch3x3dbl_1", "branch3x3dbl_2", ("branch3x3dbl_3a", "branch3x3dbl_3b")), ("pool", "branch_pool")]


class _Layer:
    """One launch of the frozen plan: prepared weights and the folded BatchNorm, geometry from the module."""

    def __init__(self, L, st, convs):
        ws, scales, shifts = [], [], []
        for m in convs:
            bn = m.bn
            sc, sh = M.bn_fold(L, st, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
            ws.append(m.conv.weight.detach().float())
            scales.append(sc)
            shifts.append(sh)
        conv = convs[0].conv
        self.wts = M.RectWeights(torch.cat(ws))
        self.scale, self.shift = torch.cat(scales).contiguous(), torch.cat(shifts).contiguous()
        self.stride, self.pad = conv.stride[0], tuple(conv.padding)
        self.cout = self.wts.cout

    def out_hw(self, h, w):
        return (M.conv_out_size(h, self.wts.kh, self.stride, self.pad[0]), M.conv_out_size(w, self.wts.kw, self.stride, self.pad[1]))


class InceptionV3(FrozenPlanMixin, nn.Module):
    """images [N,3,H,W] -> features [N,feature] fp32: the spatial mean of the tensor at the requested tap.

    feature: 64 / 192 / 768 / 2048 (torchmetrics' widths); layers behind the tap are not run.
    weights: a state dict (the published file: `checkpoints.inception_fid()`), loaded at construction; None leaves the
        module's initial parameters (load them later with `load_state_dict`, which tolerates `fc.*` and
        `*.num_batches_tracked` entries and is strict about everything else).
    Images: uint8 are used as they are; floats are taken as [0,1] and become trunc(255 x) as a byte (torchmetrics'
        normalize=True).  resize_input=False (tests) skips the resize to 299^2; channel_div (tests) gives every width
        ceil(width / channel_div), the tap widths included."""

    def __init__(self, feature=2048, weights=None, resize_input=True, channel_div=1, lib=None):
        super().__init__()
        if isinstance(feature, bool) or not isinstance(feature, int) or feature not in FEATURES:
            raise ValueError(f"feature must be one of {FEATURES}; got {feature!r}")
        if not isinstance(channel_div, int) or channel_div < 1:
            raise ValueError(f"channel_div must be a positive integer; got {channel_div!r}")
        self.feature, self.resize_input, self.channel_div, self._lib = feature, bool(resize_input), channel_div, lib

        def c(width):
            return -(-width // channel_div)

        self.feature_width = c(feature)
        self.Conv2d_1a_3x3 = BasicConv2d(3, c(32), 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(c(32), c(32), 3)
        self.Conv2d_2b_3x3 = BasicConv2d(c(32), c(64), 3, padding=1)
        if feature >= 192:
            self.Conv2d_3b_1x1 = BasicConv2d(c(64), c(80), 1)
            self.Conv2d_4a_3x3 = BasicConv2d(c(80), c(192), 3)
        if feature >= 768:
            a1 = 3 * c(64) + c(96)  # widths of the concatenations
            self.Mixed_5b = InceptionA(c(192), c(32), c)
            self.Mixed_5c = InceptionA(a1 - c(64) + c(32), c(64), c)
            self.Mixed_5d = InceptionA(a1, c(64), c)
            self.Mixed_6a = InceptionB(a1, c)
            b = c(384) + c(96) + a1
            self.Mixed_6b = InceptionC(b, c(128), c)
            self.Mixed_6c = InceptionC(4 * c(192), c(160), c)
            self.Mixed_6d = InceptionC(4 * c(192), c(160), c)
            self.Mixed_6e = InceptionC(4 * c(192), c(192), c)
        if feature >= 2048:
            d = c(320) + c(192) + 4 * c(192)
            e = c(320) + 4 * c(384) + c(192)
            self.Mixed_7a = InceptionD(4 * c(192), c)
            self.Mixed_7b = InceptionE(d, "avg", c)
            self.Mixed_7c = InceptionE(e, "max", c)
        for p in self.parameters():
            p.requires_grad = False
        self._plan = None
        self.launches = 0  # kernel launches of the last forward
        self.eval()
        if weights is not None:
            self.load_state_dict(weights)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The published file as it is: `fc.*` (unused) and `*.num_batches_tracked` entries are dropped; with a smaller
        `feature` the layers behind the tap are dropped too, everything else is checked strictly."""
        own = set(self.state_dict().keys())
        full = InceptionV3.key_list() if self.feature < 2048 else own
        kept = {k: v for k, v in state_dict.items()
                if not (k.startswith("fc.") or k.endswith(".num_batches_tracked") or (k not in own and k in full))}
        return super().load_state_dict(kept, strict=strict, **kwargs)

    _KEYS = None
    _warned_f16 = False

    @staticmethod
    def key_list():
        """The 470 state-dict keys of the whole network (94 layers x 5 tensors)."""
        if InceptionV3._KEYS is None:  # (the names do not depend on the widths: a narrow copy is built)
            InceptionV3._KEYS = frozenset(InceptionV3(2048, channel_div=64).state_dict().keys())
        return InceptionV3._KEYS

    # ---- the frozen plan ----
    def _blocks(self):
        return [(n, m) for n, m in self.named_children() if n.startswith("Mixed_")]

    def plan(self, L, st):
        if self._plan is None:
            p = {}
            first = self.Conv2d_1a_3x3
            # hf_conv2d_direct_f32 has no output scale: the BatchNorm's goes into the weights, in fp64 and rounded once
            bn = first.bn
            sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            p["first_w"] = (first.conv.weight.detach().double() * sc[:, None, None, None]).float().contiguous()
            p["first_b"] = (bn.bias.detach().double() - bn.running_mean.double() * sc).float().contiguous()
            for name, m in self.named_children():
                if name.startswith("Conv2d_") and name != "Conv2d_1a_3x3":
                    p[name] = _Layer(L, st, [m])
            for bname, blk in self._blocks():
                heads = [ch[0] for ch in blk.order if len(ch) > 1 and ch[0] != "pool"]
                if heads:  # the 1x1 heads of the deeper branches: one launch, the consumers read slices of its result
                    p[bname + ".heads"] = _Layer(L, st, [getattr(blk, h) for h in heads])
                for ch in blk.order:
                    for item in ch[(1 if len(ch) > 1 else 0):]:
                        for nm in (item if isinstance(item, tuple) else (item,)):
                            if nm != "pool":
                                p[bname + "." + nm] = _Layer(L, st, [getattr(blk, nm)])
            self._plan = p
        return self._plan

    # ---- launches ----
    def _conv(self, ctx, layer, x, xc0, out=None, oc0=0):
        L, st, nterms = ctx
        if out is None:
            oh, ow = layer.out_hw(x.shape[2], x.shape[3])
            out = x.new_empty((x.shape[0], layer.cout, oh, ow))
        M.conv2d_rect_into(L, st, out, oc0, x, xc0, layer.wts, nterms, layer.stride, layer.pad, layer.scale, layer.shift, relu=True)
        self.launches += 1
        return out

    def _pool(self, ctx, x, mode, stride, out=None, oc0=0):
        L, st, _ = ctx
        n, c, h, w = x.shape
        if out is None:
            out = x.new_empty((n, c, h, w) if stride == 1 else (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1))
        M.pool3x3_into(L, st, out, oc0, x, 0, c, mode, stride)
        self.launches += 1
        return out

    def _mean(self, ctx, x):
        self.launches += 1
        return M.plane_mean(ctx[0], ctx[1], x)

    def _block(self, ctx, p, bname, blk, x):
        n, cin, h, w = x.shape
        down = blk.pool == "max2"
        widths = []
        for ch in blk.order:
            last = ch[-1]
            if last == "pool":
                widths.append(cin)
            else:
                widths.append(sum(p[bname + "." + nm].cout for nm in (last if isinstance(last, tuple) else (last,))))
        oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if down else (h, w)
        out = x.new_empty((n, sum(widths), oh, ow))
        heads = self._conv(ctx, p[bname + ".heads"], x, 0) if bname + ".heads" in p else None
        hc0 = oc0 = 0
        for ch, width in zip(blk.order, widths):
            if ch[0] == "pool":
                if len(ch) == 1:
                    self._pool(ctx, x, "max", 2, out, oc0)
                else:
                    pooled = self._pool(ctx, x, blk.pool, 1)
                    self._conv(ctx, p[bname + "." + ch[1]], pooled, 0, out, oc0)
            elif len(ch) == 1:
                self._conv(ctx, p[bname + "." + ch[0]], x, 0, out, oc0)
            else:
                t, tc0 = heads, hc0
                hc0 += getattr(blk, ch[0]).cout
                for item in ch[1:-1]:
                    t, tc0 = self._conv(ctx, p[bname + "." + item], t, tc0), 0
                last = ch[-1]
                c0 = oc0
                for nm in (last if isinstance(last, tuple) else (last,)):
                    self._conv(ctx, p[bname + "." + nm], t, tc0, out, c0)
                    c0 += p[bname + "." + nm].cout
            oc0 += width
        return out

    def prepare_images(self, images):
        """-> fp32 [N,3,299,299] (or the input's size with resize_input=False) in [-1, 1).  Floats outside [0,1] are clamped to it
        before they become bytes (no range check: it would synchronise the stream)."""
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f"expected images [N,3,H,W]; got {tuple(images.shape)}")
        L, st = _backend(self._lib, images)
        if images.dtype != torch.uint8:
            if not images.is_floating_point():
                raise TypeError(f"images must be uint8 or floating point in [0,1]; got {images.dtype}")
            images = (images.float() * 255).clamp(0, 255).to(torch.uint8)  # trunc, torchmetrics' normalize=True
        oh, ow = (299, 299) if self.resize_input else images.shape[2:]
        if min(oh, ow) < 75:
            raise ValueError(f"the network needs images of at least 75 x 75; got {oh} x {ow}")
        self.launches += 1
        return M.resize_bilinear_tf1(L, st, images, oh, ow, mul=1.0 / 128, add=-1.0)

    @torch.inference_mode()
    def taps(self, images):
        """-> {64: [N,c(64)], 192: ..., ...}: every tap up to `feature`."""
        self.launches = 0
        x = self.prepare_images(images)
        L, st = _backend(self._lib, x)
        mode = conv_precision()
        if mode == "f16" and not InceptionV3._warned_f16:
            InceptionV3._warned_f16 = True
            warnings.warn('conv_precision "f16": InceptionV3 runs f16x3 operands in this mode too (fp16-rounded operands are not '
                          "accurate enough for a metric's features); there is no speed-up over \"f16x3\" here")
        ctx = (L, st, _NTERMS[mode])
        p = self.plan(L, st)
        x = M.conv2d_direct(L, st, x, p["first_w"], stride=2, pad=0, bias=p["first_b"], act=M.ACT_LRELU, alpha=0.0)
        self.launches += 1
        x = self._conv(ctx, p["Conv2d_2a_3x3"], x, 0)
        x = self._conv(ctx, p["Conv2d_2b_3x3"], x, 0)
        x = self._pool(ctx, x, "max", 2)
        out = {64: self._mean(ctx, x)}
        if self.feature == 64:
            return out
        x = self._conv(ctx, p["Conv2d_3b_1x1"], x, 0)
        x = self._conv(ctx, p["Conv2d_4a_3x3"], x, 0)
        x = self._pool(ctx, x, "max", 2)
        out[192] = self._mean(ctx, x)
        if self.feature == 192:
            return out
        for bname, blk in self._blocks():
            x = self._block(ctx, p, bname, blk, x)
            if bname == "Mixed_6e":
                out[768] = self._mean(ctx, x)
        if self.feature == 2048:
            out[2048] = self._mean(ctx, x)
        return out

    def forward(self, images):
        return self.taps(images)[self.feature]
