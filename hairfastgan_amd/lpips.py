"""LPIPS and L2 / PSNR on the device: how close a result is to a target image (losses/pp_losses.py:375-529 `LPIPS`, also
models/encoder4editing/criteria/lpips, models/FeatureStyleEncoder/lpips, losses/lpips; the scoring command line
models/encoder4editing/scripts/calc_losses_on_images.py).

    python -m hairfastgan_amd.lpips --data_path DIR --gt_path DIR [--mode lpips|l2|psnr|ssim|ms_ssim] [--net alex|vgg]
                                    [--ssim_window gaussian|uniform] [--size 256] [--image_decoder pil|device] [--batch 4]

Pieces, all on the library's kernels:
  images -> features      the AlexNet / VGG16 `features` towers (published layer tables): the first layer with the z-score as
                          its input affine by hf_conv2d_direct_f32, every 3x3 layer through `encoders._fused.conv` (the fp16
                          matrix-core routes), AlexNet's 5x5 layer as a GEMM over unfolded patches, hf_maxpool2d_f32 between
  features -> distance    hf_lpips_layer_f64 per tap: normalise, subtract, square, weigh and average in one launch
  L2 / PSNR               hf_sq_err_sum_f64
  SSIM / MS-SSIM          `hairfastgan_amd.ssim` (hf_ssim_planes_f64); here only the command line's two modes
The SqueezeNet tower, the masked and the scale-weighted variants and everything with gradients are not part of this backend.

`lib=None`: the loaded HIP library on torch's current stream.  Tests hand in the CPU interpreter build of the same kernel
sources; the tower's 3x3 layers go through `encoders._fused`, which asks `_fused.lib()`.
"""
import argparse

import torch
from torch import nn

from . import _marshal as M
from .encoders import _fused as FU
from .metrics import _backend, add_pair_arguments, score_pairs, unit_range
from .metrics import load_pairs  # noqa: F401  re-exported: callers name hairfastgan_amd.lpips.load_pairs

ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
              (10, 256, 256, 3, 1, 1))  # torchvision alexnet.features: (index, cin, cout, k, stride, pad)
ALEX_POOL_BEFORE = (3, 6)             # MaxPool2d(3, 2) in front of these convs
VGG_CONVS = tuple((i, ci, co, 3, 1, 1) for i, ci, co in (
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
    (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)))
VGG_POOL_BEFORE = (5, 10, 17, 24)     # MaxPool2d(2, 2)
VGG_TAPS = (2, 7, 14, 21, 28)         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 follow these convs
TOWERS = {"alex": (ALEX_CONVS, ALEX_POOL_BEFORE, 3, tuple(c[0] for c in ALEX_CONVS)), "vgg": (VGG_CONVS, VGG_POOL_BEFORE, 2, VGG_TAPS)}
MEAN = (-0.030, -0.088, -0.188)       # pp_losses.py:404-409
STD = (0.458, 0.448, 0.450)


class _Tower(nn.Module):
    """`net` of the reference's LPIPS: `layers.<i>` = the convolutions of torchvision's `features` under their indices,
    `mean` and `std` of the z-score.  forward -> the activations after the ReLU of the tapped convolutions (not normalised:
    hf_lpips_layer_f64 does that)."""

    def __init__(self, net_type):
        super().__init__()
        self.convs, self.pool_before, self.pool_k, self.taps = TOWERS[net_type]
        self.layers = nn.ModuleDict({str(i): nn.Conv2d(ci, co, k, s, p) for i, ci, co, k, s, p in self.convs})
        self.register_buffer("mean", torch.tensor(MEAN)[None, :, None, None])
        self.register_buffer("std", torch.tensor(STD)[None, :, None, None])
        self.n_channels_list = [co for i, _, co, _, _, _ in self.convs if i in self.taps]

    def plan(self):
        std = self.std.detach().reshape(-1).float()
        plan = {"in_scale": (1.0 / std).contiguous(), "in_shift": (-self.mean.detach().reshape(-1).float() / std).contiguous()}
        for i, ci, co, k, _, _ in self.convs[1:]:
            conv = self.layers[str(i)]
            if k == 3:
                plan[i] = FU.prep_conv(conv)
            else:  # AlexNet's 5x5: the GEMM over `patches`, K = k*k*cin ordered (tap, ci); re-laid once
                w = conv.weight.detach().permute(0, 2, 3, 1).reshape(co, k * k * ci, 1, 1).contiguous()
                plan[i] = FU.PreparedConv(M.conv_prepare(FU.lib(), FU.stream(), w), 1)
        return plan

    def forward(self, x, plan, L, st):
        out = []
        for n, (i, _, _, k, s, p) in enumerate(self.convs):
            conv = self.layers[str(i)]
            if i in self.pool_before:
                x = M.maxpool2d(L, st, x, self.pool_k, 2)
            bias = conv.bias.detach()
            if n == 0:
                x = M.conv2d_direct(L, st, x, conv.weight.detach(), s, p, plan["in_scale"], plan["in_shift"], bias, M.ACT_LRELU, 0.0)
            elif k == 3:
                x = FU.conv(x, plan[i], 3, 1, bias=bias, act=M.ACT_LRELU, alpha=0.0)
            else:
                x = FU.conv(FU.patches(x, k, s, p), plan[i], 1, 1, bias=bias, act=M.ACT_LRELU, alpha=0.0)
            if i in self.taps:
                out.append(x)
        return out


class LPIPS(FU.FrozenPlanMixin, nn.Module):
    """pp_losses.py:498-526 with the reference module's state-dict keys: `net.layers.<i>.weight|bias`, `net.mean`, `net.std`,
    `lin.<j>.1.weight` [1,C,1,1].  Weights are frozen; nothing is downloaded: `load_pretrained(*checkpoints.lpips_weights())`
    or `load_state_dict` fills them.

    forward(x, y): images [N,3,H,W] fp32 in [-1,1] -> 0-d fp32, the sum over layers and batch divided by N.
    per_sample(x, y) -> [N] float64 on the device."""

    def __init__(self, net_type="alex", version="0.1", lib=None):
        if version != "0.1":
            raise ValueError("v0.1 is only supported now")
        if net_type == "squeeze":
            raise NotImplementedError("net_type 'squeeze': the SqueezeNet tower is not part of this backend; choose alex or vgg")
        if net_type not in TOWERS:
            raise NotImplementedError("choose net_type from [alex, vgg].")
        super().__init__()
        self.net_type = net_type
        self.net = _Tower(net_type)
        self.lin = nn.ModuleList([nn.Sequential(nn.Identity(), nn.Conv2d(nc, 1, 1, 1, 0, bias=False)) for nc in self.net.n_channels_list])
        for p in self.parameters():
            p.requires_grad = False
        self._lib = lib
        self._plan = None

    def load_pretrained(self, features_state_dict, lin_state_dict):
        """torchvision's `features.<i>.weight|bias` and the published `lin<j>.model.1.weight`, renamed as the reference's
        get_state_dict does (pp_losses.py:488-496: "lin" and "model." are dropped)."""
        own = {"net.mean": self.net.mean, "net.std": self.net.std}
        for k, v in features_state_dict.items():
            if k.startswith("features."):
                own["net.layers." + k[len("features."):]] = v.float()
        for k, v in lin_state_dict.items():
            own["lin." + k.replace("lin", "").replace("model.", "")] = v.float()
        return self.load_state_dict(own)

    def features(self, x):
        """The tapped activations of images [N,3,H,W]."""
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError(f"expected images [N,3,H,W]; got {tuple(x.shape)}")
        L, st = _backend(self._lib, x)
        if self._plan is None:
            self._plan = self.net.plan()
        return self.net(x.float(), self._plan, L, st)

    @torch.inference_mode()
    def per_sample(self, x, y):
        if x.shape != y.shape:
            raise ValueError(f"the two image batches differ in shape: {tuple(x.shape)}, {tuple(y.shape)}")
        L, st = _backend(self._lib, x, y)
        fx, fy = self.features(x), self.features(y)  # two calls of one shape: equal inputs give equal bits
        dist = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        for j, (a, b) in enumerate(zip(fx, fy)):
            M.lpips_layer_into(L, st, dist, a, b, self.lin[j][1].weight.detach().reshape(-1), accumulate=j > 0)
        return dist

    @torch.inference_mode()
    def forward(self, x, y):
        return (self.per_sample(x, y).sum() / x.shape[0]).float()


@torch.inference_mode()
def mse(x, y, lib=None):
    """[N] float64: the mean squared error of each image pair; x, y [N,...] both uint8 or both fp32."""
    L, st = _backend(lib, x, y)
    return M.sq_err_sum(L, st, x, y) / (x.numel() // max(x.shape[0], 1))


@torch.inference_mode()
def psnr(x, y, data_range=None, lib=None):
    """[N] float64: 10 log10(data_range^2 / mse).  uint8 images have a data range of 255; float images need an explicit
    one.  Equal images give inf."""
    if data_range is None:
        if x.dtype != torch.uint8:
            raise ValueError("float images need an explicit data_range")
        data_range = 255.0
    return 10.0 * torch.log10(float(data_range) ** 2 / mse(x, y, lib))


def main(argv=None, model=None, lib=None, device=None):
    """The command line of calc_losses_on_images.py: scores every file of --data_path against the file of the same name in
    --gt_path and writes inference_metrics/scores_<mode>.json and stat_<mode>.txt next to --data_path (`metrics.score_pairs`).
    `model`: the LPIPS module (default: LPIPS(--net) with the weights `checkpoints.lpips_weights` finds).
    -> {file name: score}."""
    parser = argparse.ArgumentParser(prog="python -m hairfastgan_amd.lpips", description="LPIPS / L2 / PSNR / SSIM / MS-SSIM of a folder of results")
    parser.add_argument("--mode", choices=("lpips", "l2", "psnr", "ssim", "ms_ssim"), default="lpips")
    parser.add_argument("--net", choices=("alex", "vgg"), default="alex")
    parser.add_argument("--ssim_window", choices=("gaussian", "uniform"), default="gaussian", help="the window of --mode ssim / ms_ssim")
    add_pair_arguments(parser, batch=4)
    args = parser.parse_args(argv)

    def score(res, gt):
        nonlocal model
        if args.mode == "psnr":
            return psnr(res, gt, lib=lib)
        if args.mode == "l2":
            return mse(unit_range(res), unit_range(gt), lib)
        if args.mode in ("ssim", "ms_ssim"):  # on the bytes themselves (data range 255)
            from . import ssim as SS

            return getattr(SS, args.mode)(res, gt, window=args.ssim_window, lib=lib)
        if model is None:
            from .checkpoints import lpips_weights

            model = LPIPS(args.net, lib=lib)
            model.load_pretrained(*lpips_weights(args.net))
            model = model.to(device if device is not None else "cuda")
        return model.per_sample(unit_range(res), unit_range(gt))

    # SSIM differences live in the third decimal
    sentence = f"Average {args.mode} is {{:.4f}}+-{{:.4f}}" if args.mode in ("ssim", "ms_ssim") else "Average loss is {:.2f}+-{:.2f}"
    return score_pairs(args, score, args.mode, sentence, device, lib)


if __name__ == "__main__":
    main()
