"""Identity similarity on the device: is the person still the same person (losses/pp_losses.py:267-296 `IDLoss`, its
three-argument form models/encoder4editing/criteria/id_loss.py; the network `Backbone(112, 50, mode="ir_se")`,
pp_losses.py:174-219 and models/encoder4editing/models/encoders/model_irse.py, weights pretrained_models/ArcFace/ir_se50.pth).

    python -m hairfastgan_amd.identity --data_path DIR --gt_path DIR [--size 256] [--image_decoder pil|device] [--batch 8]
                                       [--weights PATH]

Pieces, all on the library's kernels:
  images -> 112^2 faces   hf_crop_avgpool_f32: the crop [35:223, 32:220] and AdaptiveAvgPool2d((112, 112)) in one launch
  faces -> embeddings     the input layer and the 24 `bottleneck_IR_SE` units of `encoders.e4e` (the same fused units, unit
                          chain and conv route table), then `output_layer` as ONE Linear that carries both BatchNorms (folded
                          once per checkpoint) through the same route table, then hf_l2_normalize_rows_f32
  embeddings -> scores    hf_row_similarity_f64: the N pair similarities or the [N,M] matrix, summed in fp64
Inference only: Dropout is the identity and the BatchNorms use their running statistics.

`lib=None`: the loaded HIP library on torch's current stream.  Tests hand in the CPU interpreter build of the same kernel
sources; the network's layers go through `encoders._fused`, which asks `_fused.lib()`.
"""
import argparse

import torch
from torch import nn

from . import _marshal as M
from .encoders import _fused as FU
from .encoders.e4e import _IR_UNITS, bottleneck_IR_SE
from .metrics import _backend, add_pair_arguments, score_pairs, unit_range

CROP = (35, 32, 188, 188)  # (y0, x0, height, width): x[:, :, 35:223, 32:220], the face of a 256^2 aligned image


class Backbone(FU.FrozenPlanMixin, nn.Module):
    """pp_losses.py:174-219 with the reference's module tree, so that ir_se50.pth loads with `load_state_dict` (397 entries).
    forward(x [N,3,S,S] fp32) -> unit rows [N,512].

    units: an extension for tests - the body as a list of (in_channel, depth, stride) instead of the 24 units of IR-SE50;
    input_size may then be any multiple of the product of the strides and the Linear layer is sized to match."""

    def __init__(self, input_size=112, num_layers=50, mode="ir_se", drop_ratio=0.4, affine=True, *, units=None):
        super().__init__()
        if num_layers not in _IR_UNITS or mode != "ir_se":
            raise NotImplementedError(f"Backbone({input_size}, {num_layers}, mode='{mode}'): the reference's IDLoss uses "
                                      "Backbone(112, 50, mode='ir_se'); other depths and the plain 'ir' units are not built")
        units = _IR_UNITS[num_layers] if units is None else [tuple(u) for u in units]
        stride = 1
        for _, _, s in units:
            stride *= s
        if units is _IR_UNITS[num_layers]:
            if input_size not in (112, 224):
                raise ValueError("input_size should be 112 or 224")
        elif input_size <= 0 or input_size % stride or units[0][0] != 64:
            raise ValueError(f"units {units}: input_size must be a multiple of {stride} and the first unit takes 64 channels")
        self.input_size = input_size
        self.out_plane = input_size // stride
        depth = units[-1][1]
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, (3, 3), 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(depth), nn.Dropout(drop_ratio), nn.Flatten(),
                                          nn.Linear(depth * self.out_plane * self.out_plane, 512), nn.BatchNorm1d(512, affine=affine))
        self.body = nn.Sequential(*[bottleneck_IR_SE(i, d, s) for (i, d, s) in units])
        for p in self.parameters():
            p.requires_grad = False
        self._plan = None

    def _fold_head(self):
        """BatchNorm1d(Linear(flatten(BatchNorm2d(x)))) = W' x + b' with, in fp64 and rounded once,
        W'[o, (c, p)] = A[o] W[o, (c, p)] s[c] and b' = A (W t + b) + B: (s, t) the BatchNorm2d's affine per channel,
        (A, B) the BatchNorm1d's per output."""
        bn2, _, _, lin, bn1 = self.output_layer

        def affine(bn):
            sc = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
            if bn.weight is not None:
                sc = sc * bn.weight.detach().double()
            sh = -bn.running_mean.double() * sc
            return sc, (sh if bn.bias is None else sh + bn.bias.detach().double())

        s, t = affine(bn2)
        a, b = affine(bn1)
        px = self.out_plane * self.out_plane
        w = lin.weight.detach().double()
        bias = a * (w @ t.repeat_interleave(px) + lin.bias.detach().double()) + b
        w = a[:, None] * w * s.repeat_interleave(px)[None, :]
        return w.float().contiguous(), bias.float().contiguous()

    def plan(self):
        if self._plan is None:
            il = self.input_layer
            w, bias = self._fold_head()
            p = {"w_in": FU.prep_conv(il[0], pad=True), "bn_in": FU.fold_bn(il[1]), "slope_in": il[2].weight.detach(),
                 "head_bias": bias}
            p["head"] = FU.PreparedConv(M.conv_prepare(FU.lib(), FU.stream(), w.reshape(*w.shape, 1, 1)), 1)
            self._plan = p
        return self._plan

    @torch.inference_mode()
    def embed(self, x):
        """The embedding before l2_norm: [N,512]."""
        if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] != self.input_size or x.shape[3] != self.input_size:
            raise ValueError(f"expected faces [N,3,{self.input_size},{self.input_size}]; got {tuple(x.shape)}")
        FU.require_gpu(x)
        p = self.plan()
        x = FU.conv(x.float(), p["w_in"], 3, 1, out_scale=p["bn_in"][0], bias=p["bn_in"][1], act=M.ACT_PRELU, slope=p["slope_in"])
        xs = None
        for i, unit in enumerate(self.body):  # the unit chain of Encoder4Editing.forward
            nxt = self.body[i + 1] if i + 1 < len(self.body) else None
            oh, ow = (x.shape[2] - 1) // unit.stride + 1, (x.shape[3] - 1) // unit.stride + 1
            x, xs = unit.forward_chain(x, xs, nxt if (nxt is not None and nxt.takes_split(oh, ow)) else None)
        n = x.shape[0]
        # one route at every batch (a sample's bits do not change with its batch): the 1x1 GEMM reads the 51 MB of weights once
        # per launch, hf_linear_f32 once per 8 rows (DESIGN.md 4.28 has both measured)
        return FU.conv(x.reshape(n, -1, 1, 1), p["head"], 1, 1, bias=p["head_bias"]).reshape(n, -1)

    @torch.inference_mode()
    def forward(self, x):
        return M.l2_normalize_rows(FU.lib(), FU.stream(), self.embed(x))


class IDLoss(nn.Module):
    """pp_losses.py:267-296 (two arguments) and e4e's criteria/id_loss.py (three).  facenet: a `Backbone` with its weights
    loaded (default: Backbone(112, 50, drop_ratio=0.6, mode="ir_se") with the file `checkpoints.arcface()` finds).
    crop: (y0, x0, height, width) of the face inside the images, default the reference's [35:223, 32:220] of a 256^2 image;
    it is average-pooled to the facenet's input size."""

    def __init__(self, facenet=None, lib=None, crop=None):
        super().__init__()
        if facenet is None:
            from .checkpoints import arcface

            facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se")
            facenet.load_state_dict(arcface())
        self.facenet = facenet.eval()
        self.crop = tuple(CROP if crop is None else crop)
        self._lib = lib

    @torch.inference_mode()
    def extract_feats(self, x):
        """Images [N,3,H,W] fp32 in [-1,1] -> unit embeddings [N,512]."""
        y0, x0, ch, cw = self.crop
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError(f"expected images [N,3,H,W]; got {tuple(x.shape)}")
        if x.shape[2] < y0 + ch or x.shape[3] < x0 + cw:
            raise ValueError(f"images of {x.shape[2]} x {x.shape[3]} do not hold the face crop [{y0}:{y0 + ch}, {x0}:{x0 + cw}] "
                             "(the reference crops 256^2 images; downsample 1024^2 results by 4 first)")
        L, st = _backend(self._lib, x)
        size = self.facenet.input_size
        return self.facenet(M.crop_avgpool(L, st, x.float(), y0, x0, ch, cw, size, size))

    @torch.inference_mode()
    def similarity(self, y_hat, y):
        """[N] float64: the cosine similarity of each pair's embeddings."""
        if y_hat.shape != y.shape:
            raise ValueError(f"the two image batches differ in shape: {tuple(y_hat.shape)}, {tuple(y.shape)}")
        L, st = _backend(self._lib, y_hat, y)
        return M.row_similarity(L, st, self.extract_feats(y_hat), self.extract_feats(y), paired=True)

    @torch.inference_mode()
    def similarity_matrix(self, a, b):
        """[N,M] float64: every image of a against every image of b."""
        L, st = _backend(self._lib, a, b)
        return M.row_similarity(L, st, self.extract_feats(a), self.extract_feats(b), paired=False)

    @torch.inference_mode()
    def forward(self, y_hat, y, x=None):
        """(y_hat, y) -> 0-d fp32 mean(1 - similarity); (y_hat, y, x) -> (loss, sim_improvement, id_logs) of e4e."""
        L, st = _backend(self._lib, y_hat, y)
        f_hat, f_y = self.extract_feats(y_hat), self.extract_feats(y)
        target = M.row_similarity(L, st, f_hat, f_y, paired=True)
        loss = ((1.0 - target).sum() / target.shape[0]).float()
        if x is None:
            return loss
        f_x = self.extract_feats(x)
        rows = torch.stack([target, M.row_similarity(L, st, f_hat, f_x), M.row_similarity(L, st, f_y, f_x)]).tolist()
        id_logs = [{"diff_target": t, "diff_input": i, "diff_views": v} for t, i, v in zip(*rows)]
        improvement = sum(d["diff_target"] - d["diff_views"] for d in id_logs) / len(id_logs)
        return loss, improvement, id_logs


def main(argv=None, model=None, lib=None, device=None):
    """Scores every file of --data_path against the file of the same name in --gt_path and writes
    inference_metrics/scores_id.json (file -> similarity) and stat_id.txt next to --data_path (`metrics.score_pairs`).
    `model`: an IDLoss (default: the IR-SE50 with the weights of --weights or of `checkpoints.arcface`).
    -> {file name: similarity}."""
    parser = argparse.ArgumentParser(prog="python -m hairfastgan_amd.identity", description="identity similarity of a folder of results")
    add_pair_arguments(parser, batch=8)
    parser.add_argument("--weights", type=str, default=None, help="ir_se50.pth (default: pretrained_models/ArcFace/ir_se50.pth)")
    args = parser.parse_args(argv)

    def score(res, gt):
        nonlocal model
        if model is None:
            from .checkpoints import ARCFACE_PATH, arcface

            facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se")
            facenet.load_state_dict(arcface(path=args.weights or ARCFACE_PATH))
            model = IDLoss(facenet.to(device if device is not None else "cuda"), lib=lib)
        return model.similarity(unit_range(res), unit_range(gt))

    return score_pairs(args, score, "id", "Average similarity is {:.2f}+-{:.2f}", device, lib)


if __name__ == "__main__":
    main()
