#!/usr/bin/env python
"""Times the device identity embedding (hairfastgan_amd.identity.IDLoss.extract_feats: crop, pool, IR-SE50 at 112^2, unit rows)
at batch 1, 8 and 32 against the reference's route on the same GPU - the same layer tables in eager torch on the module's own
parameters - and the embedding head alone (BatchNorm2d, Linear 25088 -> 512, BatchNorm1d as one folded Linear) on its two
routes, the 1x1-conv GEMM and hf_linear_f32, against the three eager layers; writes profiles/identity_bench.json together with
the kernel route every convolution of one forward pass took.  Device events around `--iters` back-to-back calls after a warm-up
of every shape, the routes alternating, median of `--rounds` windows; weights are seeded random (the timing does not depend on
their values).  Ratios are reported as measured, below 1 included.

    python tools/bench_identity.py [--iters 10] [--rounds 5] [--out profiles/identity_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd import identity as ID  # noqa: E402
from hairfastgan_amd.encoders import _fused as FU  # noqa: E402

BATCHES = (1, 8, 32)


def eager_unit(u, x):
    shortcut = x[:, :, ::u.stride, ::u.stride] if isinstance(u.shortcut_layer, nn.MaxPool2d) else u.shortcut_layer(x)
    r = u.res_layer[:5](x)
    se = u.res_layer[5]
    return r * torch.sigmoid(se.fc2(F.relu(se.fc1(r.mean((2, 3), keepdim=True))))) + shortcut


def eager_feats(idl, x):
    """pp_losses.py:278-282 and 215-219 in eager torch."""
    y0, x0, ch, cw = idl.crop
    net = idl.facenet
    x = F.adaptive_avg_pool2d(x[:, :, y0:y0 + ch, x0:x0 + cw], (net.input_size, net.input_size))
    x = net.input_layer(x)
    for u in net.body:
        x = eager_unit(u, x)
    x = net.output_layer(x)
    return x / torch.norm(x, 2, 1, True)


def record_routes(idl, x):
    """[k, cin, cout, input plane, stride, route, hands a pre-split result on] of every conv() of one forward pass, in call
    order; the route is what `_fused.conv_route` answers for the call."""
    from hairfastgan_amd.encoders import e4e

    seen = []
    inner = FU.conv

    def spy(x, w, k, stride=1, presplit=False, split_out=None, **kw):
        pre = isinstance(x, M.SplitActivation)
        h, wd = x.shape[-2], x.shape[-1]
        route = FU.conv_route(w, h, wd, k, stride, kw, pre, None if pre or x.dim() != 4 else x.shape[0])
        out = inner(x, w, k, stride, presplit, split_out, **kw)
        seen.append([k, w.cin_true, w.cout_true, h, stride, route, bool(split_out is not None and out[0] is not None)])
        return out

    FU.conv = e4e.conv = spy
    try:
        idl.extract_feats(x)
    finally:
        FU.conv = e4e.conv = inner
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_bench.json"))
    args = ap.parse_args()
    BC.require_gpu("bench_identity.py")
    dev = torch.device("cuda:0")
    L, st = _runtime.lib(), _runtime.stream()
    result = {"metric": "identity", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
              "conv_precision": _runtime.conv_precision(), "extract_feats": {}, "head": {}}
    g = torch.Generator().manual_seed(5)
    net = ID.Backbone(112, 50, "ir_se", drop_ratio=0.6)
    net.load_state_dict(BC.seeded_bn_state(net))
    idl = ID.IDLoss(net.to(dev))
    with torch.inference_mode():
        result["routes_batch1"] = record_routes(idl, (torch.rand(1, 3, 256, 256, generator=g) * 2 - 1).to(dev))
        for batch in BATCHES:
            x = (torch.rand(batch, 3, 256, 256, generator=g) * 2 - 1).to(dev)
            entry = BC.compare({"device": lambda: idl.extract_feats(x), "eager": lambda: eager_feats(idl, x)}, args.iters, args.rounds)
            entry["eager_over_device"] = round(entry["eager_ms"] / entry["device_ms"], 3)
            entry["max_component_difference"] = float((idl.extract_feats(x) - eager_feats(idl, x)).abs().max())
            result["extract_feats"][f"b{batch}"] = entry
            print("extract_feats", batch, json.dumps(entry), flush=True)
        # the head alone, on the activations the body hands it
        plan = net.plan()
        w_lin, b_lin = net._fold_head()
        for batch in BATCHES:
            feats = torch.randn(batch, 512, 7, 7, generator=g).to(dev)
            flat = feats.reshape(batch, -1)
            fns = {"conv_route": lambda: FU.conv(feats.reshape(batch, -1, 1, 1), plan["head"], 1, 1, bias=plan["head_bias"]),
                   "linear_route": lambda: M.linear(L, st, flat, w_lin, b_lin),
                   "eager": lambda: net.output_layer(feats)}
            entry = BC.compare(fns, args.iters, args.rounds)
            a, b, c = (fn().reshape(batch, -1) for fn in fns.values())
            entry["conv_minus_eager"], entry["linear_minus_eager"] = float((a - c).abs().max()), float((b - c).abs().max())
            entry["conv_route_kernel"] = FU.conv_route(plan["head"], 1, 1, 1, 1, {"bias": plan["head_bias"]}, batch=batch)
            result["head"][f"b{batch}"] = entry
            print("head", batch, json.dumps(entry), flush=True)
    result["note"] = ("device: IDLoss.extract_feats (hf_crop_avgpool_f32, the fused IR-SE units, the folded head, "
                      "hf_l2_normalize_rows_f32); eager: the reference's layers in eager torch on the same GPU and parameters; head: "
                      "the folded Linear as a 1x1 conv through the route table (what the product runs), as hf_linear_f32, and the "
                      "three eager layers; device events around back-to-back calls, the routes alternating, medians of the windows")
    print(json.dumps(result))
    BC.write_json(args.out, result)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
