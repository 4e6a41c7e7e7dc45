#!/usr/bin/env python
"""Times the device FID Inception-v3 (hairfastgan_amd.inception.InceptionV3(2048): resize to 299^2, 94 conv layers, pools, the
2048-wide tap) at batch 1, 32 and 128 against the same layer tables in eager torch on the same GPU and parameters, counts the
kernel launches of one forward pass, and times FrechetDistance.compute() at d = 2048 with 2000 samples a side; writes
profiles/inception_bench.json.  Device events around `--iters` back-to-back calls after a warm-up of every shape, the routes
alternating, median of `--rounds` windows; weights are seeded random (the timing does not depend on their values).  Ratios are
reported as measured, below 1 included.

    python tools/bench_inception.py [--rounds 3] [--no_frechet] [--out profiles/inception_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd.inception import InceptionV3  # noqa: E402
from hairfastgan_amd.metrics import FrechetDistance  # noqa: E402

BATCHES = {1: 10, 32: 3, 128: 2}  # batch -> calls per window


def eager_bc(m, x):
    return F.relu(m.bn(m.conv(x)))


def eager_block(blk, x):
    outs = []
    for ch in blk.order:
        if ch[0] == "pool":
            if blk.pool == "max2":
                p = F.max_pool2d(x, 3, 2)
            elif blk.pool == "avg":
                p = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
            else:
                p = F.max_pool2d(x, 3, 1, 1)
            outs.append(eager_bc(getattr(blk, ch[1]), p) if len(ch) > 1 else p)
            continue
        t = x
        for item in ch:
            if isinstance(item, tuple):
                outs.extend(eager_bc(getattr(blk, nm), t) for nm in item)
                t = None
            else:
                t = eager_bc(getattr(blk, item), t)
        if t is not None:
            outs.append(t)
    return torch.cat(outs, 1)


def eager_features(net, images):
    """The network in eager torch (torch's own bilinear resize stands in for the TF1 one: the same cost)."""
    x = F.interpolate(images.float(), size=(299, 299), mode="bilinear", align_corners=False)
    x = (x - 128) / 128
    x = eager_bc(net.Conv2d_2b_3x3, eager_bc(net.Conv2d_2a_3x3, eager_bc(net.Conv2d_1a_3x3, x)))
    x = F.max_pool2d(x, 3, 2)
    x = eager_bc(net.Conv2d_4a_3x3, eager_bc(net.Conv2d_3b_1x1, x))
    x = F.max_pool2d(x, 3, 2)
    for _, blk in net._blocks():
        x = eager_block(blk, x)
    return x.mean((2, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no_frechet", action="store_true", help="skip the d = 2048 FrechetDistance.compute() timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception_bench.json"))
    args = ap.parse_args()
    BC.require_gpu("bench_inception.py")
    dev = torch.device("cuda:0")
    result = {"metric": "inception_fid", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "conv_precision": _runtime.conv_precision(), "features_2048": {}}
    g = torch.Generator().manual_seed(5)
    net = InceptionV3(2048)
    net.load_state_dict(BC.seeded_bn_state(net))
    net = net.to(dev)

    with torch.inference_mode():
        for batch, iters in BATCHES.items():
            x = torch.randint(0, 256, (batch, 3, 299, 299), generator=g).to(torch.uint8).to(dev)
            entry = BC.compare({"device": lambda: net(x), "eager": lambda: eager_features(net, x)}, iters, args.rounds)
            entry["iters"] = iters
            entry["eager_over_device"] = round(entry["eager_ms"] / entry["device_ms"], 3)
            entry["images_per_s_device"] = round(1000.0 * batch / entry["device_ms"], 1)
            entry["max_feature_difference"] = float((net(x) - eager_features(net, x)).abs().max())
            result["features_2048"][f"b{batch}"] = entry
            result["launches_per_forward"] = net.launches
            print("features_2048", batch, json.dumps(entry), flush=True)
            BC.write_json(args.out, result)
        if not args.no_frechet:
            fid = FrechetDistance(lambda f: f)
            fid.update_features((torch.randn(2000, 2048, generator=g) * 0.3 + 0.5).to(dev), True)
            fid.update_features((torch.randn(2000, 2048, generator=g) * 0.35 + 0.45).to(dev), False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = float(fid.compute())
            torch.cuda.synchronize()
            result["frechet_compute_d2048_n2000"] = {"seconds": round(time.perf_counter() - t0, 3), "value": value,
                                                     "info": {k: (v if isinstance(v, (int, float, str)) else str(v))
                                                              for k, v in (fid.last_info or {}).items()}}
            print("frechet", json.dumps(result["frechet_compute_d2048_n2000"]), flush=True)
    result["note"] = ("device: InceptionV3(2048) on uint8 [B,3,299,299] (hf_resize_bilinear_tf1_f32, hf_conv2d_direct_f32, "
                      "hf_conv2d_rect_f16_f32, hf_pool3x3_f32, hf_plane_mean_f32); eager: the same module tree's layers in eager torch "
                      "on the same GPU and parameters; device events around back-to-back calls, the routes alternating, medians of "
                      "the windows; frechet: one FrechetDistance.compute() (two Jacobi eigensolves) timed on the host around a "
                      "device synchronisation")
    print(json.dumps(result))
    BC.write_json(args.out, result)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
