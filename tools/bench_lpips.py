#!/usr/bin/env python
"""Times the device LPIPS (hairfastgan_amd.lpips.LPIPS.per_sample) at 256^2 and 1024^2, batch 1 and 32, for both towers, and
hf_lpips_layer_f64 alone, against the reference's route on the same GPU - the same layer tables in eager torch (z-score,
Conv2d / ReLU / MaxPool2d, then normalise x 2, subtract, square, 1x1 conv, mean: five passes per layer) - and writes
profiles/lpips_bench.json.  Device events around `--iters` back-to-back calls after a warm-up of every shape, the two routes
alternating, median of `--rounds` windows; weights are seeded random (the timing does not depend on their values).  Ratios are
reported as measured, below 1 included.  The layer kernel's bytes are the algorithm's: both maps once (C H W 8 bytes per
sample) over its time.

    python tools/bench_lpips.py [--iters 10] [--rounds 5] [--out profiles/lpips_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd import lpips as LP  # noqa: E402

LAYER_SHAPES = ((32, 64, 63, 63), (32, 256, 15, 15), (1, 64, 256, 256), (32, 64, 256, 256), (32, 512, 16, 16), (4, 64, 1024, 1024))


def seeded_state(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.startswith("lin."):
            sd[k] = torch.rand(v.shape, generator=g) * (2.0 / v.shape[1])
        elif k.endswith(".weight"):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
        else:
            sd[k] = v
    return sd


def eager_lpips(model, x, y):
    """The reference's route (pp_losses.py:415-428, 469-471, 520-526) in eager torch on the module's own parameters -> [N]."""
    net = model.net

    def tower(t):
        t = (t - net.mean) / net.std
        out = []
        for i, _, _, _, s, p in net.convs:
            if i in net.pool_before:
                t = F.max_pool2d(t, net.pool_k, 2)
            conv = net.layers[str(i)]
            t = F.relu(F.conv2d(t, conv.weight, conv.bias, s, p))
            if i in net.taps:
                out.append(t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10))
        return out

    res = [lin((a - b) ** 2).mean((2, 3), True) for a, b, lin in zip(tower(x), tower(y), model.lin)]
    return torch.cat(res, 1).sum((1, 2, 3))


def eager_layer(fx, fy, w):
    nx = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
    return F.conv2d((nx - ny) ** 2, w.reshape(1, -1, 1, 1)).mean((2, 3)).reshape(-1)


def compare(device_fn, eager_fn, iters, rounds):
    """bench_common.compare of the two routes, with their ratio, in this file's key order."""
    t = BC.compare({"device": device_fn, "eager": eager_fn}, iters, rounds)
    return {"device_ms": t["device_ms"], "eager_ms": t["eager_ms"], "eager_over_device": round(t["eager_ms"] / t["device_ms"], 3),
            "device_min_max_ms": t["device_min_max_ms"], "eager_min_max_ms": t["eager_min_max_ms"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    args = ap.parse_args()
    BC.require_gpu("bench_lpips.py")
    dev = torch.device("cuda:0")
    L, st = _runtime.lib(), _runtime.stream()
    result = {"metric": "lpips", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
              "conv_precision": _runtime.conv_precision(), "per_sample": {}, "layer": {}}
    g = torch.Generator().manual_seed(5)
    with torch.inference_mode():
        for net_type in ("alex", "vgg"):
            model = LP.LPIPS(net_type)
            model.load_state_dict(seeded_state(model))
            model = model.to(dev).eval()
            for size, batch in ((256, 1), (256, 32), (1024, 1), (1024, 32)):
                x = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).to(dev)
                y = (x + 0.1 * torch.randn(x.shape, generator=g).to(dev)).contiguous()
                iters = max(1, args.iters // (8 if size == 1024 and batch == 32 else 1))
                try:
                    entry = compare(lambda: model.per_sample(x, y), lambda: eager_lpips(model, x, y), iters, args.rounds)
                    a, b = model.per_sample(x, y), eager_lpips(model, x, y).double()
                    entry["max_relative_difference"] = float(((a - b).abs() / b.abs()).max())
                except RuntimeError as e:  # e.g. the eager route out of memory at 1024^2 x 32
                    entry = {"error": str(e).splitlines()[0]}
                result["per_sample"][f"{net_type}_{size}_b{batch}"] = entry
                print(net_type, size, batch, json.dumps(entry), flush=True)
                del x, y
                torch.cuda.empty_cache()
        for shape in LAYER_SHAPES:
            n, c, h, w = shape
            fx = torch.randn(shape, generator=g).clamp_min(0).to(dev)
            fy = torch.randn(shape, generator=g).clamp_min(0).to(dev)
            lin_w = (torch.rand(c, generator=g) * (2.0 / c)).to(dev)
            dist = torch.empty(n, dtype=torch.float64, device=dev)
            entry = compare(lambda: M.lpips_layer_into(L, st, dist, fx, fy, lin_w), lambda: eager_layer(fx, fy, lin_w), args.iters, args.rounds)
            nbytes = 8.0 * n * c * h * w
            entry["algorithmic_bytes"] = nbytes
            entry["device_GBps_incl_launch_and_allocation"] = round(nbytes / entry["device_ms"] / 1e6, 1)
            result["layer"]["x".join(map(str, shape))] = entry
            print(shape, json.dumps(entry), flush=True)
            del fx, fy
            torch.cuda.empty_cache()
    result["note"] = ("device: LPIPS.per_sample / hf_lpips_layer_f64 (two launches and a workspace allocation per call); eager: the "
                      "reference's route in eager torch on the same GPU and parameters; device events around back-to-back calls, "
                      "the routes alternating, medians of the windows")
    print(json.dumps(result))
    BC.write_json(args.out, result)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
