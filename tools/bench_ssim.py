#!/usr/bin/env python
"""Times the device SSIM (hairfastgan_amd.ssim.ssim, uint8 images, the default Gaussian window) at 256^2 and 1024^2, batch 1 and
32, and MS-SSIM at 1024^2, batch 1 and 8, against two yardsticks taken in the same run on the same GPU, and writes
profiles/ssim_bench.json:
  eager   the same formula in eager torch fp64 - five separable conv2d pairs plus the elementwise tail (F.avg_pool2d between the
          scales of MS-SSIM): the route a user has today
  copy    a device-to-device copy of the bytes the kernel must read (both uint8 images once; for MS-SSIM the first level only),
          as the floor
Device events around `--iters` back-to-back calls (a quarter of that, at least one, from 8 Mi pixels per batch upwards: each
entry records its own `iters`) after a warm-up of every shape, the three routes alternating, median of `--rounds` windows.
Ratios are reported as measured, below 1 included; `copy_over_device` is the achieved fraction of the copy rate.  The device figures include the launches (two or three per scale), the workspace and output allocations and the few
elementwise torch operations of the host function.

    python tools/bench_ssim.py [--iters 10] [--rounds 5] [--out profiles/ssim_bench.json]
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
from hairfastgan_amd import ssim as SS  # noqa: E402

SSIM_CASES = ((256, 1), (256, 32), (1024, 1), (1024, 32))
MS_SSIM_CASES = ((1024, 1), (1024, 8))


def eager_maps(x, y, taps, c1, c2, cn):
    """x, y [P,1,H,W] float64 -> (S, cs) maps, in the expression order of the kernel."""
    f = lambda z: F.conv2d(F.conv2d(z, taps.view(1, 1, 1, -1)), taps.view(1, 1, -1, 1))  # noqa: E731
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    a2, b2 = 2 * vxy + c2, vx + vy + c2
    return ((2 * ux * uy + c1) * a2) / ((ux * ux + uy * uy + c1) * b2), a2 / b2


def eager_ssim(x, y, taps, c1, c2, cn=1.0):
    n, c, h, w = x.shape
    s, _ = eager_maps(x.double().reshape(n * c, 1, h, w), y.double().reshape(n * c, 1, h, w), taps, c1, c2, cn)
    return s.mean((1, 2, 3)).reshape(n, c).mean(1)


def eager_ms_ssim(x, y, taps, c1, c2, weights=SS.MS_SSIM_WEIGHTS):
    n, c, h, w = x.shape
    x, y = x.double().reshape(n * c, 1, h, w), y.double().reshape(n * c, 1, h, w)
    vals = []
    for j, wt in enumerate(weights):
        s, cs = eager_maps(x, y, taps, c1, c2, 1.0)
        vals.append((s if j == len(weights) - 1 else cs).mean((1, 2, 3)).clamp_min(0) ** wt)
        x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return torch.stack(vals).prod(0).reshape(n, c).mean(1)


def compare(device_fn, eager_fn, copy_fn, iters, rounds):
    t = BC.compare({"device": device_fn, "eager": eager_fn, "copy": copy_fn}, iters, rounds)
    t["eager_over_device"] = round(t["eager_ms"] / t["device_ms"], 3)
    t["copy_over_device"] = round(t["copy_ms"] / t["device_ms"], 4)
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    args = ap.parse_args()
    BC.require_gpu("bench_ssim.py")
    dev = torch.device("cuda:0")
    result = {"metric": "ssim", "device": torch.cuda.get_device_name(0), "iters_requested": args.iters, "rounds": args.rounds, "ssim": {},
              "ms_ssim": {}}
    g = torch.Generator().manual_seed(5)
    taps = torch.tensor(SS.window_taps("gaussian")[0], dtype=torch.float64, device=dev)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    with torch.inference_mode():
        for name, cases, device_fn, eager_fn in (("ssim", SSIM_CASES, SS.ssim, eager_ssim), ("ms_ssim", MS_SSIM_CASES, SS.ms_ssim, eager_ms_ssim)):
            for size, batch in cases:
                x = torch.randint(0, 256, (batch, 3, size, size), generator=g, dtype=torch.uint8)
                y = (x.int() + torch.randint(-24, 25, x.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8).to(dev)
                x = x.to(dev)
                src, dst = torch.stack([x, y]), torch.empty((2,) + tuple(x.shape), dtype=torch.uint8, device=dev)
                iters = max(1, args.iters // (4 if size * size * batch >= 8 << 20 else 1))
                try:
                    entry = compare(lambda: device_fn(x, y), lambda: eager_fn(x, y, taps, c1, c2), lambda: dst.copy_(src), iters, args.rounds)
                    entry["max_difference"] = float((device_fn(x, y) - eager_fn(x, y, taps, c1, c2)).abs().max())
                except RuntimeError as e:  # e.g. the eager route out of memory
                    entry = {"error": str(e).splitlines()[0]}
                entry["iters"] = iters
                entry["read_bytes"] = src.numel()
                if "device_ms" in entry:
                    entry["device_GBps_of_read_bytes"] = round(src.numel() / entry["device_ms"] / 1e6, 1)
                    entry["copy_GBps_read_plus_write"] = round(2 * src.numel() / entry["copy_ms"] / 1e6, 1)
                result[name][f"{size}_b{batch}"] = entry
                print(name, size, batch, json.dumps(entry), flush=True)
                del x, y, src, dst
                torch.cuda.empty_cache()
    result["note"] = ("device: hairfastgan_amd.ssim on uint8 images, Gaussian 11 window (one fused fp64 launch plus the finish per scale, with "
                      "the allocations of a call); eager: the same formula in eager torch fp64 on the same GPU; copy: a device-to-device "
                      "copy of the bytes the kernel reads; device events around back-to-back calls, the routes alternating, medians of "
                      "the windows")
    print(json.dumps(result))
    BC.write_json(args.out, result)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
