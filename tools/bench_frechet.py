#!/usr/bin/env python
"""Times the device Frechet distance (hairfastgan_amd.metrics.FrechetDistance) at the size of FID-CLIP - d = 512, 2000
samples a side - and writes profiles/frechet_bench.json.  By the host clock, synchronised, warmed up, median of --iters:

* `compute()`: two hf_frechet_stats_f64, two Jacobi eigensolves around the congruence, the finish - the distance as a
  device double (the sweeps and launches of both solves are recorded);
* 32 `update_features` calls of 128 samples (hf_frechet_accumulate_f64);
* the host route the reference takes for the same statistics: sum / cov_sum copied to the CPU, torchmetrics' formula there
  with torch.linalg.eigvals in fp64 (as many CPU threads as torch uses by default);
* for context, the same formula with torch.linalg.eigvals on the device tensors.

    python tools/bench_frechet.py [--iters 5] [--out profiles/frechet_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import metrics as MT  # noqa: E402

D, N, BATCH = 512, 2000, 128


def host_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "iters": iters}


def reference_route(total1, cov1, n1, total2, cov2, n2):
    """torchmetrics' _compute_fid on whatever device the statistics are on."""
    mu1, mu2 = total1 / n1, total2 / n2
    s1 = (cov1 - n1 * torch.outer(mu1, mu1)) / (n1 - 1)
    s2 = (cov2 - n2 * torch.outer(mu2, mu2)) / (n2 - 1)
    a = (mu1 - mu2).square().sum()
    b = s1.trace() + s2.trace()
    c = torch.linalg.eigvals(s1 @ s2).sqrt().real.sum()
    return a + b - 2 * c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    mix = torch.randn(D, D, generator=g) / D ** 0.5
    real = (torch.randn(N, D, generator=g) @ mix + 0.3).to(dev)
    fake = (torch.randn(N, D, generator=g) * torch.linspace(0.2, 2.0, D) + 0.1).to(dev)
    fid = MT.FrechetDistance(lambda x: x)

    def updates():
        fid.reset()
        for k in range(32):
            fid.update_features(fake[(k * BATCH) % (N - BATCH):][:BATCH], real=False)

    result = {"metric": "frechet", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
              "torch_threads": torch.get_num_threads(), "d": D, "samples_per_side": N}
    result["update_features_32x128"] = host_ms(updates, args.warmup, args.iters)
    fid.reset()
    for side, feats in ((True, real), (False, fake)):
        for k in range(0, N, BATCH):
            fid.update_features(feats[k:k + BATCH], real=side)
    value = fid.compute()
    result["compute"] = host_ms(fid.compute, args.warmup, args.iters)
    sweeps = fid.last_info["sweeps"]
    result["compute"].update(distance=value.item(), sweeps=list(sweeps), launches=sum(s * (D - 1) + s + 3 for s in sweeps) + 8)

    (t1, c1, n1), (t2, c2, n2) = fid.state(True), fid.state(False)

    def host_route():
        return reference_route(t1.cpu(), c1.cpu(), N, t2.cpu(), c2.cpu(), N).item()

    def device_eigvals():
        return reference_route(t1, c1, N, t2, c2, N).item()

    ref = host_route()
    result["host_route_cpu_eigvals"] = host_ms(host_route, args.warmup, args.iters)
    result["host_route_cpu_eigvals"]["distance"] = ref
    try:
        on_device = device_eigvals()
        result["torch_eigvals_on_device"] = host_ms(device_eigvals, args.warmup, args.iters)
        result["torch_eigvals_on_device"]["distance"] = on_device
    except RuntimeError as e:  # no device eigvals in this torch build
        result["torch_eigvals_on_device"] = {"error": str(e).splitlines()[0]}
    result["relative_difference_to_host_route"] = abs(value.item() - ref) / max(1.0, abs(ref))
    result["host_over_device"] = round(result["host_route_cpu_eigvals"]["median_ms"] / result["compute"]["median_ms"], 3)
    result["note"] = ("compute(): hairfastgan_amd.metrics.FrechetDistance.compute() to a device double; host route: the statistics "
                      "copied to the CPU and torchmetrics' formula with torch.linalg.eigvals (fp64) there; all by the host clock, "
                      "synchronised")
    print(json.dumps(result))
    BC.write_json(args.out, result)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
