"""What the tools/bench_*.py scripts state once: the timing windows, seeded BatchNorm statistics, the no-GPU exit and the JSON
epilogue.  Imported as `bench_common` by scripts run as `python tools/bench_<name>.py` (their own directory is on sys.path)."""
import json
import os
import statistics

import torch


def require_gpu(script):
    if not torch.cuda.is_available():
        raise SystemExit(f"{script} measures on the GPU; none found")


def window_ms(fn, iters):
    """Milliseconds per call: device events around `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(fns, iters, rounds):
    """fns: {name: callable}; the routes alternate inside every round -> {name_ms: median, name_min_max_ms: [...]}"""
    for fn in fns.values():
        fn()  # warm-up of every shape
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, iters))
    out = {}
    for k, t in times.items():
        out[f"{k}_ms"] = statistics.median(t)
        out[f"{k}_min_max_ms"] = [min(t), max(t)]
    return out


def device_ms(fn, warmup, iters):
    """Every call between device events of its own, after `warmup` calls and a synchronisation."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "iters": iters}


def time_ms(fn, reps):
    """median milliseconds of `fn` between device events (after three warm-up calls)"""
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(statistics.median(times))


def seeded_bn_state(model, seed=0):
    """torch's default init with BatchNorm statistics away from (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(model.state_dict())
    for k, v in sd.items():
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.02 * torch.randn(v.shape, generator=g)
    return sd


def write_json(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f)
        f.write("\n")
