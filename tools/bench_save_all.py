#!/usr/bin/env python3
"""`--save_all` (hairfastgan_amd.hair_swap.SaveAllRecorder; csrc/export.h) on the GPU, synthetic weights.  Prints ONE JSON
line (kept as profiles/save_all_bench.json):

* `to_bytes` on [13,3,1024,1024] - the thirteen 1024^2 images one swap dumps - for both layouts and roundings: median
  time, bytes moved (12 read + 3 written per pixel) per second, next to a plain device-to-device copy of the same byte
  count timed in the same run; `labels_to_rgb` on [7,1,512,512];
* one swap with args.save_all on and off (median wall seconds, device-synchronised), and the recorder's share split into
  the two extra generator calls, quantisation + colouring, the copy to the host, and PNG / npz encoding on the host.

`--png_encoder device` runs the swap with the recorder's PNG files made on the GPU (csrc/png.h): "bytes_s" then holds the
encodes as well, "copy_s" the copy of the encoded files and "encode_s" only the file writes.

usage: python tools/bench_save_all.py [--reps N] [--swaps N] [--png_encoder {pil,device}]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (the synthetic HairFast of the flagship benchmark)
from hairfastgan_amd import hair_swap as HS  # noqa: E402
from hairfastgan_amd import image_utils as IU  # noqa: E402


def _time(fn, reps):
    """median milliseconds of `fn` between device events (after two warm-up calls)"""
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--swaps", type=int, default=5)
    ap.add_argument("--png_encoder", choices=("pil", "device"), default="pil")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_save_all needs a GPU"
    dev = torch.device("cuda:0")
    res = {"metric": "save_all", "device": torch.cuda.get_device_name(0), "png_encoder": a.png_encoder}
    # ---- the kernels ----
    x = torch.rand(13, 3, 1024, 1024, generator=torch.Generator().manual_seed(0)).mul(2).sub(1).to(dev)
    nbytes = x.numel() * 5  # 4 read + 1 written per element
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)  # a copy of n bytes moves 2 n: the same traffic
    dst = torch.empty_like(src)
    copy_ms = _time(lambda: dst.copy_(src), a.reps)
    kern = {"shape": list(x.shape), "bytes_moved": nbytes, "device_copy": {"ms": round(copy_ms, 4), "TBps": round(nbytes / copy_ms / 1e9, 3)}}
    with torch.inference_mode():
        for rounding in IU.ROUNDINGS:
            for layout in IU.LAYOUTS:
                vr = (-1, 1) if rounding == "floor" else (0, 1)
                ms = _time(lambda: IU.to_bytes(x, vr, rounding, layout), a.reps)
                kern[f"to_bytes_{rounding}_{layout}"] = {"ms": round(ms, 4), "TBps": round(nbytes / ms / 1e9, 3),
                                                        "fraction_of_copy": round(copy_ms / ms, 3)}
        # the torch composition of the reference, on the device (six elementwise launches and the permute copy)
        ms = _time(lambda: ((x + 1) / 2).clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous(), a.reps)
        kern["torch_composition_floor_hwc_ms"] = round(ms, 4)
        labels = torch.randint(0, 19, (7, 1, 512, 512), device=dev)
        kern["labels_to_rgb_7x512x512_ms"] = round(_time(lambda: IU.labels_to_rgb(labels), a.reps), 4)
    res["kernels"] = kern
    del x, src, dst
    # ---- one swap ----
    _, sd = bench.build_generator(dev)
    hf = bench.build_hairfast(sd, dev)
    g = torch.Generator().manual_seed(1)
    images = [torch.randint(0, 256, (3, 1024, 1024), dtype=torch.uint8, generator=g).to(dev) for _ in range(3)]
    out_dir = tempfile.mkdtemp(prefix="save_all_bench_")
    hf.args.save_all_dir = HS.Path(out_dir)
    hf.args.png_encoder = a.png_encoder

    def swap_s(save_all, times=None):
        hf.args.save_all = save_all
        HS.SAVE_ALL_TIMES = times
        torch.cuda.synchronize()
        t0 = time.time()
        hf.swap(*images, exp_name="bench")
        torch.cuda.synchronize()
        HS.SAVE_ALL_TIMES = None
        return time.time() - t0

    for on in (False, True, False, True):  # warm-up: lazily derived weights, allocator pools, the page cache of the files
        swap_s(on)
    off = [swap_s(False) for _ in range(a.swaps)]
    on = [swap_s(True) for _ in range(a.swaps)]
    split = []
    for _ in range(a.swaps):  # a run of its own: the split synchronises the device between the phases
        t = {}
        t["wall_s"] = swap_s(True, t)
        split.append(t)
    files = sorted(os.path.relpath(os.path.join(dp, f), out_dir) for dp, _, fs in os.walk(out_dir) for f in fs)
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    res["swap"] = {"save_all_off_s": med(off), "save_all_on_s": med(on), "files": len(files),
                   "file_bytes": sum(os.path.getsize(os.path.join(out_dir, f)) for f in files),
                   "split_s": {k: med([t[k] for t in split]) for k in ("forwards_s", "bytes_s", "copy_s", "encode_s", "wall_s")},
                   "note": "weights and images are synthetic: the PNG encoder sees noise-like images, a real face compresses faster"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
