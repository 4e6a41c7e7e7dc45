#!/usr/bin/env python3
"""The device JPEG encoder (hf_jpeg_encode_u8; csrc/jpeg.h) against PIL (libjpeg on one core) on the host.  Prints ONE JSON
line (kept as profiles/jpeg_bench.json).

* uint8 [13,1024,1024,3] and [1,1024,1024,3] of the formula photograph of tests/png_checks.py (`photo(1024)`), at quality 75 /
  4:2:0 and quality 95 / 4:4:4;
* one 4000 x 6000 photograph from the same formula (a 4000-row crop of `photo(6000)`), at the same two settings -

the device time of the three launches by HIP events (median of --reps after warm-up; beside it the host clock around --reps
calls that end in a synchronise, per call), PIL's encode of the same image with
the same arguments and restart_marker_rows=1 on the same host (median wall seconds over --host_reps), the file size (the
device file must EQUAL PIL's, byte for byte) and, beside it, the size of the device PNG of the same image.

usage: python tools/bench_jpeg.py [--reps N] [--host_reps N]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd._runtime import lib, stream  # noqa: E402
from tests import png_checks as K  # noqa: E402

SETTINGS = [(75, "4:2:0"), (95, "4:4:4")]


def _wall(fn, reps):
    """the cross-check: milliseconds per call by the host clock around `reps` calls that end in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _pil(img, quality, subsampling, reps):
    import PIL.Image

    times, data = [], b""
    for _ in range(reps):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        PIL.Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)
        times.append(time.perf_counter() - t0)
        data = buf.getvalue()
    return float(np.median(times)), data


def _png_bytes(L, st, one):
    """Size of the device PNG of the image; None where the PNG encoder does not take the shape (a row above 24639 bytes)."""
    h, w, c = one.shape
    if L.hf_png_bound(h, w, c) <= 0:
        return None
    _, sizes = M.png_encode(L, st, one[None], 3)
    return int(sizes.cpu()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_jpeg needs a GPU"
    assert a.reps >= 20, "median of at least 20"
    dev = torch.device("cuda:0")
    L, st = lib(), stream()
    res = {"metric": "jpeg_encode", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "reps": a.reps,
           "host_reps": a.host_reps}
    images = {"photo_1024": (K.photo(1024), (13, 1)), "photo_4000x6000": (np.ascontiguousarray(K.photo(6000)[:4000]), (1,))}
    out = {}
    for name, (host, batches) in images.items():
        one = torch.from_numpy(host).to(dev)
        entry = {"raw_bytes": int(host.size), "device_png_bytes": _png_bytes(L, st, one)}
        for quality, subsampling in SETTINGS:
            sub = M.JPEG_SUBSAMPLINGS[subsampling]
            pil_s, pil_file = _pil(host, quality, subsampling, a.host_reps)
            setting = {"pil_s_per_image": round(pil_s, 4), "file_bytes": len(pil_file)}
            for batch in batches:
                x = one[None].expand(batch, -1, -1, -1).contiguous()
                files, sizes = M.jpeg_encode(L, st, x, quality, sub)
                n = sizes.cpu().tolist()
                for k in {0, batch - 1}:
                    assert files[k, :n[k]].cpu().numpy().tobytes() == pil_file, (name, quality, subsampling, batch, k)
                ms = BC.time_ms(lambda: M.jpeg_encode(L, st, x, quality, sub), a.reps)
                wall = _wall(lambda: M.jpeg_encode(L, st, x, quality, sub), a.reps)
                setting[f"batch_{batch}"] = {"device_ms": round(ms, 4), "device_ms_per_image": round(ms / batch, 4),
                                             "host_clock_ms_per_call": round(wall, 4),
                                             "speedup_vs_pil_per_image": round(pil_s * 1e3 / (ms / batch), 1)}
                del files, x
            entry[f"q{quality}_{subsampling}"] = setting
        out[name] = entry
        del one
        torch.cuda.empty_cache()
    res["images"] = out
    res["note"] = ("device_ms includes the allocation of the output and workspace tensors by the caching allocator; the device "
                   "file equals PIL's byte for byte, so file_bytes is both")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
