#!/usr/bin/env python3
"""The device PNG decoder (image_utils.decode_png -> hf_png_decode_u8; csrc/png_decode.h) against the host path it can
replace, `_read_image_rgb` (PIL, zlib on one core) + `.to("cuda")`, for the same files on the same machine.  Prints ONE JSON
line (kept as profiles/png_decode_bench.json).

Files (the formula photograph of tests/png_checks.py):
* 3 and 96 1024^2 files written by Pillow at compress_level 6 (one deflate stream: the serial route);
* 3 and 96 1024^2 files written by this project's encoder (encode_png: 128 independent segments each);
* one 4000 x 3000 file written by Pillow at compress_level 6.

Both paths are timed by the host clock from the file on disk to the pixels on the device, ending in a synchronise: the
device path reads the file, walks the chunks, copies the streams, launches and synchronises.  Per case: the median of the
runs of each path with min and max, the ratio of the medians, the segments decoded independently per file (status word), the
device-only time of the launches (HIP events, the streams already on the device) and its split by kernel (torch.profiler:
the two inflate passes, the unfilter wavefront, the rest).  Every device image must equal PIL's.

usage: python tools/bench_png_decode.py [--reps N]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd import image_utils as IU  # noqa: E402
from hairfastgan_amd._runtime import lib, stream  # noqa: E402
from hairfastgan_amd.hair_swap import _read_image_rgb  # noqa: E402
from tests import png_checks as K  # noqa: E402


def _wall(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def _device_only(paths, reps):
    """milliseconds of the launches alone (HIP events), the segments per file, and the split of one call by kernel"""
    datas = [open(p, "rb").read() for p in paths]
    heads = [IU.parse_png_header(d) for d in datas]
    hd = heads[0]
    streams = [b"".join(d[at:at + n] for at, n in x.idat) for d, x in zip(datas, heads)]
    dev = torch.device("cuda:0")
    stream_t = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(dev)
    off_t = torch.from_numpy(np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)).to(dev)
    L, st = lib(), stream()

    def run():
        return M.png_decode(L, st, stream_t, off_t, max(map(len, streams)), None, hd.height, hd.width, hd.color_type)

    for _ in range(2):
        _, _, status = run()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    status = status.cpu().numpy()
    assert not status[:, 0].any(), status
    split = None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        split = {"inflate": 0.0, "unfilter": 0.0, "other": 0.0}
        for ev in prof.events():
            if "pngd_" not in ev.name:
                continue
            us = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
            split["inflate" if "pngd_inflate" in ev.name else "unfilter" if "pngd_unfilter" in ev.name else "other"] += us / 1e3
        split = {k: round(v, 3) for k, v in split.items()}
    except Exception as e:  # the profiler is a convenience of the tool: the timings above do not depend on it
        split = {"error": repr(e)[:200]}
    return float(np.median(times)), [int(v) for v in sorted(set(status[:, 1].tolist()))], split


def main():
    import PIL.Image

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_png_decode needs a GPU"
    assert a.reps >= 20, "median of at least 20"
    res = {"metric": "png_decode", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "reps": a.reps,
           "files": "png_checks.photo; Pillow compress_level 6, or image_utils.encode_png"}
    root = tempfile.mkdtemp(prefix="png_decode_bench_")
    small = [np.roll(K.photo(1024), 37 * k, 1) for k in range(3)]
    big = np.ascontiguousarray(K.photo(4000)[:3000])
    cases = {}

    def write(name, imgs, own=False):
        paths = [os.path.join(root, f"{name}_{k}.png") for k in range(len(imgs))]
        if own:
            for p, data in zip(paths, IU.encode_png(torch.from_numpy(np.stack(imgs)).cuda())):
                with open(p, "wb") as fh:
                    fh.write(data)
        else:
            for p, img in zip(paths, imgs):
                PIL.Image.fromarray(img, "RGB").save(p, format="PNG", compress_level=6)
        return paths

    cases["3x1024_pil_level6"] = write("a", small)
    cases["96x1024_pil_level6"] = [cases["3x1024_pil_level6"][k % 3] for k in range(96)]
    cases["3x1024_encode_png"] = write("b", small, own=True)
    cases["96x1024_encode_png"] = [cases["3x1024_encode_png"][k % 3] for k in range(96)]
    cases["1x4000x3000_pil_level6"] = write("c", [big])
    out = {}
    for name, paths in cases.items():
        host_fn = lambda: [_read_image_rgb(p).to("cuda") for p in paths]  # noqa: E731
        dev_fn = lambda: IU.decode_png(paths)  # noqa: E731
        for got, ref in zip(dev_fn()[:3], host_fn()[:3]):
            assert torch.equal(got.permute(2, 0, 1), ref), name
        reps = a.reps if (len(paths) < 96 and "4000" not in name) else max(5, a.reps // 4)
        host, dev = _wall(host_fn, reps), _wall(dev_fn, reps)
        hm, dm = float(np.median(host)), float(np.median(dev))
        ms, segments, split = _device_only(paths[:3], reps)
        out[name] = {"files": len(paths), "file_bytes": [os.path.getsize(p) for p in paths[:3]], "runs": reps,
                     "host_ms_median": round(hm, 3), "host_ms_min": round(min(host), 3), "host_ms_max": round(max(host), 3),
                     "device_ms_median": round(dm, 3), "device_ms_min": round(min(dev), 3), "device_ms_max": round(max(dev), 3),
                     "host_over_device": round(hm / dm, 2), "device_faster_beyond_host_spread": bool(max(dev) < min(host)),
                     "segments_per_file": segments, "launches_ms": round(ms, 3), "launches_split_ms": split}
        torch.cuda.empty_cache()
    res["cases"] = out
    res["note"] = ("host path: _read_image_rgb (PIL) + .to('cuda') per file; device path: image_utils.decode_png of the same paths in one "
                   "call; both by the host clock from the file to the pixels on the device, synchronised.  launches_ms: the kernels "
                   "alone for the (up to three distinct) files of the case, streams already on the device; launches_split_ms: one such "
                   "call by kernel; segments_per_file: status[:, 1]")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
