#!/usr/bin/env python3
"""The device JPEG decoder (image_utils.decode_jpeg -> hf_jpeg_decode_u8; csrc/jpeg_decode.h) against the host path it can
replace, `_read_image_rgb` (PIL, libjpeg-turbo on one core) + `.to("cuda")`, for the same files on the same machine.  Prints
ONE JSON line (kept as profiles/jpeg_decode_bench.json).

Files (the formula photograph of tests/png_checks.py, written by Pillow at quality 90, 4:2:0):
* three 1024^2 files without restart markers, in one call;
* the same with one restart interval per MCU row;
* one 4000 x 3000 file without restart markers;
* 96 1024^2 files in one call (without, and with, restart markers).

Both paths are timed by the host clock from the file on disk to the pixels on the device, ending in a synchronise: the
device path reads the file, parses the header, copies the scan, launches and synchronises.  Per case: the median of --reps
runs of each path, the spread of the host path (min, max, standard deviation), the ratio of the medians, whether the device
path wins by more than that spread, the synchronisation passes the entropy decoder needed per file (status word) and the
device-only time of the launches at sub_bytes 8, 16, 32 and 64 (HIP events, the scans already on the device).  Every device
image must equal PIL's.

usage: python tools/bench_jpeg_decode.py [--reps N]"""
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


def _device_only(paths, sub, reps):
    """milliseconds of the launches alone (HIP events), and the passes per file"""
    datas = [open(p, "rb").read() for p in paths]
    heads = [IU.parse_jpeg_header(d) for d in datas]
    hd = heads[0]
    scans = [d[x.scan_start:] for d, x in zip(datas, heads)]
    dev = torch.device("cuda:0")
    scan_t = torch.from_numpy(np.frombuffer(b"".join(scans), np.uint8).copy()).to(dev)
    off_t = torch.from_numpy(np.cumsum([0] + [len(s) for s in scans]).astype(np.int64)).to(dev)
    tab_t = torch.from_numpy(np.stack([x.tables for x in heads])).to(dev)
    L, st = lib(), stream()

    def run():
        return M.jpeg_decode(L, st, scan_t, off_t, max(map(len, scans)), tab_t, hd.height, hd.width, hd.components, hd.hs, hd.vs,
                             hd.restart_interval, sub_bytes=sub)

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
    return float(np.median(times)), [int(v) for v in sorted(set(status[:, 1].tolist()))]


def main():
    import PIL.Image

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_jpeg_decode needs a GPU"
    assert a.reps >= 20, "median of at least 20"
    res = {"metric": "jpeg_decode", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "reps": a.reps,
           "files": "png_checks.photo, Pillow quality 90, 4:2:0"}
    root = tempfile.mkdtemp(prefix="jpeg_decode_bench_")
    small = [np.roll(K.photo(1024), 37 * k, 1) for k in range(3)]
    big = np.ascontiguousarray(K.photo(4000)[:3000])
    cases = {}

    def write(name, imgs, **kw):
        paths = []
        for k, img in enumerate(imgs):
            paths.append(os.path.join(root, f"{name}_{k}.jpg"))
            PIL.Image.fromarray(img, "RGB").save(paths[-1], format="JPEG", quality=90, subsampling=2, **kw)
        return paths

    cases["3x1024_no_restart"] = write("a", small)
    cases["3x1024_restart_per_mcu_row"] = write("b", small, restart_marker_rows=1)
    cases["1x4000x3000_no_restart"] = write("c", [big])
    cases["96x1024_no_restart"] = [cases["3x1024_no_restart"][k % 3] for k in range(96)]
    cases["96x1024_restart_per_mcu_row"] = [cases["3x1024_restart_per_mcu_row"][k % 3] for k in range(96)]
    out = {}
    for name, paths in cases.items():
        host_fn = lambda: [_read_image_rgb(p).to("cuda") for p in paths]  # noqa: E731
        dev_fn = lambda: IU.decode_jpeg(paths)  # noqa: E731
        for got, ref in zip(dev_fn()[:3], host_fn()[:3]):
            assert torch.equal(got.permute(2, 0, 1), ref), name
        reps = a.reps if len(paths) < 96 else max(5, a.reps // 4)
        host, dev = _wall(host_fn, reps), _wall(dev_fn, reps)
        hm, dm = float(np.median(host)), float(np.median(dev))
        entry = {"files": len(paths), "file_bytes": [os.path.getsize(p) for p in paths[:3]], "runs": reps,
                 "host_ms_median": round(hm, 3), "host_ms_min": round(min(host), 3), "host_ms_max": round(max(host), 3),
                 "host_ms_std": round(float(np.std(host)), 3), "device_ms_median": round(dm, 3), "device_ms_min": round(min(dev), 3),
                 "device_ms_max": round(max(dev), 3), "host_over_device": round(hm / dm, 2),
                 "device_faster_beyond_host_spread": bool(dm < min(host))}
        uniq = paths[:3]
        entry["launches_ms_by_sub_bytes"] = {}
        for sub in (8, 16, 32, 64):
            ms, passes = _device_only(uniq, sub, a.reps)
            entry["launches_ms_by_sub_bytes"][str(sub)] = {"ms": round(ms, 3), "passes": passes}
        ms, passes = _device_only(uniq, 0, a.reps)
        entry["launches_ms_default"] = round(ms, 3)
        entry["passes_per_file_default"] = passes
        out[name] = entry
        torch.cuda.empty_cache()
    res["cases"] = out
    res["note"] = ("host path: _read_image_rgb (PIL) + .to('cuda') per file; device path: image_utils.decode_jpeg of the same paths in "
                   "one call; both by the host clock from the file to the pixels on the device, synchronised.  launches_ms: the "
                   "kernels alone for the (up to three distinct) files of the case, scans already on the device; passes: the most "
                   "synchronisation passes any window of a file needed")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
