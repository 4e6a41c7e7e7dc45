#!/usr/bin/env python3
"""The device PNG encoder (hf_png_encode_u8; csrc/png.h) against PIL on the host.  Prints ONE JSON line (kept as
profiles/png_bench.json).  For uint8 [13,1024,1024,3] - the thirteen large images one `--save_all` swap writes - and
[1,1024,1024,3], and for each kind of content:

* "photo" / "labels": the two formula images of tests/png_checks.py at 1024^2 (a smooth picture with N(0, 3) noise; a
  19-colour label map);
* "generator" / "parse" (GPU only, --no-generator skips them): the synthetic-weight generator's output quantised by
  `to_bytes`, and `labels_to_rgb` of a blocky random label map -

the device time of the three launches by HIP events (median of --reps after warm-up), a device-to-device copy of the same
number of input bytes timed beside it, PIL `compress_level=6` and `=1` of the same bytes on the host (median wall seconds
per image over --host_reps images), and all file sizes.  Every device file is decoded by PIL and compared with the input.

usage: python tools/bench_png.py [--reps N] [--host_reps N] [--no-generator]"""
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
from hairfastgan_amd import image_utils as IU  # noqa: E402
from hairfastgan_amd._runtime import lib, stream  # noqa: E402
from tests import png_checks as K  # noqa: E402


def _pil(img, level, reps):
    import PIL.Image

    times, size = [], 0
    for _ in range(reps):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        PIL.Image.fromarray(img).save(buf, format="PNG", compress_level=level)
        times.append(time.perf_counter() - t0)
        size = buf.tell()
    return {"s_per_image": round(float(np.median(times)), 4), "bytes": size}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--no-generator", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_png needs a GPU"
    assert a.reps >= 20, "median of at least 20"
    dev = torch.device("cuda:0")
    L, st = lib(), stream()
    res = {"metric": "png_encode", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "segment_rows": int(L.hf_png_segment_rows(1024, 1024, 3)), "reps": a.reps}
    contents = {"photo": torch.from_numpy(K.photo(1024)).to(dev), "labels": torch.from_numpy(K.label_image(1024).copy()).to(dev)}
    if not a.no_generator:
        import bench

        g, _ = bench.build_generator(dev)
        with torch.inference_mode():
            w = torch.randn(1, 18, 512, generator=torch.Generator().manual_seed(0)).to(dev)
            img, _ = g([w], input_is_latent=True, return_latents=False)
            contents["generator"] = IU.to_bytes(img.float(), (-1, 1), "floor", "hwc")[0].clone()
            blocks = torch.randint(0, 19, (1, 1, 16, 16), generator=torch.Generator().manual_seed(1)).float()
            parse = torch.nn.functional.interpolate(blocks, size=(1024, 1024), mode="bilinear").round().long().to(dev)
            contents["parse"] = IU.labels_to_rgb(parse)[0].clone()
        del g
    out = {}
    for name, one in contents.items():
        host = one.cpu().numpy()
        entry = {"raw_bytes": int(host.size), "pil_level_6": _pil(host, 6, a.host_reps), "pil_level_1": _pil(host, 1, a.host_reps)}
        for batch in (13, 1):
            x = one[None].expand(batch, -1, -1, -1).contiguous()
            files, sizes = M.png_encode(L, st, x, 3)
            n = sizes.cpu().tolist()
            assert len(set(n)) == 1  # batch-invariant
            for k in {0, batch - 1}:
                assert np.array_equal(K.decode_pil(files[k, :n[k]].cpu().numpy().tobytes())[0], host), (name, batch, k)
            ms = BC.time_ms(lambda: M.png_encode(L, st, x, 3), a.reps)
            dst = torch.empty_like(x)
            copy_ms = BC.time_ms(lambda: dst.copy_(x), a.reps)
            entry[f"batch_{batch}"] = {"device_ms": round(ms, 4), "device_ms_per_image": round(ms / batch, 4),
                                       "device_copy_ms": round(copy_ms, 4), "times_the_copy": round(ms / copy_ms, 1),
                                       "file_bytes": n[0],
                                       "speedup_vs_pil_level_1_per_image": round(entry["pil_level_1"]["s_per_image"] * 1e3 / (ms / batch), 1),
                                       "speedup_vs_pil_level_6_per_image": round(entry["pil_level_6"]["s_per_image"] * 1e3 / (ms / batch), 1)}
        entry["file_over_pil_level_1"] = round(entry["batch_1"]["file_bytes"] / entry["pil_level_1"]["bytes"], 3)
        entry["file_over_pil_level_6"] = round(entry["batch_1"]["file_bytes"] / entry["pil_level_6"]["bytes"], 3)
        out[name] = entry
    res["contents"] = out
    res["note"] = ("device_ms includes the allocation of the output and workspace tensors by the caching allocator; the generator "
                   "runs on synthetic weights, its image is noise-like")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
