#!/usr/bin/env python
"""Times pasting the aligned result back into the photograph (hairfastgan_amd.face_align.paste_back) at output size 1024 and
writes profiles/paste_bench.json.  Per photograph (HIP events around the call on the launch stream, warmed up, median of
--iters runs):

* `paste_back` as called: float result in, float photograph out (quantise, clone, Lanczos reduction of the result where the
  face is smaller than the crop, the fused warp + composite launch, byte / 255);
* the fused launch alone (hf_paste_quad_u8 on the region of interest);
* the PIL restatement (tests/paste_ref.py) on the same host, for context.

Cases: a face smaller than the crop (the result is reduced first), a face larger than the crop (the warp enlarges) and a
12-megapixel photograph with a large face.

    python tools/bench_paste.py [--iters 20] [--out profiles/paste_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import PIL.Image  # noqa: E402
import torch  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd import face_align as FA  # noqa: E402
from tests import align_ref as R  # noqa: E402
from tests import paste_ref as PR  # noqa: E402

S = 1024
# name -> (photo width, height, image seed, landmark arguments)
CASES = {
    "down": (600, 500, 11, (300, 230, 80, 7.0)),
    "up": (2400, 2000, 12, (1200, 920, 400, 7.0)),
    "photo_12mp": (4000, 3000, 13, (2000, 1400, 700, -4.0)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L, st = _runtime.lib(), _runtime.stream()
    F = np.random.default_rng(7).integers(0, 256, (S, S, 3), dtype=np.uint8)
    F_u8 = torch.from_numpy(F.transpose(2, 0, 1).copy()).to(dev)
    F_float = FA.unit_float(F_u8)
    result = {"device": torch.cuda.get_device_name(0), "output_size": S, "feather": 0.1, "cases": {}}
    for name, (w, h, seed, lm_args) in CASES.items():
        arr, lm = R.image(w, h, seed), R.landmarks(*lm_args)
        img = torch.from_numpy(arr.transpose(2, 0, 1).copy()).to(dev)
        stages = {}
        out = FA.paste_bytes(L, st, img, F_u8, lm, output_size=S, stages=stages)
        inv = stages["inverse"]
        x0, y0, x1, y1 = inv["roi"]
        coef = FA.quad_coefficients(inv["quad"], x1 - x0, y1 - y0)
        entry = {"photo": [w, h], "shrink": stages["plan"]["shrink"], "n": inv["n"], "roi": list(inv["roi"]),
                 "roi_pixels": (x1 - x0) * (y1 - y0)}
        entry["paste_back"] = BC.device_ms(lambda: FA.paste_back(img, F_float, lm, output_size=S), args.warmup, args.iters)
        work = img.clone()  # (pasted over again at every run: the time does not depend on the bytes)
        entry["paste_quad_launch"] = BC.device_ms(lambda: M.paste_quad_u8(L, st, work, stages["result"], stages["mask"], coef, inv["roi"]),
                                                  args.warmup, args.iters)
        photo, res = PIL.Image.fromarray(arr, "RGB"), PIL.Image.fromarray(F, "RGB")
        cpu = []
        for _ in range(args.cpu_repeats):
            t0 = time.perf_counter()
            ref = PR.paste(photo, res, lm)
            cpu.append((time.perf_counter() - t0) * 1e3)
        entry["cpu_restatement_pil_ms"] = {"median_ms": statistics.median(cpu), "min_ms": min(cpu), "repeats": len(cpu)}
        entry["bytes_equal_restatement"] = bool(np.array_equal(out.cpu().numpy().transpose(1, 2, 0), np.asarray(ref["out"])))
        result["cases"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
