#!/usr/bin/env python
"""Times native face alignment (hairfastgan_amd.face_align) on the three geometries of tests/golden/align.npz and writes
profiles/align_bench.json:

* `align_face` per image (HIP events around the call on the launch stream, warmed up, median of --iters runs) with the
  fused transform + resize launch and with the chained pair;
* the transform + resize step alone, both forms (the step the fused kernel replaces);
* the CPU restatement (tests/align_ref.py: PIL + scipy, what the reference runs) on the same host.

    python tools/bench_align.py [--iters 20] [--out profiles/align_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import PIL.Image  # noqa: E402
import torch  # noqa: E402

import bench_common as BC  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd import face_align as FA  # noqa: E402
from tests import align_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L, st = _runtime.lib(), _runtime.stream()
    result = {"device": torch.cuda.get_device_name(0), "output_size": 1024, "transform_size": 4096, "cases": {}}
    for name, case in R.GOLDEN_CASES.items():
        arr, lm = R.case_inputs(case)
        img = torch.from_numpy(arr.transpose(2, 0, 1).copy()).to(dev)
        stages = {}
        FA.align_bytes(L, st, img, lm, stages=stages)
        plan, padded = stages["plan"], stages["padded"]
        entry = {"image": [case[0], case[1]], "shrink": plan["shrink"], "crop": plan["crop"], "pad": plan["pad"],
                 "transform_input": list(plan["size"])}
        for key, fused in (("fused", True), ("chained", False)):
            entry[f"align_face_{key}"] = BC.device_ms(lambda: FA.align_face([img], [lm], fused=fused), args.warmup, args.iters)
            entry[f"transform_resize_{key}"] = BC.device_ms(
                lambda: FA.transform_resize(L, st, padded, plan["quad"], 4096, 1024, fused=fused), args.warmup, args.iters)
        pil = PIL.Image.fromarray(arr, "RGB")
        cpu = []
        for _ in range(args.cpu_repeats):
            t0 = time.perf_counter()
            R.align(pil, lm)
            cpu.append((time.perf_counter() - t0) * 1e3)
        entry["cpu_restatement_pil_scipy_ms"] = {"median_ms": statistics.median(cpu), "min_ms": min(cpu), "repeats": len(cpu)}
        result["cases"][name] = entry
        print(name, json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
