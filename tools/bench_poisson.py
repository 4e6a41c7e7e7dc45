#!/usr/bin/env python3
"""Poisson image blending (hairfastgan_amd.image_utils) at the reference's size, one pair of 1024^2 images: time of the
mask stage (one BiSeNet parse of both images, dilation, quantisation), of the solver at maxn in {115, 1000, 5000} for
every sweep depth T of hf_poisson_jacobi_f32, and of the default call.  Prints ONE JSON line.

Per sweep: microseconds and the bytes the launch form implies (each launch reads X, B and the mask of its tiles with
their halo of T pixels and writes X once; divided by the T sweeps it runs).
usage: python tools/bench_poisson.py [--reps N]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hairfastgan_amd import _marshal as M  # noqa: E402
from hairfastgan_amd import _runtime  # noqa: E402
from hairfastgan_amd import image_utils as IU  # noqa: E402
from hairfastgan_amd.face_parsing import BiSeNet  # noqa: E402

TILE = 64  # csrc/poisson.h kPoissonTile


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


def sweep_bytes(h, w, channels, T):
    """bytes one launch of depth T moves per sweep it runs: X (fp32) and B (fp32) read and the mask (u8, one plane per
    image) read over every tile plus halo, X written over the tile"""
    tiles = ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
    region = tiles * (TILE + 2 * T) ** 2
    return (channels * region * (4 + 4 + 1) + channels * h * w * 4) / T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_poisson needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = BiSeNet(19).eval().to(dev)
    H = W = a.size
    g = torch.Generator().manual_seed(1)
    finals = torch.rand(1, 3, H, W, generator=g).to(dev)
    faces = torch.rand(1, 3, H, W, generator=g).to(dev)
    L, st = _runtime.lib(), _runtime.stream()
    rng = np.random.default_rng(0)
    src, tgt = (torch.from_numpy(v).to(dev) for v in rng.integers(0, 256, (2, 1, 3, H, W), dtype=np.uint8))
    yy, xx = np.mgrid[:H, :W]
    mask = torch.from_numpy(np.where((yy - H * 0.45) ** 2 + (xx - W * 0.5) ** 2 <= (0.42 * H) ** 2, 255, 0).astype(np.uint8))
    mask = mask[None, None].to(dev)
    res = {"metric": "poisson_blend", "size": [H, W], "device": torch.cuda.get_device_name(0),
           "mask_fraction": float((mask >= 128).float().mean())}
    with torch.inference_mode():
        res["mask_stage_ms"] = _time(lambda: IU.blend_masks(net, finals, faces, 30), a.reps)
        res["setup_finish_ms"] = _time(lambda: IU.poisson_solve(L, st, src, tgt, mask, 0), a.reps)
        solver = {}
        ref = None
        for T in M.POISSON_TBLOCKS:
            row = {}
            for maxn in (115, 1000, 5000):
                row[str(maxn)] = _time(lambda: IU.poisson_solve(L, st, src, tgt, mask, maxn, T), max(3, a.reps // (maxn // 115)))
            # per sweep: the slope between 1000 and 5000 sweeps (setup, finish and the remainder launch cancel)
            us = (row["5000"] - row["1000"]) * 1e3 / 4000
            nbytes = sweep_bytes(H, W, 3, T)
            out = IU.poisson_solve(L, st, src, tgt, mask, 115, T)[0]
            ref = out if ref is None else ref
            solver[str(T)] = {"ms": row, "us_per_sweep": round(us, 3), "bytes_per_sweep": int(nbytes),
                              "implied_TBps": round(nbytes / (us * 1e-6) / 1e12, 2), "same_bytes_as_T1": bool(torch.equal(out, ref))}
        res["solver"] = solver
        best = min(solver, key=lambda k: solver[k]["us_per_sweep"])
        res["fastest_T"] = int(best)
        res["default_T"] = IU.DEFAULT_TBLOCK
        res["default_call_ms"] = _time(lambda: IU.poisson_blend(finals, faces, parsing=net), a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
