#!/usr/bin/env python
"""Writes tests/golden/mask_colors.npz from the REFERENCE's own `mask_to_rgb(pred, 0)`
(models/CtrlHair/util/mask_color_util.py:15-64), what `save_vis_mask` draws a `--save_all` mask PNG with.

Run by hand on the CPU where a checkout of the reference is available; never by a test, smoke() or bench.py:

    python tools/make_export_golden.py --reference /path/to/HairFastGAN

The file holds `labels` (int64 [2,5,7]: every value of 0..20 and 255, repeated to fill the shape) and `rgb`
(uint8 [2,5,7,3]: the reference's colours for them, one call per map).  hairfastgan_amd.image_utils.LABEL_COLORS and
hf_labels_to_rgb_i64 are tested against it (tests/export_checks.py)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 5, 7)
VALUES = list(range(21)) + [255]


def golden_labels():
    n = int(np.prod(SHAPE))
    return np.resize(np.array(VALUES, np.int64), n).reshape(SHAPE)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds models/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mask_colors.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    mod = importlib.import_module("models.CtrlHair.util.mask_color_util")
    labels = golden_labels()
    rgb = np.stack([mod.mask_to_rgb(m, 0) for m in labels])
    assert rgb.shape == SHAPE + (3,) and rgb.dtype == np.uint8
    np.savez_compressed(args.out, labels=labels, rgb=rgb)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
