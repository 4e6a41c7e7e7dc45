#!/usr/bin/env python
"""Writes tests/golden/align.npz from the REFERENCE's own `align_face` (utils/shape_predictor.py:80-194).

Run by hand where a checkout of the reference is available; never by a test, smoke() or bench.py:

    python tools/make_align_golden.py --reference /path/to/HairFastGAN

The reference module is imported with stub modules for `dlib`, `torchvision` and `utils.drive` (none of them touches the
image work), `Image.ANTIALIAS = Image.LANCZOS` (removed from Pillow 10) and `get_landmark_from_tensors` replaced by one
that returns the given landmarks.  Inputs are the seeded recipes of tests/align_ref.py (GOLDEN_CASES); per case the
file holds the recipe, the landmarks, a fixed 128^2 crop and the every-8th-pixel grid of the 1024^2 result (a full
result is 3 MB of incompressible bytes).

For the padded case it also holds the reference's padded image at the bytes the tie rule covers: the positions where the
restatement's float32 value before `rint` lies within 1e-3 of a half-integer (tests/align_ref.tie_eligible).  The
reference runs here under whatever numpy is installed; under numpy 2 its fade mask is float64, the restatement's is the
float32 of the reference's pinned numpy 1.x - the two can round a tie differently and nothing else: this tool asserts
that every other byte of the padded image is equal.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import PIL.Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import align_ref as R  # noqa: E402

CROP = (448, 576)  # rows and columns of the stored crop
GRID = 8


def load_reference(path):
    for name in ("dlib", "torchvision", "torchvision.transforms", "utils", "utils.drive"):
        sys.modules.pop(name, None)
    dlib = types.ModuleType("dlib")
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.update({"dlib": dlib, "torchvision": tv, "torchvision.transforms": tv.transforms})
    pkg = types.ModuleType("utils")
    pkg.__path__ = [os.path.join(path, "utils")]
    drive = types.ModuleType("utils.drive")
    drive.open_url = None
    sys.modules.update({"utils": pkg, "utils.drive": drive})
    if not hasattr(PIL.Image, "ANTIALIAS"):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    return importlib.import_module("utils.shape_predictor")


def reference_align(mod, img, lm):
    """-> (the reference's 1024^2 PIL result, the byte image it built in the pad branch or None)."""
    captured = []
    fromarray = PIL.Image.fromarray

    def spy(arr, *a, **k):
        captured.append(np.array(arr))
        return fromarray(arr, *a, **k)

    mod.get_landmark_from_tensors = lambda tensors, predictor: (list(tensors), [np.array(lm)])
    PIL.Image.fromarray = spy
    try:
        [out] = mod.align_face([img], predictor=object(), return_tensors=False)
    finally:
        PIL.Image.fromarray = fromarray
    return out, (captured[0] if captured else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds utils/shape_predictor.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "align.npz"))
    args = ap.parse_args()
    mod = load_reference(os.path.abspath(args.reference))
    data = {"numpy_version": np.array(np.__version__), "pillow_version": np.array(PIL.__version__),
            "crop": np.array(CROP), "grid": np.array(GRID)}
    for name, case in R.GOLDEN_CASES.items():
        arr, lm = R.case_inputs(case)
        img = PIL.Image.fromarray(arr, "RGB")
        out, padded = reference_align(mod, img, lm)
        out = np.asarray(out)
        assert out.shape == (1024, 1024, 3)
        S = R.align(img, lm)
        plan = S["plan"]
        assert (padded is not None) == (plan["pad"] is not None), name
        data[f"{name}_recipe"] = np.array([case[0], case[1], case[2]])
        data[f"{name}_lm_args"] = np.array(case[3], np.float64)
        data[f"{name}_lm"] = lm
        data[f"{name}_crop"] = out[CROP[0]:CROP[1], CROP[0]:CROP[1]].copy()
        data[f"{name}_grid"] = out[::GRID, ::GRID].copy()
        line = f"{name}: shrink {plan['shrink']}, crop {plan['crop']}, pad {plan['pad']}"
        if padded is not None:
            eligible = R.tie_eligible(S["pre"])
            mine = np.asarray(S["padded"])
            differ = mine != padded
            assert not (differ & ~eligible).any(), "the restatement's padded image differs from the reference's off the ties"
            assert np.abs(mine.astype(int) - padded)[differ].max(initial=0) <= 1
            idx = np.flatnonzero(eligible)
            data[f"{name}_tie_index"] = idx.astype(np.int64)
            data[f"{name}_tie_bytes"] = padded.reshape(-1)[idx]
            data[f"{name}_pad_shape"] = np.array(padded.shape)
            line += f"; padded {padded.shape}, {idx.size} tie-eligible bytes ({idx.size / eligible.size:.5f}), {int(differ.sum())} differ"
        print(line, "; restatement == reference:", bool(np.array_equal(np.asarray(S["out"]), out)))
    np.savez_compressed(args.out, **data)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
