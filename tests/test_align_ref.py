"""CPU tests of the face-alignment restatement (tests/align_ref.py) against the reference's own `align_face`
(tests/golden/align.npz, written by tools/make_align_golden.py), of `alignment_plan` against the restatement, and of the
argument errors of `swap(align=True, ...)`.

Unpadded cases: byte-equal.  Padded case: the golden file holds the reference's padded bytes where the tie rule allows a
difference (the restatement's float32 value before rint within 1e-3 of a half-integer; the tool asserted equality
everywhere else); the restatement continued from the padded image with those bytes must give the reference's result
byte for byte."""
import functools
from types import SimpleNamespace

import numpy as np
import PIL.Image
import pytest
import torch

from hairfastgan_amd import face_align as FA
from tests import align_checks as K
from tests import align_ref as R


@functools.lru_cache(maxsize=None)
def _restated(name):
    arr, lm = R.case_inputs(R.GOLDEN_CASES[name])
    return R.align(PIL.Image.fromarray(arr, "RGB"), lm)


def _samples(G, out):
    (r0, r1), step = G["crop"], int(G["grid"])
    return out[r0:r1, r0:r1], out[::step, ::step]


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_equals_reference(golden, name):
    G = golden("align.npz")
    case = R.GOLDEN_CASES[name]
    assert tuple(G[f"{name}_recipe"]) == case[:3] and tuple(G[f"{name}_lm_args"]) == case[3]
    assert np.array_equal(G[f"{name}_lm"], R.case_inputs(case)[1])
    S = _restated(name)
    P = S["plan"]
    assert {"inside": P["shrink"] < 2 and P["pad"] is None and P["crop"] is not None,
            "corner": P["shrink"] < 2 and P["pad"] is not None,
            "shrink": P["shrink"] >= 2 and P["qsize_input"] >= 4096 and P["pad"] is None}[name]
    out = S["out"]
    if P["pad"] is not None:
        eligible = R.tie_eligible(S["pre"])
        assert (int(eligible.sum()), eligible.size) == K.TIE_COUNTS["golden_" + name]
        assert eligible.sum() <= 1e-3 * eligible.size
        assert np.array_equal(np.flatnonzero(eligible), G[f"{name}_tie_index"]) and tuple(G[f"{name}_pad_shape"]) == S["pre"].shape
        padded = np.asarray(S["padded"]).copy()
        theirs = G[f"{name}_tie_bytes"]
        flat = padded.reshape(-1)
        k = int((flat[G[f"{name}_tie_index"]] != theirs).sum())
        assert np.abs(flat[G[f"{name}_tie_index"]].astype(int) - theirs).max() <= 1
        flat[G[f"{name}_tie_index"]] = theirs
        print(f"{name}: {k} of {theirs.size} tie-eligible bytes of the padded image differ from the reference's")
        if k:
            out = R.finish(PIL.Image.fromarray(padded, "RGB"), P)
    crop, grid = _samples(G, np.asarray(out))
    assert np.array_equal(crop, G[f"{name}_crop"]) and np.array_equal(grid, G[f"{name}_grid"])


@pytest.mark.parametrize("cases,sizes", [(R.GOLDEN_CASES, (1024, 4096)), (R.SMALL_CASES, (64, 256)), (K.PAD_CASES, (1024, 4096))])
def test_alignment_plan_equals_restatement(cases, sizes):
    for name, case in cases.items():
        lm = R.landmarks(*case[3])
        for padding in (True, False):
            mine = FA.alignment_plan(lm, case[0], case[1], *sizes, enable_padding=padding)
            ref = R.plan(lm, case[0], case[1], *sizes, enable_padding=padding)
            assert set(mine) == set(ref)
            for key, v in ref.items():
                if isinstance(v, np.ndarray):
                    assert mine[key].dtype == np.float64 and np.array_equal(mine[key], v), (name, key)
                else:
                    assert mine[key] == v and type(mine[key]) is type(v), (name, key, mine[key], v)
        as_float = FA.alignment_plan(lm.astype(np.float64), case[0], case[1], *sizes)  # dlib gives ints; floats plan alike
        padded = R.plan(lm, case[0], case[1], *sizes)
        assert all(as_float[k] == padded[k] for k in ("shrink", "rsize", "crop", "pad", "size")), name
        assert np.array_equal(as_float["quad"], padded["quad"])


def test_host_tables():
    # a pass at scale 4 has 24 taps inside the image, 25 table columns, weights that sum to 2^22 within the rounding
    bounds, kk = FA.lanczos_coeffs(4096, 1024)
    assert kk.shape == (1024, 25) and tuple(bounds[3]) == (2, 24) and tuple(bounds[0]) == (0, 14) and tuple(bounds[1023]) == (4082, 14)
    assert np.abs(kk.sum(1) - (1 << 22)).max() <= 12
    w, radius = FA.gaussian_weights(12.0)
    assert radius == 48 and w.size == 97 and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    mx, my = FA.fade_ramps(7, 5, (2, 2, 3, 1))
    assert mx.dtype == np.float32 and my.dtype == np.float32 and mx[0] == 1 and my[-1] == 1 and mx.shape == (7,)


def _bare_hairfast(detector=None):
    from hairfastgan_amd.hair_swap import HairFast

    hf = HairFast.__new__(HairFast)  # the argument checks of align=True run before any network is touched
    hf.args = SimpleNamespace(device="cpu")
    hf.landmark_detector = detector
    return hf


def test_swap_align_argument_errors():
    img = torch.zeros(3, 40, 40, dtype=torch.uint8)
    lm = R.landmarks(20, 16, 8)
    hf = _bare_hairfast()
    with pytest.raises(NotImplementedError, match="dlib"):
        hf.swap(img, img, img, align=True)
    with pytest.raises(NotImplementedError, match="dlib"):
        hf.swap_batch([(img, img, img)], align=True)
    with pytest.raises(ValueError, match=r"\[68, 2\]"):
        hf.swap(img, img, img, align=True, landmarks=[lm, lm[:67], lm])
    with pytest.raises(ValueError, match=r"\[68, 2\]"):
        hf.swap(img, img, img, align=True, landmarks=[lm, lm.T, lm])
    with pytest.raises(ValueError, match="one \\[68,2\\] array per image"):
        hf.swap(img, img, img, align=True, landmarks=[lm, lm])
    with pytest.raises(ValueError, match=r"\[68, 2\]"):
        _bare_hairfast(lambda image: np.zeros((5, 2))).swap(img, img, img, align=True)
    with pytest.raises(ValueError, match="3-channel"):
        hf.swap(torch.zeros(4, 40, 40, dtype=torch.uint8), img, img, align=True, landmarks=[lm, lm, lm])
    with pytest.raises(ValueError, match="one triple"):
        hf.swap_batch([(img, img, img)], align=True, landmarks=[[lm, lm, lm], [lm, lm, lm]])
    with pytest.raises(ValueError, match="3-channel"):
        FA.align_face([torch.zeros(1, 40, 40)], [lm])
    with pytest.raises(ValueError, match="one \\[68,2\\] landmark array per image"):
        FA.align_face([img, img], [lm])
    seen = []

    def detector(image):
        seen.append((image.dtype, image.shape))
        return np.zeros((5, 2))

    with pytest.raises(ValueError):
        _bare_hairfast(detector).swap(torch.zeros(3, 30, 40), img, img, align=True)
    assert seen == [(np.dtype("uint8"), (30, 40, 3))]  # the detector sees a uint8 HWC array
