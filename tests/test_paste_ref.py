"""CPU tests of the paste-back contract itself: the PIL restatement (tests/paste_ref.py) undoes the alignment restatement
(tests/align_ref.py) to a small fraction of a pixel, Pillow's byte rules are the ones csrc/paste.h states, the mask and ROI
invariants hold, and the product's host geometry (face_align.paste_plan, feather_mask) is the restatement's."""
import numpy as np
import PIL.Image
import PIL.ImageChops
import pytest

from hairfastgan_amd import face_align as FA
from tests import align_ref as R
from tests import paste_ref as PR

# (photo width, height, landmark arguments, S, blob sigma, bound in pixels, measured worst centroid error of this restatement,
#  the same with the `+ 0.5` of the map's origin left out)
ROUND_TRIPS = {
    "plain": (600, 500, (300, 230, 80, 7.0), 256, 3.0, 0.1, 0.0054, 0.71),
    "shrink8": (1300, 1300, (650, 620, 262, -4.0), 64, 40.0, 0.5, 0.161, 5.68),
}


def _blob_centres(lm_args):
    cx, cy, eye, _ = lm_args  # around the face: inside the crop and away from its feathered rim
    return [(cx - 0.9 * eye, cy - 0.4 * eye), (cx + 0.8 * eye + 0.37, cy + 0.1 * eye), (cx + 0.13, cy + 1.3 * eye + 0.61),
            (cx - 0.5 * eye - 0.29, cy + 0.9 * eye)]


def round_trip_error(name, paste=PR.paste):
    """Worst distance between a blob's centroid in the photograph and in (align, then paste onto black)."""
    w, h, lm_args, S, sigma, _, _, _ = ROUND_TRIPS[name]
    lm = R.landmarks(*lm_args)
    centres = _blob_centres(lm_args)
    photo = PR.blob_image(w, h, centres, sigma)
    crop = R.align(PIL.Image.fromarray(photo, "RGB"), lm, S, 4 * S)
    if name == "shrink8":
        assert crop["plan"]["shrink"] == 8
    back = np.asarray(paste(PIL.Image.new("RGB", (w, h)), crop["out"], lm)["out"])[:, :, 0]
    worst = 0.0
    for cx, cy in centres:
        ax, ay = PR.centroid(photo[:, :, 0], cx, cy, 4 * sigma)
        bx, by = PR.centroid(back, cx, cy, 4 * sigma)
        assert back[int(cy), int(cx)] > 100  # the blob did come back
        worst = max(worst, float(np.hypot(ax - bx, ay - by)))
    return worst


@pytest.mark.parametrize("name", list(ROUND_TRIPS))
def test_blob_centroid_round_trip(name):
    bound, measured = ROUND_TRIPS[name][5], ROUND_TRIPS[name][6]
    err = round_trip_error(name)
    print(f"{name}: worst centroid error {err:.4f} px (bound {bound}, recorded {measured})")
    assert err <= bound
    assert 2 * measured <= bound  # the recorded figure keeps a factor of two below the bound


def test_blend_rule_all_inputs():
    """Image.composite over all 256^3 (a, b, m): t = a m + b (255 - m) + 128, ((t >> 8) + t) >> 8."""
    idx = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
    a, b, m = idx >> 16, (idx >> 8) & 255, idx & 255
    im = [PIL.Image.fromarray(v.astype(np.uint8), "L") for v in (a, b, m)]
    ref = np.asarray(PIL.Image.composite(im[0], im[1], im[2]))
    t = a * m + b * (255 - m) + 128
    assert np.array_equal((((t >> 8) + t) >> 8).astype(np.uint8), ref)


def test_multiply_rule_all_inputs():
    a = np.repeat(np.arange(256, dtype=np.int32)[:, None], 256, axis=1)
    b = a.T
    ref = np.asarray(PIL.ImageChops.multiply(PIL.Image.fromarray(a.astype(np.uint8), "L"), PIL.Image.fromarray(b.astype(np.uint8), "L")))
    assert np.array_equal((a * b // 255).astype(np.uint8), ref)


@pytest.mark.parametrize("case", ["inside", "corner"])
def test_mask_and_roi_invariants(case):
    w, h, seed, lm_args = R.SMALL_CASES[case]
    photo = R.image(w, h, seed)
    lm = R.landmarks(*lm_args)
    S = 64
    F = PIL.Image.fromarray(np.random.default_rng(5).integers(0, 256, (S, S, 3), dtype=np.uint8), "RGB")
    img = PIL.Image.fromarray(photo, "RGB")
    zero = np.zeros((S, S), np.uint8)
    assert np.array_equal(np.asarray(PR.paste(img, F, lm, 0.1, zero)["out"]), photo)
    assert np.array_equal(np.asarray(PR.paste(img, F, lm, 0.0, zero.astype(np.float32))["out"]), photo)
    for feather in (0.1, 0.0):
        st = PR.paste(img, F, lm, feather)
        x0, y0, x1, y1 = st["inverse"]["roi"]
        out = np.asarray(st["out"])
        rest = np.ones((h, w), bool)
        rest[y0:y1, x0:x1] = False
        assert np.array_equal(out[rest], photo[rest]) and (out != photo).any()
        unmasked = np.asarray(st["warped_mask"]) == 0  # outside the result, or on the rim where the feather rounds to 0
        assert np.array_equal(out[y0:y1, x0:x1][unmasked], photo[y0:y1, x0:x1][unmasked])
    assert np.array_equal(np.asarray(img), photo)  # the input image is left alone


@pytest.mark.parametrize("w,h,lm_args,S", [(150, 125, (75, 57, 20, 7.0), 64), (150, 125, (75, 57, 20, 7.0), 256),
                                           (150, 125, (24, 22, 20, 7.0), 64), (300, 260, (150, 120, 40, 30.0), 128),
                                           (300, 260, (150, 120, 40, -4.0), 16), (1300, 1300, (650, 620, 262, -4.0), 64),
                                           (600, 500, (300, 230, 80, 7.0), 1024)])
def test_paste_plan_is_the_restatement(w, h, lm_args, S):
    """The product's vector form and the restatement's scalar form of the inverse geometry: the same float64 bits."""
    lm = R.landmarks(*lm_args)
    inv = PR.inverse(R.plan(lm, w, h, S))
    got = FA.paste_plan(FA.alignment_plan(lm, w, h, S))
    assert np.array_equal(got["A"], np.array(inv["A"])) and np.array_equal(got["b"], np.array(inv["b"]))
    assert got["det"] == inv["det"] and got["n"] == inv["n"] and got["roi"] == inv["roi"]
    assert np.array_equal(got["quad"].flatten(), np.array(inv["data"]))
    # the quad is the inverse of the map: ROI corners -> crop coordinates -> photograph
    back = (got["quad"] * (S / got["n"])) @ got["A"].T + got["b"]
    x0, y0, x1, y1 = got["roi"]
    assert np.allclose(back, [[x0, y0], [x0, y1], [x1, y1], [x1, y0]], atol=1e-9)


def test_paste_plan_without_overlap():
    """A face whose mapped crop misses the photograph entirely cannot come from alignment_plan (it raises); a hand-made
    plan far outside gives no ROI."""
    lm = R.landmarks(75, 57, 20, 7.0)
    plan = FA.alignment_plan(lm, 150, 125, 64)
    plan["quad"] = plan["quad"] + 1000.0
    assert FA.paste_plan(plan)["roi"] is None and FA.paste_plan(plan)["quad"] is None


@pytest.mark.parametrize("n,feather", [(64, 0.1), (80, 0.1), (17, 0.25), (16, 0.0), (1, 0.1), (33, 0.7)])
def test_feather_mask(n, feather):
    m = FA.feather_mask(n, feather)
    assert m.dtype == np.uint8 and m.shape == (n, n)
    assert np.array_equal(m, PR.feather_plane(n, feather))
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1, ::-1])
    if feather == 0.0:
        assert (m == 255).all()
    elif feather <= 0.25 and n >= 16:
        assert m[n // 2, n // 2] == 255 and m[0, 0] < 30 and (np.diff(m[n // 2, : n // 2].astype(int)) >= 0).all()
    with pytest.raises(ValueError):
        FA.feather_mask(n, -0.1)
