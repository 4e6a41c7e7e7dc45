"""TEST INFRASTRUCTURE - the comparisons of the face-alignment kernels (csrc/align.h) with the CPU restatement
(tests/align_ref.py), shared by the hipsim tests (tests/test_sim_align.py) and the GPU tests (tests/test_gpu_align.py):
every function takes the library, the stream and the device to run on.

Byte rule: resize, transform, the fused kernel and the unpadded alignments are byte-equal to PIL - integer arithmetic, or
double with one defined truncation.  Tie rule (pad stage): a byte may differ from the restatement's, by one level, only
where the restatement's float32 value before `rint` lies within 1e-3 of a half-integer; the number of such differences
cannot exceed the number of eligible bytes, which is counted per input below (TIE_COUNTS; inputs chosen so that it is at
most 0.1 % of the bytes).  If the pad stage differs anywhere, the stages after it are compared byte for byte with the
restatement continued from the padded image under test.
"""
import functools

import numpy as np
import PIL.Image
import torch

from hairfastgan_amd import face_align as FA
from tests import align_ref as R

# pad-stage inputs: (width, height, image seed, landmark arguments) -> plan at 1024 / 4096 (no shrink at these sizes)
PAD_CASES = {
    "four_sides": (30, 30, 30, (15, 12, 10, 5.0)),       # qsize 40: sigma 0.8, radius 3; the quad leaves on all four sides
    "one_side": (800, 800, 50, (170, 380, 150, -3.0)),   # qsize 600: sigma 12, radius 48; the quad leaves on the left only
    "none": (600, 500, 11, (300, 230, 80, 7.0)),         # max(pad) <= border - 4: the plan does not pad
}
# tie-eligible bytes of the padded image (restatement, counted on the CPU) / all bytes - each at most 0.1 %
TIE_COUNTS = {
    "four_sides": (7, 8910),
    "one_side": (1320, 3106356),
    "golden_corner": (566, 798768),
    "small_corner": (28, 52272),
}


def chw(arr_hwc, device):
    return torch.from_numpy(np.ascontiguousarray(arr_hwc.transpose(2, 0, 1))).to(device)


def hwc(t):
    return t.cpu().numpy().transpose(1, 2, 0)


# (input width, input height, output width, output height): the three target sizes on noise of 97 x 131 in both
# orientations, and two that enlarge one axis by more than a few taps.  Together: both axes shrink; one axis unchanged
# (131 -> 131: the pass is skipped); one axis UPSCALED (97 -> 131, 97 -> 150, 131 -> 200: scale < 1, the filter scale
# clamps to 1, 7 table columns, rows of 6 or 7 taps cut at both edges) while the other shrinks.
RESIZE_CASES = [(97, 131, 40, 31), (97, 131, 131, 50), (97, 131, 65, 48),
                (131, 97, 40, 31), (131, 97, 131, 50), (131, 97, 65, 48),
                (97, 131, 150, 48), (97, 131, 65, 200)]


@functools.lru_cache(maxsize=None)
def noise(width, height):
    return np.random.default_rng(width).integers(0, 256, (height, width, 3), dtype=np.uint8)


def check_resize(L, st, device, in_w, in_h, out_w, out_h):
    arr = noise(in_w, in_h)
    for size_in, size_out in ((in_w, out_w), (in_h, out_h)):  # the labels above, checked
        if size_out > size_in:
            assert FA.lanczos_coeffs(size_in, size_out)[1].shape[1] == 7
    ref = np.asarray(PIL.Image.fromarray(arr, "RGB").resize((out_w, out_h), PIL.Image.LANCZOS))
    got = hwc(FA.resize_lanczos(L, st, chw(arr, device), out_w, out_h))
    assert np.array_equal(got, ref), (out_w, out_h, int(np.abs(got.astype(int) - ref).max()))


QUADS = {
    # NW, SW, SE, NE on a 120 x 90 image: rotated, two corners outside / the identity mapping (axis-aligned, the image's own corners)
    "rotated": np.array([[-20.3, 10.2], [15.1, 95.7], [110.4, 70.3], [80.2, -12.9]]),
    "identity": np.array([[0.0, 0.0], [0.0, 90.0], [120.0, 90.0], [120.0, 0.0]]) - 0.5,
}


@functools.lru_cache(maxsize=None)
def noise_120x90():
    return np.random.default_rng(1).integers(0, 256, (90, 120, 3), dtype=np.uint8)


def check_transform(L, st, device, name):
    arr, quad = noise_120x90(), QUADS[name]
    img = PIL.Image.fromarray(arr, "RGB")
    if name == "identity":
        out_w, out_h = 120, 90
        ref = np.asarray(img.transform((out_w, out_h), PIL.Image.QUAD, (quad + 0.5).flatten(), PIL.Image.BILINEAR))
        got = hwc(FA.M.quad_bilinear_u8(L, st, chw(arr, device), FA.quad_coefficients(quad + 0.5, out_w, out_h), out_h, out_w))
        assert np.array_equal(ref, arr)  # the mapping is the identity
    else:
        ref = np.asarray(R.transform(img, quad, 256))
        got = hwc(FA.quad_transform(L, st, chw(arr, device), quad, 256))
        assert 0.02 < (ref == 0).all(-1).mean() < 0.5  # part of the output lies outside the image
    assert np.array_equal(got, ref), (name, int(np.abs(got.astype(int) - ref).max()))


def check_fused_small(L, st, device):
    """transform 256 -> output 64, and 200 -> 50 (partial 32 x 32 tiles at the right and bottom rim): the fused launch, the
    chained pair and PIL give the same bytes."""
    for name, quad in QUADS.items():
        arr = noise_120x90()
        for tsize, osize in ((256, 64), (200, 50)):
            ref = np.asarray(R.resize(R.transform(PIL.Image.fromarray(arr, "RGB"), quad, tsize), osize))
            fused = hwc(FA.transform_resize(L, st, chw(arr, device), quad, tsize, osize, fused=True))
            pair = hwc(FA.transform_resize(L, st, chw(arr, device), quad, tsize, osize, fused=False))
            assert np.array_equal(fused, pair) and np.array_equal(pair, ref), (name, tsize, osize)
    try:
        FA.transform_resize(L, st, chw(noise_120x90(), device), QUADS["rotated"], 192, 64, fused=True)
    except ValueError:
        pass
    else:
        raise AssertionError("ratio 3 has no fused instance")
    pair = hwc(FA.transform_resize(L, st, chw(noise_120x90(), device), QUADS["rotated"], 192, 64))  # the fallback
    assert np.array_equal(pair, np.asarray(R.resize(R.transform(PIL.Image.fromarray(noise_120x90(), "RGB"), QUADS["rotated"], 192), 64)))


def assert_tie_rule(got_u8, pre_ref, count_key):
    """got_u8 against rint(pre_ref) under the tie rule -> number of differing bytes."""
    ref = R.to_bytes(pre_ref)
    eligible = R.tie_eligible(pre_ref)
    n_eligible, n_bytes = TIE_COUNTS[count_key]
    assert (int(eligible.sum()), eligible.size) == (n_eligible, n_bytes), (count_key, int(eligible.sum()), eligible.size)
    assert n_eligible <= 1e-3 * n_bytes
    differ = got_u8 != ref
    k = int(differ.sum())
    assert not (differ & ~eligible).any(), (count_key, int((differ & ~eligible).sum()))
    assert k == 0 or int(np.abs(got_u8.astype(int) - ref)[differ].max()) <= 1
    assert k <= n_eligible
    return k


@functools.lru_cache(maxsize=None)
def pad_case(name):
    case = PAD_CASES[name]
    arr, lm = R.case_inputs(case)
    P = R.plan(lm, case[0], case[1])
    cropped = np.asarray(R.crop(PIL.Image.fromarray(arr, "RGB"), P))
    pre = R.pad_float(cropped, P["pad"], P["blur"]) if P["pad"] is not None else None
    return P, cropped, pre


def check_pad(L, st, device, name):
    P, cropped, pre = pad_case(name)
    if name == "none":
        assert P["pad"] is None and FA.alignment_plan(R.case_inputs(PAD_CASES[name])[1], 600, 500)["pad"] is None
        return None
    radius = FA.gaussian_weights(P["blur"])[1]
    assert {"four_sides": 1 <= radius <= 3 and P["blur"] < 1, "one_side": 11 < P["blur"] < 13}[name], (radius, P["blur"])
    got, got_pre = FA.pad_blur_fade(L, st, chw(cropped, device), P["pad"], P["blur"], return_float=True)
    k = assert_tie_rule(hwc(got), pre, name)
    print(f"pad {name}: pads {P['pad']}, sigma {P['blur']:.2f}, radius {radius}: {k} bytes differ (ties), "
          f"float image max |diff| {float(np.abs(hwc(got_pre) - pre).max()):.3g}")
    return k


def check_pad_invalid(L, st, device):
    img = torch.zeros(3, 8, 8, dtype=torch.uint8, device=device)
    try:
        FA.pad_blur_fade(L, st, img, (2, 2, 2, 2), 3.0)  # radius 12 >= the padded side 12
    except RuntimeError as e:
        assert "invalid argument" in str(e)
    else:
        raise AssertionError("radius >= padded side must be refused")


def check_align_against_restatement(L, st, device, case, output_size, transform_size, count_key=None, as_float=False):
    """align_bytes on one case against every stage of the restatement."""
    arr, lm = R.case_inputs(case)
    S = R.align(PIL.Image.fromarray(arr, "RGB"), lm, output_size, transform_size)
    img = chw(arr, device)
    if as_float:  # the truncating byte conversion: values strictly between the byte levels, on both sides of them
        img = FA.to_bytes((img.float() + 0.75).div(255), device)
        assert torch.equal(img, chw(arr, device))
    stages = {}
    out = hwc(FA.align_bytes(L, st, img, lm, output_size, transform_size, stages=stages))
    assert np.array_equal(hwc(stages["shrunk"]), np.asarray(S["shrunk"]))
    assert np.array_equal(hwc(stages["cropped"]), np.asarray(S["cropped"]))
    expect = S["out"]
    if S["pre"] is not None:
        k = assert_tie_rule(hwc(stages["padded"]), S["pre"], count_key)
        if k:
            expect = R.finish(PIL.Image.fromarray(hwc(stages["padded"]), "RGB"), S["plan"])
    else:
        assert stages["pre"] is None
    assert np.array_equal(out, np.asarray(expect))
    return out, S
