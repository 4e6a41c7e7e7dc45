"""TEST INFRASTRUCTURE - the comparisons of the paste-back path (csrc/paste.h, face_align.paste_bytes) with the PIL
restatement (tests/paste_ref.py), shared by the hipsim tests (tests/test_sim_paste.py) and the GPU tests
(tests/test_gpu_paste.py): every function takes the library, the stream and the device to run on.

Byte rule, no tie rule: every stage is integer arithmetic (Lanczos resize, multiply, composite) or the double path with one
truncation that the alignment tests already pin to Pillow (the QUAD transform), so the device result equals PIL's byte for
byte - the resized result, the mask plane and the pasted photograph.
"""
import functools

import numpy as np
import PIL.Image
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import face_align as FA
from tests import align_ref as R
from tests import paste_ref as PR
from tests.align_checks import chw, hwc

# name -> (photo width, height, image seed, landmark arguments, S, expected n, expected ROI)
CASES = {
    "up": (150, 125, 21, (75, 57, 20, 7.0), 64, 64, (29, 14, 121, 106)),           # n = S: the warp upsamples
    "down": (150, 125, 21, (75, 57, 20, 7.0), 256, 81, (29, 14, 121, 106)),        # side 80.71: Lanczos 256 -> 81 first
    "corner": (150, 125, 21, (24, 22, 20, 7.0), 64, 64, (0, 0, 70, 71)),           # padded plan, ROI cut at the photograph's corner
    "rot30": (300, 260, 31, (150, 120, 40, 30.0), 128, 128, (38, 14, 258, 234)),   # ROI corners well outside the crop
    "shrink": (300, 260, 31, (150, 120, 40, -4.0), 16, 16, (67, 41, 239, 213)),    # shrink factor 5 enters the map
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (photo uint8 HWC, result F uint8 [S,S,3] of seeded noise, landmarks)."""
    w, h, seed, lm_args, S, _, _ = CASES[name]
    F = np.random.default_rng(1000 + S).integers(0, 256, (S, S, 3), dtype=np.uint8)
    return R.image(w, h, seed), F, R.landmarks(*lm_args)


@functools.lru_cache(maxsize=None)
def user_mask(S):
    """A crop-space float mask in [0,1]: noise, with exact zeros and ones among the values."""
    m = np.random.default_rng(2000 + S).random((S, S)).astype(np.float32)
    m[: S // 8] = 0.0
    m[-(S // 8):] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def reference(name, feather, with_mask):
    photo, F, lm = inputs(name)
    mask = user_mask(F.shape[0]) if with_mask else None
    return PR.paste(PIL.Image.fromarray(photo, "RGB"), PIL.Image.fromarray(F, "RGB"), lm, feather, mask)


def check_paste(L, st, device, name, feather=0.1, with_mask=False):
    """paste_bytes on one case against every stage of the restatement."""
    _, _, _, _, S, n, roi = CASES[name]
    photo, F, lm = inputs(name)
    ref = reference(name, feather, with_mask)
    assert (ref["inverse"]["n"], ref["inverse"]["roi"]) == (n, roi), (name, ref["inverse"]["n"], ref["inverse"]["roi"])
    if name == "shrink":
        assert ref["plan"]["shrink"] == 5
    if name == "corner":
        assert ref["plan"]["pad"] is not None
    if name == "rot30":  # part of the ROI samples outside the result: warped mask 0, the photograph's bytes kept
        outside = np.asarray(ref["warped_mask"]) == 0
        x0, y0, x1, y1 = roi
        assert 0.2 < outside.mean() < 0.6
        assert np.array_equal(np.asarray(ref["out"])[y0:y1, x0:x1][outside], photo[y0:y1, x0:x1][outside])
    mask = FA.mask_bytes(user_mask(S), S, device) if with_mask else None
    img = chw(photo, device)
    stages = {}
    out = FA.paste_bytes(L, st, img, chw(F, device), lm, mask, feather, S, stages=stages)
    assert torch.equal(img, chw(photo, device))  # the photograph handed in is not modified
    assert stages["inverse"]["n"] == n and stages["inverse"]["roi"] == roi
    assert np.array_equal(hwc(stages["result"]), np.asarray(ref["result"])), name
    assert np.array_equal(stages["mask"].cpu().numpy(), np.asarray(ref["mask"])), name
    got, want = hwc(out), np.asarray(ref["out"])
    assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.abs(got.astype(int) - want).max()))
    x0, y0, x1, y1 = roi
    rest = np.ones(photo.shape[:2], bool)
    rest[y0:y1, x0:x1] = False
    assert np.array_equal(got[rest], photo[rest])   # nothing outside the ROI is touched
    assert (got != photo).any()
    return out


def check_multiply(L, st, device):
    """All 256^2 byte pairs against ImageChops.multiply."""
    import PIL.ImageChops

    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    b = np.ascontiguousarray(a.T)
    ref = np.asarray(PIL.ImageChops.multiply(PIL.Image.fromarray(a, "L"), PIL.Image.fromarray(b, "L")))
    got = M.multiply_u8(L, st, torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)).cpu().numpy()
    assert np.array_equal(got, ref)


def check_paste_invalid(L, st, device):
    photo = torch.zeros(3, 8, 8, dtype=torch.uint8, device=device)
    src = torch.zeros(3, 4, 4, dtype=torch.uint8, device=device)
    mask = torch.zeros(4, 4, dtype=torch.uint8, device=device)
    coef = FA.quad_coefficients(np.array([[0.0, 0.0], [0.0, 4.0], [4.0, 4.0], [4.0, 0.0]]), 4, 4)
    for roi in ((0, 0, 9, 4), (0, 0, 4, 9), (-1, 0, 4, 4), (0, -1, 4, 4), (4, 0, 4, 4), (0, 5, 4, 4)):  # leaves the photograph / empty
        try:
            M.paste_quad_u8(L, st, photo, src, mask, coef, roi)
        except RuntimeError as e:
            assert "invalid argument" in str(e)
        else:
            raise AssertionError(f"ROI {roi} on an 8 x 8 photograph must be refused")
    for bad in (lambda: M.paste_quad_u8(L, st, photo, src[:2], mask, coef, (0, 0, 4, 4)),        # planes differ
                lambda: M.paste_quad_u8(L, st, photo, src, mask[:3], coef, (0, 0, 4, 4)),        # mask not n x n
                lambda: M.paste_quad_u8(L, st, photo[:, :, ::2], src, mask, coef, (0, 0, 4, 4)),  # in place needs a contiguous photograph
                lambda: M.paste_quad_u8(L, st, photo, src, mask, coef[:7], (0, 0, 4, 4))):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a malformed paste call must be refused")
    assert not photo.any()
    M.paste_quad_u8(L, st, photo, src + 200, mask + 255, coef, (2, 2, 6, 6))  # the identity map onto a 4 x 4 ROI
    expect = torch.zeros_like(photo)
    expect[:, 2:6, 2:6] = 200
    assert torch.equal(photo, expect)
