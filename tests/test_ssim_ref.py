"""CPU tests of the SSIM restatements (tests/ssim_ref.py), of what tests/ssim_checks.py records about them, and of the host
surface of hairfastgan_amd.ssim that needs no kernel: the disagreement of the two fp64 restatements the device thresholds are
built on is measured again and must not exceed the recorded figures; the fp32 evaluation of the same formula misses the rule."""
import numpy as np
import pytest
import torch

from hairfastgan_amd import ssim as SS
from tests import ssim_checks as K
from tests import ssim_ref as R


@pytest.mark.parametrize("family", K.FAMILIES)
def test_restatements_agree_within_the_recorded_gap(family):
    gaps = [K.restatement_gap(shape, family) for shape in K.KERNEL_SHAPES]
    mean, pixel = max(g[0] for g in gaps), max(g[1] for g in gaps)
    print(family, f"plane means {mean:.2e} pixels {pixel:.2e}")
    assert mean <= K.D_MEAN[family] and pixel <= K.D_MAP[family], (family, mean, pixel)


def test_ms_ssim_restatements_agree_within_the_recorded_gap():
    worst = 0.0
    for hw, weights, kind in K.MS_CASES:
        for noise in K.MS_NOISES:
            x, y = K.ms_case(hw, noise)
            worst = max(worst, float((K.ms_truth(hw, weights, kind, noise)[0] - K.ms_ssim_scipy(x, y, kind, weights)).abs().max()))
    print("ms_ssim", worst)
    assert worst <= K.MS_D


def test_fp32_evaluation_misses_the_rule():
    """The rule is tight enough to notice an fp32 kernel: on the general shapes the fp32 conv form misses it in the noise
    families (a few 1e-7 against a threshold of 1e-14) and by far in the offset family."""
    for family in ("noise4", "noise24", "offset"):
        results = [K.fp32_misses(shape, family) for shape in K.KERNEL_SHAPES[4:6]]
        print(family, results)
        assert all(m for m, _ in results), (family, results)
    assert K.fp32_misses((6, 70, 64, 11), "offset")[1] > 1e-3


def test_floor_covers_the_restatements():
    """The floor bounds any fp64 evaluation: the scipy form stays within it of the conv form, pixel by pixel, wherever the
    floor (and not 8 d) is what decides."""
    for shape in K.KERNEL_SHAPES:
        planes, h, w, win = shape
        x, y = K.plane_case(planes, h, w, "offset")
        s, cs, fs, fcs = K.plane_truth(shape, "offset")
        s2, cs2 = R.scipy_maps(x.numpy(), y.numpy(), K.WINDOWS[win], 1.0)
        assert bool(((s - torch.from_numpy(s2)).abs() <= fs).all()) and bool(((cs - torch.from_numpy(cs2)).abs() <= fcs).all()), shape


def test_families_are_where_they_should_be():
    shape = (6, 70, 64, 11)
    means = {f: float(K.plane_truth(shape, f)[0].mean()) for f in K.FAMILIES}
    print(means)
    assert abs(means["independent"]) < 0.05 and means["noise4"] > 0.97 and 0.6 < means["noise24"] < 0.9 and 0.2 < means["noise64"] < 0.5
    assert means["inverted"] < -0.5
    s, cs = K.plane_truth(shape, "inverted")[:2]
    assert float(cs.max()) < 0.0
    taps, cn = R.window("gaussian")
    assert len(taps) == 11 and cn == 1.0 and abs(taps.sum() - 1.0) < 1e-15
    assert R.window("uniform")[1] == 49 / 48


def test_ms_ssim_values():
    """About 0.9975 and 0.72 at 176 x 177 with noise 4 and 64 (structured 8-bit images, five scales, Gaussian 11)."""
    hw, weights, kind = K.MS_CASES[0]
    assert abs(float(K.ms_truth(hw, weights, kind, 4)[0]) - 0.9975) < 2e-3
    assert abs(float(K.ms_truth(hw, weights, kind, 64)[0]) - 0.72) < 3e-2


def test_window_taps_match_the_restatement():
    for kind in ("gaussian", "uniform"):
        taps, cn = SS.window_taps(kind)
        ref, cn_ref = R.window(kind)
        assert cn == cn_ref and np.abs(np.asarray(taps) - ref).max() <= 2.0 ** -52
    assert len(SS.window_taps("gaussian", sigma=0.5)[0]) == 5 and len(SS.window_taps("uniform", 3)[0]) == 3
    for bad in (dict(window="gaussian", win_size=4), dict(window="uniform", win_size=13), dict(window="gaussian", sigma=3.0), dict(window="box")):
        with pytest.raises(ValueError):
            SS.window_taps(**bad)
