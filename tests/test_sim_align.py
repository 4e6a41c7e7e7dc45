"""hipsim tests of the face-alignment kernels (csrc/align.h): the product's kernel sources interpreted on the CPU against
PIL / scipy through the restatement (tests/align_ref.py) - byte for byte; the pad stage under the tie rule of
tests/align_checks.py."""
import numpy as np
import pytest
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import face_align as FA
from tests import align_checks as K
from tests import align_ref as R

CPU = torch.device("cpu")


@pytest.mark.parametrize("in_w,in_h,out_w,out_h", K.RESIZE_CASES)
def test_resize_lanczos(simlib, in_w, in_h, out_w, out_h):
    K.check_resize(simlib, None, CPU, in_w, in_h, out_w, out_h)


@pytest.mark.parametrize("name", list(K.QUADS))
def test_quad_transform(simlib, name):
    K.check_transform(simlib, None, CPU, name)


def test_fused_equals_chained_pair(simlib):
    K.check_fused_small(simlib, None, CPU)


@pytest.mark.parametrize("name", ["four_sides", "none"])  # (one_side: radius 48 on 10^6 pixels - the GPU test)
def test_pad(simlib, name):
    K.check_pad(simlib, None, CPU, name)
    if name == "none":
        K.check_pad_invalid(simlib, None, CPU)


@pytest.mark.parametrize("name", list(R.SMALL_CASES))
def test_align_small(simlib, name):
    K.check_align_against_restatement(simlib, None, CPU, R.SMALL_CASES[name], 64, 256,
                                      count_key="small_corner" if name == "corner" else None, as_float=name == "inside")


def test_unit_float_is_a_true_division(simlib):
    b = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(M.u8_to_unit(simlib, None, b), b.float().div(255))


def test_invalid_arguments(simlib):
    img = torch.zeros(3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="invalid argument"):
        simlib_call = simlib.hf_resize_lanczos_u8(img.data_ptr(), None, img.data_ptr(), 3, 8, 8, 8, 8, None, None, 0, None, None, 0, None)
        M.check(simlib, simlib_call, "hf_resize_lanczos_u8")
    with pytest.raises(ValueError):
        M.resize_lanczos_u8(simlib, None, img, 4, 4, None, None)
    with pytest.raises(TypeError):
        FA.resize_lanczos(simlib, None, img.float(), 4, 4)


@pytest.mark.parametrize("h,w,pad,blur", [(23, 31, (40, 35, 33, 38), 6.0),    # pads wider than the image: np.pad reflects repeatedly
                                          (40, 50, (30, 25, 28, 26), 12.0),   # sigma 12: radius 48, several tiles of halo
                                          (70, 9, (3, 4, 5, 6), 0.3)])        # radius 1
def test_pad_float_image_bits(simlib, h, w, pad, blur):
    """Noise through the pad stage: the interpreter runs IEEE arithmetic like numpy and scipy, so beyond the tie rule the
    float32 image before rint is the restatement's bit for bit (and with it every byte)."""
    arr = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pre = R.pad_float(arr, pad, blur)
    got, got_pre = FA.pad_blur_fade(simlib, None, K.chw(arr, CPU), pad, blur, return_float=True)
    assert np.array_equal(K.hwc(got_pre), pre)
    assert np.array_equal(K.hwc(got), R.to_bytes(pre))
