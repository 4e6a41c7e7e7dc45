"""The numpy restatement of the JPEG decoder (tests/jpeg_decode_ref.py), the oracle of the device decoder's tests, pinned to
Pillow's libjpeg-turbo: the pixels of `Image.open(f).convert("RGB")`, exactly."""
import io

import numpy as np
import PIL.Image
import pytest

from tests import jpeg_decode_checks as K
from tests import jpeg_decode_ref as D


def pil_pixels(data):
    with PIL.Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def same_as_pil(data):
    got, want = D.decode(data), pil_pixels(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], np.abs(got.astype(int) - want).max())


@pytest.mark.parametrize("mode", K.MODES, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_modes_qualities(shape, mode):
    for q in K.QUALITIES:
        for data in K.grid_files(shape, mode, q):
            same_as_pil(data)


@pytest.mark.parametrize("width", [2, 3, 4, 5, 6])
def test_narrow_images_take_the_plain_upsampler(width):
    """a downsampled width of 1 or 2 is replicated, not interpolated"""
    for mode in (1, 2):
        for h in (3, 16):
            same_as_pil(K.pil_file(K.noise((h, width, 3), width), 90, mode))


def test_optimised_and_custom_tables():
    for mode in K.MODES:
        same_as_pil(K.pil_file(K.picture((37, 53), mode), 75, mode, optimize=True))
        for step in (1, 255):
            same_as_pil(K.pil_file(K.picture((24, 40), mode), None, mode, qtables=[[step] * 64] * 2))


def test_restart_intervals():
    for mode in K.MODES:
        img = K.picture((37, 53), mode)
        for kw in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
            data = K.pil_file(img, 90, mode, **kw)
            assert D.parse(data).ri > 0
            same_as_pil(data)
    data = K.pil_file(K.picture((80, 8), 0), 75, 0, restart_marker_rows=1)  # 10 intervals: the RST index wraps
    assert data.count(b"\xFF\xD0") == 2
    same_as_pil(data)


def test_noise_checkerboard_flat():
    for mode in K.MODES:
        c = 1 if mode == "grey" else 3
        same_as_pil(K.pil_file(K.noise((64, 96, c), 3), 100, mode))
        same_as_pil(K.pil_file(np.full((40, 56, c), 97, np.uint8), 75, mode))
        y, x = np.mgrid[0:24, 0:40]
        same_as_pil(K.pil_file(np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], c, 2), 100, mode))


@pytest.mark.parametrize("name", sorted(K.EXTREME_FILES))
def test_extreme_coefficients(name):
    """writer-built files: coefficients no encoder emits; the IDCT result leaves the signed 10-bit range, where a wrapping
    range-limit table and the saturation Pillow's libjpeg-turbo applies differ"""
    same_as_pil(K.EXTREME_FILES[name]())


def test_unchanged_mode_and_refusals():
    data = K.pil_file(K.picture((17, 9), "grey"), 75, "grey")
    assert D.decode(data, "unchanged").shape == (17, 9, 1)
    assert np.array_equal(D.decode(data, "unchanged")[:, :, 0], D.decode(data)[:, :, 1])
    for what, (data, word) in K.refused_files().items():
        with pytest.raises(ValueError, match=word):
            D.decode(data)
