"""The oracle of the device JPEG encoder's tests pinned to Pillow: tests/jpeg_ref.py must give, WHOLE FILE and byte for byte,
what `Image.save(format="JPEG", quality=, subsampling=, restart_marker_rows=1)` writes, for every shape, subsampling and
quality the device checks use (tests/jpeg_checks.py).  CPU only; it fails - it does not skip - where Pillow lacks
libjpeg-turbo or the restart_marker_rows argument, since then nothing pins the oracle."""
import io

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests.png_checks import smooth

SHAPES = [(1, 1), (8, 8), (7, 13), (16, 16), (17, 9), (9, 33), (24, 40), (37, 53), (150, 21), (80, 8), (33, 97)]
QUALITIES = [10, 30, 75, 92, 95, 100]
MODES = ["grey", 0, 1, 2]


def test_pillow_is_the_reference_build():
    import PIL.Image
    from PIL import features

    assert features.check_feature("libjpeg_turbo"), "Pillow without libjpeg-turbo: the oracle cannot be pinned"
    a, b = io.BytesIO(), io.BytesIO()
    im = PIL.Image.fromarray(smooth((40, 24, 3), 0))
    im.save(a, format="JPEG", restart_marker_rows=1)
    im.save(b, format="JPEG")
    assert b"\xFF\xDD" in a.getvalue() and b"\xFF\xDD" not in b.getvalue(), "Pillow ignores restart_marker_rows"


def _inputs(shape, mode):
    c = 1 if mode == "grey" else 3
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    return [smooth(shape + (c,), shape[1]), rng.integers(0, 256, size=shape + (c,)).astype(np.uint8)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_file_equals_pillow(shape, mode):
    sub = 2 if mode == "grey" else mode
    for img in _inputs(shape, mode):
        for q in QUALITIES:
            ours, theirs = R.encode(img, q, sub).data, R.pil_encode(img, q, sub)
            assert ours == theirs, (shape, mode, q, len(ours), len(theirs),
                                    next((k for k, (x, y) in enumerate(zip(ours, theirs)) if x != y), None))


def test_quality_extremes_and_structure():
    img = smooth((24, 40, 3), 3)
    for q in (1, 2, 49, 50, 51, 99):
        assert R.encode(img, q, 2).data == R.pil_encode(img, q, 2)
    enc = R.encode(img, 75, 2)
    assert len(enc.intervals) == 2 and enc.blocks[0].shape == (4, 6, 64) and enc.blocks[1].shape == (2, 3, 64)
    assert enc.data.count(b"\xFF\xD0") == 1 and enc.data.endswith(b"\xFF\xD9")
    assert sum(v for k, v in enc.hist.items() if k.startswith("dc")) == 2 * 3 * 6
