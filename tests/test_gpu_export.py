"""GPU tests (-m gpu) of the `--save_all` byte kernels (csrc/export.h) through the C ABI and the public functions of
hairfastgan_amd.image_utils: byte-equal to the reference's torch expressions evaluated on the CPU and to its mask colours
(tests/export_checks.py has the inputs and the rules)."""
import numpy as np
import pytest
import torch

from tests import export_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("value_range", K.RANGES)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_to_bytes(shape, value_range, rounding, layout):
    K.check_to_bytes(*gpu_ctx(), shape, value_range, rounding, layout)


def test_to_bytes_unaligned_base():
    K.check_to_bytes_unaligned(*gpu_ctx())


def test_to_bytes_general_range():
    K.check_general_range(*gpu_ctx())


def test_labels_to_rgb():
    K.check_labels_to_rgb(*gpu_ctx())
    K.check_palette_is_the_goldens()


def test_invalid_arguments():
    K.check_invalid(*gpu_ctx())


def test_public_functions(tmp_path):
    """to_bytes / labels_to_rgb / save_image on GPU tensors: the marshalled calls' bytes, a single image without its batch
    axis, and the PNG save_image writes decoded again."""
    import PIL.Image

    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    x = next(K.chunks((2, 3, 8, 12)))
    for value_range in K.RANGES:
        for rounding in IU.ROUNDINGS:
            for layout in IU.LAYOUTS:
                got = IU.to_bytes(x.to(dev), value_range, rounding, layout)
                assert torch.equal(got.cpu(), K.expected_bytes(x, value_range, rounding, layout))
    assert torch.equal(IU.to_bytes(x[1].to(dev)).cpu(), K.expected_bytes(x, (-1, 1), "floor", "hwc")[1])
    labels, rgb = K.golden_masks()
    got = IU.labels_to_rgb(torch.from_numpy(labels).to(dev)[:, None])
    assert np.array_equal(got.cpu().numpy(), rgb)
    assert np.array_equal(IU.labels_to_rgb(torch.from_numpy(labels[0]).to(dev)).cpu().numpy(), rgb[0])
    IU.save_image(x[0].to(dev), tmp_path / "one.png")
    with PIL.Image.open(tmp_path / "one.png") as im:
        assert np.array_equal(np.asarray(im), K.expected_bytes(x[:1], (0, 1), "nearest", "hwc")[0].numpy())
