"""hipsim tests of the `--save_all` byte kernels (csrc/export.h): the product's kernel source interpreted on the CPU
against the reference's torch expressions and its mask colours - byte for byte (tests/export_checks.py)."""
import pytest
import torch

from tests import export_checks as K

CPU = torch.device("cpu")


def test_entry_points_are_bound(simlib):
    assert simlib.hf_abi_version() == 13
    assert hasattr(simlib, "hf_image_to_bytes_f32") and hasattr(simlib, "hf_labels_to_rgb_i64")


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("value_range", K.RANGES)
@pytest.mark.parametrize("shape", K.SHAPES)
def test_to_bytes(simlib, shape, value_range, rounding, layout):
    K.check_to_bytes(simlib, None, CPU, shape, value_range, rounding, layout)


def test_to_bytes_unaligned_base(simlib):
    K.check_to_bytes_unaligned(simlib, None, CPU)


def test_to_bytes_general_range(simlib):
    K.check_general_range(simlib, None, CPU)


def test_labels_to_rgb(simlib):
    K.check_labels_to_rgb(simlib, None, CPU)
    K.check_palette_is_the_goldens()


def test_invalid_arguments(simlib):
    K.check_invalid(simlib, None, CPU)


def test_public_functions_refuse_cpu_tensors():
    from hairfastgan_amd import image_utils as IU

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.to_bytes(torch.zeros(1, 3, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.labels_to_rgb(torch.zeros(1, 1, 4, 8, dtype=torch.int64))
