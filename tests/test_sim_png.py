"""hipsim tests of the device PNG encoder (csrc/png.h): the product's kernel source interpreted on the CPU, every file
decoded again by the checks' own parser (struct, zlib, numpy) and by PIL (tests/png_checks.py)."""
import pytest
import torch

from tests import png_checks as K

CPU = torch.device("cpu")


def test_entry_points_are_bound(simlib):
    assert simlib.hf_abi_version() == 13
    for name in ("hf_png_bound", "hf_png_segment_rows", "hf_png_workspace_bytes", "hf_png_encode_u8"):
        assert hasattr(simlib, name)
    assert simlib.hf_png_segment_rows(1024, 1024, 3) == 8 and simlib.hf_png_segment_rows(256, 256, 3) == 16


@pytest.mark.parametrize("shape", K.TINY)
def test_tiny_and_ragged(simlib, shape):
    K.check_tiny(simlib, None, CPU, shape)


def test_heights_around_a_segment(simlib):
    K.check_heights(simlib, None, CPU)


def test_input_base_offset_by_one_byte(simlib):
    K.check_offset_base(simlib, None, CPU)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_filter_modes(simlib, mode):
    K.check_filter(simlib, None, CPU, mode)


def test_runs(simlib):
    K.check_runs(simlib, None, CPU)


def test_incompressible_takes_stored_blocks(simlib):
    K.check_incompressible(simlib, None, CPU)


def test_deep_code_is_length_limited(simlib):
    K.check_deep_code(simlib, None, CPU)


def test_batch_invariant_and_deterministic(simlib):
    K.check_batch_invariance(simlib, None, CPU)


def test_size_conditions(simlib):
    K.check_sizes(simlib, None, CPU)


def test_invalid_arguments(simlib):
    K.check_invalid(simlib, None, CPU)


def test_marshalled_call(simlib):
    K.check_marshalled(simlib, None, CPU)


def test_public_functions_refuse_cpu_tensors(tmp_path):
    from hairfastgan_amd import image_utils as IU

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.encode_png(torch.zeros(1, 4, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.save_image(torch.zeros(3, 4, 8), tmp_path / "a.png", encoder="device")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.save_images(torch.zeros(2, 3, 4, 8), [tmp_path / "a.png", tmp_path / "b.png"])
    assert not list(tmp_path.iterdir())
