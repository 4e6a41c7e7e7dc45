"""hipsim tests of the device JPEG encoder (csrc/jpeg.h): the product's kernel source interpreted on the CPU, every file
compared byte for byte with the numpy restatement of libjpeg's pipeline that tests/test_jpeg_ref.py pins to Pillow, and
opened by PIL (tests/jpeg_checks.py)."""
import pytest
import torch

from tests import jpeg_checks as K

CPU = torch.device("cpu")


def test_entry_points_are_bound(simlib):
    assert simlib.hf_abi_version() == 13
    for name in ("hf_jpeg_bound", "hf_jpeg_chunk_mcus", "hf_jpeg_workspace_bytes", "hf_jpeg_encode_u8"):
        assert hasattr(simlib, name)
    assert simlib.hf_jpeg_chunk_mcus(3, 2) == 42 and simlib.hf_jpeg_bound(8, 8, 1, 0) == 334 + 2 * 208 + 2


@pytest.mark.parametrize("mode", K.MODES, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_ragged(simlib, shape, mode):
    K.check_tiny(simlib, None, CPU, shape, mode)


def test_restart_index_wraps(simlib):
    K.check_restart_wrap(simlib, None, CPU)


def test_chunk_boundary(simlib):
    K.check_chunk_boundary(simlib, None, CPU)


def test_symbol_coverage(simlib):
    K.check_symbols(simlib, None, CPU)


def test_bound_holds_for_noise(simlib):
    K.check_bound(simlib, None, CPU)


def test_batch_invariant_and_deterministic(simlib):
    K.check_batch_invariance(simlib, None, CPU)


def test_invalid_arguments(simlib):
    K.check_invalid(simlib, None, CPU)


def test_marshalled_call(simlib):
    K.check_marshalled(simlib, None, CPU)


def test_public_functions_refuse_cpu_tensors(tmp_path):
    from hairfastgan_amd import image_utils as IU

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.encode_jpeg(torch.zeros(1, 4, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.encode_jpeg(torch.zeros(4, 8, dtype=torch.uint8), quality=90, subsampling="4:4:4")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.save_image(torch.zeros(3, 4, 8), tmp_path / "a.jpg", encoder="device", format="jpeg")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.save_images(torch.zeros(2, 3, 4, 8), [tmp_path / "a.jpg", tmp_path / "b.jpg"], format="jpeg", quality=90)
    assert not list(tmp_path.iterdir())
