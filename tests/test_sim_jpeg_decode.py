"""hipsim tests of the device JPEG decoder (csrc/jpeg_decode.h): the product's kernel source interpreted on the CPU, every image
compared byte for byte with the numpy restatement of libjpeg's decoder that tests/test_jpeg_decode_ref.py pins to Pillow
(tests/jpeg_decode_checks.py).  The malformed scans run here only."""
import pytest
import torch

from tests import jpeg_decode_checks as K

CPU = torch.device("cpu")


def test_entry_points_are_bound(simlib):
    assert simlib.hf_abi_version() == 13
    for name in ("hf_jpeg_decode_workspace_bytes", "hf_jpeg_decode_u8"):
        assert hasattr(simlib, name)
    assert simlib.hf_jpeg_decode_workspace_bytes(1, 8, 8, 1, 1, 1, 0, 100) == 128 + 64 + 16


@pytest.mark.parametrize("mode", K.MODES, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_modes_qualities(simlib, shape, mode):
    K.check_grid(simlib, None, CPU, shape, mode)


def test_several_windows(simlib):
    K.check_windows(simlib, None, CPU)


def test_flat_and_checkerboard(simlib):
    K.check_flat(simlib, None, CPU)


def test_stuffed_bytes_at_boundaries(simlib):
    K.check_stuffing(simlib, None, CPU)


def test_custom_tables_and_extreme_coefficients(simlib):
    K.check_custom_tables(simlib, None, CPU)


def test_restart_intervals(simlib):
    K.check_restart(simlib, None, CPU)


def test_batch_invariant_and_deterministic(simlib):
    K.check_batch(simlib, None, CPU)


def test_float_output(simlib):
    K.check_float(simlib, None, CPU)


def test_invalid_arguments(simlib):
    K.check_invalid(simlib, None, CPU)


def test_marshalled_call(simlib):
    K.check_marshalled(simlib, None, CPU)


def test_header_refusals():
    K.check_refusals()


@pytest.mark.parametrize("name", sorted(K.malformed_cases()))
def test_malformed_scan(simlib, name):
    K.check_malformed(simlib, None, CPU, name)


def test_public_functions_without_a_gpu(tmp_path):
    from hairfastgan_amd import image_utils as IU

    data = K.pil_file(K.picture((24, 40), 2), 75, 2)
    hd = IU.parse_jpeg_header(data)
    assert (hd.height, hd.width, hd.components, hd.hs, hd.vs, hd.restart_interval) == (24, 40, 3, 2, 2, 0)
    assert data[hd.scan_start - 3:hd.scan_start] == b"\x00\x3F\x00"
    (tmp_path / "a.jpg").write_bytes(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_jpeg(data, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_jpeg([tmp_path / "a.jpg"], dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="progressive"):
        IU.parse_jpeg_header(K.refused_files()["progressive"][0])
    with pytest.raises(ValueError):
        IU.read_images([tmp_path / "a.jpg"], decoder="gpu")
    assert tuple(IU.read_images([tmp_path / "a.jpg"])[0].shape) == (3, 24, 40)
