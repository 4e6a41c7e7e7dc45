"""hipsim tests of the device PNG decoder (csrc/png_decode.h): the product's kernel source interpreted on the CPU, every image
compared byte for byte with Pillow's (tests/png_decode_checks.py has the inputs and the rules).  The malformed streams run
here only.  Every case runs here, the match of distance 32768 included: the interpreter takes about a second for it."""
import pytest
import torch

from tests import png_decode_checks as K
from tests.metric_common import patch_host_modules

CPU = torch.device("cpu")


def test_entry_points_are_bound(simlib):
    assert simlib.hf_abi_version() == 13
    for name in ("hf_png_decode_workspace_bytes", "hf_png_decode_u8"):
        assert hasattr(simlib, name)
    assert simlib.hf_png_decode_workspace_bytes(1, 1, 1, 0, 100) > 0


@pytest.mark.parametrize("color_type", K.COLOR_TYPES, ids=lambda c: f"type{c}")
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_colour_types_levels(simlib, shape, color_type):
    K.check_grid(simlib, None, CPU, shape, color_type)


def test_every_filter_type(simlib):
    K.check_filters(simlib, None, CPU)


def test_palettes(simlib):
    K.check_palette(simlib, None, CPU)


def test_idat_structure(simlib):
    K.check_idat_structure(simlib, None, CPU)


def test_matches(simlib):
    K.check_matches(simlib, None, CPU)


def test_hand_assembled_dynamic_block(simlib):
    K.check_hand_block(simlib, None, CPU)


def test_segments_of_the_projects_encoder(simlib):
    K.check_encoder_files(simlib, None, CPU)


def test_full_and_sync_flushes(simlib):
    K.check_flushes(simlib, None, CPU)


def test_false_candidates(simlib):
    K.check_false_candidates(simlib, None, CPU)


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


def test_header_fields():
    K.check_header_fields()


@pytest.mark.parametrize("name", sorted(K.malformed_cases()))
def test_malformed_stream(simlib, name, monkeypatch):
    """the case's error code on guarded buffers, and ValueError from decode_png (its library calls pointed at the interpreter)"""
    from hairfastgan_amd import image_utils as IU

    K.check_malformed(simlib, None, CPU, name)
    data, stream_of, code = K.malformed_cases()[name]
    patch_host_modules(monkeypatch, simlib, ["hairfastgan_amd.image_utils"])
    good = K.pil_file(K.picture((5, 9), 1), 0)
    bad = K.png_file(5, 9, 0, bytes(stream_of(K.idat_stream(data))))
    assert torch.equal(IU.decode_png(good, device="cpu"), torch.from_numpy(K.reference(good).copy()))
    with pytest.raises(ValueError, match=r"corrupt PNG \(file 1\)"):
        IU.decode_png([good, bad], device="cpu")


def test_public_functions_without_a_gpu(tmp_path):
    from hairfastgan_amd import image_utils as IU

    data = K.pil_file(K.picture((24, 40), 3), 2)
    hd = IU.parse_png_header(data)
    assert (hd.height, hd.width, hd.color_type, hd.channels) == (24, 40, 2, 3)
    (tmp_path / "a.png").write_bytes(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_png(data, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_png([tmp_path / "a.png"], dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="interlace"):
        IU.parse_png_header(K.refused_files()["interlaced"][0])
    with pytest.raises(ValueError, match="mode"):
        IU.decode_png(data, mode="L")
    ref = IU.read_images([tmp_path / "a.png"], decoder="pil")[0]  # unchanged: PIL on the host
    assert not ref.is_cuda and tuple(ref.shape) == (3, 24, 40) and torch.equal(ref, torch.from_numpy(K.reference(data).copy()).permute(2, 0, 1))
    assert tuple(IU.read_images([tmp_path / "a.png"])[0].shape) == (3, 24, 40)
