"""GPU tests (-m gpu) of the device PNG decoder (csrc/png_decode.h) through the C ABI and the host layer
(image_utils.decode_png, read_images): every image compared byte for byte with Pillow's (tests/png_decode_checks.py has the
inputs and the rules).  Malformed streams are not run here: they belong to the CPU interpreter
(tests/test_sim_png_decode.py)."""
import numpy as np
import pytest
import torch

from tests import png_decode_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


def test_entry_points_are_bound():
    L, _, _ = gpu_ctx()
    assert L.hf_abi_version() == 13
    assert L.hf_png_decode_workspace_bytes(1, 1, 1, 0, 100) > 0


@pytest.mark.parametrize("color_type", K.COLOR_TYPES, ids=lambda c: f"type{c}")
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_colour_types_levels(shape, color_type):
    K.check_grid(*gpu_ctx(), shape, color_type)


def test_every_filter_type():
    K.check_filters(*gpu_ctx())


def test_palettes():
    K.check_palette(*gpu_ctx())


def test_idat_structure():
    K.check_idat_structure(*gpu_ctx())


def test_matches():
    K.check_matches(*gpu_ctx())


def test_hand_assembled_dynamic_block():
    K.check_hand_block(*gpu_ctx())


def test_segments_of_the_projects_encoder():
    K.check_encoder_files(*gpu_ctx())


def test_full_and_sync_flushes():
    K.check_flushes(*gpu_ctx())


def test_false_candidates():
    K.check_false_candidates(*gpu_ctx())


def test_batch_invariant_and_deterministic():
    K.check_batch(*gpu_ctx())


def test_float_output():
    K.check_float(*gpu_ctx())


def test_invalid_arguments():
    K.check_invalid(*gpu_ctx())


def test_marshalled_call():
    K.check_marshalled(*gpu_ctx())


def test_decode_png_forms(tmp_path):
    """bytes, a path, lists of both in mixed geometries and colour types: each image equals Pillow's, wherever it stands in
    the list; the float form is the CPU's byte / 255; unsupported files raise ValueError."""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    files = [K.pil_file(K.picture((37, 53), 3, 1), 2), K.pil_file(K.picture((24, 40), 4, 2), 6, 9),
             K.pil_file(K.picture((37, 53), 3, 3), 2, 1), K.pil_file(K.picture((17, 9), 1), 0),
             K.pil_file(K.noise((37, 53, 1), 4), 3), K.pil_file(K.noise((37, 53, 2), 5), 4, 0), K.flush_files()[0], K.flush_files()[1]]
    paths = []
    for k, data in enumerate(files):
        paths.append(tmp_path / f"{k}.png")
        paths[-1].write_bytes(data)
    one = IU.decode_png(files[0])
    assert one.is_cuda and one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), K.reference(files[0]))
    assert torch.equal(IU.decode_png(paths[0]), one) and torch.equal(IU.decode_png(str(paths[0])), one)
    mixed = [files[0], paths[1], str(paths[2]), files[3], files[4], paths[5], files[6], paths[7]]
    first = None
    for order in (range(8), reversed(range(8))):
        order = list(order)
        got = IU.decode_png([mixed[k] for k in order])
        assert isinstance(got, list) and len(got) == 8
        for k, img in zip(order, got):
            assert np.array_equal(img.cpu().numpy(), K.reference(files[k])), k
        first = first or {k: img for k, img in zip(order, got)}
    again = IU.decode_png(mixed)
    assert all(torch.equal(again[k], first[k]) for k in range(8))  # two calls, the same bits
    for k in (1, 3, 4, 5):
        own = IU.decode_png(files[k], mode="unchanged")
        assert np.array_equal(own.cpu().numpy(), K.reference(files[k], "unchanged")), k
    f = IU.decode_png(files[1], dtype=torch.float32)
    assert tuple(f.shape) == (3, 24, 40) and torch.equal(f.cpu(), torch.from_numpy(K.reference(files[1]).copy()).permute(2, 0, 1) / 255)
    assert IU.decode_png([]) == []
    for what, (data, word) in K.refused_files().items():
        with pytest.raises(ValueError, match=word):
            IU.decode_png([files[0], data])
    with pytest.raises(ValueError, match="mode"):
        IU.decode_png(files[0], mode="L")
    with pytest.raises(TypeError):
        IU.decode_png(files[0], dtype=torch.float16)
    with pytest.raises(TypeError):
        IU.decode_png(np.zeros(4, np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_png(files[0], device="cpu")


def test_encode_png_round_trip():
    """the project's own files: encode_png's output decodes to the pixels it was made from, RGB and grey, for an image of
    several segments"""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    imgs = torch.from_numpy(np.stack([K.picture((96, 700), 3, k) for k in range(2)])).to(dev)
    files = IU.encode_png(imgs)
    for data, img, src in zip(files, IU.decode_png(files), imgs):
        assert torch.equal(img, src) and np.array_equal(img.cpu().numpy(), K.reference(data))
    grey = imgs[0, :, :, 0].contiguous()
    assert torch.equal(IU.decode_png(IU.encode_png(grey), mode="unchanged")[:, :, 0], grey)
