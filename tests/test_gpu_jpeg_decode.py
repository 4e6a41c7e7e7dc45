"""GPU tests (-m gpu) of the device JPEG decoder (csrc/jpeg_decode.h) through the C ABI and the host layer
(image_utils.decode_jpeg, read_images): every image compared byte for byte with the numpy restatement of libjpeg's decoder
that tests/test_jpeg_decode_ref.py pins to Pillow, and with Pillow itself (tests/jpeg_decode_checks.py has the inputs and
the rules).  Malformed scans are not run here: they belong to the CPU interpreter (tests/test_sim_jpeg_decode.py)."""
import numpy as np
import pytest
import torch

from tests import jpeg_decode_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


def test_entry_points_are_bound():
    L, _, _ = gpu_ctx()
    assert L.hf_abi_version() == 13
    assert L.hf_jpeg_decode_workspace_bytes(1, 8, 8, 1, 1, 1, 0, 100) == 128 + 64 + 16


@pytest.mark.parametrize("mode", K.MODES, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_modes_qualities(shape, mode):
    K.check_grid(*gpu_ctx(), shape, mode)


def test_several_windows():
    K.check_windows(*gpu_ctx())


def test_flat_and_checkerboard():
    K.check_flat(*gpu_ctx())


def test_stuffed_bytes_at_boundaries():
    K.check_stuffing(*gpu_ctx())


def test_custom_tables_and_extreme_coefficients():
    K.check_custom_tables(*gpu_ctx())


def test_restart_intervals():
    K.check_restart(*gpu_ctx())


def test_batch_invariant_and_deterministic():
    K.check_batch(*gpu_ctx())


def test_float_output():
    K.check_float(*gpu_ctx())


def test_invalid_arguments():
    K.check_invalid(*gpu_ctx())


def test_marshalled_call():
    K.check_marshalled(*gpu_ctx())


def _pil_rgb(data):
    import io

    import PIL.Image

    with PIL.Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def test_decode_jpeg_forms(tmp_path):
    """bytes, a path, lists of both in mixed geometries: each image equals Pillow's, wherever it stands in the list; the float
    form is the CPU's byte / 255; unsupported and corrupt files raise ValueError."""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    files = [K.pil_file(K.picture((37, 53), 2, 1), 75, 2), K.pil_file(K.picture((24, 40), 0, 2), 90, 0),
             K.pil_file(K.picture((37, 53), 2, 3), 75, 2), K.pil_file(K.picture((17, 9), "grey"), 75, "grey"),
             K.pil_file(K.picture((37, 53), 2, 4), 75, 2, restart_marker_rows=1), K.pil_file(K.noise((37, 53, 3), 5), 100, 2, optimize=True)]
    paths = []
    for k, data in enumerate(files):
        paths.append(tmp_path / f"{k}.jpg")
        paths[-1].write_bytes(data)
    one = IU.decode_jpeg(files[0])
    assert one.is_cuda and one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), _pil_rgb(files[0]))
    assert torch.equal(IU.decode_jpeg(paths[0]), one) and torch.equal(IU.decode_jpeg(str(paths[0])), one)
    mixed = [files[0], paths[1], str(paths[2]), files[3], files[4], paths[5]]
    for order in (range(6), reversed(range(6))):
        order = list(order)
        got = IU.decode_jpeg([mixed[k] for k in order])
        assert isinstance(got, list) and len(got) == 6
        for k, img in zip(order, got):
            assert np.array_equal(img.cpu().numpy(), _pil_rgb(files[k])), k
    grey = IU.decode_jpeg(files[3], mode="unchanged")
    assert tuple(grey.shape) == (17, 9, 1) and np.array_equal(grey.cpu().numpy()[:, :, 0], _pil_rgb(files[3])[:, :, 0])
    f = IU.decode_jpeg(files[1], dtype=torch.float32)
    assert tuple(f.shape) == (3, 24, 40) and torch.equal(f.cpu(), torch.from_numpy(_pil_rgb(files[1]).transpose(2, 0, 1).copy()).float().div(255))
    chw = IU.read_images(paths[:3], decoder="device")
    for t, ref in zip(chw, IU.read_images(paths[:3], decoder="pil")):
        assert t.is_cuda and torch.equal(t.cpu(), ref)
    assert IU.decode_jpeg([]) == []
    for what, (data, word) in K.refused_files().items():
        with pytest.raises(ValueError, match=word):
            IU.decode_jpeg([files[0], data])
    with pytest.raises(ValueError, match="mode"):
        IU.decode_jpeg(files[0], mode="L")
    with pytest.raises(TypeError):
        IU.decode_jpeg(files[0], dtype=torch.float16)
    with pytest.raises(TypeError):
        IU.decode_jpeg(np.zeros(4, np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.decode_jpeg(files[0], device="cpu")


def test_encode_jpeg_round_trip():
    """the project's own files: encode_jpeg's output (one restart interval per MCU row) decodes to the pixels PIL decodes
    from it, at every subsampling, for an image wider than one chunk of the encoder"""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    imgs = torch.from_numpy(np.stack([K.picture((96, 700), 0, k) for k in range(2)])).to(dev)
    for name in IU.JPEG_SUBSAMPLINGS:
        files = IU.encode_jpeg(imgs, quality=90, subsampling=name)
        for data, img in zip(files, IU.decode_jpeg(files)):
            assert np.array_equal(img.cpu().numpy(), _pil_rgb(data)), name
    data = IU.encode_jpeg(imgs[0, :, :, 0].contiguous(), quality=60)
    assert np.array_equal(IU.decode_jpeg(data).cpu().numpy(), _pil_rgb(data))
