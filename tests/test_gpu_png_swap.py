"""GPU tests (-m gpu) of `args.image_decoder` for PNG paths (hair_swap.py): PNG files handed to swap are decoded on the
device (image_utils.decode_png), and the swap returns the same bits as with PIL.  One swap per decoder and case."""
import numpy as np
import PIL.Image
import pytest
import torch

from tests import png_decode_checks as K
from tests.test_gpu_jpeg_swap import _with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hf():
    from tests.test_gpu_schedule import _hairfast

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return _hairfast(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def faces(tmp_path_factory):
    """three 1024^2 PNG files - PIL at level 6, PIL at level 1, this project's encoder through save_images - a JPEG of the
    second and an interlaced copy of the first"""
    from hairfastgan_amd import image_utils as IU

    root = tmp_path_factory.mktemp("png_swap")
    imgs = [K.picture((1024, 1024), 3, 40 + k) for k in range(3)]
    paths = [root / f"face{k}.png" for k in range(3)]
    PIL.Image.fromarray(imgs[0], "RGB").save(paths[0], compress_level=6)
    PIL.Image.fromarray(imgs[1], "RGB").save(paths[1], compress_level=1)
    IU.save_images(torch.from_numpy(imgs[2]).permute(2, 0, 1)[None].float().div(255).cuda(), [paths[2]])
    assert np.array_equal(np.asarray(PIL.Image.open(paths[2])), imgs[2])
    PIL.Image.fromarray(imgs[1], "RGB").save(root / "face1.jpg", format="JPEG", quality=90)
    (root / "laced.png").write_bytes(K.adam7_file(imgs[0]))
    assert np.array_equal(np.asarray(PIL.Image.open(root / "laced.png").convert("RGB")), imgs[0])
    return root, paths


def test_swap_from_png_paths(hf, faces):
    root, paths = faces
    ref = _with(hf, "pil", lambda: hf.swap(*paths, seed=7))
    got = _with(hf, "device", lambda: hf.swap(*paths, seed=7))
    assert got.shape == (3, 1024, 1024) and torch.equal(got, ref)
    assert torch.equal(_with(hf, None, lambda: hf.swap(*paths, seed=7)), ref)  # without args.image_decoder nothing changes


def test_swap_from_a_mixed_triple(hf, faces):
    root, paths = faces
    mixed = (paths[0], root / "face1.jpg", torch.from_numpy(np.asarray(PIL.Image.open(paths[2]).convert("RGB")).transpose(2, 0, 1).copy()))
    assert torch.equal(_with(hf, "device", lambda: hf.swap(*mixed, seed=7)), _with(hf, "pil", lambda: hf.swap(*mixed, seed=7)))


def test_a_png_the_device_refuses_goes_through_pil(hf, faces):
    from hairfastgan_amd import image_utils as IU

    root, paths = faces
    with pytest.raises(ValueError, match="interlace"):
        IU.parse_png_header((root / "laced.png").read_bytes())
    triple = (root / "laced.png", paths[1], paths[2])
    assert torch.equal(_with(hf, "device", lambda: hf.swap(*triple, seed=7)), _with(hf, "pil", lambda: hf.swap(*triple, seed=7)))


def test_read_images_dispatches_by_signature(faces, tmp_path):
    from hairfastgan_amd import image_utils as IU

    root, paths = faces
    mixed = [paths[0], root / "face1.jpg", paths[2]]
    got = IU.read_images(mixed, decoder="device")
    for t, ref in zip(got, IU.read_images(mixed, decoder="pil")):
        assert t.is_cuda and t.dtype == torch.uint8 and torch.equal(t.cpu(), ref)
    (tmp_path / "x.bin").write_bytes(b"GIF89a" + bytes(20))
    with pytest.raises(ValueError, match="neither a PNG nor a JPEG"):
        IU.read_images([paths[0], tmp_path / "x.bin"], decoder="device")
