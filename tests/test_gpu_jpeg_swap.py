"""GPU tests (-m gpu) of `args.image_decoder` (hair_swap.py): JPEG paths handed to swap / swap_batch / swap(align=True) are
decoded on the device, and the swap returns the same bits as with PIL."""
import numpy as np
import PIL.Image
import pytest
import torch

from tests import jpeg_decode_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hf():
    from tests.test_gpu_schedule import _hairfast

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return _hairfast(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def faces(tmp_path_factory):
    """three 1024^2 JPEG files (4:2:0, 4:4:4, 4:2:2 with restart markers), a PNG and a progressive JPEG of the first"""
    root = tmp_path_factory.mktemp("jpeg_swap")
    imgs = [K.picture((1024, 1024), 0, 30 + k) for k in range(3)]
    kw = [dict(quality=90, subsampling=2), dict(quality=95, subsampling=0), dict(quality=75, subsampling=1, restart_marker_rows=1)]
    paths = []
    for k, (img, a) in enumerate(zip(imgs, kw)):
        paths.append(root / f"face{k}.jpg")
        PIL.Image.fromarray(img, "RGB").save(paths[-1], format="JPEG", **a)
    PIL.Image.fromarray(imgs[0], "RGB").save(root / "face0.png")
    PIL.Image.fromarray(imgs[0], "RGB").save(root / "progressive.jpg", format="JPEG", progressive=True)
    return root, paths


def _with(hf, decoder, call):
    if decoder is None:
        if hasattr(hf.args, "image_decoder"):
            del hf.args.image_decoder
    else:
        hf.args.image_decoder = decoder
    try:
        return call()
    finally:
        hf.args.image_decoder = "pil"


def test_swap_from_jpeg_paths(hf, faces):
    root, paths = faces
    ref = _with(hf, "pil", lambda: hf.swap(*paths, seed=7))
    got = _with(hf, "device", lambda: hf.swap(*paths, seed=7))
    assert got.shape == (3, 1024, 1024) and torch.equal(got, ref)
    assert torch.equal(_with(hf, None, lambda: hf.swap(*paths, seed=7)), ref)  # without args.image_decoder nothing changes
    assert torch.equal(_with(hf, "device", lambda: hf.swap(str(paths[0]), paths[1], paths[1], seed=7)),
                       _with(hf, "pil", lambda: hf.swap(str(paths[0]), paths[1], paths[1], seed=7)))  # a repeated path
    # a PNG path still goes through PIL; a tensor is taken as it is
    mixed = (root / "face0.png", paths[1], torch.from_numpy(np.asarray(PIL.Image.open(paths[2]).convert("RGB")).transpose(2, 0, 1).copy()))
    assert torch.equal(_with(hf, "device", lambda: hf.swap(*mixed, seed=7)), _with(hf, "pil", lambda: hf.swap(*mixed, seed=7)))
    with pytest.raises(ValueError, match="progressive"):
        _with(hf, "device", lambda: hf.swap(root / "progressive.jpg", paths[1], paths[2], seed=7))
    assert _with(hf, "pil", lambda: hf.swap(root / "progressive.jpg", paths[1], paths[2], seed=7)).shape == (3, 1024, 1024)


def test_swap_batch_from_jpeg_paths(hf, faces):
    _, paths = faces
    triples = [tuple(paths), (paths[1], paths[2], paths[0])]
    ref = _with(hf, "pil", lambda: hf.swap_batch(triples, seed=7))
    got = _with(hf, "device", lambda: hf.swap_batch(triples, seed=7))
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, ref))


def test_swap_align_from_a_jpeg_photograph(hf, tmp_path):
    from tests import align_ref as AR

    photo, lm = AR.image(300, 200, 41), AR.landmarks(150, 95, 40, 7.0)
    assert photo.shape == (200, 300, 3)
    path = tmp_path / "photo.jpg"
    PIL.Image.fromarray(photo, "RGB").save(path, format="JPEG", quality=92)
    ref = _with(hf, "pil", lambda: hf.swap(path, path, path, align=True, landmarks=[lm, lm, lm], seed=7))
    got = _with(hf, "device", lambda: hf.swap(path, path, path, align=True, landmarks=[lm, lm, lm], seed=7))
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, ref))


def test_parser_has_image_decoder():
    from hairfastgan_amd.hair_swap import get_parser

    assert get_parser().parse_args([]).image_decoder == "pil"
    assert get_parser().parse_args(["--image_decoder", "device"]).image_decoder == "device"
    with pytest.raises(SystemExit):
        get_parser().parse_args(["--image_decoder", "gpu"])
