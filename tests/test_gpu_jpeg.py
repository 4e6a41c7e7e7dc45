"""GPU tests (-m gpu) of the device JPEG encoder (csrc/jpeg.h) through the C ABI and the host layer (image_utils.encode_jpeg,
save_image / save_images with format="jpeg"): every file compared byte for byte with the numpy restatement of libjpeg's
pipeline that tests/test_jpeg_ref.py pins to Pillow, and with Pillow itself (tests/jpeg_checks.py has the inputs and the
rules)."""
import io

import numpy as np
import PIL.Image
import pytest
import torch

from tests import jpeg_checks as K
from tests import jpeg_ref as R
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", K.MODES, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_ragged(shape, mode):
    K.check_tiny(*gpu_ctx(), shape, mode)


def test_restart_index_wraps():
    K.check_restart_wrap(*gpu_ctx())


def test_chunk_boundary():
    K.check_chunk_boundary(*gpu_ctx())


def test_symbol_coverage():
    K.check_symbols(*gpu_ctx())


def test_bound_holds_for_noise():
    K.check_bound(*gpu_ctx())


def test_batch_invariant_and_deterministic():
    K.check_batch_invariance(*gpu_ctx())


def test_invalid_arguments():
    K.check_invalid(*gpu_ctx())


def test_marshalled_call():
    K.check_marshalled(*gpu_ctx())


def test_encode_jpeg_shapes():
    """Every input form of encode_jpeg; a single image comes back as bytes; the arguments reach the file."""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    rgb = np.stack([K.smooth((19, 21, 3), k) for k in range(2)])
    grey = rgb[..., 0]
    t = torch.from_numpy
    for arg, expect in [(t(rgb), list(rgb)), (t(grey[..., None].copy()), list(grey[..., None])), (t(grey.copy()), list(grey[..., None])),
                        (t(rgb[0]), rgb[0]), (t(grey[0].copy()), grey[0][..., None])]:
        got = IU.encode_jpeg(arg.to(dev))
        if isinstance(expect, list):
            assert isinstance(got, list) and len(got) == len(expect)
            assert got == [R.pil_encode(img, 75, 2) for img in expect]
        else:
            assert isinstance(got, bytes) and got == R.pil_encode(expect, 75, 2)
    for name, sub in IU.JPEG_SUBSAMPLINGS.items():
        for q in (30, 92):
            assert IU.encode_jpeg(t(rgb[0]).to(dev), quality=q, subsampling=name) == R.pil_encode(rgb[0], q, sub)
    assert IU.encode_jpeg(t(rgb[0].transpose(1, 0, 2)).to(dev).permute(1, 0, 2)) == R.pil_encode(rgb[0], 75, 2)  # a strided view
    for bad in ({"quality": 0}, {"quality": 101}, {"quality": 75.0}, {"subsampling": "4:1:1"}, {"subsampling": 2}):
        with pytest.raises(ValueError):
            IU.encode_jpeg(t(rgb[0]).to(dev), **bad)
    with pytest.raises(ValueError):
        IU.encode_jpeg(t(rgb).to(dev)[..., :2])
    with pytest.raises(TypeError):
        IU.encode_jpeg(t(rgb[0]).to(dev).float())
    with pytest.raises(TypeError):
        IU.encode_jpeg(rgb[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.encode_jpeg(t(rgb))


def _pil_jpeg(u8, quality, subsampling):
    buf = io.BytesIO()
    PIL.Image.fromarray(u8, "RGB").save(buf, format="JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)
    return buf.getvalue()


def test_save_image_and_save_images_jpeg(tmp_path):
    """format="jpeg": the device encoder, the PIL encoder and Pillow's own save of to_bytes(...) write one and the same file;
    format=None still writes what it wrote: PNG bytes that decode to to_bytes(...)."""
    from hairfastgan_amd import image_utils as IU
    from tests import png_checks as PK

    _, _, dev = gpu_ctx()
    rng = np.random.default_rng(0)
    one = torch.from_numpy(rng.random((1, 3, 40, 72), dtype=np.float32)).to(dev)
    many = torch.from_numpy(rng.random((3, 3, 40, 72), dtype=np.float32) * 2 - 1).to(dev)
    ref = IU.to_bytes(one, (0, 1), "nearest", "hwc").cpu().numpy()[0]
    IU.save_image(one, tmp_path / "dev.jpg", encoder="device", format="jpeg")
    IU.save_image(one[0], tmp_path / "pil.jpg", format="jpeg")
    IU.save_image(one, tmp_path / "dev90.jpg", encoder="device", format="jpeg", quality=90, subsampling="4:4:4")
    IU.save_image(one, tmp_path / "pil90.jpg", encoder="pil", format="jpeg", quality=90, subsampling="4:4:4")
    assert (tmp_path / "dev.jpg").read_bytes() == (tmp_path / "pil.jpg").read_bytes() == _pil_jpeg(ref, 75, "4:2:0")
    assert (tmp_path / "dev90.jpg").read_bytes() == (tmp_path / "pil90.jpg").read_bytes() == _pil_jpeg(ref, 90, "4:4:4")
    refs = IU.to_bytes(many, (-1, 1), "floor", "hwc").cpu().numpy()
    for enc in IU.ENCODERS:
        paths = [tmp_path / f"{enc}_{k}.jpg" for k in range(3)]
        IU.save_images(many, paths, value_range=(-1, 1), rounding="floor", encoder=enc, format="jpeg", quality=60, subsampling="4:2:2")
        for k, p in enumerate(paths):
            assert p.read_bytes() == _pil_jpeg(refs[k], 60, "4:2:2"), (enc, k)
    # format=None: as before - the device encoder writes PNG whatever the suffix, PIL chooses by the suffix
    IU.save_image(one, tmp_path / "named.jpg", encoder="device")
    IU.save_images(many, [tmp_path / f"plain_{k}.png" for k in range(3)], value_range=(-1, 1), rounding="floor")
    IU.save_image(one, tmp_path / "suffix.png")
    IU.save_image(one, tmp_path / "suffix.jpg")
    assert np.array_equal(PK.decode((tmp_path / "named.jpg").read_bytes())[0], ref)
    assert np.array_equal(PK.decode_pil((tmp_path / "suffix.png").read_bytes())[0], ref)
    for k in range(3):
        assert np.array_equal(PK.decode((tmp_path / f"plain_{k}.png").read_bytes())[0], refs[k])
    with PIL.Image.open(tmp_path / "suffix.jpg") as im:
        assert im.format == "JPEG"
    before = sorted(p.name for p in tmp_path.iterdir())
    for exc, kw in [(TypeError, {"quality": 90}), (TypeError, {"subsampling": "4:4:4"}), (ValueError, {"format": "webp"}),
                    (ValueError, {"format": "jpeg", "quality": 0}), (ValueError, {"format": "jpeg", "subsampling": "4:1:1"})]:
        for enc in IU.ENCODERS:
            with pytest.raises(exc):
                IU.save_image(one, tmp_path / "no.jpg", encoder=enc, **kw)
            with pytest.raises(exc):
                IU.save_images(many, [tmp_path / f"no_{k}.jpg" for k in range(3)], encoder=enc, **kw)
    with pytest.raises(TypeError):
        IU.save_image(one, tmp_path / "no.jpg", encoder="device", format="jpeg", optimize=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == before


def test_encode_jpeg_of_paste_back():
    """A pasted-back photograph of 96 x 128 to JPEG on the device: the uint8 form through its [H,W,3] view, the float form
    through save_image's bytes - both the file PIL writes of the same array, decoding to the same pixels."""
    from hairfastgan_amd import face_align as FA
    from hairfastgan_amd import image_utils as IU
    from tests import align_ref as AR

    _, _, dev = gpu_ctx()
    photo, lm = AR.image(128, 96, 41), AR.landmarks(64, 44, 16, 7.0)
    result = np.random.default_rng(5).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    pasted = FA.paste_back(photo, PIL.Image.fromarray(result, "RGB"), lm, output_size=64, return_tensors=False, device=dev)
    assert pasted.dtype == torch.uint8 and tuple(pasted.shape) == (3, 96, 128)
    hwc = pasted.permute(1, 2, 0)
    data = IU.encode_jpeg(hwc, quality=90)
    ref = _pil_jpeg(np.ascontiguousarray(hwc.cpu().numpy()), 90, "4:2:0")
    assert data == ref
    got, mode, size, fmt = K.decode_pil(data)
    assert (mode, size, fmt) == ("RGB", (128, 96), "JPEG") and np.array_equal(got, K.decode_pil(ref)[0])
    as_float = FA.paste_back(photo, PIL.Image.fromarray(result, "RGB"), lm, output_size=64, device=dev)
    assert IU.encode_jpeg(IU.to_bytes(as_float, (0, 1), "nearest"), quality=90) == ref  # byte / 255 quantises back to the byte
