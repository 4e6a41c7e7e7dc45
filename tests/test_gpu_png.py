"""GPU tests (-m gpu) of the device PNG encoder (csrc/png.h) through the C ABI and the host layer (image_utils.encode_png,
save_image(encoder="device"), save_images, SaveAllRecorder(png_encoder="device")): every file decoded again by the checks'
own parser and by PIL (tests/png_checks.py has the decoders, the inputs and the rules)."""
import numpy as np
import pytest
import torch

from tests import png_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", K.TINY)
def test_tiny_and_ragged(shape):
    K.check_tiny(*gpu_ctx(), shape)


def test_heights_around_a_segment():
    K.check_heights(*gpu_ctx())


def test_input_base_offset_by_one_byte():
    K.check_offset_base(*gpu_ctx())


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_filter_modes(mode):
    K.check_filter(*gpu_ctx(), mode)


def test_runs():
    K.check_runs(*gpu_ctx())


def test_incompressible_takes_stored_blocks():
    K.check_incompressible(*gpu_ctx())


def test_deep_code_is_length_limited():
    K.check_deep_code(*gpu_ctx())


def test_batch_invariant_and_deterministic():
    K.check_batch_invariance(*gpu_ctx())


def test_size_conditions():
    K.check_sizes(*gpu_ctx())


def test_invalid_arguments():
    K.check_invalid(*gpu_ctx())


def test_marshalled_call():
    K.check_marshalled(*gpu_ctx())


def test_encode_png_shapes():
    """Every input form of encode_png; a single image comes back as bytes."""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    rgb = np.stack([K.smooth((9, 21, 3), k) for k in range(2)])
    grey = rgb[..., 0]
    t = torch.from_numpy
    for arg, expect in [(t(rgb), list(rgb)), (t(grey[..., None].copy()), list(grey[..., None])), (t(grey.copy()), list(grey[..., None])),
                        (t(rgb[0]), rgb[0]), (t(grey[0].copy()), grey[0][..., None])]:
        got = IU.encode_png(arg.to(dev))
        if isinstance(expect, list):
            assert isinstance(got, list) and len(got) == len(expect)
            for data, img in zip(got, expect):
                assert np.array_equal(K.decode(data)[0], img)
        else:
            assert isinstance(got, bytes) and np.array_equal(K.decode(got)[0], expect)
    for name, mode in IU.PNG_FILTERS.items():
        data = IU.encode_png(t(rgb[0]).to(dev), filter=name)
        pixels, rows = K.decode(data)
        assert np.array_equal(pixels, rgb[0]) and (mode == 3 or (rows == mode).all())
    with pytest.raises(ValueError):
        IU.encode_png(t(rgb[0]).to(dev), filter="paeth")
    with pytest.raises(TypeError):
        IU.encode_png(t(rgb[0]).to(dev).float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IU.encode_png(t(rgb))


def test_save_image_and_save_images(tmp_path):
    """save_image(encoder="device") and save_images on floats: the files decode to to_bytes(...)."""
    from hairfastgan_amd import image_utils as IU

    _, _, dev = gpu_ctx()
    rng = np.random.default_rng(0)
    one = torch.from_numpy(rng.random((1, 3, 64, 96), dtype=np.float32)).to(dev)
    many = torch.from_numpy(rng.random((3, 3, 64, 96), dtype=np.float32) * 2 - 1).to(dev)
    IU.save_image(one, tmp_path / "one.png", encoder="device")
    IU.save_image(one[0], tmp_path / "one_pil.png")
    ref = IU.to_bytes(one, (0, 1), "nearest", "hwc").cpu().numpy()[0]
    for name in ("one.png", "one_pil.png"):
        data = (tmp_path / name).read_bytes()
        assert np.array_equal(K.decode_pil(data)[0], ref), name
    assert np.array_equal(K.decode((tmp_path / "one.png").read_bytes())[0], ref)
    paths = [tmp_path / f"many_{k}.png" for k in range(3)]
    IU.save_images(many, paths, value_range=(-1, 1), rounding="floor")
    ref = IU.to_bytes(many, (-1, 1), "floor", "hwc").cpu().numpy()
    for k, p in enumerate(paths):
        assert np.array_equal(K.decode(p.read_bytes())[0], ref[k]) and np.array_equal(K.decode_pil(p.read_bytes())[0], ref[k])
    IU.save_images(many, [tmp_path / f"pil_{k}.png" for k in range(3)], value_range=(-1, 1), rounding="floor", encoder="pil")
    for k in range(3):
        assert np.array_equal(K.decode_pil((tmp_path / f"pil_{k}.png").read_bytes())[0], ref[k])
    with pytest.raises(TypeError):
        IU.save_image(one, tmp_path / "no.png", encoder="device", compress_level=1)
    with pytest.raises(ValueError):
        IU.save_image(one, tmp_path / "no.png", encoder="zlib")
    with pytest.raises(ValueError):
        IU.save_images(many, paths[:2])
    assert not (tmp_path / "no.png").exists()


def test_save_all_recorder_device_encoder(tmp_path):
    """A recorder fed blending(...) and shape(...) only (render(None): nothing was embedded, no generator runs): the device
    encoder writes the same file set as the PIL one, and every file decodes to the same pixels."""
    from hairfastgan_amd.hair_swap import SaveAllRecorder

    _, _, dev = gpu_ctx()
    g = torch.Generator().manual_seed(0)
    I_blend = (torch.rand(1, 3, 64, 96, generator=g) * 2 - 1).to(dev)
    I_final = (torch.rand(1, 3, 64, 96, generator=g) * 2 - 1).to(dev)
    S = torch.rand(1, 18, 512, generator=g).to(dev)
    F_ = torch.rand(1, 8, 4, 4, generator=g).to(dev)
    masks = {n: torch.randint(0, 19, (1, 1, 32, 48), generator=g).to(dev) for n in ("face", "shape")}
    masks["shape"][0, 0, :4, :5] = 255  # the unknown label: white
    target = torch.randint(0, 19, (1, 1, 32, 48), generator=g).to(dev)
    written = {}
    for enc in ("pil", "device"):
        rec = SaveAllRecorder(tmp_path / enc, png_encoder=enc)
        rec.begin(["exp"])
        rec.shape([("face", "shape")], {n: {"mask": m} for n, m in masks.items()}, [target])
        rec.blending([("face", "shape", "color")], S, I_blend, S, F_, I_final)
        rec.render(None)
        written[enc] = sorted(str(p.relative_to(tmp_path / enc)) for p in rec.write())
    assert written["pil"] == written["device"] and sum(n.endswith(".png") for n in written["pil"]) == 6
    for name in written["pil"]:
        a, b = tmp_path / "pil" / name, tmp_path / "device" / name
        if name.endswith(".png"):
            pa, pb = K.decode_pil(a.read_bytes()), K.decode_pil(b.read_bytes())
            assert pa[1] == pb[1] == "RGB" and pa[2] == pb[2] and np.array_equal(pa[0], pb[0]), name
            assert np.array_equal(K.decode(b.read_bytes())[0], pa[0]), name
        else:
            with np.load(a) as za, np.load(b) as zb:
                assert sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files)
    with pytest.raises(ValueError):
        SaveAllRecorder(tmp_path, png_encoder="zlib")
