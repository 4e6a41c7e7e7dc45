"""CPU tests of the FID Inception-v3 restatement (tests/inception_ref.py) and of what needs no kernel: the conditions the
network checks put on their inputs, the recorded fp32 yardstick, the module tree's state dict and the weights finder."""
import pytest
import torch

from tests import inception_checks as K
from tests import inception_ref as R


def test_planes():
    """The planes the definition states: 299^2 -> 149, 147, 147, 73, 73, 71, 35, 17, 8; 75^2 -> 37, 35, 35, 17, 17, 15, 7, 3, 1."""
    from hairfastgan_amd import _marshal as M

    for size, want in ((299, [149, 147, 147, 73, 73, 71, 35, 17, 8]), (75, [37, 35, 35, 17, 17, 15, 7, 3, 1])):
        p = M.conv_out_size(size, 3, 2, 0)
        got = [p, p - 2, p - 2]
        got.append((got[-1] - 3) // 2 + 1)
        got += [got[-1], got[-1] - 2]
        for _ in range(3):
            got.append((got[-1] - 3) // 2 + 1)
        assert got == want
    t = R.forward(R.discriminating_state(8), R.byte_images(75), torch.float64, 8, False)
    assert [tuple(t[k].shape) for k in R.TAPS] == [(3, 8), (3, 24), (3, 96), (3, 256)]


@pytest.mark.parametrize("kind", ["tiny", "full"])
def test_conditions(kind):
    K.check_conditions(kind)


@pytest.mark.parametrize("kind", ["tiny", "full"])
def test_fp32_yardstick(kind):
    K.check_fp32_yardstick(kind)


def test_resize_restatement():
    """299 -> 299 is the identity, 598 -> 299 takes every second pixel, and the half-pixel look-alike is another function."""
    x = R.byte_images(64)[:1].double()
    assert torch.equal(R.resize_tf1(x, 64, 64), x)
    big = torch.arange(598 * 598, dtype=torch.float64).reshape(1, 1, 598, 598) % 251
    assert torch.equal(R.resize_tf1(big, 299, 299), big[:, :, ::2, ::2])
    assert not torch.equal(R.resize_tf1(x, 299, 299), R.resize_tf1(x, 299, 299, half_pixel=True))
    assert float((R.resize_tf1(x.float(), 299, 299).double() - R.resize_tf1(x, 299, 299)).abs().max()) <= K.RESIZE_BOUND


def test_state_dict():
    K.check_state_dict()


def test_constructor_refusals():
    from hairfastgan_amd import metrics as MT
    from hairfastgan_amd.inception import InceptionV3

    for bad in (0, 100, 1008, "2048", True):
        with pytest.raises(ValueError):
            InceptionV3(bad, channel_div=8)
    with pytest.raises(NotImplementedError, match="Inception"):
        MT.FrechetDistance(2048)


def test_weights_finder(tmp_path, monkeypatch):
    from hairfastgan_amd import checkpoints as C
    from hairfastgan_amd.inception import InceptionV3

    monkeypatch.delenv("HAIRFAST_INCEPTION_WEIGHTS", raising=False)
    monkeypatch.setattr(C, "TORCH_HUB_CACHE", str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        C.inception_fid()
    sd = R.discriminating_state(8)
    sd["fc.bias"] = torch.zeros(1008)
    (tmp_path / "hub").mkdir()
    torch.save(sd, tmp_path / "hub" / C.INCEPTION_FID_FILE)
    assert set(C.inception_fid()) == set(sd)
    torch.save(sd, tmp_path / "elsewhere.pth")
    monkeypatch.setenv("HAIRFAST_INCEPTION_WEIGHTS", str(tmp_path / "elsewhere.pth"))
    monkeypatch.setattr(C, "TORCH_HUB_CACHE", str(tmp_path / "none"))
    net = InceptionV3(2048, weights=C.inception_fid(), channel_div=8)
    assert torch.equal(net.Mixed_7c.branch_pool.bn.running_var, sd["Mixed_7c.branch_pool.bn.running_var"])
    assert set(C.inception_fid(path=str(tmp_path / "elsewhere.pth"))) == set(sd)
