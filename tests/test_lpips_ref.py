"""CPU tests of the LPIPS restatements (tests/lpips_ref.py), of what tests/lpips_checks.py records about them, and of the host
surface of hairfastgan_amd.lpips that needs no kernel: the fp32 errors the device thresholds are built on are measured again
and must not exceed the recorded figures, the seeded towers are alive at every tap, the state dict has the reference module's
keys and `load_pretrained` renames the published ones."""
import pytest
import torch

from hairfastgan_amd import lpips as LP
from tests import lpips_checks as K
from tests import lpips_ref as R


@pytest.mark.parametrize("family", K.LAYER_FAMILIES)
def test_layer_fp32_error_is_within_the_recorded_one(family):
    worst = max(K.layer_fp32_error(shape, family) for shape in K.LAYER_SHAPES)
    print(family, worst)
    assert worst <= K.LAYER_MEASURED[family], (family, worst)


@pytest.mark.parametrize("net_type", ["alex", "vgg"])
def test_lpips_fp32_error_is_within_the_recorded_one(net_type):
    for noise in K.NOISES:
        worst = max(K.lpips_fp32_error(n, size, noise) for n, size in K.LPIPS_SIM + K.LPIPS_GPU if n == net_type)
        print(net_type, noise, worst)
        assert worst <= K.LPIPS_MEASURED[(net_type, noise)], (net_type, noise, worst)


def test_layer_floor_covers_the_fp32_evaluation():
    """The floor is a bound of any fp32 evaluation: torch's own stays below it."""
    for family in K.LAYER_FAMILIES:
        for shape in K.LAYER_SHAPES:
            fx, fy, w = K.layer_case(shape, family)
            err = (R.lpips_layer(fx, fy, w, torch.float32).double() - K.layer_truth(shape, family)[0]).abs()
            assert bool((err <= K.layer_truth(shape, family)[1]).all()), (family, shape)


def test_layer_restatement_equals_the_five_pass_form():
    """normalise x 2, subtract, square, 1x1 conv, mean - with torch's own conv2d."""
    fx, fy, w = K.layer_case((3, 64, 15, 15), "independent")
    fx, fy = fx.double(), fy.double()
    nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    want = torch.nn.functional.conv2d((nx - ny) ** 2, w.double().reshape(1, -1, 1, 1)).mean((2, 3)).reshape(-1)
    assert float((R.lpips_layer(fx, fy, w) - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("net_type,size", K.LPIPS_SIM + K.LPIPS_GPU)
def test_towers_are_alive(net_type, size):
    """40 - 60 % of the activations are non-zero at every tap: a dead tower would pass every comparison."""
    x = K.lpips_images(net_type, size, K.NOISES[0])[0]
    for j, a in enumerate(R.tower(R.random_weights(net_type), net_type, x)):
        alive = float((a > 0).double().mean())
        assert 0.40 <= alive <= 0.60, (net_type, size, j, alive)


@pytest.mark.parametrize("net_type", ["alex", "vgg"])
def test_state_dict_round_trip_and_load_pretrained(net_type):
    sd = R.random_weights(net_type)
    model = LP.LPIPS(net_type)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    model.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    assert not any(p.requires_grad for p in model.parameters())
    features = {"features." + k[len("net.layers."):]: v for k, v in sd.items() if k.startswith("net.layers.")}
    features["classifier.1.weight"] = torch.zeros(3, 3)  # torchvision's file carries the classifier too
    lin = {f"lin{k.split('.')[1]}.model.1.weight": v for k, v in sd.items() if k.startswith("lin.")}
    other = LP.LPIPS(net_type)
    other._plan = {"stale": True}
    other.load_pretrained(features, lin)
    assert other._plan is None
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    taps = {"alex": [64, 192, 384, 256, 256], "vgg": [64, 128, 256, 512, 512]}[net_type]
    assert [m[1].weight.shape[1] for m in other.lin] == taps


def test_unsupported_towers_raise():
    with pytest.raises(NotImplementedError):
        LP.LPIPS("squeeze")
    with pytest.raises(NotImplementedError):
        LP.LPIPS("resnet")
    with pytest.raises(ValueError):
        LP.LPIPS("alex", version="0.0")


def test_weights_finder_names_the_missing_file(monkeypatch, tmp_path):
    from hairfastgan_amd import checkpoints

    monkeypatch.setenv("HAIRFAST_LPIPS_TOWER", str(tmp_path / "alexnet.pth"))
    with pytest.raises(FileNotFoundError, match="alexnet.pth"):
        checkpoints.lpips_weights("alex")
    sd = R.random_weights("alex")
    torch.save({"features." + k[len("net.layers."):]: v for k, v in sd.items() if k.startswith("net.layers.")}, tmp_path / "alexnet.pth")
    monkeypatch.setenv("HAIRFAST_LPIPS_LIN", str(tmp_path / "alex.pth"))
    with pytest.raises(FileNotFoundError, match="alex.pth"):
        checkpoints.lpips_weights("alex")
    torch.save({f"lin{k.split('.')[1]}.model.1.weight": v for k, v in sd.items() if k.startswith("lin.")}, tmp_path / "alex.pth")
    model = LP.LPIPS("alex")
    model.load_pretrained(*checkpoints.lpips_weights("alex"))
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    with pytest.raises(NotImplementedError):
        checkpoints.lpips_weights("squeeze")


def test_bilinear_tables():
    """Triangle filter: an upscale by 4 has at most 3 taps, a reduction by 4 spreads over 9; every row sums to 2^22 +- taps."""
    from hairfastgan_amd import face_align as FA

    for a, b, ksize in ((64, 256, 3), (1024, 256, 9), (53, 16, 9)):
        bounds, kk = FA.bilinear_coeffs(a, b)
        assert bounds.shape == (b, 2) and kk.shape == (b, ksize)
        assert abs(kk.sum(1) - (1 << 22)).max() <= ksize and (kk >= 0).all()
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= a).all()
