"""CPU tests of the identity restatements (tests/identity_ref.py), of what tests/identity_checks.py records about them, and of
the host surface of hairfastgan_amd.identity that needs no kernel: the restated network equals the reference's own class on
one state dict, the fp32 errors the device thresholds are built on are measured again and must not exceed the recorded
figures, the seeded weights and images discriminate, the state dict has the reference class's keys, and the weights finder
names what it looked for."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from hairfastgan_amd import identity as ID
from tests import identity_checks as K
from tests import identity_ref as R

REFERENCE = os.path.join(os.environ.get("HAIRFAST_REFERENCE", "/root/reference"), "models", "encoder4editing")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_se50_state_keys.json")


def _golden_keys():
    with open(GOLDEN) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_restatement_equals_the_reference_class():
    """One state dict in the reference's model_irse.Backbone and in the restatement: equal fp64 embeddings to 1e-12, and the
    committed key fixture is what the reference class has."""
    sys.path.insert(0, REFERENCE)
    try:
        from models.encoders.model_irse import Backbone
    finally:
        sys.path.remove(REFERENCE)
    ref = Backbone(112, 50, "ir_se", drop_ratio=0.6)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == _golden_keys()
    ref.load_state_dict(K.state("full"))
    ref = ref.double().eval()
    x = torch.nn.functional.adaptive_avg_pool2d(R.discriminating_images()[:2].double()[:, :, 35:223, 32:220], (112, 112))
    with torch.no_grad():
        want = ref(x)
    got = K.truth("full")[0][:2]
    assert float((got - want).abs().max()) <= 1e-12


def test_state_dict_has_the_reference_keys():
    keys = _golden_keys()
    assert len(keys) == 397
    model = ID.Backbone()
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == keys
    assert {k: tuple(v.shape) for k, v in R.Backbone().state_dict().items()} == keys
    model._plan = {"stale": True}
    model.load_state_dict(K.state("full"))
    assert model._plan is None and not any(p.requires_grad for p in model.parameters())
    assert all(torch.equal(v, K.state("full")[k]) for k, v in model.state_dict().items())
    assert ID.Backbone(224).output_layer[3].in_features == 512 * 14 * 14
    assert "output_layer.4.weight" not in ID.Backbone(affine=False).state_dict()
    small = ID.Backbone(K.SMALL_SIZE, units=list(K.SMALL_UNITS))
    assert small.output_layer[3].in_features == 128 * 7 * 7
    small.load_state_dict(K.state("small"))


def test_refusals():
    K.check_refusals()


def test_restated_crop_and_pool_is_torchs():
    """The fp64 restatement against torch.nn.AdaptiveAvgPool2d on the cropped copy; the ordered fp32 form stays within the
    kernel's bound of it."""
    for name, n, c, h, w, crop, oh, ow, _ in K.POOL_CASES:
        x = np.random.default_rng(5).standard_normal((n, c, h, w)).astype(np.float32)
        y0, x0, ch, cw = crop
        want = torch.nn.AdaptiveAvgPool2d((oh, ow))(torch.from_numpy(x).double()[:, :, y0:y0 + ch, x0:x0 + cw]).numpy()
        got, count, big = R.crop_avgpool(x, *crop, oh, ow)
        assert float(np.abs(got - want).max()) <= 1e-14, name
        assert (np.abs(R.crop_avgpool_ordered(x, *crop, oh, ow).astype(np.float64) - got) <= (count + 2) * R.U32 * big).all(), name
    assert int(R.crop_avgpool(x, 2, 1, 9, 11, 1, 1)[1].max()) == 99


@pytest.mark.parametrize("kind", ["tiny", "small", "full"])
def test_fp32_error_is_within_the_recorded_one(kind):
    comp, sim = K.fp32_errors(kind)
    print(kind, comp, sim)
    assert comp <= K.EMB_MEASURED[kind] and sim <= K.SIM_MEASURED[kind], (kind, comp, sim)
    assert comp >= K.EMB_MEASURED[kind] / 8 and sim >= K.SIM_MEASURED[kind] / 8  # the record is not a loose one either


def test_inputs_discriminate():
    K.check_full_conditions()
    want, shortcut = K.truth("small")
    assert float((want[0] * want[1]).sum()) <= 0.9 and float((want * shortcut).sum(1).abs().max()) <= 0.9


def test_head_fold_equals_the_three_layers():
    """BatchNorm2d, Linear and BatchNorm1d as one Linear: the folded weights against the modules in fp64."""
    for affine in (True, False):
        sd = R.discriminating_state(list(K.SMALL_UNITS), K.SMALL_SIZE, 3, affine)
        model = ID.Backbone(K.SMALL_SIZE, units=list(K.SMALL_UNITS), affine=affine)
        model.load_state_dict(sd)
        w, b = model._fold_head()
        x = torch.randn(3, 128, 7, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        ref = R.network(sd, list(K.SMALL_UNITS), K.SMALL_SIZE, affine=affine).output_layer(x).detach()
        got = x.reshape(3, -1) @ w.double().T + b.double()
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        assert float((ref - ref.mean()).abs().max()) > 0.1


def test_weights_finder(tmp_path):
    from hairfastgan_amd import checkpoints

    with pytest.raises(FileNotFoundError) as e:
        checkpoints.arcface(root=str(tmp_path))
    assert "ArcFace/ir_se50.pth" in str(e.value) and "model_ir_se50.pth" in str(e.value)
    sd = K.state("small")
    os.makedirs(tmp_path / "pretrained_models")
    torch.save(sd, tmp_path / "pretrained_models" / "model_ir_se50.pth")  # e4e's place is tried second
    found = checkpoints.arcface(root=str(tmp_path))
    assert set(found) == set(sd) and all(torch.equal(found[k], sd[k]) for k in sd)
    os.makedirs(tmp_path / "pretrained_models" / "ArcFace")
    torch.save({"only": torch.zeros(1)}, tmp_path / "pretrained_models" / "ArcFace" / "ir_se50.pth")
    assert set(checkpoints.arcface(root=str(tmp_path))) == {"only"}
    assert set(checkpoints.arcface(path=str(tmp_path / "pretrained_models" / "model_ir_se50.pth"))) == set(sd)
