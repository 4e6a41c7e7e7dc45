"""hipsim tests of the identity-similarity kernels (csrc/identity.h) and their host mirror (hairfastgan_amd.identity): the
product's kernel sources interpreted on the CPU against the torch / numpy restatements (tests/identity_ref.py) by the checks of
tests/identity_checks.py.  The network is two units at 28^2 (planes 28, 14 and 7) here; IR-SE50 at 112^2 runs on the GPU."""

import pytest
import torch

from tests import identity_checks as K
from tests.metric_common import patch_host_modules

CPU = torch.device("cpu")


@pytest.fixture()
def sim_fused(simlib, monkeypatch):
    """The network's layers go through encoders._fused and encoders.e4e, which ask their own lib() / stream()."""
    import hairfastgan_amd.encoders  # noqa: F401

    patch_host_modules(monkeypatch, simlib, ["hairfastgan_amd.encoders._fused", "hairfastgan_amd.encoders.e4e"])
    prev = simlib.hf_set_batch_invariant(1)  # the product's default (_runtime.lib() hands it to the library)
    yield simlib
    simlib.hf_set_batch_invariant(prev)


@pytest.mark.parametrize("case", K.POOL_CASES, ids=[c[0] for c in K.POOL_CASES])
def test_crop_avgpool(simlib, case):
    K.check_crop_avgpool(simlib, None, CPU, *case)


def test_crop_avgpool_refusals(simlib):
    K.check_crop_avgpool_refusals(simlib, None, CPU)


@pytest.mark.parametrize("d", K.NORM_DIMS)
def test_normalize(simlib, d):
    K.check_normalize(simlib, None, CPU, d)


def test_similarity(simlib):
    K.check_similarity(simlib, None, CPU)


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_network(sim_fused, mode):
    from hairfastgan_amd import _runtime

    with _runtime.conv_precision_scope(mode):
        K.check_network(sim_fused, None, CPU, "small", every_row=False)


def test_forward(sim_fused):
    K.check_forward(sim_fused, None, CPU, "tiny")


def test_cli(sim_fused, tmp_path):
    K.check_cli(sim_fused, None, CPU, str(tmp_path))
