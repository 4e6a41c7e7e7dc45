"""hipsim tests of the LPIPS and L2 / PSNR kernels (csrc/lpips.h) and their host mirror (hairfastgan_amd.lpips): the product's
kernel sources interpreted on the CPU against the torch / numpy restatements (tests/lpips_ref.py) by the checks of
tests/lpips_checks.py."""

import pytest
import torch

from tests import lpips_checks as K
from tests.metric_common import patch_host_modules

CPU = torch.device("cpu")


@pytest.fixture()
def sim_fused(simlib, monkeypatch):
    """The towers' 3x3 and 5x5 layers go through encoders._fused, which asks its own lib() / stream()."""
    import hairfastgan_amd.encoders  # noqa: F401

    patch_host_modules(monkeypatch, simlib, ["hairfastgan_amd.encoders._fused"])
    return simlib


@pytest.mark.parametrize("k,stride,h,w", K.POOL_CASES)
def test_maxpool(simlib, k, stride, h, w):
    K.check_maxpool(simlib, None, CPU, k, stride, h, w)


@pytest.mark.parametrize("w,h,ow,oh", K.RESIZE_CASES)
def test_resize_bilinear(simlib, w, h, ow, oh):
    K.check_resize_bilinear(simlib, None, CPU, w, h, ow, oh)


@pytest.mark.parametrize("variant", K.CONV_VARIANTS)
@pytest.mark.parametrize("case", K.CONV_CASES)
def test_conv_direct(simlib, case, variant):
    K.check_conv_direct(simlib, None, CPU, *case, variant)


def test_conv_direct_refusals(simlib):
    K.check_conv_direct_refusals(simlib, None, CPU)


@pytest.mark.parametrize("family", K.LAYER_FAMILIES)
@pytest.mark.parametrize("shape", K.LAYER_SHAPES)
def test_layer(simlib, shape, family):
    K.check_layer(simlib, None, CPU, shape, family)


@pytest.mark.parametrize("shape", K.LAYER_SHAPES)
def test_layer_conditions(simlib, shape):
    K.check_layer_conditions(simlib, None, CPU, shape)


def test_layer_refusals(simlib):
    K.check_layer_refusals(simlib, None, CPU)


@pytest.mark.parametrize("net_type,size", K.LPIPS_SIM)
def test_lpips(sim_fused, net_type, size):
    K.check_lpips(sim_fused, None, CPU, net_type, size, whole_batch=(net_type, size) == K.LPIPS_SIM[0],
                  shared_x=(net_type, size) == ("vgg", 48))  # 2.7 GMAC per VGG pass at 48^2: minutes in the interpreter


def test_psnr(simlib):
    K.check_psnr(simlib, None, CPU)


def test_cli(sim_fused, tmp_path):
    K.check_cli(sim_fused, None, CPU, str(tmp_path))
