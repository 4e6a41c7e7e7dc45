"""hipsim tests of the SSIM kernel (csrc/ssim.h) and its host mirror (hairfastgan_amd.ssim): the product's kernel sources
interpreted on the CPU against the fp64 restatements (tests/ssim_ref.py) by the checks of tests/ssim_checks.py."""

import pytest
import torch

from tests import ssim_checks as K
from tests.metric_common import patch_host_modules

CPU = torch.device("cpu")


def test_tile_constants(simlib):
    K.check_tile_constants(simlib)


@pytest.mark.parametrize("dtype", list(K.DTYPES))
@pytest.mark.parametrize("shape", K.KERNEL_SHAPES)
def test_kernel(simlib, shape, dtype):
    K.check_kernel(simlib, None, CPU, shape, dtype)


def test_next_level_f64(simlib):
    K.check_next_level_f64(simlib, None, CPU)


def test_kernel_refusals(simlib):
    K.check_kernel_refusals(simlib, None, CPU)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("hw", K.HOST_SHAPES)
def test_ssim(simlib, hw, window):
    K.check_ssim(simlib, None, CPU, hw, window)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("hw", K.HOST_SHAPES)
def test_conditions(simlib, hw, window):
    K.check_conditions(simlib, None, CPU, hw, window)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_mask(simlib, window):
    K.check_mask(simlib, None, CPU, K.HOST_SHAPES[1], window)


def test_host_refusals(simlib):
    K.check_host_refusals(simlib, None, CPU)


@pytest.mark.parametrize("hw,weights,kind", K.MS_CASES)
def test_ms_ssim(simlib, hw, weights, kind):
    K.check_ms_ssim(simlib, None, CPU, hw, weights, kind)


def test_cli(simlib, monkeypatch, tmp_path):
    import hairfastgan_amd.encoders  # noqa: F401  the LPIPS tower of the re-run lpips / l2 / psnr check asks encoders._fused

    patch_host_modules(monkeypatch, simlib, ["hairfastgan_amd.encoders._fused"])
    K.check_cli(simlib, None, CPU, str(tmp_path))
