"""GPU tests (-m gpu) of the SSIM / MS-SSIM path: the kernel of csrc/ssim.h through the C ABI and the host mirror
hairfastgan_amd.ssim against the fp64 restatements (tests/ssim_ref.py) by the checks of tests/ssim_checks.py."""
import pytest

from tests import ssim_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


def test_tile_constants():
    K.check_tile_constants(gpu_ctx()[0])


@pytest.mark.parametrize("dtype", list(K.DTYPES))
@pytest.mark.parametrize("shape", K.KERNEL_SHAPES)
def test_kernel(shape, dtype):
    K.check_kernel(*gpu_ctx(), shape, dtype)


def test_next_level_f64():
    K.check_next_level_f64(*gpu_ctx())


def test_kernel_refusals():
    K.check_kernel_refusals(*gpu_ctx())


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("hw", K.HOST_SHAPES)
def test_ssim(hw, window):
    K.check_ssim(*gpu_ctx(), hw, window)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("hw", K.HOST_SHAPES)
def test_conditions(hw, window):
    K.check_conditions(*gpu_ctx(), hw, window)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_mask(window):
    K.check_mask(*gpu_ctx(), K.HOST_SHAPES[1], window)


def test_host_refusals():
    K.check_host_refusals(*gpu_ctx())


@pytest.mark.parametrize("hw,weights,kind", K.MS_CASES)
def test_ms_ssim(hw, weights, kind):
    K.check_ms_ssim(*gpu_ctx(), hw, weights, kind)


@pytest.mark.parametrize("decoder", ["pil", "device"])
def test_cli(tmp_path, decoder):
    K.check_cli(*gpu_ctx(), str(tmp_path), decoder)
