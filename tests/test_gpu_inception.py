"""GPU tests (-m gpu) of the FID Inception-v3 path: the kernels of csrc/conv_rect.h and csrc/inception.h through the C ABI and
the host mirror hairfastgan_amd.inception against the torch restatement (tests/inception_ref.py) by the checks of
tests/inception_checks.py.  `full` - the real widths, 64^2 bytes resized to 299^2 - runs here only."""
import pytest

from tests import inception_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("label", list(K.RECT_CASES))
def test_rect_conv(label, mode):
    K.check_rect(*gpu_ctx(), label, mode)


def test_rect_conv_refusals():
    K.check_rect_refusals(*gpu_ctx())


@pytest.mark.parametrize("mode,stride,plane", K.POOL_CASES, ids=[f"{m}-s{s}-{p[0]}x{p[1]}" for m, s, p in K.POOL_CASES])
def test_pool(mode, stride, plane):
    K.check_pool(*gpu_ctx(), mode, stride, plane)


def test_pool_refusals():
    K.check_pool_refusals(*gpu_ctx())


@pytest.mark.parametrize("label", list(K.RESIZE_CASES))
def test_resize(label):
    K.check_resize(*gpu_ctx(), label)


def test_resize_refusals():
    K.check_resize_refusals(*gpu_ctx())


@pytest.mark.parametrize("mode", K.NET_MODES)
@pytest.mark.parametrize("kind", ["tiny", "full"])
def test_network(kind, mode):
    """All four taps against fp64 within max(8 x torch's fp32 CPU error, 3 * 2^-24 max |feature|), equal bits twice and per row.
    Measured at the 2048 tap: tiny f16x3 4.2e-7 / f32 4.7e-7 (threshold 5.5e-6), full f16x3 5.3e-6 / f32 3.9e-6 (2.2e-5).
    "f16" and "auto" run the f16x3 form (a metric's features are fp32-class in every mode) and meet the same threshold; operands
    rounded to fp16 would not: 1.0e-4 at tiny's 64 tap (threshold 9.8e-7), 2.5e-4 at full's (1.5e-6), measured with nterms = 1."""
    K.check_conditions(kind)
    K.check_network(*gpu_ctx(), kind, mode)


def test_refusals():
    K.check_refusals(*gpu_ctx())


@pytest.mark.parametrize("feature", [64, 192])
def test_frechet(feature):
    K.check_frechet(*gpu_ctx(), feature)


def test_cli(tmp_path):
    K.check_cli(*gpu_ctx(), str(tmp_path), feature=2048)
