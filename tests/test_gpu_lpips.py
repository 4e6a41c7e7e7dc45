"""GPU tests (-m gpu) of the LPIPS and L2 / PSNR path: the kernels of csrc/lpips.h through the C ABI and the host mirror
hairfastgan_amd.lpips against the torch / numpy restatements (tests/lpips_ref.py) by the checks of tests/lpips_checks.py.
AlexNet at 272^2 runs here only: its 3x3 layers reach the tiled fp16 matrix-core route there."""
import pytest

from tests import lpips_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,stride,h,w", K.POOL_CASES)
def test_maxpool(k, stride, h, w):
    K.check_maxpool(*gpu_ctx(), k, stride, h, w)


@pytest.mark.parametrize("w,h,ow,oh", K.RESIZE_CASES)
def test_resize_bilinear(w, h, ow, oh):
    K.check_resize_bilinear(*gpu_ctx(), w, h, ow, oh)


@pytest.mark.parametrize("variant", K.CONV_VARIANTS)
@pytest.mark.parametrize("case", K.CONV_CASES)
def test_conv_direct(case, variant):
    K.check_conv_direct(*gpu_ctx(), *case, variant)


def test_conv_direct_refusals():
    K.check_conv_direct_refusals(*gpu_ctx())


@pytest.mark.parametrize("family", K.LAYER_FAMILIES)
@pytest.mark.parametrize("shape", K.LAYER_SHAPES)
def test_layer(shape, family):
    K.check_layer(*gpu_ctx(), shape, family)


@pytest.mark.parametrize("shape", K.LAYER_SHAPES)
def test_layer_conditions(shape):
    K.check_layer_conditions(*gpu_ctx(), shape)


def test_layer_refusals():
    K.check_layer_refusals(*gpu_ctx())


@pytest.mark.parametrize("net_type,size", K.LPIPS_SIM + K.LPIPS_GPU)
def test_lpips(net_type, size):
    K.check_lpips(*gpu_ctx(), net_type, size, whole_batch=True)


def test_lpips_tiled_route():
    """AlexNet's 3x3 layers at 272^2 (16 x 16 planes) are taken by the tiled fp16 matrix-core kernel."""
    from hairfastgan_amd.encoders import _fused as FU

    model = K.make_model(*gpu_ctx()[::2], "alex")
    model.features(K.lpips_images("alex", 272, K.NOISES[0])[0].to("cuda:0"))
    for i in (6, 8, 10):
        assert FU.conv_route(model._plan[i], 16, 16, 3, 1, {"bias": None, "act": 1, "alpha": 0.0}, batch=2) == FU.TILED_F16


def test_psnr():
    K.check_psnr(*gpu_ctx())


@pytest.mark.parametrize("decoder", ["pil", "device"])
def test_cli(tmp_path, decoder):
    K.check_cli(*gpu_ctx(), str(tmp_path), decoder)
