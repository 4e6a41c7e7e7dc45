"""GPU tests (-m gpu) of the identity-similarity path: the kernels of csrc/identity.h through the C ABI and the host mirror
hairfastgan_amd.identity against the torch / numpy restatements (tests/identity_ref.py) by the checks of
tests/identity_checks.py.  The full IR-SE50 at 112^2 (planes 112, 56, 28, 14 and 7) runs here only."""
import pytest

from tests import identity_checks as K
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.POOL_CASES, ids=[c[0] for c in K.POOL_CASES])
def test_crop_avgpool(case):
    K.check_crop_avgpool(*gpu_ctx(), *case)


def test_crop_avgpool_refusals():
    K.check_crop_avgpool_refusals(*gpu_ctx())


@pytest.mark.parametrize("d", K.NORM_DIMS)
def test_normalize(d):
    K.check_normalize(*gpu_ctx(), d)


def test_similarity():
    K.check_similarity(*gpu_ctx())


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("kind", ["small", "full"])
def test_network(kind, mode):
    from hairfastgan_amd import _runtime

    if kind == "full":
        K.check_full_conditions()
    with _runtime.conv_precision_scope(mode):
        K.check_network(*gpu_ctx(), kind)
        if kind == "full":
            K.check_similarity_full(*gpu_ctx())


@pytest.mark.parametrize("kind", ["tiny", "small", "full"])
def test_forward(kind):
    K.check_forward(*gpu_ctx(), kind)


@pytest.mark.parametrize("decoder", ["pil", "device"])
def test_cli(tmp_path, decoder):
    K.check_cli(*gpu_ctx(), str(tmp_path), decoder)
