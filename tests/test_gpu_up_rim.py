"""GPU tests (-m gpu): the edge kernel of the two-pass upsampling conv (csrc/convh.hip, conv_up_rim_h) against the rim tile
families it replaces (hf_debug_set_tuning bit 5), bit for bit, and against the oracle - tests/up_rim_checks.py; then one
generator forward whose 32^2 -> 64^2 block takes the route."""
import pytest
import torch

from oracle import cases as C
from tests import up_rim_checks as K

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("shape", K.CASES)
def test_up_rim_kernel_equals_rim_families(shape, nterms):
    from hairfastgan_amd._runtime import lib, stream

    K.check_case(lib(), stream(), _dev(), shape, nterms)


def test_generator64_equal_bits_with_rim_families(monkeypatch):
    """Generator(64), batch 2: the 512 -> 512 transposed conv from 32^2 takes its input pre-split (two passes, below the
    one-kernel form's 128 rows) - the image with the edge kernel equals the image with the rim families in every bit."""
    from hairfastgan_amd import _marshal as M
    from hairfastgan_amd._runtime import lib
    from hairfastgan_amd.stylegan2.model import Generator

    dev = _dev()
    size = 64
    g = Generator(size, 512, 2, channel_multiplier=2).eval()
    g.load_state_dict(C.generator_params({k: tuple(v.shape) for k, v in g.state_dict().items()}))
    g = g.to(dev)
    lat, nz, _ = C.generator_inputs(size, 2, 0)
    lat, nz = lat.to(dev), [n.to(dev) for n in nz]
    up_pre, real_up = [], M.modconv3x3_up

    def up(lib_, st, x, *a, **k):
        if isinstance(x, M.SplitActivation):
            up_pre.append(x.shape[2])
        return real_up(lib_, st, x, *a, **k)

    monkeypatch.setattr(M, "modconv3x3_up", up)
    L = lib()
    img = {}
    try:
        with torch.inference_mode():
            for bits in (0, K.RIM_FAMILIES):
                L.hf_debug_set_tuning(bits)
                img[bits], _ = g([lat], input_is_latent=True, noise=nz)
                torch.cuda.synchronize()
    finally:
        L.hf_debug_set_tuning(0)
    assert up_pre == [32, 32]  # the route was taken, once per forward
    assert img[0].shape == (2, 3, size, size)
    assert torch.equal(img[0], img[K.RIM_FAMILIES])
