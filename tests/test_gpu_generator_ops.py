"""GPU tests (-m gpu): the generator's glue kernels called directly on the hardware - 64-lane shuffles, the DPP lane shifts of
the split blur, hipcc's contraction - with asymmetric filter taps, against fp64 restatements with ATen's own fp32 error as
the yardstick; the asymmetric separable filter through every conv route that contains one; bit-exact pairs, batch
invariance, no stray writes - tests/generator_ops_checks.py."""
import pytest
import torch

from tests import generator_ops_checks as K

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("op,case", K.cases(gpu=True), ids=K.case_id)
def test_generator_op(op, case):
    from hairfastgan_amd._runtime import lib, stream

    dev = _dev()
    K.CHECKS[op](lib(), stream(), dev, case)


@pytest.mark.parametrize("op", K.BATCH_OPS)
def test_generator_op_batch_invariance(op):
    from hairfastgan_amd._runtime import lib, stream

    dev = _dev()
    K.check_batch_invariance(lib(), stream(), dev, op)


def test_generator_op_size_refusals():
    from hairfastgan_amd._runtime import lib

    _dev()
    K.check_size_refusals(lib())
