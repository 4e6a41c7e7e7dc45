"""GPU tests (-m gpu): the 1x1-conv GEMM on the fp16 matrix cores (csrc/gemm_h.hip) called directly on the hardware - the real
LDS-DMA staging and MFMA, both tile forms on ragged planes, stride 2, several images per tile, pre-split input, 128-channel
blocks, split-K in both forms, the virtual split, grouped launches, one-term operands - against the fp64 contract with a
per-element operand bound; bit-exact pairs, batch invariance, no stray writes - tests/gemm_checks.py."""
import pytest
import torch

from tests import gemm_checks as K

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("op,case", K.cases(gpu=True), ids=K.case_id)
def test_conv1x1_direct(op, case):
    from hairfastgan_amd._runtime import lib, stream

    K.CHECKS[op](lib(), stream(), _dev(), case)


@pytest.mark.parametrize("op", K.BATCH_OPS)
def test_conv1x1_batch_invariance(op):
    from hairfastgan_amd._runtime import lib, stream

    K.check_batch_invariance(lib(), stream(), _dev(), op)
