"""GPU tests (-m gpu): every small kernel called directly on the hardware - 64-lane shuffles, hipcc's contraction, second
trips of the grid-stride loops, launch geometry that changes with the batch - against fp64 restatements with ATen's own
fp32 error as the yardstick; batch invariance bit for bit; no stray writes - tests/small_ops_checks.py."""
import pytest
import torch

from tests import small_ops_checks as K

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("op,case", K.cases(gpu=True), ids=K.case_id)
def test_small_op(golden, op, case):
    from hairfastgan_amd._runtime import lib, stream

    if op == "bicubic_down":
        K.check_bicubic_down(lib(), stream(), _dev(), case, golden)
    else:
        K.CHECKS[op](lib(), stream(), _dev(), case)


@pytest.mark.parametrize("op", K.BATCH_OPS)
def test_small_op_batch_invariance(op):
    from hairfastgan_amd._runtime import lib, stream

    K.check_batch_invariance(lib(), stream(), _dev(), op)


@pytest.mark.parametrize("op", K.BIG_BATCH_OPS)
def test_small_op_batch_invariance_across_the_grid_cap(op):
    from hairfastgan_amd._runtime import lib, stream

    K.check_big_batch_invariance(lib(), stream(), _dev(), op)
