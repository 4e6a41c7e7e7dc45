"""CPU tests (kernel sources interpreted by tests/hipsim): every small kernel called directly, at the smallest shapes that
reach each of its branches, against fp64 restatements with ATen's own fp32 error as the yardstick; batch invariance bit
for bit; no stray writes - tests/small_ops_checks.py."""
import pytest
import torch

from tests import small_ops_checks as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("op,case", K.cases(gpu=False), ids=K.case_id)
def test_small_op(simlib, golden, op, case):
    if op == "bicubic_down":
        K.check_bicubic_down(simlib, None, CPU, case, golden)
    else:
        K.CHECKS[op](simlib, None, CPU, case)


@pytest.mark.parametrize("op", K.BATCH_OPS)
def test_small_op_batch_invariance(simlib, op):
    K.check_batch_invariance(simlib, None, CPU, op)


@pytest.mark.parametrize("op", K.BIG_BATCH_OPS)
def test_small_op_batch_invariance_across_the_grid_cap(simlib, op):
    K.check_big_batch_invariance(simlib, None, CPU, op)


def test_small_op_size_refusals(simlib):
    K.check_size_refusals(simlib)
