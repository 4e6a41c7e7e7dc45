"""CPU tests (kernel sources interpreted by tests/hipsim): the generator's glue kernels called directly - the FIR and blur
passes, ToRGB, the style kernels, bias / noise / activation - with asymmetric filter taps, at the smallest shapes that reach
each branch, against fp64 restatements with ATen's own fp32 error as the yardstick; the asymmetric separable filter through
every conv route that contains one; bit-exact pairs, batch invariance, no stray writes - tests/generator_ops_checks.py."""
import pytest
import torch

from tests import generator_ops_checks as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("op,case", K.cases(gpu=False), ids=K.case_id)
def test_generator_op(simlib, op, case):
    K.CHECKS[op](simlib, None, CPU, case)


@pytest.mark.parametrize("op", K.BATCH_OPS)
def test_generator_op_batch_invariance(simlib, op):
    K.check_batch_invariance(simlib, None, CPU, op)


def test_generator_op_size_refusals(simlib):
    K.check_size_refusals(simlib)
