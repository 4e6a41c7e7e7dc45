"""hipsim tests of the paste-back kernels (csrc/paste.h): the product's kernel sources interpreted on the CPU against PIL
through the restatement (tests/paste_ref.py) - byte for byte (tests/paste_checks.py)."""
import pytest
import torch

from tests import paste_checks as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", list(K.CASES))
def test_paste(simlib, name):
    K.check_paste(simlib, None, CPU, name)


def test_paste_user_mask_without_feather(simlib):
    K.check_paste(simlib, None, CPU, "down", feather=0.0, with_mask=True)


def test_multiply_all_byte_pairs(simlib):
    K.check_multiply(simlib, None, CPU)


def test_invalid_arguments(simlib):
    K.check_paste_invalid(simlib, None, CPU)
