"""hipsim tests of the Frechet-distance kernels (csrc/frechet.h) and their host mirror (hairfastgan_amd.metrics): the
product's kernel sources interpreted on the CPU against the numpy / mpmath restatements (tests/frechet_ref.py) by the checks
of tests/frechet_checks.py."""
import pytest
import torch

from tests import frechet_checks as K
from tests import frechet_ref as R

CPU = torch.device("cpu")


@pytest.mark.parametrize("n,d", K.ACCUMULATE_SHAPES)
def test_accumulate(simlib, n, d):
    K.check_accumulate(simlib, None, CPU, n, d)


def test_accumulate_split(simlib):
    K.check_accumulate_split(simlib, None, CPU)


def test_accumulate_f16(simlib):
    K.check_accumulate_f16(simlib, None, CPU)


def test_reset(simlib):
    K.check_reset(simlib, None, CPU)


@pytest.mark.parametrize("d", K.EIG_SIZES)
@pytest.mark.parametrize("family", R.EIG_FAMILIES)
def test_eigh(simlib, family, d):
    K.check_eigh(simlib, None, CPU, family, d)


@pytest.mark.parametrize("case", list(K.DIST_CASES))
def test_distance(simlib, case):
    K.check_distance(simlib, None, CPU, *case, K.DIST_CASES[case])


def test_files(simlib, tmp_path):
    K.check_files(simlib, None, CPU, str(tmp_path))


def test_cli(simlib, tmp_path):
    K.check_cli(simlib, None, CPU, str(tmp_path))


def test_errors(simlib):
    K.check_errors(simlib, None, CPU)
