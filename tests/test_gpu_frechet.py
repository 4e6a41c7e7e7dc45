"""GPU tests (-m gpu) of the Frechet-distance path: the kernels of csrc/frechet.h through the C ABI and the host mirror
hairfastgan_amd.metrics against the numpy / mpmath restatements (tests/frechet_ref.py) by the checks of
tests/frechet_checks.py - the statistics bit for bit, the eigensolver and the distance within thresholds derived from
numpy's own error.  The d = 512 cases (about 9000 launches per eigensolve) run in a child process under a time limit."""
import os
import subprocess
import sys

import pytest

from tests import frechet_checks as K
from tests import frechet_ref as R
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,d", K.ACCUMULATE_SHAPES)
def test_accumulate(n, d):
    K.check_accumulate(*gpu_ctx(), n, d)


def test_accumulate_split():
    K.check_accumulate_split(*gpu_ctx())


def test_accumulate_f16():
    K.check_accumulate_f16(*gpu_ctx())


def test_reset():
    K.check_reset(*gpu_ctx())


@pytest.mark.parametrize("d", K.EIG_SIZES)
@pytest.mark.parametrize("family", R.EIG_FAMILIES)
def test_eigh(family, d):
    K.check_eigh(*gpu_ctx(), family, d)


@pytest.mark.parametrize("case", list(K.DIST_CASES))
def test_distance(case):
    K.check_distance(*gpu_ctx(), *case, K.DIST_CASES[case])


def test_size_512_under_a_time_limit():
    """Every matrix family and the (512, 300, 700) distance at d = 512, in a child process that is ended after 120 s."""
    code = ("import torch\n"
            "from hairfastgan_amd import _runtime\n"
            "from tests import frechet_checks as K\n"
            "from tests import frechet_ref as R\n"
            "ctx = (_runtime.lib(), _runtime.stream(), torch.device('cuda:0'))\n"
            "for family in R.EIG_FAMILIES:\n"
            "    K.check_eigh(*ctx, family, 512)\n"
            "K.check_distance(*ctx, *K.DIST_CASE_GPU[0], K.DIST_CASE_GPU[1])\n"
            "print('size 512 ok')\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "size 512 ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def test_clip_model():
    K.check_clip_model(*gpu_ctx())


@pytest.mark.parametrize("decoder", ["pil", "device"])
def test_files(tmp_path, decoder):
    K.check_files(*gpu_ctx(), str(tmp_path), decoder)


def test_cli(tmp_path):
    K.check_cli(*gpu_ctx(), str(tmp_path))


def test_errors():
    K.check_errors(*gpu_ctx())
