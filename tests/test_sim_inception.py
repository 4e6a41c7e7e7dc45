"""hipsim tests of the FID Inception-v3 path: the product's kernel sources (csrc/conv_rect.h, csrc/inception.h) interpreted on
the CPU and their host mirror (hairfastgan_amd.inception, the --fid column of hairfastgan_amd.metrics) against the torch
restatement (tests/inception_ref.py) by the checks of tests/inception_checks.py.  The network runs at channel_div = 8 on 75^2
images here (planes 37, 35, 35, 17, 17, 15, 7, 3, 1); the real widths at 299^2 run on the GPU.
At 75^2 Mixed_7c's plane is a single pixel and there is no resize, so at network level nothing here tells Mixed_7c's max pool from
an average or the TF1 resize from a half-pixel one: test_pool and test_resize do that for the kernels, the GPU's `full` case for
the network (tests/inception_checks.py, check_conditions)."""
import pytest
import torch

from tests import inception_checks as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("label", list(K.RECT_CASES))
def test_rect_conv(simlib, label, mode):
    K.check_rect(simlib, None, CPU, label, mode)


def test_rect_conv_refusals(simlib):
    K.check_rect_refusals(simlib, None, CPU)


@pytest.mark.parametrize("mode,stride,plane", K.POOL_CASES, ids=[f"{m}-s{s}-{p[0]}x{p[1]}" for m, s, p in K.POOL_CASES])
def test_pool(simlib, mode, stride, plane):
    K.check_pool(simlib, None, CPU, mode, stride, plane)


def test_pool_refusals(simlib):
    K.check_pool_refusals(simlib, None, CPU)


@pytest.mark.parametrize("label", list(K.RESIZE_CASES))
def test_resize(simlib, label):
    K.check_resize(simlib, None, CPU, label)


def test_resize_refusals(simlib):
    K.check_resize_refusals(simlib, None, CPU)


@pytest.mark.parametrize("mode", K.NET_MODES)
def test_network(simlib, mode):
    """All four taps against fp64 within max(8 x torch's fp32 CPU error, 3 * 2^-24 max |feature|), equal bits twice and per row.
    Measured at the 2048 tap: tiny f16x3 4.2e-7 / f32 4.7e-7 (threshold 5.5e-6), full f16x3 5.3e-6 / f32 3.9e-6 (2.2e-5).
    "f16" and "auto" run the f16x3 form (a metric's features are fp32-class in every mode) and meet the same threshold; operands
    rounded to fp16 would not: 1.0e-4 at tiny's 64 tap (threshold 9.8e-7), 2.5e-4 at full's (1.5e-6), measured with nterms = 1."""
    # every row against its single-image call under f16x3 and f32; "f16" and "auto" run f16x3's code and compare row 1 only
    # (two interpreted forward passes less each: interpreter time, nothing else)
    K.check_network(simlib, None, CPU, "tiny", mode, every_row=mode in ("f16x3", "f32"))


def test_refusals(simlib):
    K.check_refusals(simlib, None, CPU)


@pytest.mark.parametrize("feature", [64, 192])
def test_frechet(simlib, feature):
    from hairfastgan_amd import _runtime

    with _runtime.conv_precision_scope("f32"):  # the interpreter runs the padded matrix-core tiles slowly; test_network covers them
        K.check_frechet(simlib, None, CPU, feature)


def test_cli(simlib, tmp_path):
    from hairfastgan_amd import _runtime

    with _runtime.conv_precision_scope("f32"):
        K.check_cli(simlib, None, CPU, str(tmp_path))
