"""CPU tests (hipsim): the edge kernel of the two-pass upsampling conv (csrc/convh.hip, conv_up_rim_h) against the rim tile
families it replaces, bit for bit, and against the oracle - tests/up_rim_checks.py; and the launches themselves, written down
by hipsim's plan recording: that hf_debug_set_tuning bit 5 really switches between the two forms the parity is asserted on."""
import os
import subprocess
import sys

import pytest
import torch

from tests import up_rim_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("shape", K.CASES)
def test_up_rim_kernel_equals_rim_families(simlib, shape, nterms):
    # the split form of the blur pass reads the same intermediate: checked once here (the interpreter takes seconds per launch),
    # on every case by the GPU tests
    K.check_case(simlib, None, torch.device("cpu"), shape, nterms, with_split=shape == K.CASES[0])


# hf_modconv3x3_up_f16_pre_f32 on a 40 x 16 plane, 32 -> 64 channels, with the tuning word clear, then with bit 5 set
CHILD = r"""
import ctypes, importlib.util, os, sys
import numpy as np
root, so = sys.argv[1], sys.argv[2]
spec = importlib.util.spec_from_file_location("hf_lib", os.path.join(root, "hairfastgan_amd", "_lib.py"))
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
lib = _lib.bind(ctypes.CDLL(so))
batch, cin, cout, h, w = 1, 32, 64, 40, 16
pitch = lib.hf_modconv_up_pitch(w)
xh = np.zeros((batch, cin // 8, h, w, 8), np.float16)
wt = np.zeros(9 * cin * cout + 16, np.float16)
d = np.ones((batch, cout), np.float32)
tmp = np.zeros((batch, cout, 2 * h + 1, pitch), np.float32)
p = lambda a: a.ctypes.data
for bits in (0, 32):
    lib.hf_debug_set_tuning(bits)
    rc = lib.hf_modconv3x3_up_f16_pre_f32(p(tmp), p(xh), p(xh), p(wt), p(wt), 3, p(d), batch, cin, cout, h, w, pitch, None)
    print(rc, lib.hf_debug_last_path())
"""


def test_tuning_bit5_switches_between_edge_kernel_and_rim_families(simlib, tmp_path):
    plan = tmp_path / "plan.txt"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, simlib._name], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "HIPSIM_PLAN": str(plan)})
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "581", "0", "581"]
    lines = plan.read_text().splitlines()
    assert len(lines) == 3, lines  # bit clear: main launch + edge kernel; bit set: one launch
    main, rim, old = lines
    # interior only: three 16 x 16 tiles of the 40 x 16 plane, one 64-channel tile
    assert " grid=3,1,1 block=512,1,1 " in main and " n_tiles=3 " in main and " n_geom=1 g0=0,0,40,16,4,4,0,1,3,1,0 " in main, main
    # the edge: one wave per block, (1 row tile + 2 column tiles) x 2 tiles of 32 channels; arguments row_tiles, position tiles
    assert " grid=6,1,1 block=64,1,1 lds=0 : " in rim and rim.endswith("} P P 1 3"), rim
    assert rim.split(" grid=")[0] != main.split(" grid=")[0]  # another kernel
    # bit 5: the same main kernel over three families - interior, row Y = 40 (17 positions), column X = 16 (40 positions)
    assert old.split(" grid=")[0] == main.split(" grid=")[0]
    assert " grid=5,1,1 block=512,1,1 " in old and " n_tiles=5 " in old and " n_geom=3 " in old, old
    assert " g1=40,0,1,17," in old and " g2=0,16,40,1," in old, old
