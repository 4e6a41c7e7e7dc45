"""hipsim's launch-plan recording (HIPSIM_PLAN=FILE, the proof tool of DESIGN 4.17): a launch is written down, not run."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one 64 -> 64 channel same-resolution layer on an 8 x 32 plane: a single 64 co x 256 px tile (configuration 51, f16x3)
CHILD = r"""
import ctypes, importlib.util, os, sys
import numpy as np
root, so = sys.argv[1], sys.argv[2]
spec = importlib.util.spec_from_file_location("hf_lib", os.path.join(root, "hairfastgan_amd", "_lib.py"))
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
lib = _lib.bind(ctypes.CDLL(so))
batch, cin, cout, h, w = 1, 64, 64, 8, 32
x = np.ones((batch, cin, h, w), np.float32)
out = np.full((batch, cout, h, w), 7.0, np.float32)
wt = np.zeros(9 * cin * cout + 16, np.float16)
s = np.ones((batch, cin), np.float32)
d = np.ones((batch, cout), np.float32)
bias = np.zeros(cout, np.float32)
p = lambda a: a.ctypes.data
rc = lib.hf_modconv3x3_f16_f32(p(out), p(x), p(wt), p(wt), 3, p(s), p(d), None, None, 0, p(bias), batch, cin, cout, h, w,
                               0.2, 2.0 ** 0.5, None)
print(rc, lib.hf_debug_last_path(), float(out.min()), float(out.max()))
"""


def run_child(simlib, env):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, simlib._name], capture_output=True, text=True, timeout=120,
                       env={**{k: v for k, v in os.environ.items() if k != "HIPSIM_PLAN"}, **env})
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_plan_recording_writes_the_launch_and_does_not_run_it(simlib, tmp_path):
    plan = tmp_path / "plan.txt"
    rc, path, lo, hi = run_child(simlib, {"HIPSIM_PLAN": str(plan)})
    assert (rc, path) == ("0", "551")
    assert (lo, hi) == ("7.0", "7.0")  # the kernel did not run
    lines = plan.read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("launch @"), lines
    # conv_mfma_h<3, 1, 2, 2, 4, ...>: 2 stages x 2 parts x (9 x 2 x 64 weight + 2 x 340 halo units) x 16 B,
    # + s [2][64] + the epilogue tables [2][3][64], floats
    lds = 2 * 2 * (9 * 2 * 64 + 2 * 340) * 16 + (2 * 64 + 2 * 3 * 64) * 4
    assert f" grid=1,1,1 block=512,1,1 lds={lds} : " in lines[0]
    for field in ("splits=1 ", "swap_xy=0 ", "n_tiles=1 ", "dims=1,64,64,8,32 ", "act=1 ", "n_geom=1 g0=0,0,8,32,5,3,0,1,1,1,0 "):
        assert field in lines[0], (field, lines[0])
    assert lines[0].endswith("} P P")
    # the recorded offset is a function of the library: its symbol names the instantiation with its argument values
    # (through binutils' nm, as tools/launch_trace.py resolves it: where there is none the line's form above is the check)
    if shutil.which("nm") is None:
        return
    offset = int(lines[0].split()[1][1:], 16)
    syms = subprocess.run(["nm", "--defined-only", simlib._name], capture_output=True, text=True, check=True).stdout.splitlines()
    names = [ln.split(" ", 2)[2] for ln in syms if int(ln.split(" ", 1)[0], 16) == offset]
    assert any("conv_mfma_hILi3ELi1ELi2ELi2ELi4ELb1ELb0ELi32ELb0ELb0E" in n for n in names), names


def test_without_the_variable_the_kernel_runs(simlib):
    rc, path, lo, hi = run_child(simlib, {})
    assert (rc, path) == ("0", "551")
    assert (lo, hi) == ("0.0", "0.0")  # zero weights, zero bias: the layer's output
