"""TEST INFRASTRUCTURE - what the check modules (tests/*_checks.py), the GPU tests and the hipsim tests state once: which
library a host function is handed, an expected exception, a tensor's bits, the GPU tests' context, pointing host modules at
the interpreter build, and reading back what a paired-folder command line wrote.  A plain module: no fixtures."""
import json
import os
import sys

import numpy as np


def inject(L, device):
    """The `lib` argument of the host modules: the interpreter build on CPU tensors, the product's own library on the GPU."""
    return L if device.type == "cpu" else None


def raises(kind, fn, text=None):
    try:
        fn()
    except kind as e:
        assert text is None or text in str(e), str(e)
    else:
        raise AssertionError(f"{kind.__name__} expected")


def bits(t):
    """The bit patterns of a float64 (-> uint64) or float32 (-> uint32) tensor."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}[a.dtype])


def gpu_ctx():
    """(library, stream, device) of a `-m gpu` test; without a GPU the test fails, it does not skip."""
    import pytest
    import torch

    from hairfastgan_amd import _runtime

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return _runtime.lib(), _runtime.stream(), torch.device("cuda:0")


def patch_host_modules(monkeypatch, simlib, module_names):
    """Points the lib() / stream() / require_gpu of the named (imported) product modules at the interpreter build."""
    for name in module_names:
        mod = sys.modules[name]
        monkeypatch.setattr(mod, "lib", lambda: simlib)
        monkeypatch.setattr(mod, "stream", lambda: None)
        monkeypatch.setattr(mod, "require_gpu", lambda *a: None)


def read_scores(root, tag):
    """(scores_<tag>.json as a dict in file order, the text of stat_<tag>.txt) of root/inference_metrics."""
    out = os.path.join(root, "inference_metrics")
    with open(os.path.join(out, f"scores_{tag}.json")) as f:
        saved = json.load(f)
    with open(os.path.join(out, f"stat_{tag}.txt")) as f:
        return saved, f.read()
