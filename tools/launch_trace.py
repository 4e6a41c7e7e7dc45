#!/usr/bin/env python3
"""Proves that a host-side refactor leaves the sequence of C calls unchanged (the Python counterpart of
tools/compare_isa.sh).  A recording proxy stands in for the bound library (_lib._LIB) before the package is used and
writes one line per C call: name, every integer / float argument, 0 or P for each pointer, and the return value.  Run
it on the base revision (--root a `git worktree` of it) and on the working tree, same cases, and diff the two files.
The package reads its HAIRFAST_* switches at import: one process per configuration.

  tools/launch_trace.py [--root DIR] [--dry] [--hook] [--out FILE] CASE...
  CASE  gen:BATCH[:START:END]   Generator(1024) forward, random noise (START > 0: with a layer_in of the right shape)
        embed                   the Embedding stage of one swap (e4e, FS encoder, BiSeNet, generator 3->3 / 0->3)
        swap | swap_batch:N     whole swaps (GPU only: a dry swap stops at the shape adaptor's scatter_ of its labels)
  --hook  gen: a forward hook on one StyledConv (the blocks around it leave the fused fast path)
  --dry   no GPU: launches (last argument = the stream) are recorded and skipped, host-only queries (workspace sizes,
          pitches, *_output_ok, *_slabs) are answered by tests/hipsim/libhairfast_sim.so; tensors stay uninitialised."""
import argparse
import ctypes
import os
import sys

ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--dry", action="store_true")
ap.add_argument("--hook", action="store_true")
ap.add_argument("--out", default="-")
ap.add_argument("cases", nargs="+")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)

import torch  # noqa: E402

from hairfastgan_amd import _lib, _runtime  # noqa: E402

assert os.path.dirname(_lib.__file__) == os.path.join(root, "hairfastgan_amd"), _lib.__file__
out = sys.stdout if args.out == "-" else open(args.out, "w")


class Recorder:
    def __init__(self, real, dry):
        self._real, self._dry, self._name = real, dry, real._name

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = fn.argtypes or []
        skip = self._dry and bool(types) and types[-1] is ctypes.c_void_p  # the stream comes last: a launch

        def call(*a):
            ret = 0 if skip else fn(*a)
            shown = [("0" if not v else "P") if t not in (ctypes.c_int, ctypes.c_longlong, ctypes.c_float) else repr(v)
                     for t, v in zip(types, a)]
            print(name, *shown, "->", ret, file=out)
            return ret

        self.__dict__[name] = call
        return call


if args.dry:
    real = _lib.bind(ctypes.CDLL(os.path.join(root, "tests", "hipsim", "libhairfast_sim.so")))
    _runtime.require_gpu = lambda *t: None
    _runtime.stream = lambda: None
    torch.cuda.is_current_stream_capturing = lambda: False
else:
    real = _lib.load()
_lib._LIB = Recorder(real, args.dry)

import bench  # noqa: E402  (the synthetic-weight builders; imports nothing of the package at module level)

dev = torch.device("cpu" if args.dry else "cuda:0")
gen, sd = bench.build_generator(dev)
hf = None
rng = torch.Generator().manual_seed(1)
for case in args.cases:
    kind, *nums = case.split(":")
    nums = [int(n) for n in nums]
    print("#", case, file=out)
    torch.manual_seed(7)
    with torch.inference_mode():
        if kind == "gen":
            batch, start, end = (nums + [0, 8])[:3]
            lat = torch.randn(batch, 18, 512, device=dev)
            layer_in = None
            if start > 0:
                layer_in = torch.randn(batch, gen.convs[2 * start - 2].conv.in_channel, 2 ** (start + 1), 2 ** (start + 1), device=dev)
            handle = gen.convs[5].register_forward_hook(lambda m, i, o: None) if args.hook else None
            gen([lat], input_is_latent=True, layer_in=layer_in, start_layer=start, end_layer=end)
            if handle is not None:
                handle.remove()
            continue
        hf = hf or bench.build_hairfast(sd, dev)
        images = [torch.randint(0, 256, (3, 1024, 1024), dtype=torch.uint8, generator=rng) for _ in range(3 * max(nums + [1]))]
        if kind == "embed":
            hf.embed.embedding_images({im: [n] for im, n in zip(images, ("face", "shape", "color"))})
        elif kind == "swap":
            hf.swap(*images, seed=7)
        elif kind == "swap_batch":
            hf.swap_batch([tuple(images[3 * t:3 * t + 3]) for t in range(nums[0])], seed=7)
        else:
            raise SystemExit(f"unknown case {case!r}")
if not args.dry:
    torch.cuda.synchronize()
out.close()
