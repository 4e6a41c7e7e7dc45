#!/usr/bin/env python3
"""Proves that a host-side refactor leaves the sequence of C calls unchanged (the Python counterpart of
tools/compare_isa.sh).  A recording proxy stands in for the bound library (_lib._LIB) before the package is used and
writes one line per C call: name, every integer / float argument, 0 or P for each pointer, and the return value.  Run
it on the base revision (--root a `git worktree` of it) and on the working tree, same cases, and diff the two files.
The package reads its HAIRFAST_* switches at import: one process per configuration.

  tools/launch_trace.py [--root DIR] [--dry | --plan FILE] [--hook] [--out FILE] CASE...
  CASE  gen:BATCH[:START:END]   Generator(1024) forward, random noise (START > 0: with a layer_in of the right shape)
        embed                   the Embedding stage of one swap (e4e, FS encoder, BiSeNet, generator 3->3 / 0->3)
        swap | swap_batch:N     whole swaps (GPU only: a dry swap stops at the shape adaptor's scatter_ of its labels)
  --hook  gen: a forward hook on one StyledConv (the blocks around it leave the fused fast path)
  --dry   no GPU: launches (last argument = the stream) are recorded and skipped, host-only queries (workspace sizes,
          pitches, *_output_ok, *_slabs) are answered by tests/hipsim/libhairfast_sim.so; tensors stay uninitialised.
  --plan FILE  --dry one level down: the launches go through to the hipsim library, whose hipLaunchKernelGGL (HIPSIM_PLAN
          set) writes each kernel launch to FILE instead of running it - the kernel instantiation with its template
          argument values (offsets resolved through `nm -C`), grid, block, dynamic LDS bytes, the plan fields of a
          ConvParams.  After the cases a sweep re-issues every distinct fp16 convolution call they made, straight at the
          entry points, with the batches, operand modes and debug hooks a dry case cannot reach (see sweep())."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--dry", action="store_true")
ap.add_argument("--plan")
ap.add_argument("--hook", action="store_true")
ap.add_argument("--out", default="-")
ap.add_argument("cases", nargs="+")
args = ap.parse_args()
if args.plan:
    args.dry = True
    open(args.plan, "w").close()
    os.environ["HIPSIM_PLAN"] = os.path.abspath(args.plan)  # read by the library at its first launch
root = os.path.abspath(args.root)
sys.path.insert(0, root)

import torch  # noqa: E402

from hairfastgan_amd import _lib, _runtime  # noqa: E402

assert os.path.dirname(_lib.__file__) == os.path.join(root, "hairfastgan_amd"), _lib.__file__
out = sys.stdout if args.out == "-" else open(args.out, "w")


class Recorder:
    def __init__(self, real, dry):
        self._real, self._dry, self._name = real, dry, real._name
        self.calls = {}  # --plan: every distinct fp16 convolution call of the cases, for the sweep

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = fn.argtypes or []
        skip = self._dry and bool(types) and types[-1] is ctypes.c_void_p  # the stream comes last: a launch

        def call(*a):
            ret = 0 if skip else fn(*a)
            shown = [("0" if not v else "P") if t not in (ctypes.c_int, ctypes.c_longlong, ctypes.c_float) else repr(v)
                     for t, v in zip(types, a)]
            print(name, *shown, "->", ret, file=out)
            if args.plan and name in SWEPT:
                self.calls.setdefault((name, *shown), [bool(v) if t not in NUMERIC else v for t, v in zip(types, a)])
            return ret

        self.__dict__[name] = call
        return call


NUMERIC = (ctypes.c_int, ctypes.c_longlong, ctypes.c_float)
ENC = ("hf_conv2d_f16_f32", "hf_conv2d_f16_split_f32", "hf_conv1x1_f16_f32")
GEN = ("hf_modconv3x3_f16_f32", "hf_modconv3x3_f16_rgb_f32", "hf_modconv3x3_f16_pre_f32", "hf_modconv3x3_f16_pre_image_f32",
       "hf_modconv3x3_up_f16_f32", "hf_modconv3x3_up_f16_pre_f32", "hf_modconv3x3_up_blur_f16_f32",
       "hf_modconv3x3_small_f16_f32", "hf_modconv3x3_small_up_blur_f16_f32")
SWEPT = ENC + GEN

if args.dry:
    real = _lib.bind(ctypes.CDLL(os.path.join(root, "tests", "hipsim", "libhairfast_sim.so")))
    _runtime.require_gpu = lambda *t: None
    _runtime.stream = lambda: None
    torch.cuda.is_current_stream_capturing = lambda: False
else:
    real = _lib.load()
_lib._LIB = Recorder(real, args.dry and not args.plan)

import bench  # noqa: E402  (the synthetic-weight builders; imports nothing of the package at module level)


def mark(text):  # --plan: a heading in the plan file (the library appends to the same file, line by line)
    if args.plan:
        with open(args.plan, "a") as f:
            f.write(text + "\n")


dev = torch.device("cpu" if args.dry else "cuda:0")
gen, sd = bench.build_generator(dev)
hf = None
rng = torch.Generator().manual_seed(1)
for case in args.cases:
    kind, *nums = case.split(":")
    nums = [int(n) for n in nums]
    print("#", case, file=out)
    mark("# " + case)
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


def sweep(lib):
    """The entry points directly, for what a dry case cannot reach.  Pointers are one dummy buffer (nothing runs).
    encoder convs (every distinct call of the cases): batch 3 and 96 x nterms 1, 3 x pre-split input or not x
      batch-invariant off, on, with the workspace / split-output queries of each shape; at batch 3 and 96 again under
      every debug-hook value the tests use (TUNINGS, BLOCKS below).  The fill thresholds among them only bite on launches
      of a few blocks, so the small shapes of the tests that set them (ENC_SMALL) run under every hook value too;
    generator layers (same-resolution, ToRGB-fused, split-output, image, two-pass and one-kernel upsampling, small-plane):
      batch 1, 3, 8, 32 x nterms as called and flipped x (as called, without modulation, as a 64 -> 32 channel layer,
      the one-kernel upsampling conv on register-staged input); at batch 1 and 8 again under every forced tile
      configuration and every hook value."""
    header = open(os.path.join(root, "include", "hairfast_hip.h")).read()
    names = {m.group(1): [p.split()[-1].lstrip("*") for p in m.group(2).split(",")]
             for m in re.finditer(r"^(?:int|long long) (hf_\w+)\(([^;{]*)\);", header, re.M)}
    assert all(n in names for n in SWEPT), [n for n in SWEPT if n not in names]
    dummy = (ctypes.c_float * 4096)()

    def issue(name, vals, **change):
        fn = getattr(lib, name)
        v = dict(zip(names[name], vals))
        v.update({k: c for k, c in change.items() if k in v})
        if "workspace_floats" in v:
            v["workspace"], v["workspace_floats"] = True, 1 << 40
        real = [(dummy if t is not ctypes.c_void_p else ctypes.addressof(dummy)) if x is True else (None if x is False else x)
                for t, x in zip(getattr(lib._real, name).argtypes, v.values())]
        fn(*real)
        return v

    # hf_debug_set_tuning / hf_debug_set_persistent_blocks values of tests/test_sim_encoders.py, test_sim_kernels.py,
    # test_sim_gemm.py, test_gpu_parity.py, test_gpu_encoders.py (bits 24-31: the block count that fills "the chip")
    TUNINGS = (2, 4, 8, 16, 1 << 8, (1 << 8) | 8, 1 << 24, (1 << 24) | 2, 3 << 24, 4 << 24, (4 << 24) | 2, 5 << 24, 6 << 24, 10 << 24,
               13 << 24, (13 << 24) | (1 << 8), 18 << 24, 26 << 24)
    BLOCKS = (1, 3, 4, 5, 7, 64)
    # (batch, cin, cout, h, w, stride, groups) of test_conv2d_f16_stride2_multi_tile_form and the persistent-form test
    ENC_SMALL = ((2, 48, 64, 40, 72, 2, 1), (1, 32, 128, 64, 64, 2, 2), (2, 32, 128, 24, 72, 1, 1), (2, 16, 64, 32, 32, 1, 3),
                 (2, 32, 64, 40, 40, 2, 1), (5, 16, 64, 16, 32, 1, 1))
    enc = [(k[0], c) for k, c in lib.calls.items() if k[0] in ENC]
    gen = [(k[0], c) for k, c in lib.calls.items() if k[0] in GEN]

    def enc_pass(batches, nterms_list, pres, queries):
        for name, c in enc:
            for batch in batches:
                for nterms in nterms_list:
                    for pre in pres:
                        ch = {} if pre is None else dict(x=not pre, x_hi=pre, x_lo=pre)
                        if pre:
                            ch.update(in_scale=False, in_shift=False)
                        v = issue(name, c, batch=batch, nterms=nterms, **ch)
                        if queries and name != "hf_conv1x1_f16_f32":
                            lib.hf_conv2d_f16_split_output_ok(batch, v["cin"], v["cout"], v["h"], v["w"], v["stride"], nterms, int(bool(v["x_hi"])))
                if queries:
                    q = lib.hf_conv1x1_f16_workspace_floats if name == "hf_conv1x1_f16_f32" else lib.hf_conv2d_f16_workspace_floats
                    q(batch, *(dict(zip(names[name], c))[k] for k in ("cin", "cout", "h", "w", "stride")), dict(zip(names[name], c)).get("groups", 1))

    def enc_small_pass():
        like = [c for name, c in enc if name == "hf_conv2d_f16_f32"]
        for batch, cin, cout, h, w, stride, groups in ENC_SMALL if like else ():
            for nterms in (3, 1):
                for pre in (True, False):
                    issue("hf_conv2d_f16_f32", like[0], batch=batch, cin=cin, cout=cout, h=h, w=w, stride=stride, groups=groups,
                          x_group_stride=batch * cin * h * w if groups > 1 else 0, nterms=nterms, x=not pre, x_hi=pre, x_lo=pre,
                          in_scale=False, in_shift=False, residual=True)

    def gen_variants(name, v):
        yield {}
        if v.get("s") is True:
            yield dict(s=False)  # no modulation: the kernels without the s table
        if (v["cin"], v["cout"]) != (64, 32):
            yield dict(cin=64, cout=32)  # cout % 64 != 0: the 32-channel forms (53 / 55 / 63)
        if name == "hf_modconv3x3_up_blur_f16_f32" and v["x_hi"]:
            yield dict(x=True, x_hi=False, x_lo=False, s=True)  # register-staged input

    def gen_pass(batches, flip=True):
        for name, c in gen:
            v = dict(zip(names[name], c))
            for batch in batches:
                for var in gen_variants(name, v):
                    issue(name, c, batch=batch, **var)
                    if flip and "nterms" in v:
                        issue(name, c, batch=batch, nterms=4 - v["nterms"], **var)
                    elif flip:  # the one-kernel upsampling conv: nterms 1 = no lo parts
                        lo = not v["wt_lo"]
                        issue(name, c, batch=batch, **{**var, "wt_lo": lo, "x_lo": lo and var.get("x_hi", v["x_hi"]), "split_lo": lo and v["split_hi"]})

    for bi in (0, 1):
        print("# sweep batch_invariant", bi, file=out, flush=True)
        lib.hf_set_batch_invariant(bi)
        enc_pass((3, 96), (1, 3), (False, True), True)
        gen_pass((1, 3, 8, 32))
    lib.hf_set_batch_invariant(0)
    for tune in (0,) + TUNINGS:
        lib.hf_debug_set_tuning(tune)
        for bi in (0, 1):
            lib.hf_set_batch_invariant(bi)
            enc_small_pass()
            if tune:
                enc_pass((3, 96), (3,), (None,), False)
        lib.hf_set_batch_invariant(0)
        if tune:
            gen_pass((1, 8))
    for blocks in BLOCKS:
        lib.hf_debug_set_persistent_blocks(blocks)
        for tune in (0, 8, 1 << 8, (1 << 8) | 8):
            lib.hf_debug_set_tuning(tune)
            enc_small_pass()
            if tune == 0:
                enc_pass((3, 96), (3,), (None,), False)
            if tune in (0, 8):
                gen_pass((1, 8))
    lib.hf_debug_set_tuning(0)
    lib.hf_debug_set_persistent_blocks(0)
    for same, up in [(c, 0) for c in (51, 52, 53, 54, 55, 56)] + [(0, 61), (0, 63)]:
        lib.hf_debug_set_dispatch(same, up)
        gen_pass((1, 8))
    lib.hf_debug_set_dispatch(0, 0)


if args.plan:
    mark("# sweep")
    sweep(_lib._LIB)
    # kernel offsets -> names: the internal-linkage instantiations appear in the symbol table with their template arguments
    so = os.path.join(root, "tests", "hipsim", "libhairfast_sim.so")
    syms = {}
    # (a demangler that does not know _Float16 leaves those names mangled: the values are as plain there - ILi3ELi1ELb0E...)
    for line in subprocess.run([os.environ.get("NM", "nm"), "-C", "--defined-only", so], check=True, capture_output=True,
                               text=True).stdout.splitlines():
        addr, kind, name = line.split(" ", 2)
        if kind in "tTwW":
            syms.setdefault(int(addr, 16), name)
    text = re.sub(r"@([0-9a-f]+)", lambda m: syms.get(int(m.group(1), 16), m.group(0)), open(args.plan).read())
    open(args.plan, "w").write(text)
if not args.dry:
    torch.cuda.synchronize()
out.close()
