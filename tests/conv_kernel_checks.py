"""TEST INFRASTRUCTURE - the checks of the generator's convolution kernels (csrc/modconv.hip, convh.hip, convrow.hip), one
statement of each property, shared by the hipsim tests (tests/test_sim_kernels.py) and the GPU tests
(tests/test_gpu_parity.py).  Built like tests/generator_ops_checks.py; the rules of tests/small_ops_checks.py are imported
(Case, _sync, exact), not copied.  The conv kernels are held against each other and the oracle at the bounds their tests
had, which the accuracy rule (a yardstick of ATen's own error) does not state: it is not used here.  Every check takes
(lib, st, dev, case).

Inputs come from torch.manual_seed on the CPU and are copied to the device: a case has the same numbers on both devices.
styled_layer() is the one statement of a styled layer's operands (also for generator_ops_checks.py and up_rim_checks.py).

What differs per device is a parameter, not a second copy:
* tolerance against the oracle: TOL on the interpreter, REL (and the mean-square and RMS terms of the GPU suite's close()) on the
  GPU; where the twins of a check bounded the same quantity differently, each device keeps its bound (`per_device`);
* repetition: the interpreter is deterministic - one launch proves what it can; on the GPU a launch is repeated (`repeats`)
  and must return the same bits (an LDS slot handed over too early shows as a mismatch between launches);
* tile form: cfg None lets the dispatch choose and asserts that the path id is in the family's set; a cfg forces the form
  through hf_debug_set_dispatch and asserts 500 + cfg exactly.  The transposed conv has no forced forms (its form follows from
  cout alone): a cfg there is only asserted.

Case tables: CASES[op] = (the cases the interpreter ran before this module, the GPU's).  Every interpreter case also runs on the
GPU; a GPU case also runs on the interpreter when its MFMA work B*cin*cout*H*W is at most HALF that of the largest interpreter
case of the same table (size class 0; 2 = GPU only, as in small_ops_checks).  The cap at the full work admitted the 8M-work
shapes of f16_matrix_cores and presplit_input, 23 s of interpreter time on a file that takes about 115 s; at half, eight small
pipelined instantiations remain (about 1 s)."""
import contextlib
import math
import types

import pytest
import torch

from hairfastgan_amd import _marshal as M
from oracle import ref_stylegan2 as O
from tests.small_ops_checks import Case, _sync, exact

TOL = 2e-5   # interpreter: of max(1, |ref|max)
REL = 1e-4   # GPU: close() of tests/test_gpu_parity.py
SAME_FORMS, SAME_PRE_FORMS, UP_FORMS = (551, 552, 553, 555), (571, 572, 573, 575, 579), (561, 563)


def _gpu(dev):
    return dev.type == "cuda"


def per_device(dev, sim, gpu):
    return gpu if _gpu(dev) else sim


def repeats(dev, n):
    return n if _gpu(dev) else 1


@contextlib.contextmanager
def debug(lib, hook, *args):
    """hf_debug_set_<hook>(*args) for the body; cleared (all zero) afterwards, also when the body raises."""
    fn = getattr(lib, "hf_debug_set_" + hook)
    fn(*args)
    try:
        yield
    finally:
        fn(*[0] * len(args))


# --------------------------------------------------------------------------------------------------------------------
# operands, routes, references, comparisons
# --------------------------------------------------------------------------------------------------------------------
def styled_layer(lib, st, dev, shape, seed, up, rgb=False):
    """One styled 3x3 layer (B, cin, cout, H, W): .cpu holds the seeded CPU tensors (for the oracle); the namespace itself their
    device copies x, wgt, mw, mb, sty, nz (output resolution), nw, bias, the prepared wt, wsq, s, dm, the fp16 split hi, lo (None
    unless cin % 16 == 0) and the product's blur kernel k4; rgb: also a ToRGB's wrgb, mwr, mbr, styr, brgb, skip and wtr, sr."""
    B, cin, cout, H, W = shape
    torch.manual_seed(seed)
    r = torch.randn
    c = types.SimpleNamespace(x=r(B, cin, H, W), wgt=r(1, cout, cin, 3, 3), mw=r(cin, 16), mb=r(cin), sty=r(B, 16),
                              nz=r(B, 1, 2 * H, 2 * W) if up else r(B, 1, H, W), nw=torch.tensor([0.3]), bias=r(cout))
    if rgb:
        c.wrgb, c.mwr, c.mbr, c.styr, c.brgb, c.skip = r(1, 3, cout, 1, 1), r(cout, 16), r(cout), r(B, 16), r(3), r(B, 3, H // 2, W // 2)
    L = types.SimpleNamespace(cpu=c, shape=shape, up=up, **{k: v.to(dev) for k, v in vars(c).items()})
    L.wt, L.wsq = M.prepare_weights(lib, st, L.wgt)
    L.s = M.modulation(lib, st, L.sty, L.mw, L.mb)
    L.dm = M.demod(lib, st, L.s, L.wsq)
    L.hi, L.lo = M.split_weights_f16(lib, st, L.wt) if cin % 16 == 0 else (None, None)
    L.k4 = O.blur_kernel_1d_to_2d(gain=4.0).to(dev)
    if rgb:
        L.wtr = M.prepare_weights(lib, st, L.wrgb)[0]
        L.sr = M.modulation(lib, st, L.styr, L.mwr, L.mbr)
    return L


def tail(L, on=True):
    return (L.nz, L.nw, L.bias) if on else (None, None, None)


def conv_f32(lib, st, L, with_tail=True):
    """The exact-fp32 MFMA kernel (csrc/modconv.hip) of the layer."""
    if L.up:
        return M.modconv3x3_up(lib, st, L.x, L.wt, L.s, L.dm, L.k4, *tail(L, with_tail))
    return M.modconv3x3(lib, st, L.x, L.wt, L.s, L.dm, *tail(L, with_tail))


def conv_f16(lib, st, L, nterms=3):
    """csrc/convh.hip on fp32 input: same resolution, or the two-pass upsampling conv."""
    if L.up:
        return M.modconv3x3_up(lib, st, L.x, L.wt, L.s, L.dm, L.k4, *tail(L), f16=(L.hi, L.lo, nterms))
    return M.modconv3x3_f16(lib, st, L.x, L.hi, L.lo, nterms, L.s, L.dm, *tail(L))


def presplit(L, x=None, lo=True):
    xh, xl = M.split_activation_reference(L.x if x is None else x, L.s)
    return M.SplitActivation(xh, xl if lo else None, None)


def oracle(L, with_tail=True):
    c = L.cpu
    y = O.modulated_conv2d(c.x, c.sty, c.wgt, c.mw, c.mb, True, L.up)
    return O.fused_leaky_relu(y + c.nw * c.nz, c.bias) if with_tail else y


def within(what, y, ref, tol, *also):
    """max |y - ref| < tol * max(1, |ref|max); `also`: further tensors whose maximum caps the scale (a bound that one twin
    stated on the kernel reference's scale and the other on the oracle's is held on the smaller of the two)."""
    _sync(y.device)
    y, ref = y.detach().cpu().double(), ref.detach().cpu().double()
    assert y.shape == ref.shape, (what, tuple(y.shape), tuple(ref.shape))
    err = float((y - ref).abs().max())
    scale = max(1.0, min(float(t.abs().max()) for t in (ref,) + also))
    print(f"conv_kernels {what}: max-abs {err:.2e}, bound {tol * scale:.2e}")
    assert err < tol * scale, (what, err, tol * scale)
    return y, ref, err, scale


def close(dev, what, y, ref):
    """Against the oracle: TOL on the interpreter, REL on the GPU; the mean-square and relative-RMS terms on both."""
    y, ref, err, scale = within(what, y, ref, per_device(dev, TOL, REL))
    mse = float(((y - ref) ** 2).mean())
    assert mse <= 1e-8 * max(1.0, float(ref.var())), (what, mse)
    rms_ref = float((ref ** 2).mean()) ** 0.5
    assert rms_ref <= 1e-6 or mse ** 0.5 <= 0.3 * REL * rms_ref, (what, mse ** 0.5 / rms_ref)


def same_bits(what, got, want):
    """exact() for tensors and for SplitActivations (a missing lo part must be missing on both sides)."""
    if isinstance(want, M.SplitActivation):
        exact("conv_kernels", what + " hi", got.hi, want.hi)
        assert (got.lo is None) == (want.lo is None), what
        if want.lo is not None:
            exact("conv_kernels", what + " lo", got.lo, want.lo)
    else:
        exact("conv_kernels", what, got, want)


def path_is(lib, cfg, base, family):
    path = lib.hf_debug_last_path()
    assert (path == base + cfg) if cfg else (path in family), (path, cfg, family)


# --------------------------------------------------------------------------------------------------------------------
# csrc/modconv.hip: the fp32 MFMA kernels
# --------------------------------------------------------------------------------------------------------------------
def check_tile_geometries(lib, st, dev, case):
    """Ragged / tiny / odd shapes: multi-image tiles (4x4), several tiles per plane with ragged edges, cout % 32 != 0,
    cout % 4 != 0, cin % 8 != 0, 1-pixel planes - same resolution and transposed, against the oracle."""
    (shape,) = case.args
    L = styled_layer(lib, st, dev, shape, 1, False)
    for up in (False, True):
        L.up = up
        close(dev, f"tile_geometries {case.label} up {L.up}", conv_f32(lib, st, L, False), oracle(L, False))


def check_pipelined(lib, st, dev, case):
    """Every instantiation of the double-buffered kernel (register-staged, DMA-staged, transposed) forced through
    hf_debug_set_dispatch on shapes with ragged tiles - and that the forced kernel really ran (no fall-back)."""
    shape, cfg = case.args
    L = styled_layer(lib, st, dev, shape, cfg, 20 <= cfg < 30)
    with debug(lib, "dispatch", 0 if L.up else cfg, cfg if L.up else 0):
        y = conv_f32(lib, st, L, False)
        assert lib.hf_debug_last_path() == 200 + cfg, "shape fell back from the pipelined kernel"
    close(dev, f"pipelined {case.label}", y, oracle(L, False))


# --------------------------------------------------------------------------------------------------------------------
# csrc/convh.hip: the fp16 matrix-core kernels
# --------------------------------------------------------------------------------------------------------------------
def _f16_vs_f32_and_oracle(lib, st, dev, what, L, y, nterms, tol):
    ref = conv_f32(lib, st, L)
    within(what + " vs fp32 kernel", y, ref, tol)
    if L.shape[1] <= 64:  # the oracle runs on the host
        full = oracle(L)
        within(what + " vs oracle", y, full, per_device(dev, TOL, 1e-5) if nterms == 3 else tol, ref)


def check_f16_matrix_cores(lib, st, dev, case):
    """Split (hi, lo) fp16 operands reproduce the exact-fp32 kernel to fp32-class accuracy, plain fp16 operands to operand
    rounding; odd chunk counts, ragged rows / columns, noise + bias + lrelu epilogue; and the weight split itself round-trips."""
    shape, cfg, nterms, tol = case.args
    L = styled_layer(lib, st, dev, shape, 7, False)
    # hi + lo carries 2^k * weight (k: power-of-two pre-scale putting max|w| at 2^13) to 2^-22 relative of the LARGEST
    # weight - and, because of the pre-scale, of every weight above 2^-15 of it
    unscale = M.split_weights_unscale(L.hi)
    _sync(dev)
    wt = L.wt.cpu()
    assert 2 ** 13 <= float(wt.abs().max()) / unscale < 2 ** 14 and math.log2(unscale) == round(math.log2(unscale))
    back = (L.hi.cpu().float() + L.lo.cpu().float()).permute(1, 0, 2, 4, 3).reshape(wt.shape) * unscale
    assert float((back - wt).abs().max()) < 3e-7 * float(wt.abs().max())
    rel = ((back.double() - wt.double()).abs() / wt.double().abs().clamp_min(1e-30))[wt.abs() > 2.0 ** -14 * wt.abs().max()]
    assert float(rel.max()) < 2.0 ** -21
    with debug(lib, "dispatch", cfg or 0, 0):
        y = conv_f16(lib, st, L, nterms)
        path_is(lib, cfg, 500, SAME_FORMS)
    _f16_vs_f32_and_oracle(lib, st, dev, f"f16_matrix_cores {case.label}", L, y, nterms, tol)


def check_up_f16_matrix_cores(lib, st, dev, case):
    """Transposed conv: interior tiles plus the rim row / column, + blur + noise + bias + lrelu, against the exact-fp32
    path and the oracle."""
    shape, cfg, nterms, tol = case.args
    L = styled_layer(lib, st, dev, shape, 11, True)
    assert M.modconv3x3_up_f16_supported(*shape[1:])
    y = conv_f16(lib, st, L, nterms)
    path_is(lib, cfg, 500, UP_FORMS)
    _f16_vs_f32_and_oracle(lib, st, dev, f"up_f16_matrix_cores {case.label}", L, y, nterms, tol)


def check_persistent_tile_walk(lib, st, dev, case):
    """Resident blocks walking several tiles as one pipeline: hand-over across rows, images (the second s slot) and - transposed -
    the rim, block counts that do not divide the tile count (0 = the chip's): the exact-fp32 kernel's result at 5e-6 and the
    oracle's for any block count.  GPU: four launches, equal bits (no LDS slot races between waves)."""
    shape, up, blocks = case.args
    L = styled_layer(lib, st, dev, shape, 5, up)
    ref, full = conv_f32(lib, st, L), oracle(L)
    with debug(lib, "persistent_blocks", blocks):
        first = None
        for i in range(repeats(dev, 4)):
            y = conv_f16(lib, st, L)
            within(f"persistent_tile_walk {case.label} launch {i}", y, ref, 5e-6)
            first = y.clone() if first is None else first
            same_bits("persistent_tile_walk repeat", y, first)
    within(f"persistent_tile_walk {case.label} vs oracle", y, full, TOL)


def check_fused_torgb(lib, st, dev, case):
    """ToRGB's 1x1 modulated conv in the conv epilogue (hf_modconv3x3_f16_rgb_f32) + the finishing pass (bias + upsampled skip
    through hf_torgb_f32 with identity weights) == conv then ToRGB; the conv output itself is unchanged bit for bit."""
    (shape,) = case.args
    B, cin, cout, H, W = shape
    L = styled_layer(lib, st, dev, shape, 9, False, rgb=True)
    assert M.modconv3x3_f16_supported(cin, cout, H, W) and cout % 32 == 0  # what the kernel takes (torgb_fusable: the policy)
    y, raw = M.modconv3x3_f16(lib, st, L.x, L.hi, L.lo, 3, L.s, L.dm, *tail(L), rgb=(L.wtr, L.sr))
    same_bits("fused_torgb conv output", y, conv_f16(lib, st, L))
    slabs = M.torgb_slabs(cout)  # one partial sum per 64 (32) output channels, added by the finishing pass
    assert raw.shape == (B, 3 * slabs, H, W)
    eye = torch.eye(3).repeat(slabs, 1).reshape(1, 3 * slabs, 3).to(dev)
    rgb = M.torgb(lib, st, raw, eye, None, L.brgb, L.skip, L.k4)
    within(f"fused_torgb {case.label}", rgb, M.torgb(lib, st, y, L.wtr, L.sr, L.brgb, L.skip, L.k4), 2e-5)


def _blur_pair(lib, st, dev, L):
    """hf_blur_noise_bias_act_f32 and its split form on one random intermediate: (fp32 activation, SplitActivation for L.s)."""
    B, cin, _, H, W = L.shape
    pitch = lib.hf_modconv_up_pitch(W // 2)
    tmp, nz, nw, b = (t.to(dev) for t in (torch.randn(B, cin, H + 1, pitch), torch.randn(B, 1, H, W), torch.tensor([0.2]), torch.randn(cin)))
    x, act = torch.empty(B, cin, H, W, device=dev), M.SplitActivation.empty(B, cin, H, W, dev)
    args = (tmp.data_ptr(), L.k4.data_ptr(), nz.data_ptr(), nw.data_ptr(), H * W, b.data_ptr())
    M.check(lib, lib.hf_blur_noise_bias_act_f32(x.data_ptr(), *args, B, cin, H + 1, W + 1, pitch, 0.2, 2 ** 0.5, st), "blur")
    M.check(lib, lib.hf_blur_noise_bias_act_split_f16(act.hi.data_ptr(), act.lo.data_ptr(), *args, L.s.data_ptr(), B, cin, H + 1, W + 1,
                                                      pitch, 0.2, 2 ** 0.5, st), "blur split")
    _sync(dev)
    same_bits("presplit: blur's split output", act, presplit(L, x))
    return x, act


def check_presplit_input(lib, st, dev, case):
    """Pre-split, K-blocked activations staged by LDS-DMA (hf_modconv3x3_f16_pre_f32) give the bit-identical result of the
    kernel that loads fp32 activations and splits them itself: ragged planes (zero-filled halo), odd chunk counts, every tile
    shape (forms 51 / 52 forced, 53 chosen).  producer: the activation comes from the blur pass, fp32 and split (H, W even).
    GPU: three launches."""
    shape, cfg, nterms, producer = case.args
    L = styled_layer(lib, st, dev, shape, 17, False)
    x, act = _blur_pair(lib, st, dev, L) if producer else (L.x, presplit(L))
    with debug(lib, "dispatch", cfg if cfg in (51, 52) else 0, 0):
        ref = M.modconv3x3_f16(lib, st, x, L.hi, L.lo, nterms, L.s, L.dm, *tail(L))
        for _ in range(repeats(dev, 3)):
            y = M.modconv3x3_f16_pre(lib, st, act, L.hi, L.lo, nterms, L.dm, *tail(L))
            path_is(lib, cfg, 520, SAME_PRE_FORMS)
            same_bits(f"presplit_input {case.label}", y, ref)


def check_presplit_chain(lib, st, dev, case):
    """Split output of the same-resolution epilogue (split_hi / lo) is the split of s_next * out bit for bit, and the transposed
    conv on it (hf_modconv3x3_up_f16_pre_f32, incl. the rim) equals the transposed conv that loads the fp32 activation."""
    ((B, cin, cup, H, W),) = case.args
    L1 = styled_layer(lib, st, dev, (B, cin, cin, H, W), 23, False)
    L2 = styled_layer(lib, st, dev, (B, cin, cup, H, W), 24, True)
    assert M.modconv3x3_f16_supported(cin, cin, H, W)
    act, f1 = presplit(L1), (L1.hi, L1.lo, 3, L1.dm) + tail(L1)
    out, nxt = M.modconv3x3_f16_pre(lib, st, act, *f1, split_for=L2.s)
    L2.x = out
    same_bits("presplit_chain split output", nxt, presplit(L2))
    only_split = M.modconv3x3_f16_pre(lib, st, act, *f1, split_for=L2.s, want_out=False)
    assert only_split[0] is None
    same_bits("presplit_chain split output alone", only_split[1].hi, nxt.hi)
    ref = conv_f16(lib, st, L2)
    y = M.modconv3x3_up(lib, st, nxt, L2.wt, None, L2.dm, L2.k4, *tail(L2), f16=(L2.hi, L2.lo, 3))
    assert lib.hf_debug_last_path() in (581, 583)
    same_bits(f"presplit_chain {case.label}", y, ref)


def check_f16_split_range(lib, st, dev, case):
    """f16x3 against the exact-fp32 kernel with styles / activations scaled by 1e+-2 ... 1e+-5: styles are normalised away
    exactly (hf_style_normalize_f32), weights are pre-scaled into the normal fp16 range; the error follows the model of
    include/hairfast_hip.h (2^-22 relative per operand, 2^-25 absolute once |s*x| < 2^-3); nothing clamps."""
    shape, sty_scale, x_scale = case.args
    L = styled_layer(lib, st, dev, shape, 3, False)
    L.x = L.x * x_scale
    M.f16_overflow_count(lib, reset=True)
    L.s = M.modulation(lib, st, L.sty * sty_scale, L.mw, L.mb * sty_scale)
    L.dm = M.demod(lib, st, L.s, L.wsq)
    s0, d0 = L.s.clone(), L.dm.clone()
    M.style_normalize(lib, st, L.s, L.dm)
    assert 1.0 <= float(L.s.abs().amax(1).min()) and float(L.s.abs().amax(1).max()) < 2.0
    ref = conv_f32(lib, st, L, False)
    # exact power-of-two rescaling: the fp32 kernel returns the very same bits with either pair
    same_bits("f16_split_range normalised styles", ref, M.modconv3x3(lib, st, L.x, L.wt, s0, d0, None, None, None))
    y = M.modconv3x3_f16(lib, st, L.x, L.hi, L.lo, 3, L.s, L.dm, None, None, None)
    y_pre = M.modconv3x3_f16_pre(lib, st, presplit(L), L.hi, L.lo, 3, L.dm, None, None, None)  # the producer-side split
    _sync(dev)
    assert torch.isfinite(y).all() and torch.isfinite(y_pre).all()
    tol, scale = 5e-6 + 6e-8 / min(1.0, x_scale), float(ref.abs().max())
    for name, got in (("fp32 input", y), ("pre-split input", y_pre)):
        err = float((got - ref).abs().max())
        print(f"conv_kernels f16_split_range {case.label} {name}: {err / scale:.2e} of |ref|max, bound {tol:.2e}")
        assert err < tol * scale, (case.label, name, err / scale)
    assert M.f16_overflow_count(lib) == 0


def check_f16_split_saturates(lib, st, dev, case):
    """Activations beyond the fp16-pair range (|s*x| > 131008 after normalisation): both parts saturate - no inf / NaN - the
    clamp counter reports it and resets; the blur pass that writes a split activation saturates too."""
    shape, seed, x_scale = case.args
    L = styled_layer(lib, st, dev, shape, seed, True)
    M.style_normalize(lib, st, L.s, L.dm)
    L.x = L.x * x_scale
    M.f16_overflow_count(lib, reset=True)
    y = M.modconv3x3_f16(lib, st, L.x, L.hi, L.lo, 3, L.s, L.dm, None, None, None)
    assert torch.isfinite(y).all()
    assert M.f16_overflow_count(lib, reset=True) > 0
    assert M.f16_overflow_count(lib) == 0
    big = M.modconv3x3_up(lib, st, L.x, L.wt, L.s, L.dm, L.k4, None, None, None, f16=(L.hi, L.lo, 3), split_for=(None, L.s, True))
    assert torch.isfinite(big.hi.float()).all() and torch.isfinite(big.lo.float()).all()
    assert M.f16_overflow_count(lib, reset=True) > 0


# --------------------------------------------------------------------------------------------------------------------
# the upsampling StyledConv as one kernel (csrc/convh.hip FUSE)
# --------------------------------------------------------------------------------------------------------------------
def _fused(lib, st, L, x=None, nterms=3, **kw):
    pre = isinstance(x, M.SplitActivation)
    return M.modconv3x3_up_fused(lib, st, L.x if x is None else x, L.hi, L.lo if nterms == 3 else None, None if pre else L.s, L.dm,
                                 M.blur_factors(L.k4), *tail(L), nterms=nterms, **kw)


def check_up_fused_blur(lib, st, dev, case):
    """Transposed conv + 4x4 blur + noise + bias + lrelu in one kernel against the two-pass path (same MFMA products; the
    separable 4+4-tap blur only reassociates the 16-tap sum: 2e-6) and the oracle: fp32 and split output, fp32 and pre-split
    input, several tiles per dimension with ragged edges, two cout tiles.  GPU: a second launch returns the same bits."""
    (shape,) = case.args
    B, cin, cout, H, W = shape
    L = styled_layer(lib, st, dev, shape, 13, True)
    M.style_normalize(lib, st, L.s, L.dm)
    assert M.blur_factors(L.k4) is not None and M.blur_factors(torch.rand(4, 4)) is None
    assert M.modconv3x3_up_fused_supported(cin, cout, H, W)
    ref = conv_f16(lib, st, L)
    y = _fused(lib, st, L)
    assert lib.hf_debug_last_path() == 573
    within(f"up_fused_blur {case.label} vs two passes", y, ref, 2e-6)
    for _ in range(repeats(dev, 2) - 1):
        same_bits("up_fused_blur repeat", _fused(lib, st, L), y)
    if cin <= 64 and H * W <= 10000:  # the oracle runs on the host
        within(f"up_fused_blur {case.label} vs oracle", y, oracle(L), per_device(dev, TOL, 1e-5), ref)
    s2 = (torch.rand(B, cout) + 0.5).to(dev)
    want = types.SimpleNamespace(x=y, s=s2)
    same_bits("up_fused_blur split output", _fused(lib, st, L, split_for=s2), presplit(want))
    act = presplit(L)
    same_bits("up_fused_blur pre-split input, split output", _fused(lib, st, L, act, split_for=s2), presplit(want))
    assert lib.hf_debug_last_path() == 593
    same_bits("up_fused_blur pre-split input", _fused(lib, st, L, act), y)
    assert lib.hf_debug_last_path() == 593


def check_up_fused_blur_plain_fp16(lib, st, dev, case):
    """The one-kernel form with plain fp16 operands (nterms 1; wt_lo NULL at the C ABI): the two-pass fp16 path's products
    (operands rounded identically; the separable blur reassociates), the split output has a hi part only = fp16(s_next * out),
    the stage buffer is sized for the epilogue's exchange."""
    (shape,) = case.args
    L = styled_layer(lib, st, dev, shape, 3, True)
    M.style_normalize(lib, st, L.s, L.dm)
    ref = conv_f16(lib, st, L, 1)
    y = _fused(lib, st, L, nterms=1)
    within("up_fused_blur_plain_fp16 vs two passes", y, ref, 2e-6)
    within("up_fused_blur_plain_fp16 vs oracle", y, oracle(L), 2e-2)  # fp16 operands
    s2 = (torch.rand(shape[0], shape[2]) + 0.5).to(dev)
    act = presplit(L, lo=False)
    sp = _fused(lib, st, L, act, nterms=1, split_for=s2)
    assert sp.lo is None
    same_bits("up_fused_blur_plain_fp16 split output", sp, presplit(types.SimpleNamespace(x=_fused(lib, st, L, act, nterms=1), s=s2), lo=False))


def check_up_fused_blur_persistent(lib, st, dev, case):
    """The fused kernel under the resident-block tile walk: the LDS stage buffer that carries the vertical exchange is handed
    back to the next tile's DMA prefetch; several images (second parameter slot)."""
    shape, blocks = case.args
    L = styled_layer(lib, st, dev, shape, 77, True)
    ref = _fused(lib, st, L)
    with debug(lib, "persistent_blocks", blocks):
        same_bits("up_fused_blur_persistent", _fused(lib, st, L), ref)
        same_bits("up_fused_blur_persistent pre-split input", _fused(lib, st, L, presplit(L)), ref)
    within(f"up_fused_blur_persistent {case.label} vs oracle", ref, oracle(L), TOL)


# --------------------------------------------------------------------------------------------------------------------
# csrc/convrow.hip
# --------------------------------------------------------------------------------------------------------------------
def check_conv_rows(lib, st, dev, case):
    """32 -> 32 channels, pre-split input: the row pipeline (weights in registers, 18-slot LDS ring refilled by LDS-DMA) against
    the tiled kernel it replaces (hf_debug_set_tuning bit 4), bit for bit: fp32 output, fused ToRGB partial sums, the finished
    image (bias + x2-upsampled skip through a 16-row LDS ring of skip rows) against the raw product + the finishing launch, no
    noise, plain fp16 operands; strips at both image borders, several super-steps, ring wrap-around; against the exact-fp32
    kernel within the f16x3 tolerance.  GPU: three launches - a ring slot overwritten or read too early shows as a mismatch."""
    (shape,) = case.args
    L = styled_layer(lib, st, dev, shape, shape[3] + shape[4], False, rgb=True)
    rgb, eye = (L.wtr, L.sr), torch.eye(3).reshape(1, 3, 3).to(dev)
    pre = lambda act, nterms, **kw: M.modconv3x3_f16_pre(lib, st, act, L.hi, L.lo, nterms, L.dm, *tail(L), rgb=rgb, **kw)  # noqa: E731
    image = lambda act, nterms: M.modconv3x3_f16_pre_image(lib, st, act, L.hi, L.lo, nterms, L.dm, *tail(L), rgb, L.brgb, L.skip, L.k4)  # noqa: E731
    for nterms, act in ((3, presplit(L)), (1, presplit(L, lo=False))):
        with debug(lib, "tuning", 16):
            ref_out, ref_raw = pre(act, nterms)
            assert lib.hf_debug_last_path() in (573, 575)
            if nterms == 3:  # the tiled form asked for: the library declines, the caller keeps the two launches
                assert image(act, nterms) is None
        want_img = M.torgb(lib, st, ref_raw, eye, None, L.brgb, L.skip, L.k4)
        for _ in range(repeats(dev, 3)):
            out, raw = pre(act, nterms)
            assert lib.hf_debug_last_path() == 579
            same_bits(f"conv_rows nterms {nterms} out", out, ref_out)
            same_bits(f"conv_rows nterms {nterms} raw", raw, ref_raw)
            img = image(act, nterms)
            assert lib.hf_debug_last_path() == 579
            same_bits(f"conv_rows nterms {nterms} image", img, want_img)
        if nterms == 3:
            out3 = out
            same_bits("conv_rows raw alone", pre(act, 3, want_out=False)[1], ref_raw)
            plain = M.modconv3x3_f16_pre(lib, st, act, L.hi, L.lo, 3, L.dm, None, None, L.bias)
            assert lib.hf_debug_last_path() == 579
            same_bits("conv_rows no noise", plain, M.modconv3x3_f16(lib, st, L.x, L.hi, L.lo, 3, L.s, L.dm, None, None, L.bias))
            if shape[0] * shape[3] * shape[4] <= 1 << 20:
                within(f"conv_rows {case.label} vs fp32 kernel", out, conv_f32(lib, st, L), 2e-5)
    assert not torch.equal(out, out3)  # plain fp16 operands: other bits than f16x3


# --------------------------------------------------------------------------------------------------------------------
# the case tables.  A row is (id, shape, further arguments); the id is the one pytest gave the case before this module.
# --------------------------------------------------------------------------------------------------------------------
def _work(row):
    return math.prod(row[1])


def _table(sim, gpu):
    """(interpreter's cases, GPU's cases); a GPU case is of size class 0 (also on the interpreter) up to half the MFMA work of
    the interpreter's largest case, else 2."""
    cap = max(map(_work, sim)) // 2
    return [Case(r[0], r[1:], 0) for r in sim], [Case(r[0], r[1:], 0 if _work(r) <= cap else 2) for r in gpu]


def _each(rows, tails):
    """rows x tails, a tail being (id suffix, further arguments): two stacked parametrize decorators."""
    return [(r[0] + suffix,) + r[1:] + more for r in rows for suffix, more in tails]


NTERMS = [("-3-5e-06", (3, 5e-6)), ("-1-0.004", (1, 4e-3))]  # (nterms, bound against the exact-fp32 kernel)
_GEOM = [("4x4 planes", (3, 8, 8, 4, 4)), ("cin 12, cout 34", (1, 12, 34, 40, 72)), ("cout 33, 9x5", (2, 16, 33, 9, 5)),
         ("2x2 planes", (5, 8, 64, 2, 2)), ("1x1 plane", (1, 8, 8, 1, 1))]
_RANGE = [("100000.0-1.0", 1e5, 1.0), ("1e-05-1.0", 1e-5, 1.0), ("1.0-5000.0", 1.0, 5e3), ("1.0-0.01", 1.0, 1e-2),
          ("1.0-0.0001", 1.0, 1e-4), ("10000.0-5000.0", 1e4, 5e3)]
_WALK = (3, 64, 64, 64, 96)

CASES = {
    "tile_geometries": _table(
        _GEOM + [("70x1 plane", (2, 8, 40, 70, 1))],
        _GEOM + [("72x72", (2, 64, 128, 72, 72)), ("130x66", (1, 128, 64, 130, 66)), ("batch 9", (9, 32, 32, 32, 32)),
                 ("cin 40", (2, 40, 256, 16, 16))]),
    # (shape, instantiation)
    "pipelined": _table(
        [("11-shape0", (2, 16, 128, 16, 32), 11),   # 128 co x 256 px, 8 waves
         ("12-shape1", (1, 16, 64, 24, 40), 12),    # 64 co x 256 px, ragged plane
         ("13-shape2", (2, 8, 32, 16, 16), 13),     # 32 co x 256 px, 16-wide rows
         ("14-shape3", (1, 16, 128, 8, 32), 14), ("15-shape4", (2, 8, 64, 8, 8), 15), ("16-shape5", (1, 8, 32, 32, 32), 16),
         ("31-shape6", (2, 16, 128, 16, 32), 31),   # DMA-staged variants (rows of 32 pixels)
         ("32-shape7", (1, 16, 64, 24, 64), 32), ("33-shape8", (2, 8, 32, 8, 96), 33),
         ("34-shape9", (1, 16, 128, 12, 32), 34),   # ragged: 12 rows with 4-row tiles
         ("21-shape10", (2, 16, 64, 8, 32), 21),    # up: 64 co x 128 px x 4 phases (+ rim launch)
         ("22-shape11", (1, 8, 32, 16, 32), 22), ("23-shape12", (1, 8, 64, 6, 40), 23), ("24-shape13", (1, 8, 64, 16, 32), 24),
         ("25-shape14", (2, 8, 32, 4, 32), 25)],
        [("11-shape0", (2, 64, 128, 40, 64), 11), ("12-shape1", (1, 32, 64, 24, 40), 12), ("13-shape2", (2, 16, 32, 48, 96), 13),
         ("14-shape3", (1, 32, 128, 8, 32), 14), ("15-shape4", (2, 16, 64, 8, 8), 15), ("16-shape5", (1, 16, 32, 32, 64), 16),
         ("31-shape6", (2, 64, 128, 40, 64), 31), ("32-shape7", (1, 32, 64, 24, 64), 32), ("33-shape8", (2, 16, 32, 44, 96), 33),
         ("34-shape9", (1, 32, 128, 12, 32), 34), ("21-shape10", (2, 32, 64, 8, 32), 21), ("22-shape11", (1, 16, 32, 16, 32), 22),
         ("23-shape12", (1, 16, 64, 6, 40), 23), ("24-shape13", (1, 32, 64, 16, 32), 24), ("25-shape14", (2, 16, 32, 4, 32), 25)]),
    # (shape, tile form, nterms, bound)
    "f16_matrix_cores": _table(
        _each([("51-shape0", (2, 32, 64, 8, 32), 51), ("51-shape1", (1, 48, 128, 20, 70), 51), ("52-shape2", (1, 48, 64, 20, 40), 52),
               ("53-shape3", (1, 16, 32, 16, 64), 53)], NTERMS),
        _each([("shape0", (2, 64, 64, 32, 32), None), ("shape1", (1, 48, 128, 20, 70), None), ("shape2", (2, 512, 512, 64, 64), None),
               ("shape3", (1, 32, 32, 100, 64), None)], NTERMS)),
    "up_f16_matrix_cores": _table(
        _each([("61-shape0", (1, 32, 64, 16, 16), 61), ("61-shape1", (2, 16, 64, 9, 40), 61), ("63-shape2", (1, 16, 32, 16, 32), 63)],
              NTERMS),
        _each([("shape0", (2, 64, 64, 16, 16), None), ("shape1", (1, 48, 128, 20, 70), None), ("shape2", (2, 512, 256, 64, 64), None),
               ("shape3", (1, 64, 32, 40, 64), None)], NTERMS)),
    # (shape, up, resident blocks)
    "persistent_tile_walk": _table(
        [("1-False", (3, 32, 64, 16, 32), False, 1), ("1-True", (2, 32, 64, 16, 32), True, 1),
         ("3-False", (3, 32, 64, 16, 32), False, 3), ("3-True", (2, 32, 64, 16, 32), True, 3),
         ("5-False", (3, 32, 64, 16, 32), False, 5), ("5-True", (2, 32, 64, 16, 32), True, 5)],
        [("0-shape0-False", _WALK, False, 0), ("0-shape0-True", _WALK, True, 0), ("7-shape1-False", _WALK, False, 7),
         ("7-shape1-True", _WALK, True, 7), ("64-shape2-False", _WALK, False, 64), ("64-shape2-True", _WALK, True, 64),
         ("4-shape3-False", (9, 32, 64, 16, 32), False, 4), ("4-shape3-True", (9, 32, 64, 16, 32), True, 4)]),  # 4: a new image per step
    "fused_torgb": _table(
        [("shape0", (2, 32, 64, 16, 32)), ("shape1", (1, 16, 32, 20, 40)), ("shape2", (1, 32, 128, 16, 32)), ("shape3", (1, 16, 96, 16, 32))],
        [("shape0", (2, 64, 64, 64, 64)), ("shape1", (1, 32, 32, 96, 128)), ("shape2", (2, 256, 256, 64, 64)), ("shape3", (1, 64, 96, 32, 64))]),
    # (shape, tile form, nterms, activation from the blur pass)
    "presplit_input": _table(
        _each([("51-shape0", (2, 32, 64, 8, 32), 51), ("51-shape1", (1, 48, 128, 20, 70), 51), ("52-shape2", (1, 48, 64, 20, 40), 52),
               ("53-shape3", (1, 16, 32, 16, 64), 53)], [("-3", (3, False)), ("-1", (1, False))]),
        [("shape0", (2, 64, 64, 32, 32), None, 3, True), ("shape1", (1, 48, 128, 20, 70), None, 3, True),
         ("shape2", (2, 512, 512, 64, 64), None, 3, True), ("shape3", (1, 32, 32, 100, 128), None, 3, True),
         ("shape4", (9, 32, 64, 16, 32), None, 3, True)]),
    "presplit_chain": _table([("shape0", (2, 64, 64, 8, 32)), ("shape1", (1, 32, 32, 16, 32)), ("shape2", (2, 64, 32, 20, 40))], []),
    # (shape, style scale, activation scale)
    "f16_split_range": _table(
        [(i, (1, 32, 64, 8, 32), a, b) for i, a, b in _RANGE],
        [(i, (2, 128, 128, 64, 64), a, b) for i, a, b in _RANGE + [("1000.0-1000.0", 1e3, 1e3), ("0.001-0.001", 1e-3, 1e-3)]]),
    # (shape, seed, activation scale)
    "f16_split_saturates": _table([("1x32x64x8x32", (1, 32, 64, 8, 32), 3, 4e4)], [("1x64x64x32x32", (1, 64, 64, 32, 32), 5, 2e5)]),
    "up_fused_blur": _table(
        [("1-16-32-16-32", (1, 16, 32, 16, 32)), ("2-32-32-20-45", (2, 32, 32, 20, 45)), ("1-16-64-30-61", (1, 16, 64, 30, 61))],
        [("shape0", (2, 64, 32, 512, 512)), ("shape1", (2, 128, 64, 256, 256)), ("shape2", (1, 256, 128, 128, 128)),
         ("shape3", (3, 32, 32, 75, 100)), ("shape4", (1, 512, 256, 64, 64))]),
    "up_fused_blur_plain_fp16": _table([("2x32x32x20x45", (2, 32, 32, 20, 45))], []),
    # (shape, resident blocks)
    "up_fused_blur_persistent": _table([("1", (3, 32, 32, 30, 40), 1), ("3", (3, 32, 32, 30, 40), 3)], []),
    "conv_rows": _table(
        [("1-16-64", (1, 32, 32, 16, 64)), ("2-40-128", (2, 32, 32, 40, 128)), ("1-64-192", (1, 32, 32, 64, 192))],
        [("8-1024-1024", (8, 32, 32, 1024, 1024)), ("1-1024-1024", (1, 32, 32, 1024, 1024)), ("3-256-192", (3, 32, 32, 256, 192))]),
}
CHECKS = {op: globals()["check_" + op] for op in CASES}


def cases(op, gpu):
    """The op's cases on one device: those it ran there before this module, under their ids, then the other device's."""
    sim, hw = CASES[op]
    home, guests, tag = (hw, sim, "sim_") if gpu else (sim, [c for c in hw if c.size < 2], "gpu_")
    seen = {c.args for c in home}
    return home + [Case(tag + c.label, c.args, c.size) for c in guests if c.args not in seen]


def params(op, gpu):
    return [pytest.param(c, id=c.label) for c in cases(op, gpu)]


def run_all(op, lib, st, dev):
    """For the tests that were never parametrised: every case of the device in one test."""
    for c in cases(op, _gpu(dev)):
        CHECKS[op](lib, st, dev, c)
