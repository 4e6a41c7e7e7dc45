"""TEST INFRASTRUCTURE - direct checks of the 1x1-conv GEMM on the fp16 matrix cores (csrc/gemm_h.hip, hf_conv1x1_f16_f32),
shared by the hipsim tests (tests/test_sim_gemm.py) and the GPU tests (tests/test_gpu_gemm.py).  Built like
tests/generator_ops_checks.py: every check takes (lib, st, dev, case); the rules of tests/small_ops_checks.py (accuracy, exact,
sentinels, batch invariance) are imported, not copied.

Reference: the contract at the head of gemm_h.hip restated in torch fp64 on the CPU -
    y = act( out_scale * sum_ci W[co,ci] * (in_scale*x + in_shift)[source pixel] + bias (+ residual) ) (+ residual)
Inputs come from torch.manual_seed on the CPU; what is summed carries a DC offset (x = randn + 3, w = (randn + 0.5) / sqrt(cin)):
a dropped or double-counted term moves a result by about 1/K of full scale.

Accuracy rule (accuracy_f16), per element.  With xh = the affine-transformed input in fp64,
    A = |out_scale| * (|W| . |xh|),   S = |out_scale| * sum_ci |W|,
    |y - ref64| <= Lip * (c * A + 2^-25 * S) + FACTOR * E_t + 4 * 2^-23 * max |ref64|.
c: f16x3 operands are carried as hi + lo with relative error <= 2^-22 each and the lo*lo product (<= 2^-22 relative) is not
formed: c = 3 * 2^-22 (the model of include/hairfast_hip.h); nterms 1: both operands rounded to fp16, c = 2 * 2^-11.
2^-25 * S: the fp16 subnormal floor of an activation's lo part.  Lip: the activation's Lipschitz constant - 1 for none, LReLU
and PReLU with slopes <= 1; QuickGELU's is computed below.  E_t: ATen fp32 on the CPU against ref64, the yardstick of
small_ops_checks.accuracy, whose FACTOR and last term these are."""
import contextlib

import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from tests.conv_kernel_checks import per_device
from tests.small_ops_checks import ROWS, Case, _c, _guard_ok, _guarded, _offset_view, _sync, accuracy, exact, invariant  # noqa: F401

C_F16X3 = 3 * 2.0 ** -22
C_F16 = 2 * 2.0 ** -11
LO_FLOOR = 2.0 ** -25
OPERAND_ROWS = []            # (label, largest per-element E_k / (2^-22 * A)) of this process's f16x3 cases, in run order


def _qgelu_lipschitz():
    """max |d/dv (v * sigmoid(1.702 v))| on a grid of step 1e-5 over [-12, 12] (the derivative tends to 0 and 1 outside)."""
    v = torch.linspace(-12.0, 12.0, 2400001, dtype=torch.float64)
    s = torch.sigmoid(1.702 * v)
    return float((s + 1.702 * v * s * (1.0 - s)).abs().max())


LIP_QGELU = _qgelu_lipschitz()
ACTS = {"none": M.ACT_NONE, "lrelu": M.ACT_LRELU, "prelu": M.ACT_PRELU, "qgelu": M.ACT_QGELU}


def lipschitz(act):
    return LIP_QGELU if act == "qgelu" else 1.0


def restated(x, w, o, stride=1, act="none", alpha=0.0, res_first=False):
    """The contract in x's dtype.  x [B,cin,H,W], w [cout,cin]; o: the optional operands isc, ish, osc, bias, slope, res."""
    cv = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    xh = x
    if o.get("isc") is not None:
        xh = xh * cv(o["isc"])
    if o.get("ish") is not None:
        xh = xh + cv(o["ish"])
    v = F.conv2d(xh[:, :, ::stride, ::stride], w[:, :, None, None])
    if o.get("osc") is not None:
        v = v * cv(o["osc"])
    if o.get("bias") is not None:
        v = v + cv(o["bias"])
    res = o.get("res")
    if res is not None and res_first:
        v = v + res
    if act == "lrelu":
        v = F.leaky_relu(v, alpha)
    elif act == "prelu":
        v = torch.where(v > 0, v, v * cv(o["slope"]))
    elif act == "qgelu":
        v = v * torch.sigmoid(1.702 * v)
    return v + res if res is not None and not res_first else v


def operand_sums(x, w, o, stride=1):
    """(A, S) of the rule, fp64, in the output's shape."""
    d = {k: (None if v is None else v.double()) for k, v in o.items()}
    xh = x.double()
    if d.get("isc") is not None:
        xh = xh * d["isc"].view(1, -1, 1, 1)
    if d.get("ish") is not None:
        xh = xh + d["ish"].view(1, -1, 1, 1)
    a = F.conv2d(xh[:, :, ::stride, ::stride].abs(), w.double().abs()[:, :, None, None])
    s = w.double().abs().sum(1).view(1, -1, 1, 1).expand_as(a)
    if d.get("osc") is not None:
        a, s = a * d["osc"].abs().view(1, -1, 1, 1), s * d["osc"].abs().view(1, -1, 1, 1)
    return a, s


def accuracy_f16(op, label, got, x, w, o, stride=1, act="none", alpha=0.0, res_first=False, nterms=3, channels=None):
    """got against the fp64 contract under the rule above; channels: the output channels got holds (a slice of w's rows)."""
    if channels is not None:
        w = w[channels]
        o = {k: (v if v is None or k in ("isc", "ish") else v[:, channels] if k == "res" else v[channels]) for k, v in o.items()}
    d = {k: (None if v is None else v.double()) for k, v in o.items()}
    ref64 = restated(x.double(), w.double(), d, stride, act, alpha, res_first)
    t32 = restated(x, w, o, stride, act, alpha, res_first)
    a, s = operand_sums(x, w, o, stride)
    c = C_F16X3 if nterms == 3 else C_F16
    accuracy(op, label, got, ref64, t32, extra=lipschitz(act) * (c * a + LO_FLOOR * s), tag="gemm")
    if nterms == 3:
        r = float(((got.detach().cpu().double() - ref64).abs() / (2.0 ** -22 * a)).max())
        OPERAND_ROWS.append((f"{op} {label}", r))
        print(f"gemm {op} {label}: largest E_k / (2^-22 A) {r:.2f}")
    return ref64


# --------------------------------------------------------------------------------------------------------------------
# operands and launches
# --------------------------------------------------------------------------------------------------------------------
def prep(lib, st, w):
    """conv weight [cout, cin] (or grouped [G, cout, cin]) on the device -> (hi, lo) blobs."""
    if w.ndim == 3:
        wt = torch.stack([M.conv_prepare(lib, st, wg[:, :, None, None]) for wg in w])
    else:
        wt = M.conv_prepare(lib, st, w[:, :, None, None])
    return M.conv_split_weights_f16(lib, st, wt)


def layer(seed, B, cin, cout, H, W, stride=1, affine=False, osc=False, bias=False, act="none", res=False, zero_mean=False, groups=0,
          shared=True):
    """Seeded CPU operands of one launch: x, w and the dict o of optional ones (None where absent).  groups: w, bias [G, ...]
    and, unless shared, x [G, B, cin, H, W]."""
    torch.manual_seed(seed)
    dc_x, dc_w = (0.0, 0.0) if zero_mean else (3.0, 0.5)
    g = (groups,) if groups else ()
    x = torch.randn(*(g if groups and not shared else ()), B, cin, H, W) + dc_x
    w = (torch.randn(*g, cout, cin) + dc_w) / cin ** 0.5
    oh, ow = (H - 1) // stride + 1, (W - 1) // stride + 1
    o = {"isc": torch.rand(cin) + 0.5 if affine else None, "ish": torch.randn(cin) * 0.1 if affine else None,
         "osc": torch.rand(cout) + 0.5 if osc else None, "bias": torch.randn(*g, cout) if bias else None,
         "slope": torch.rand(cout) if act == "prelu" else None, "res": torch.randn(B, cout, oh, ow) if res else None}
    return x, w, o


def launch(lib, st, dev, x, hi, lo, cout, o, stride=1, act="none", alpha=0.0, res_first=False, nterms=3, affine_in_launch=True, **kw):
    """M.conv1x1_f16 with the operands of `o` on the device; x: a device tensor or a SplitActivation."""
    dv = lambda k: None if o.get(k) is None else o[k].to(dev)  # noqa: E731
    return M.conv1x1_f16(lib, st, x, hi, lo, nterms, cout, stride=stride, in_scale=dv("isc") if affine_in_launch else None,
                         in_shift=dv("ish") if affine_in_launch else None, out_scale=dv("osc"), bias=dv("bias"),
                         act=ACTS[act] | (M.ACT_RESIDUAL_FIRST if res_first else 0), slope=dv("slope"), alpha=alpha, residual=dv("res"), **kw)


def _expect(lib, label, shape, path, split, stride=1, groups=1):
    """The launch just made took tile form `path`; the size query says split-K (True) / no split (False)."""
    if path is not None:
        assert lib.hf_debug_last_path() == path, (label, lib.hf_debug_last_path(), path)
    if split is not None:
        B, cin, cout, H, W = shape
        n = lib.hf_conv1x1_f16_workspace_floats(B, cin, cout, H, W, stride, groups)
        assert (n > 0) == split, (label, n)


@contextlib.contextmanager
def plans(lib, binv, tuning=0):
    """hf_set_batch_invariant(binv) and hf_debug_set_tuning(tuning) for the body, restored also when it raises.  The library's
    default differs between the suites (the product switches batch-invariant plans on, the bare interpreter library has them
    off) and the split-K plan follows the mode: a check that states `split` or a path pins the mode, 0 = plans from the launch's
    own batch."""
    prev = lib.hf_set_batch_invariant(binv)
    lib.hf_debug_set_tuning(tuning)
    try:
        yield
    finally:
        lib.hf_set_batch_invariant(prev)
        lib.hf_debug_set_tuning(0)


@contextlib.contextmanager
def splitk_inkernel(lib, dev, on):
    """The in-kernel split-K reduction on / off for the body; yields counters() = the absolute sum of the arrival counters (0
    when off).  GPU: hairfastgan_amd._runtime's switch and its per-stream buffer; interpreter: a buffer registered here."""
    def gpu():
        from hairfastgan_amd import _runtime

        prev = _runtime.set_splitk_inkernel(on)
        try:
            _runtime.stream()  # registers (or drops) this thread's counter buffer
            yield (lambda: int(_runtime._counter_bufs[_runtime._counter_tls.key[:2]].abs().sum())) if on else (lambda: 0)
        finally:
            _runtime.set_splitk_inkernel(prev)

    def sim():
        counters = torch.zeros(4096, dtype=torch.int32)
        if on:
            lib.hf_set_splitk_counters(counters.data_ptr(), counters.numel())
        else:
            lib.hf_set_splitk_counters(None, 0)
        try:
            yield lambda: int(counters.abs().sum())
        finally:
            lib.hf_set_splitk_counters(None, 0)

    yield from per_device(dev, sim, gpu)()


# --------------------------------------------------------------------------------------------------------------------
# the checks
# --------------------------------------------------------------------------------------------------------------------
def check_form(lib, st, dev, case):
    """Register-staged input: the fp64 rule, the tile form, the split query; offset: x one float into its storage."""
    shape, opt, path, split, nterms, offset = case.args
    B, cin, cout, H, W = shape
    x, w, o = layer(300, *shape, **opt)
    kw = {k: opt[k] for k in ("stride", "act") if k in opt}
    kw.update(alpha=0.2 if opt.get("act") == "lrelu" else 0.0, res_first=opt.get("res") == "first", nterms=nterms)
    hi, lo = prep(lib, st, w.to(dev))
    xd = _offset_view(x, dev) if offset else x.to(dev)
    with plans(lib, 0):
        y = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
        _expect(lib, case.label, shape, path, split, kw.get("stride", 1))
        aligned = launch(lib, st, dev, x.to(dev), hi, lo, cout, o, **kw) if offset else None
    accuracy_f16("form", case.label, y, x, w, o, **kw)
    if offset:  # scalar plane loads either way: the aligned launch's bits
        exact("form", case.label + " == aligned call", y, aligned.cpu())


def check_presplit(lib, st, dev, case):
    """Pre-split input (hf_split_activation_f16 carries the affine; staged by LDS-DMA): the fp64 rule, and the bits of the
    register-staged launch with the same affine."""
    shape, opt, path, split = case.args
    cout = shape[2]
    x, w, o = layer(301, *shape, **opt)
    kw = {"act": opt.get("act", "none")}
    hi, lo = prep(lib, st, w.to(dev))
    xd = x.to(dev)
    dv = lambda k: None if o[k] is None else o[k].to(dev)  # noqa: E731
    xs = M.split_activation_f16(lib, st, xd, dv("isc"), dv("ish"))
    with plans(lib, 0):
        y = launch(lib, st, dev, xs, hi, lo, cout, o, affine_in_launch=False, **kw)
        _expect(lib, case.label, shape, path, split)
        staged = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
    accuracy_f16("presplit", case.label, y, x, w, o, **kw)
    exact("presplit", case.label + " == register-staged", y, staged.cpu())


def check_wide(lib, st, dev, case):
    """The 128-channel block form (path 706; hf_debug_set_tuning bits 24-31 = 1: every launch counts as chip-filling): the fp64
    rule, and the bits of the 64-channel form (tuning bit 1)."""
    shape, opt, pre, split = case.args
    cout = shape[2]
    x, w, o = layer(302, *shape, **opt)
    kw = {"act": opt.get("act", "none")}
    hi, lo = prep(lib, st, w.to(dev))
    xd = M.split_activation_f16(lib, st, x.to(dev)) if pre else x.to(dev)
    out = {}
    for never in (0, 2):
        with plans(lib, 0, (1 << 24) | never):
            out[never] = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
            _expect(lib, case.label, shape, 702 if never else 706, split)
    accuracy_f16("wide", case.label, out[0], x, w, o, **kw)
    exact("wide", case.label + " == 64-channel blocks", out[0], out[2].cpu())


def check_splitk(lib, st, dev, case):
    """Split-K: the fp64 rule; the two-launch form (slabs + splitk_reduce) equals the in-kernel reduction bit for bit, which
    leaves its counters at zero."""
    shape, opt = case.args
    cout = shape[2]
    x, w, o = layer(303, *shape, **opt)
    kw = {"act": opt.get("act", "none")}
    hi, lo = prep(lib, st, w.to(dev))
    xd = x.to(dev)
    with plans(lib, 0), splitk_inkernel(lib, dev, False):
        two = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
        _expect(lib, case.label, shape, None, True)
        _sync(dev)
    with plans(lib, 0), splitk_inkernel(lib, dev, True) as counters:
        one = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
        _sync(dev)
        assert counters() == 0, ("splitk", case.label, "counters left non-zero")
    accuracy_f16("splitk", case.label, two, x, w, o, **kw)
    exact("splitk", case.label + " in-kernel == two launches", one, two.cpu())


VSPLIT = ((4, 256, 64, 5, 7), {"act": "prelu", "bias": True})   # case 8's layer: 8 stages, the canonical plan splits them in 4


def check_vsplit(lib, st, dev, case):
    """The virtual K split of a batch-invariant plan (the block walks the slabs itself): the fp64 rule, no workspace, and the
    bits of the per-sample launches, which use slabs and splitk_reduce."""
    shape, opt = case.args
    B, cin, cout, H, W = shape
    x, w, o = layer(304, *shape, **opt)
    kw = {"act": opt.get("act", "none")}
    hi, lo = prep(lib, st, w.to(dev))
    xd = x.to(dev)
    with splitk_inkernel(lib, dev, False):
        with plans(lib, 1, 1 << 24):
            assert lib.hf_conv1x1_f16_workspace_floats(B, cin, cout, H, W, 1, 1) == 0, case.label
            y = launch(lib, st, dev, xd, hi, lo, cout, o, **kw)
        with plans(lib, 1):
            assert lib.hf_conv1x1_f16_workspace_floats(1, cin, cout, H, W, 1, 1) > 0, case.label
            per = torch.cat([launch(lib, st, dev, xd[b:b + 1], hi, lo, cout, o, **kw) for b in range(B)])
        _sync(dev)
    accuracy_f16("vsplit", case.label, y, x, w, o, **kw)
    exact("vsplit", case.label + " == per-sample split-K", y, per.cpu())


def check_groups(lib, st, dev, case):
    """Grouped launches, each group against fp64: bias + LReLU(0.01); own input [G, B, cin, H, W] or one shared [B, cin, H, W]."""
    G, shape, stride, shared, split = case.args
    B, cin, cout, H, W = shape
    x, w, o = layer(305, *shape, stride=stride, bias=True, groups=G, shared=shared)
    hi, lo = prep(lib, st, w.to(dev))
    with plans(lib, 0):
        y = launch(lib, st, dev, x.to(dev), hi, lo, cout, o, stride=stride, act="lrelu", alpha=0.01, groups=G, x_shared=shared)
        _expect(lib, case.label, shape, None, split, stride, G)
    _sync(dev)
    assert tuple(y.shape[:2]) == (G, B)
    for g in range(G):
        accuracy_f16("groups", f"{case.label} group {g}", y[g], x if shared else x[g], w[g], {"bias": o["bias"][g]}, stride=stride,
                     act="lrelu", alpha=0.01)


def check_saturation(lib, st, dev, case):
    """The register-staged conversion's split saturates instead of overflowing: a finite result, and the clamp is counted."""
    shape, gain = case.args
    x, w, o = layer(306, *shape)
    hi, lo = prep(lib, st, w.to(dev))
    M.f16_overflow_count(lib, reset=True)
    y = launch(lib, st, dev, ((x - 3.0) * gain).to(dev), hi, lo, shape[2], o)
    _sync(dev)
    assert bool(torch.isfinite(y).all()), case.label
    assert M.f16_overflow_count(lib, reset=True) > 0, case.label
    assert M.f16_overflow_count(lib) == 0, case.label


def check_stray(lib, st, dev, case):
    """The raw C-ABI call into a guarded buffer: rc 0, sentinels behind the output survive, the values obey the fp64 rule."""
    shape, opt = case.args
    B, cin, cout, H, W = shape
    x, w, o = layer(307, *shape, **opt)
    hi, lo = prep(lib, st, w.to(dev))
    xd, bd, sd, rd = x.to(dev), o["bias"].to(dev), o["slope"].to(dev), o["res"].to(dev)
    n = B * cout * H * W
    buf = _guarded(n, dev)
    with plans(lib, 0):
        assert lib.hf_conv1x1_f16_workspace_floats(B, cin, cout, H, W, 1, 1) == 0
        rc = lib.hf_conv1x1_f16_f32(buf.data_ptr(), xd.data_ptr(), None, None, hi.data_ptr(), lo.data_ptr(), 3, None, None, None, bd.data_ptr(),
                                    M.ACT_PRELU, sd.data_ptr(), 0.0, rd.data_ptr(), B, cin, cout, H, W, 1, 1, 0, None, 0, st)
    _guard_ok("stray", case.label, buf, n, rc)
    accuracy_f16("stray", case.label, buf[:n].view(B, cout, H, W), x, w, o, act="prelu")


def check_sliced(lib, st, dev, case):
    """A launch too large for a full fp64 product: the rule on every `step`-th output channel, all pixels."""
    shape, opt, step, path, split = case.args
    cout = shape[2]
    x, w, o = layer(308, *shape, **opt)
    kw = {"act": opt.get("act", "none")}
    hi, lo = prep(lib, st, w.to(dev))
    y = launch(lib, st, dev, x.to(dev), hi, lo, cout, o, **kw)
    _expect(lib, case.label, shape, path, split)
    accuracy_f16("sliced", case.label, y[:, ::step], x, w, o, channels=slice(None, None, step), **kw)


# --------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes that reach each branch (size classes as in small_ops_checks)
# --------------------------------------------------------------------------------------------------------------------
_FLAT = ((2, 64, 64, 9, 11), {"bias": True, "act": "prelu", "res": True})
_S2 = ((2, 32, 128, 9, 13), {"stride": 2, "affine": True, "osc": True, "act": "lrelu", "res": "first"})
CASES = {
    # ((B, cin, cout, H, W), options, path, split, nterms, offset x)
    "form": [
        _c("2x64x9x11 -> 64 bias PReLU residual: flat tile with overhang", *_FLAT, 701, False, 3, False),
        _c("2x32x9x13 -> 128 stride 2, affine, out_scale, LReLU after the residual", *_S2, 701, False, 3, False),
        _c("3x32x1x1 -> 64 stride 2 on a 1x1 plane", (3, 32, 64, 1, 1), {"stride": 2}, 701, False, 3, False),
        _c("5x32x4x4 -> 64 affine: tile of 8 images, three absent", (5, 32, 64, 4, 4), {"affine": True}, 701, False, 3, False),
        _c("3x64x8x8 -> 64 QuickGELU: two images per tile", (3, 64, 64, 8, 8), {"act": "qgelu"}, 701, False, 3, False),
        _c("1x32x8x16 -> 64: 128 pixels", (1, 32, 64, 8, 16), {}, 701, False, 3, False),
        _c("2x32x3x43 -> 64 residual: 129 pixels", (2, 32, 64, 3, 43), {"res": True}, 702, False, 3, False),
        _c("1x64x1x257 -> 64: long flat plane", (1, 64, 64, 1, 257), {}, 702, False, 3, False),
        _c("2x64x9x11 -> 64 bias PReLU residual, one-term operands", *_FLAT, 701, False, 1, False),
        _c("2x32x9x13 -> 128 stride 2, affine, out_scale, LReLU after the residual, one-term operands", *_S2, 701, False, 1, False),
        _c("1x768x2x50 -> 64 zero-mean operands: cancellation", (1, 768, 64, 2, 50), {"zero_mean": True}, 701, True, 3, False),
        _c("2x64x9x11 -> 64 bias PReLU residual, x offset view", *_FLAT, 701, False, 3, True),
    ],
    # ((B, cin, cout, H, W), options, path, split)
    "presplit": [
        _c("2x64x13x21 -> 128 affine PReLU residual", (2, 64, 128, 13, 21), {"affine": True, "bias": True, "act": "prelu", "res": True}, 702, False),
        _c("3x64x4x4 -> 64: several images per tile", (3, 64, 64, 4, 4), {}, 701, False),
    ],
    # ((B, cin, cout, H, W), options, pre-split input, split)
    "wide": [
        _c("2x64x13x21 -> 256 PReLU residual", (2, 64, 256, 13, 21), {"bias": True, "act": "prelu", "res": True}, False, False),
        _c("1x128x18x17 -> 128 pre-split", (1, 128, 128, 18, 17), {}, True, True),
    ],
    "splitk": [
        _c("1x256x2x17 -> 64 residual", (1, 256, 64, 2, 17), {"bias": True, "res": True}),
        _c("1x768x2x50 -> 128 QuickGELU", (1, 768, 128, 2, 50), {"bias": True, "act": "qgelu"}),
        _c("1x3072x2x50 -> 768", (1, 3072, 768, 2, 50), {"bias": True}, size=2),
    ],
    "vsplit": [_c("4x256x5x7 -> 64 PReLU", *VSPLIT)],
    # (G, (B, cin, cout, H, W), stride, shared input, split)
    "groups": [
        _c("G3 own 2x64x1x1 -> 64: fc_mu form", 3, (2, 64, 64, 1, 1), 1, False, False),
        _c("G3 own 3x32x4x4 -> 64", 3, (3, 32, 64, 4, 4), 1, False, False),
        _c("G2 shared 2x32x6x6 -> 64", 2, (2, 32, 64, 6, 6), 1, True, False),
        _c("G2 shared 2x32x9x7 -> 64 stride 2", 2, (2, 32, 64, 9, 7), 2, True, False),
        _c("G2 own 3x32x9x7 -> 128 stride 2", 2, (3, 32, 128, 9, 7), 2, False, False),
        _c("G3 own 1x256x2x2 -> 64 split-K", 3, (1, 256, 64, 2, 2), 1, False, True),
        _c("G11 shared 2x512x8x8 -> 64: the heads' form", 11, (2, 512, 64, 8, 8), 1, True, True),
    ],
    "saturation": [_c("1x32x5x7 -> 64, x = randn * 1e6", (1, 32, 64, 5, 7), 1e6)],
    "stray": [_c("3x32x5x7 -> 64 bias PReLU residual, raw call", (3, 32, 64, 5, 7), {"bias": True, "act": "prelu", "res": True})],
    # ((B, cin, cout, H, W), options, channel step, path, split)
    "sliced": [_c("1x768x113x50 -> 3072 bias QuickGELU: 128-channel blocks without a hook", (1, 768, 3072, 113, 50),
                  {"bias": True, "act": "qgelu"}, 48, 706, False, size=2)],
}
CHECKS = {op: globals()["check_" + op] for op in CASES}


def cases(gpu):
    return [(op, c) for op, cs in CASES.items() for c in cs if gpu or c.size < 2]


def case_id(v):
    return v.label.replace(" ", "_") if isinstance(v, Case) else str(v)


# --------------------------------------------------------------------------------------------------------------------
# batch invariance: batch-invariant mode on, fill count lowered; run(n) = the layer on the first n samples of one input
# --------------------------------------------------------------------------------------------------------------------
BATCH_LAYERS = {
    # the tile holds 1 / 4 / 8 / 8 images at 1 / 3 / 6 / 9 samples
    "several images per tile": ((9, 32, 64, 4, 4), {"affine": True}, 1 << 24),
    # fill count 4: split-K slabs at 1 and 3 samples, the virtual split at 6 and 9
    "split-K slabs meet the virtual split": ((9,) + VSPLIT[0][1:], VSPLIT[1], 4 << 24),
}
BATCH_OPS = list(BATCH_LAYERS)


def check_batch_invariance(lib, st, dev, op):
    shape, opt, tuning = BATCH_LAYERS[op]
    B, cin, cout, H, W = shape
    x, w, o = layer(330, *shape, **opt)
    hi, lo = prep(lib, st, w.to(dev))
    xd = x.to(dev)
    if op == BATCH_OPS[1]:
        with plans(lib, 1, tuning):
            assert [lib.hf_conv1x1_f16_workspace_floats(n, cin, cout, H, W, 1, 1) > 0 for n in (1, 3, 6, 9)] == [True, True, False, False]
    with splitk_inkernel(lib, dev, False), plans(lib, 1, tuning):
        invariant(op, lambda n: launch(lib, st, dev, xd[:n], hi, lo, cout, o, act=opt.get("act", "none")))
