"""TEST INFRASTRUCTURE - direct checks of the small kernels (csrc/encoder_ops.hip, vit.hip, the pooling / tanh part of
sean.hip, scale_shortcut_add_split of convh_enc.hip), shared by the hipsim tests (tests/test_sim_small_ops.py) and the GPU
tests (tests/test_gpu_small_ops.py): every function takes the library, the stream and the device to run on.

Every reference is restated here from the operation's definition, in torch fp64 on the CPU; inputs come from
torch.manual_seed on the CPU and are copied to the device.  Whatever is summed carries a DC offset of several standard
deviations, so that a dropped or double-counted element moves the result by about 1/n of full scale.

Accuracy rule (floating results):  E_k = max |kernel - ref64|,  E_t = max |ATen fp32 on the CPU - ref64|,
    E_k <= FACTOR * E_t + 4 * 2^-23 * max |ref64|.
The yardstick is ATen's own distance from fp64, never the kernel's output; FACTOR = 4 because the kernels sum in another
order than ATen (lane-strided partials, a butterfly, wave order) - an error of the same size, not the same error; the
additive term covers the cases where ATen happens to be exact.
Exactness rule: operations that select, copy or round once per element with no contraction choice equal torch fp32 bit
for bit.  Batch rule: op(x)[:k] equals op(x[:k]) bit for bit.  Stray writes: sentinels behind / around the output survive.

A case is (label, arguments..., size class): 0 and 1 = every suite (1: more than 524288 elements, the second trip of a
grid-stride loop - the interpreter takes a fraction of a second for these), 2 = GPU only."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from oracle import cases as C

FACTOR = 4.0
ULP = 2.0 ** -23
GRID = 2048 * 256            # grid_for's cap in threads: a grid-stride loop takes a second trip above this
BIG = (5, 104909)            # 5 * 104909 = 524288 + 257 = 5 * 7 * 7 * 2141: the second trip is ragged
BIG_PLANES = (5, 1, 49, 2141)
SENTINEL = -12345.5
ROWS = []                    # (op, case, E_k, E_t, bound) of this process, in run order

Case = collections.namedtuple("Case", "label args size")


def _c(label, *args, size=0):
    return Case(label, args, size)


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _offset_view(t, dev, floats=1):
    """t's values in a contiguous view that starts `floats` floats into its storage (4-byte aligned only)."""
    buf = torch.empty(t.numel() + floats, dtype=t.dtype, device=dev)
    v = buf[floats:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (buf.data_ptr() + 4 * floats) % 16
    return v


def accuracy(op, label, got, ref64, t32, factor=FACTOR, extra=0.0, tag="small_ops"):
    """extra: an additive term of the bound, a number or a tensor of ref64's shape (a per-element bound); the row then holds
    E_k and the bound of the element whose E_k / bound is largest."""
    _sync(got.device)
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (op, label, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), (op, label)
    err = (got.double() - ref64).abs()
    e_t = float((t32.double() - ref64).abs().max())
    bounds = factor * e_t + 4 * ULP * float(ref64.abs().max()) + torch.as_tensor(extra, dtype=torch.float64).expand(err.shape)
    i = int(torch.argmax(err / bounds.clamp_min(1e-300)))
    e_k, bound = float(err.reshape(-1)[i]), float(bounds.reshape(-1)[i])
    ROWS.append((op, label, e_k, e_t, bound))
    print(f"{tag} {op} {label}: E_k {e_k:.2e} E_t {e_t:.2e} bound {bound:.2e}")
    assert bool((err <= bounds).all()), (op, label, e_k, e_t, bound)


def exact(op, label, got, want):
    """Equal bits, compared on the device that holds `got` (a conv check's activation can be 1 GB)."""
    _sync(got.device)
    assert got.shape == want.shape and torch.equal(got, want.to(got.device)), (op, label)


def _guarded(n, dev):
    return torch.full((n + 64,), SENTINEL, device=dev)


def _guard_ok(op, label, buf, n, rc):
    _sync(buf.device)
    assert rc == 0, (op, label, rc)
    assert bool((buf[n:].cpu() == SENTINEL).all()), (op, label, "write behind the output")


def invariant(op, run, pairs=((6, 3), (9, 1))):
    """run(n): the operator on the first n samples of one fixed input, batch-major output."""
    for total, k in pairs:
        a, b = run(total), run(k)
        _sync(a.device)
        assert a.shape[0] == total and b.shape[0] == k and torch.equal(a[:k].cpu(), b.cpu()), (op, total, k)


# --------------------------------------------------------------------------------------------------------------------
# encoder_ops.hip
# --------------------------------------------------------------------------------------------------------------------
def check_plane_mean(lib, st, dev, case):
    shape, offset = case.args
    torch.manual_seed(101)
    x = torch.randn(shape) + 3.0
    xd = _offset_view(x, dev) if offset else x.to(dev)
    accuracy("plane_mean", case.label, M.plane_mean(lib, st, xd), x.double().mean((2, 3)), x.mean((2, 3)))
    planes, hw = shape[0] * shape[1], shape[2] * shape[3]
    buf = _guarded(planes, dev)
    rc = lib.hf_plane_mean_f32(buf.data_ptr(), xd.data_ptr(), planes, hw, st)
    _guard_ok("plane_mean", case.label, buf, planes, rc)


def check_se_gate(lib, st, dev, case):
    b, c, cr = case.args
    torch.manual_seed(102)
    pooled = torch.randn(b, c) + 3.0
    fc1, fc2 = (torch.randn(cr, c) + 0.5) / c, torch.randn(c, cr) / cr ** 0.5
    ref = torch.sigmoid(F.linear(F.relu(F.linear(pooled.double(), fc1.double())), fc2.double()))
    t32 = torch.sigmoid(F.linear(F.relu(F.linear(pooled, fc1)), fc2))
    accuracy("se_gate", case.label, M.se_gate(lib, st, pooled.to(dev), fc1.to(dev), fc2.to(dev)), ref, t32)


def _ssa_inputs(shape, stride, sc_hw, gate):
    torch.manual_seed(103)
    r = torch.randn(shape)
    g = torch.rand(shape[:2]) + 0.5 if gate else None
    sc = torch.randn(shape[:2] + sc_hw)
    want = (r if g is None else r * g[:, :, None, None]) + sc[:, :, ::stride, ::stride][:, :, :shape[2], :shape[3]]
    return r, g, sc, want


def check_scale_shortcut_add(lib, st, dev, case):
    shape, stride, sc_hw, gate = case.args
    r, g, sc, want = _ssa_inputs(shape, stride, sc_hw, gate)
    got = M.scale_shortcut_add(lib, st, r.to(dev), None if g is None else g.to(dev), sc.to(dev), stride)
    exact("scale_shortcut_add", case.label, got, want)  # one rounding per statement, no contraction


def check_scale_shortcut_add_split(lib, st, dev, case):
    shape, stride, sc_hw, gate = case.args
    r, g, sc, want = _ssa_inputs(shape, stride, sc_hw, gate)
    out, split = M.scale_shortcut_add_split(lib, st, r.to(dev), None if g is None else g.to(dev), sc.to(dev), stride)
    exact("scale_shortcut_add_split", case.label, out, want)
    hi, lo = M.split_activation_reference(want, None)
    exact("scale_shortcut_add_split", case.label + " hi", split.hi, hi)
    exact("scale_shortcut_add_split", case.label + " lo", split.lo, lo)


def check_upsample_bilinear_add(lib, st, dev, case):
    b, c, h, w, oh, ow = case.args
    torch.manual_seed(104)
    x, y = torch.randn(b, c, h, w), torch.randn(b, c, oh, ow)
    ref = F.interpolate(x.double(), (oh, ow), mode="bilinear", align_corners=True) + y.double()
    t32 = F.interpolate(x, (oh, ow), mode="bilinear", align_corners=True) + y
    accuracy("upsample_bilinear_add", case.label, M.upsample_bilinear_add(lib, st, x.to(dev), y.to(dev)), ref, t32)


def check_adaptive_avgpool_into(lib, st, dev, case):
    b, c, h, w, oh, ow = case.args
    torch.manual_seed(105)
    x = torch.randn(b, c, h, w) + 3.0
    c_off, ctot = 2, c + 3
    out = torch.full((b, ctot, oh, ow), SENTINEL, device=dev)
    M.adaptive_avgpool_into(lib, st, out, x.to(dev), c_off)
    accuracy("adaptive_avgpool_into", case.label, out[:, c_off:c_off + c], F.adaptive_avg_pool2d(x.double(), (oh, ow)),
             F.adaptive_avg_pool2d(x, (oh, ow)))
    rest = torch.cat([out[:, :c_off], out[:, c_off + c:]], 1).cpu()
    assert bool((rest == SENTINEL).all()), ("adaptive_avgpool_into", case.label, "other channels written")


def check_downscale2x(lib, st, dev, case):
    (shape,) = case.args
    torch.manual_seed(106)
    x = torch.randn(shape) + 3.0
    got = M.downscale2x(lib, st, x.to(dev))
    accuracy("downscale2x", case.label, got, F.interpolate(x.double(), scale_factor=0.5, mode="bilinear"),
             F.interpolate(x, scale_factor=0.5, mode="bilinear"))
    # a contiguous view one float into its storage (4-byte aligned): four scalar loads feed the same expression
    exact("downscale2x", case.label + " offset view", M.downscale2x(lib, st, _offset_view(x, dev)), got.cpu())


def _linear_x(x, form, dev):
    b, k = x.shape
    if form in ("view", "odd_stride"):  # big[:, :k]: row stride k + 8 (16-byte rows) / k + 3 (not a multiple of 4)
        big = torch.zeros(b, k + (8 if form == "view" else 3), device=dev)
        big[:, :k] = x.to(dev)
        return big[:, :k]
    if form == "offset":                # starts one float into its storage: the scalar-tolerant kernel
        return _offset_view(x, dev)
    return x.to(dev)


def check_linear(lib, st, dev, case):
    b, k, n, form, bias, scale = case.args
    torch.manual_seed(107)
    x, w = torch.randn(b, k) * 2 + 5, torch.randn(n, k)
    bv = torch.randn(n) if bias else None
    ref = F.linear(x.double(), w.double()) * scale + (bv.double() if bias else 0.0)
    t32 = F.linear(x, w) * scale + (bv if bias else 0.0)
    xd, wd, bd = _linear_x(x, form, dev), w.to(dev), bv.to(dev) if bias else None
    accuracy("linear", case.label, M.linear(lib, st, xd, wd, bd, scale), ref, t32)
    buf = _guarded(b * n, dev)
    rc = lib.hf_linear_f32(buf.data_ptr(), xd.data_ptr(), xd.stride(0) if b > 1 else k, wd.data_ptr(),
                           bd.data_ptr() if bias else None, b, k, n, float(scale), st)
    _guard_ok("linear", case.label, buf, b * n, rc)


def check_equal_linear(lib, st, dev, case):
    rows, k, n, lr_mul, fused = case.args
    torch.manual_seed(108)
    x, w, bv = torch.randn(rows, k) * 2 + 5, torch.randn(n, k) / lr_mul, torch.randn(n) / lr_mul
    scale = (1.0 / k ** 0.5) * lr_mul

    def eq(x_, w_, b_):  # EqualLinear.forward: linear with weight * scale, bias * lr_mul; fused leaky ReLU * sqrt(2)
        y = F.linear(x_, w_ * scale, b_ * lr_mul)
        return F.leaky_relu(y, 0.2) * 2.0 ** 0.5 if fused else y

    got = M.equal_linear(lib, st, x.to(dev), w.to(dev), bv.to(dev), lr_mul, fused)
    accuracy("equal_linear", case.label, got, eq(x.double(), w.double(), bv.double()), eq(x, w, bv))


def _pixel_norm(x, dim):
    return x * torch.rsqrt((x * x).mean(dim, keepdim=True) + 1e-8)


def check_pixel_norm(lib, st, dev, case):
    rows, dim = case.args
    torch.manual_seed(109)
    x = torch.randn(rows, dim) * 2 + 5
    xd = x.to(dev)
    accuracy("pixel_norm", case.label, M.pixel_norm(lib, st, xd), _pixel_norm(x.double(), 1), _pixel_norm(x, 1))
    buf = _guarded(rows * dim, dev)
    _guard_ok("pixel_norm", case.label, buf, rows * dim, lib.hf_pixel_norm_f32(buf.data_ptr(), xd.data_ptr(), rows, dim, st))


def check_pixel_norm_dim1(lib, st, dev, case):
    (shape,) = case.args
    torch.manual_seed(110)
    x = torch.randn(shape) * 2 + 5
    accuracy("pixel_norm_dim1", case.label, M.pixel_norm_dim1(lib, st, x.to(dev)), _pixel_norm(x.double(), 1), _pixel_norm(x, 1))


def check_layernorm(lib, st, dev, case):
    rows, dim, affine, lrelu, groups = case.args
    torch.manual_seed(111)
    x = torch.randn(rows, dim) * 2 + 5
    g = (torch.rand(groups, dim) + 0.5) if affine else None
    bt = torch.randn(groups, dim) if affine else None

    def ln(x_, g_, b_):
        y = F.layer_norm(x_, (dim,), None, None, 1e-5)
        if affine:  # row r takes the affine of group r % groups
            y = (y.view(rows // groups, groups, dim) * g_[None] + b_[None]).view(rows, dim)
        return F.leaky_relu(y, 0.01) if lrelu else y

    ref = ln(x.double(), g.double() if affine else None, bt.double() if affine else None)
    xd = x.to(dev)
    gd, bd = (g.to(dev), bt.to(dev)) if affine else (None, None)
    if affine and groups == 1:
        gd, bd = gd[0], bd[0]
    accuracy("layernorm", case.label, M.layernorm(lib, st, xd, dim, gd, bd, 1e-5, lrelu, 0.01, groups), ref, ln(x, g, bt))
    if groups == 1:
        buf = _guarded(rows * dim, dev)
        rc = lib.hf_layernorm_f32(buf.data_ptr(), xd.data_ptr(), gd.data_ptr() if affine else None, bd.data_ptr() if affine else None,
                                  rows, dim, 1e-5, 1 if lrelu else 0, 0.01, st)
        _guard_ok("layernorm", case.label, buf, rows * dim, rc)


def check_sample_layernorm(lib, st, dev, case):
    shape, channels, affine, offset, slope = case.args
    torch.manual_seed(112)
    x = torch.randn(shape) * 2 + 5
    b, c = shape[0], channels or shape[1]
    g, bt = ((torch.rand(c) + 0.5, torch.randn(c)) if affine else (None, None))

    def sln(x_, g_, b_):  # MUNIT LayerNorm: per-sample mean and UNBIASED std over C*H*W, eps added to the std
        x_ = x_[:, :c]
        flat = x_.reshape(b, -1)
        y = (x_ - flat.mean(1).view(-1, 1, 1, 1)) / (flat.std(1).view(-1, 1, 1, 1) + 1e-5)
        if affine:
            y = y * g_.view(1, -1, 1, 1) + b_.view(1, -1, 1, 1)
        return F.leaky_relu(y, slope)

    xd = _offset_view(x, dev) if offset else x.to(dev)
    got = M.sample_layernorm(lib, st, xd, g.to(dev) if affine else None, bt.to(dev) if affine else None, 1e-5, slope, channels)
    accuracy("sample_layernorm", case.label, got, sln(x.double(), g.double() if affine else None, bt.double() if affine else None),
             sln(x, g, bt))


def check_modulate(lib, st, dev, case):
    shape, lrelu = case.args
    torch.manual_seed(113)
    x, g, bt = torch.randn(shape), torch.randn(shape), torch.randn(shape)

    def mod(x_, g_, b_):
        y = x_ * (1.0 + g_) + b_
        return F.leaky_relu(y, 0.01) if lrelu else y

    accuracy("modulate", case.label, M.modulate(lib, st, x.to(dev), g.to(dev), bt.to(dev), lrelu, 0.01),
             mod(x.double(), g.double(), bt.double()), mod(x, g, bt))


def check_gate(lib, st, dev, case):
    shape, with_plane, with_bcast, plus_one = case.args
    torch.manual_seed(114)
    x, lg = torch.randn(shape), torch.randn(shape[:2])
    ap = torch.randn(shape) if with_plane else None
    ab = torch.randn(shape[:2]) if with_bcast else None

    def gate(x_, lg_, ap_, ab_):
        y = x_ * (torch.sigmoid(lg_)[:, :, None, None] + plus_one)
        if with_plane:
            y = y + ap_
        return y + ab_[:, :, None, None] if with_bcast else y

    dd = lambda t: None if t is None else t.double()  # noqa: E731
    dv = lambda t: None if t is None else t.to(dev)  # noqa: E731
    accuracy("gate", case.label, M.gate(lib, st, x.to(dev), lg.to(dev), dv(ap), dv(ab), plus_one),
             gate(x.double(), lg.double(), dd(ap), dd(ab)), gate(x, lg, ap, ab))


def check_axpby(lib, st, dev, case):
    shape, period = case.args
    torch.manual_seed(115)
    a, bv = torch.randn(shape), torch.randn(period)
    alpha, beta = 0.75, -1.25  # exact in fp32
    n = a.numel()
    assert n % period == 0 and 256 % period != 0
    ref = alpha * a.double() + beta * bv.double().repeat(n // period).view(shape)
    t32 = alpha * a + beta * bv.repeat(n // period).view(shape)
    accuracy("axpby", case.label, M.axpby(lib, st, a.to(dev), alpha, bv.to(dev), beta), ref, t32)


def check_add_bcast(lib, st, dev, case):
    shape, period = case.args
    torch.manual_seed(116)
    a, bv = torch.randn(shape), torch.randn(period)
    n = a.numel()
    assert n % period == 0 and 256 % period != 0
    exact("add_bcast", case.label, M.add_bcast(lib, st, a.to(dev), bv.to(dev)), a + bv.repeat(n // period).view(shape))


def check_bn_fold(lib, st, dev, case):
    n, with_bias = case.args
    torch.manual_seed(117)
    g, be, mu, var = torch.rand(n) + 0.5, torch.randn(n), torch.randn(n), torch.rand(n) + 0.5
    cb = torch.randn(n) if with_bias else None

    def fold(g_, be_, mu_, var_, cb_):
        s = g_ / torch.sqrt(var_ + 1e-5)
        return s, be_ + ((cb_ if with_bias else 0.0) - mu_) * s

    s, t = M.bn_fold(lib, st, g.to(dev), be.to(dev), mu.to(dev), var.to(dev), 1e-5, cb.to(dev) if with_bias else None)
    rs, rt = fold(g.double(), be.double(), mu.double(), var.double(), cb.double() if with_bias else None)
    ts, tt = fold(g, be, mu, var, cb)
    accuracy("bn_fold", case.label + " scale", s, rs, ts)
    accuracy("bn_fold", case.label + " shift", t, rt, tt)


def check_maxpool3x3s2(lib, st, dev, case):
    shape, negative = case.args
    torch.manual_seed(118)
    x = torch.randn(shape)
    if negative:  # padding must never win: every value far below zero
        x = -x.abs() - 10.0
    exact("maxpool3x3s2", case.label, M.maxpool3x3s2(lib, st, x.to(dev)), F.max_pool2d(x, 3, 2, 1))


def check_upsample_nearest(lib, st, dev, case):
    shape, oh, ow = case.args
    torch.manual_seed(119)
    x = torch.randn(shape)
    exact("upsample_nearest", case.label, M.upsample_nearest(lib, st, x.to(dev), oh, ow), F.interpolate(x, (oh, ow), mode="nearest"))


PARSING_EXCUSED = 1e-3   # at most 0.1 % of the pixels may differ, each only at a near-tie
PARSING_MARGIN = 2e-4    # of the logit scale: the rule of test_bisenet_small_image_vs_oracle


def check_parsing_mask(lib, st, dev, case):
    shape, full, out_hw, with_remap, twins = case.args
    torch.manual_seed(120)
    logits = torch.randn(shape)
    if twins:  # two classes with identical planes that win everywhere by at least 1: the lower index is the first maximum
        top = logits.max(1).values + 1.0
        logits[:, twins[0]] = top
        logits[:, twins[1]] = top
    remap = torch.randperm(shape[1]).to(torch.int32) if with_remap else None
    pick = lambda t: F.interpolate(t, out_hw, mode="nearest")  # noqa: E731
    full32 = F.interpolate(logits, full, mode="bilinear", align_corners=True)
    full64 = F.interpolate(logits.double(), full, mode="bilinear", align_corners=True)
    arg32, arg64 = full32.argmax(1, keepdim=True), full64.argmax(1, keepdim=True)
    want = pick((remap.long()[arg32] if with_remap else arg32).float()).long()
    got = M.parsing_mask(lib, st, logits.to(dev), remap.to(dev) if with_remap else None, full, out_hw)
    _sync(dev)
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.int64
    top2 = full64.topk(2, dim=1).values
    margin = pick(top2[:, :1] - top2[:, 1:2])
    scale = float(logits.abs().max())
    if not twins:
        # the inputs themselves: torch's own fp32-versus-fp64 disagreement stays under the cap, so the cap can be met
        assert float((pick(arg32.float()) != pick(arg64.float())).float().mean()) <= PARSING_EXCUSED
    diff = got != want
    print(f"small_ops parsing_mask {case.label}: {int(diff.sum())} of {diff.numel()} pixels differ from torch fp32")
    if dev.type == "cpu" or twins:
        assert not bool(diff.any()), ("parsing_mask", case.label)  # ATen's formula and operation order: bit for bit
    else:
        assert float(diff.float().mean()) <= PARSING_EXCUSED, ("parsing_mask", case.label)
        assert not bool(diff.any()) or float(margin[diff].max()) < PARSING_MARGIN * scale, ("parsing_mask", case.label)
    if twins:
        assert bool((got == min(twins)).all())


def bicubic_taps(factor):
    """Keys' cubic (a = -0.5) sampled at the 4 * factor tap centres, normalised - fp32, as the kernel receives it."""
    size, a = 4 * factor, -0.5
    ax = ((torch.arange(size, dtype=torch.float32) - float(size // 2) + 0.5) / factor).abs()
    k = torch.where(ax <= 1.0, (a + 2.0) * ax ** 3 - (a + 3.0) * ax ** 2 + 1.0,
                    torch.where(ax < 2.0, a * ax ** 3 - 5.0 * a * ax ** 2 + 8.0 * a * ax - 4.0 * a, torch.zeros_like(ax)))
    return k / k.sum()


def bicubic_restated(x, k, factor):
    """Reflect pad, then the separable filter with stride = factor: down the columns first, then along the rows."""
    c = x.shape[1]
    taps = 4 * factor
    lo = (taps - factor) // 2
    hi = taps - factor - lo
    k = k.to(x.dtype)
    y = F.conv2d(F.pad(x, (0, 0, lo, hi), mode="reflect"), k.view(1, 1, taps, 1).repeat(c, 1, 1, 1), stride=(factor, 1), groups=c)
    return F.conv2d(F.pad(y, (lo, hi, 0, 0), mode="reflect"), k.view(1, 1, 1, taps).repeat(c, 1, 1, 1), stride=(1, factor), groups=c)


def check_bicubic_down(lib, st, dev, case, golden=None):
    shape, factor, golden_key = case.args
    k = bicubic_taps(factor)
    if golden_key:
        x = C.unit_input("glue/bicubic", shape)
        # the restatement is tied to the reference's recorded output first
        rec = torch.from_numpy(golden("glue.npz")[golden_key])
        assert float((bicubic_restated(x.double(), k, factor) - rec.double()).abs().max()) < 2e-6
    else:
        torch.manual_seed(121)
        x = torch.randn(shape) + 3.0
    accuracy("bicubic_down", case.label, M.bicubic_down(lib, st, x.to(dev), k.to(dev), factor),
             bicubic_restated(x.double(), k, factor), bicubic_restated(x, k, factor))


# --------------------------------------------------------------------------------------------------------------------
# dilate_erode: the fixture written by oracle/make_golden.py --only morph (the reference's DilateErosion.mask on blobs)
# --------------------------------------------------------------------------------------------------------------------
def morph_restated(mask, radius):
    """`radius` rounds of the five-pixel cross: conv2d, then 'any' for the dilation and 'all five' for the erosion."""
    w = torch.tensor([[0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0]])[None, None]
    d, e = mask.clone(), mask.clone()
    for _ in range(radius):
        d = (F.conv2d(d, w, padding=1) > 0).float()
        e = (F.conv2d(e, w, padding=1) == 5.0).float()
    return d, e


def check_dilate_erode_morph(dilate_erode, dev, golden):
    """dilate_erode(mask, radius) -> (dilated, eroded) against tests/golden/morph.npz, bit for bit; the fixture's conditions
    are asserted again on load."""
    G = golden("morph.npz")
    small, hair = C.morph_masks()
    unpack = lambda a, shape: torch.from_numpy(np.unpackbits(a)[:int(np.prod(shape))].reshape(shape).astype(np.float32))  # noqa: E731
    for mask, radii, tag in ((small, C.MORPH_RADII, "blob"), (hair, (30,), "hair")):
        for r in radii:
            d_ref, e_ref = unpack(G[f"{tag}_dilate{r}"], mask.shape), unpack(G[f"{tag}_erode{r}"], mask.shape)
            C.morph_conditions(mask, d_ref, e_ref, r, erosion_may_be_empty=r == 30)
            d, e = dilate_erode(mask.to(dev), r)
            _sync(dev)
            assert torch.equal(d.cpu(), d_ref) and torch.equal(e.cpu(), e_ref), (tag, r)
    # the launcher's limit, radius 64, on a 17 x 40 mask against the iterated cross
    torch.manual_seed(122)
    m = (torch.rand(2, 1, 17, 40) > 0.97).float()
    m[1] = 1.0 - m[1]  # one sparse plane (dilation non-trivial), one nearly full (erosion non-trivial)
    d, e = dilate_erode(m.to(dev), 64)
    _sync(dev)
    d_ref, e_ref = morph_restated(m, 64)
    assert torch.equal(d.cpu(), d_ref) and torch.equal(e.cpu(), e_ref)


# --------------------------------------------------------------------------------------------------------------------
# vit.hip, sean.hip
# --------------------------------------------------------------------------------------------------------------------
def check_channel_layernorm(lib, st, dev, case):
    c, t, affine = case.args
    torch.manual_seed(123)
    x = torch.randn(c, t) * 2 + 5
    g, bt = ((torch.rand(c) + 0.5, torch.randn(c)) if affine else (None, None))
    ref = F.layer_norm(x.double().T, (c,), g.double() if affine else None, bt.double() if affine else None, 1e-5).T
    t32 = F.layer_norm(x.T, (c,), g, bt, 1e-5).T
    xd, gd, bd = x.to(dev), g.to(dev) if affine else None, bt.to(dev) if affine else None
    accuracy("channel_layernorm", case.label, M.channel_layernorm(lib, st, xd, gd, bd), ref, t32)
    buf = _guarded(c * t, dev)
    rc = lib.hf_channel_layernorm_f32(buf.data_ptr(), xd.data_ptr(), gd.data_ptr() if affine else None,
                                      bd.data_ptr() if affine else None, c, t, 1e-5, st)
    _guard_ok("channel_layernorm", case.label, buf, c * t, rc)


def _attention(qkv, images, seq, heads):
    """softmax(q k^T / sqrt(64)) v per (image, head) on feature-major qkv [3E, images * seq] -> [E, images * seq]."""
    e = heads * 64
    q, k, v = (t.reshape(heads, 64, images, seq).permute(2, 0, 3, 1) for t in qkv.reshape(3, e, images * seq))  # [img, head, seq, 64]
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    return (p @ v).permute(1, 3, 0, 2).reshape(e, images * seq)


def check_mha_small(lib, st, dev, case):
    images, seq, heads, gain = case.args
    torch.manual_seed(124)
    qkv = torch.randn(3 * heads * 64, images * seq) * gain
    got = M.mha_small(lib, st, qkv.to(dev), images, seq, heads)
    accuracy("mha_small", case.label, got, _attention(qkv.double(), images, seq, heads), _attention(qkv, images, seq, heads))


def _unary_input(kind):
    torch.manual_seed(125)
    return torch.randn(1000) * 2 if kind == "random" else torch.tensor([-100.0, 100.0, 0.0, -0.0, 1e-30, -20.0, 20.0, 88.0, -88.0, 0.5])


def check_quick_gelu(lib, st, dev, case):
    x = _unary_input(*case.args)
    accuracy("quick_gelu", case.label, M.quick_gelu(lib, st, x.to(dev)), x.double() * torch.sigmoid(1.702 * x.double()),
             x * torch.sigmoid(1.702 * x))


def check_tanh(lib, st, dev, case):
    x = _unary_input(*case.args)
    accuracy("tanh", case.label, M.tanh(lib, st, x.to(dev)), torch.tanh(x.double()), torch.tanh(x))


def _region_inputs(shape, crop):
    torch.manual_seed(126)
    b, c, hp, wp = shape
    h, w = hp - 2 * crop, wp - 2 * crop
    x = torch.randn(shape) * 0.5 + 1.5
    lab = torch.randint(0, 19, (b, h, w), dtype=torch.int32)
    lab[b - 1][lab[b - 1] == 4] = 5  # label 4 absent from the last sample
    return x, lab


def _region_mean(x, lab, crop, act):
    b, c, hp, wp = x.shape
    v = x[:, :, crop:hp - crop, crop:wp - crop].reshape(b, c, -1)
    if act:
        v = torch.tanh(v)
    onehot = F.one_hot(lab.reshape(b, -1).long(), 19).to(x.dtype)  # [b, hw, 19]
    cnt = onehot.sum(1)                                           # [b, 19]
    s = torch.einsum("bpl,bcp->blc", onehot, v)
    return torch.where(cnt[:, :, None] > 0, s / cnt.clamp(min=1)[:, :, None], torch.zeros_like(s))


def check_region_mean(lib, st, dev, case):
    shape, crop, act = case.args
    x, lab = _region_inputs(shape, crop)
    got = M.region_mean(lib, st, x.to(dev), lab.to(dev), crop, bool(act))
    accuracy("region_mean", case.label, got, _region_mean(x.double(), lab, crop, act), _region_mean(x, lab, crop, act))
    assert bool((got.cpu()[-1, 4] == 0).all())  # the absent label's row: exactly 0
    assert shape[0] == 1 or bool((got.cpu()[0, 4] != 0).all())


# --------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes that reach each branch
# --------------------------------------------------------------------------------------------------------------------
CASES = {
    "plane_mean": [
        _c("2x3x5x7 scalar, fewer elements than lanes", (2, 3, 5, 7), False),
        _c("1x5x8x8 vector, last block part-filled", (1, 5, 8, 8), False),
        _c("1x2x63x65 scalar, many trips", (1, 2, 63, 65), False),
        _c("3x2x64x64 block form", (3, 2, 64, 64), False),
        _c("2x3x64x66 block form, 1056 float4", (2, 3, 64, 66), False),
        _c("1x1x1x1", (1, 1, 1, 1), False),
        _c("1x5x8x8 offset view: scalar loop", (1, 5, 8, 8), True),
        _c("3x2x64x64 offset view: wave form, scalar loop", (3, 2, 64, 64), True),
    ],
    "se_gate": [_c("2,4,2", 2, 4, 2), _c("3,300,19 channels above 256 threads", 3, 300, 19), _c("1,512,32", 1, 512, 32)],
    "scale_shortcut_add": [
        _c("stride 1", (2, 3, 6, 6), 1, (6, 6), True),
        _c("stride 2, 5x7 from 9x13", (2, 3, 5, 7), 2, (9, 13), True),
        _c("no gate", (2, 3, 5, 7), 2, (9, 13), False),
        _c("524288+257 elements", BIG_PLANES, 1, BIG_PLANES[2:], True, size=1),
    ],
    # (its grid is capped at 8192 blocks of 8-channel pixels: a second trip needs 16.8 M elements, beyond a test's size)
    "scale_shortcut_add_split": [
        _c("stride 1", (2, 16, 6, 6), 1, (6, 6), True),
        _c("stride 2, 5x7 from 9x13", (2, 8, 5, 7), 2, (9, 13), True),
        _c("no gate", (2, 8, 5, 7), 2, (9, 13), False),
    ],
    "upsample_bilinear_add": [
        _c("5x7->10x14", 2, 3, 5, 7, 10, 14), _c("3x4->1x1 ratio 0", 2, 3, 3, 4, 1, 1), _c("7x9->7x9", 1, 2, 7, 9, 7, 9),
        _c("16x16->128x128", 1, 3, 16, 16, 128, 128), _c("2x2->3x257", 1, 2, 2, 2, 3, 257), _c("1x1->4x4", 2, 1, 1, 1, 4, 4),
    ],
    "adaptive_avgpool_into": [  # item counts 105, 27, 192 (8 x 8 bins: always a multiple of 4), 6
        _c("17x23->5x7 ragged overlapping bins", 1, 3, 17, 23, 5, 7), _c("64x64->3x3 bins of 484", 1, 3, 64, 64, 3, 3),
        _c("5x5->8x8 bins of one", 1, 3, 5, 5, 8, 8), _c("130x9->2x1", 1, 3, 130, 9, 2, 1),
    ],
    "downscale2x": [_c("2x2", (2, 3, 2, 2)), _c("8x12", (2, 3, 8, 12)), _c("6x130", (1, 2, 6, 130))],
    "linear": [
        _c("3,40,7", 3, 40, 7, "plain", True, 1.0),
        _c("2,33,5 scalar", 2, 33, 5, "plain", True, 1.0),
        _c("8,260,17 second trip ragged, row-group tails", 8, 260, 17, "plain", True, 1.0),
        _c("19,40,7 three row chunks", 19, 40, 7, "plain", True, 1.0),
        _c("1,1,1", 1, 1, 1, "plain", True, 1.0),
        _c("5,4096,1 K-split", 5, 4096, 1, "plain", True, 1.0),
        _c("9,4112,6 K-split, quarter 1028", 9, 4112, 6, "plain", True, 1.0),
        _c("17,8192,3 K-split", 17, 8192, 3, "plain", True, 1.0),
        _c("1,4100,5 long, wave form", 1, 4100, 5, "plain", True, 1.0),
        _c("3,40,7 no bias, scale 0.5", 3, 40, 7, "plain", False, 0.5),
        _c("9,4112,6 no bias, scale 0.5", 9, 4112, 6, "plain", False, 0.5),
        _c("3,40,7 strided view", 3, 40, 7, "view", True, 1.0),
        _c("9,4112,6 strided view", 9, 4112, 6, "view", True, 1.0),
        _c("3,40,7 row stride 43", 3, 40, 7, "odd_stride", True, 1.0),
        _c("5,4096,1 row stride 4099: wave form", 5, 4096, 1, "odd_stride", True, 1.0),
        _c("3,40,7 offset view", 3, 40, 7, "offset", True, 1.0),
        _c("8,260,17 offset view", 8, 260, 17, "offset", True, 1.0),
        _c("5,4096,1 offset view: wave form", 5, 4096, 1, "offset", True, 1.0),
    ],
    "equal_linear": [_c(f"{r} rows, lr_mul {lr}, fused {fu}", r, 512, 70, lr, fu) for r in (3, 11) for lr, fu in ((0.01, True), (1.0, False))],
    "pixel_norm": [_c("5,70", 5, 70), _c("9,63", 9, 63), _c("3,512", 3, 512), _c("1,1", 1, 1)],
    "pixel_norm_dim1": [_c("3,18,70", (3, 18, 70)), _c("2,18,512", (2, 18, 512))],
    "layernorm": [_c(f"{r},{d}" + (" affine, lrelu" if a else ""), r, d, a, a, 1)
                  for r, d in ((6, 32), (2, 255), (2, 257), (2, 576), (1, 9216)) for a in (False, True)]
    + [_c("2,576 lrelu", 2, 576, False, True, 1), _c("2,257 affine", 2, 257, True, False, 1),
       _c("6,576 grouped 3", 6, 576, True, False, 3), _c("6,32 grouped 3, lrelu", 6, 32, True, True, 3)],
    "sample_layernorm": [
        _c("3x2x1x1 n=2", (3, 2, 1, 1), None, True, False, 1.0),
        _c("2x24x6x10", (2, 24, 6, 10), None, True, False, 0.2),
        _c("1x1x128x128 one chunk", (1, 1, 128, 128), None, True, False, 0.2),
        _c("1x1x1x16385 scalar, last chunk of one", (1, 1, 1, 16385), None, True, False, 0.2),
        _c("1x1x1x16388 vector, last chunk of four", (1, 1, 1, 16388), None, True, False, 0.2),
        _c("1x3x73x75 scalar, two chunks", (1, 3, 73, 75), None, True, False, 0.2),
        _c("2x5x64x64 two chunks", (2, 5, 64, 64), None, True, False, 1.0),
        _c("2x8x6x10 channels 5 of 8", (2, 8, 6, 10), 5, True, False, 0.2),
        _c("2x8x64x64 channels 5 of 8, two chunks", (2, 8, 64, 64), 5, True, False, 0.2),
        _c("2x24x6x10 no gamma", (2, 24, 6, 10), None, False, False, 0.2),
        _c("2x24x6x10 offset view: scalar", (2, 24, 6, 10), None, True, True, 0.2),
        _c("2x5x64x64 offset view: scalar, two chunks", (2, 5, 64, 64), None, True, True, 0.2),
    ],
    "modulate": [_c("3x77", (3, 77), False), _c("3x77 lrelu", (3, 77), True), _c("524288+257 elements", BIG, True, size=1)],
    "gate": [_c(f"2x3x9x11 plane {p} bcast {b} plus {o}", (2, 3, 9, 11), p, b, o)
             for p in (False, True) for b in (False, True) for o in (0.0, 1.0)]
    + [_c("524288+257 elements", BIG_PLANES, True, True, 1.0, size=1)],
    "axpby": [_c("11x7 period 7", (11, 7), 7), _c("3x77 period 77", (3, 77), 77), _c("524288+257 elements, period 49", BIG, 49, size=1)],
    "add_bcast": [_c("11x7 period 7", (11, 7), 7), _c("3x10 period 10", (3, 10), 10), _c("524288+257 elements, period 49", BIG, 49, size=1)],
    "bn_fold": [_c(f"n={n} conv bias {cb}", n, cb) for n in (6, 300) for cb in (True, False)],
    "maxpool3x3s2": [_c("2x3x9x12", (2, 3, 9, 12), False), _c("1x2x1x1", (1, 2, 1, 1), False), _c("1x1x2x2", (1, 1, 2, 2), False),
                     _c("1x3x17x1", (1, 3, 17, 1), False), _c("2x2x64x65", (2, 2, 64, 65), False),
                     _c("2x3x9x12 all negative", (2, 3, 9, 12), True), _c("1x1x2x2 all negative", (1, 1, 2, 2), True),
                     _c("3x1x600x1200 second trip", (3, 1, 600, 1200), False, size=1)],
    "upsample_nearest": [_c("9x12->18x24", (2, 3, 9, 12), 18, 24), _c("9x12->13x17", (2, 3, 9, 12), 13, 17),
                         _c("9x12->4x5", (2, 3, 9, 12), 4, 5), _c("1x1->3x3", (2, 1, 1, 1), 3, 3),
                         _c("32x32->100x3", (1, 2, 32, 32), 100, 3), _c("16x16->512x512, three planes", (3, 1, 16, 16), 512, 512, size=1)],
    "parsing_mask": [
        _c("8x10->40x56", (2, 19, 8, 10), (40, 56), (40, 56), True, None),
        _c("8x10->40x56->16x16", (2, 19, 8, 10), (40, 56), (16, 16), True, None),
        _c("16x16->128x128->37x41", (1, 19, 16, 16), (128, 128), (37, 41), True, None),
        _c("5x5 identity", (2, 19, 5, 5), (5, 5), (5, 5), True, None),
        _c("8x10->40x56 no remap", (2, 19, 8, 10), (40, 56), (40, 56), False, None),
        _c("8x10->40x56 twin classes 3 and 11", (2, 19, 8, 10), (40, 56), (40, 56), False, (3, 11)),
    ],
    "bicubic_down": [
        _c("golden, factor 2", (2, 3, 64, 64), 2, "bicubic2"), _c("golden, factor 4", (2, 3, 64, 64), 4, "bicubic4"),
        _c("1x2x8x518 factor 2: both column loops take more than one trip", (1, 2, 8, 518), 2, None),
        _c("1025x1x128x8 factor 2: 65600 rows", (1025, 1, 128, 8), 2, None, size=2),
    ],
    "channel_layernorm": [_c("24,150", 24, 150, True), _c("768,100", 768, 100, True), _c("1024,65 last width in registers", 1024, 65, True),
                          _c("1040,70 re-reading form", 1040, 70, True), _c("17,1", 17, 1, True), _c("1,64", 1, 64, True),
                          _c("24,150 no gamma", 24, 150, False), _c("1040,70 no gamma", 1040, 70, False)],
    "mha_small": [_c("2,17,2", 2, 17, 2, 1.0), _c("3,1,2", 3, 1, 2, 1.0), _c("1,63,3", 1, 63, 3, 1.0), _c("1,64,1", 1, 64, 1, 1.0),
                  _c("2,50,12", 2, 50, 12, 1.0), _c("2,17,2 qkv * 30", 2, 17, 2, 30.0)],
    "quick_gelu": [_c("n=1000", "random"), _c("extremes", "extremes")],
    "tanh": [_c("n=1000", "random"), _c("extremes", "extremes")],
    "region_mean": [_c(f"{lab} act {a}", s, cr, a) for lab, s, cr in (("2x3x8x8 crop 1", (2, 3, 10, 10), 1),
                                                                      ("2x5x17x23 crop 1", (2, 5, 19, 25), 1),
                                                                      ("1x2x32x32 crop 0", (1, 2, 32, 32), 0)) for a in (0, 1)],
}
CHECKS = {op: globals()["check_" + op] for op in CASES}


def cases(gpu):
    """(op, case) pairs of a suite."""
    return [(op, c) for op, cs in CASES.items() for c in cs if gpu or c.size < 2]


def case_id(v):
    return v.label.replace(" ", "_") if isinstance(v, Case) else str(v)


# --------------------------------------------------------------------------------------------------------------------
# batch invariance: run(n) = the operator on the first n samples of one input, batch-major
# --------------------------------------------------------------------------------------------------------------------
def _batch_runs(lib, st, dev):
    torch.manual_seed(130)
    g = {}
    d = lambda t: t.to(dev)  # noqa: E731
    nb = 9

    x4 = d(torch.randn(nb, 3, 8, 8) + 3.0)
    g["plane_mean"] = lambda n: M.plane_mean(lib, st, x4[:n])
    xb = d(torch.randn(nb, 2, 64, 64) + 3.0)
    g["plane_mean (block form)"] = lambda n: M.plane_mean(lib, st, xb[:n])
    pooled, fc1, fc2 = d(torch.randn(nb, 300) + 3.0), d(torch.randn(19, 300) / 300), d(torch.randn(300, 19))
    g["se_gate"] = lambda n: M.se_gate(lib, st, pooled[:n], fc1, fc2)
    r8, gt8, sc8 = d(torch.randn(nb, 8, 5, 7)), d(torch.rand(nb, 8) + 0.5), d(torch.randn(nb, 8, 9, 13))
    g["scale_shortcut_add"] = lambda n: M.scale_shortcut_add(lib, st, r8[:n], gt8[:n], sc8[:n], 2)

    def ssa_split(n):
        out, sp = M.scale_shortcut_add_split(lib, st, r8[:n], gt8[:n], sc8[:n], 2)
        return torch.cat([out.reshape(n, -1), sp.hi.reshape(n, -1).float(), sp.lo.reshape(n, -1).float()], 1)

    g["scale_shortcut_add_split"] = ssa_split
    xu, yu = d(torch.randn(nb, 3, 5, 7)), d(torch.randn(nb, 3, 10, 14))
    g["upsample_bilinear_add"] = lambda n: M.upsample_bilinear_add(lib, st, xu[:n], yu[:n])

    def avgpool(n):
        out = torch.zeros(n, 5, 5, 7, device=dev)
        M.adaptive_avgpool_into(lib, st, out, xa[:n], 1)
        return out

    xa = d(torch.randn(nb, 3, 17, 23) + 3.0)
    g["adaptive_avgpool_into"] = avgpool
    xd2 = d(torch.randn(nb, 3, 8, 12))
    g["downscale2x"] = lambda n: M.downscale2x(lib, st, xd2[:n])
    xl, wl, bl = d(torch.randn(nb, 260) * 2 + 5), d(torch.randn(17, 260)), d(torch.randn(17))
    g["linear"] = lambda n: M.linear(lib, st, xl[:n], wl, bl)
    xk, wk = d(torch.randn(nb, 4112) * 2 + 5), d(torch.randn(6, 4112))
    g["linear (K-split)"] = lambda n: M.linear(lib, st, xk[:n], wk, None)
    g["equal_linear"] = lambda n: M.equal_linear(lib, st, xl[:n], wl, bl, 0.01, True)
    g["pixel_norm"] = lambda n: M.pixel_norm(lib, st, xl[:n])
    xp1 = d(torch.randn(nb, 18, 70) * 2 + 5)
    g["pixel_norm_dim1"] = lambda n: M.pixel_norm_dim1(lib, st, xp1[:n])
    gl, btl = d(torch.rand(260) + 0.5), d(torch.randn(260))
    g["layernorm"] = lambda n: M.layernorm(lib, st, xl[:n], 260, gl, btl, 1e-5, True)
    xs, gs, bs = d(torch.randn(nb, 5, 64, 64) * 2 + 5), d(torch.rand(5) + 0.5), d(torch.randn(5))
    g["sample_layernorm"] = lambda n: M.sample_layernorm(lib, st, xs[:n], gs, bs, 1e-5, 0.2)
    xm, gm, bm = d(torch.randn(nb, 77)), d(torch.randn(nb, 77)), d(torch.randn(nb, 77))
    g["modulate"] = lambda n: M.modulate(lib, st, xm[:n], gm[:n], bm[:n], True)
    xg, lg, ag = d(torch.randn(nb, 3, 9, 11)), d(torch.randn(nb, 3)), d(torch.randn(nb, 3))
    g["gate"] = lambda n: M.gate(lib, st, xg[:n], lg[:n], xg[:n], ag[:n], 1.0)
    bv7 = d(torch.randn(7))
    g["axpby"] = lambda n: M.axpby(lib, st, xm[:n], 0.75, bv7, -1.25)
    g["add_bcast"] = lambda n: M.add_bcast(lib, st, xm[:n], bv7)
    g["maxpool3x3s2"] = lambda n: M.maxpool3x3s2(lib, st, xg[:n])
    g["upsample_nearest"] = lambda n: M.upsample_nearest(lib, st, xg[:n], 13, 17)
    lgt, rm = d(torch.randn(nb, 19, 8, 10)), d(torch.randperm(19).to(torch.int32))
    g["parsing_mask"] = lambda n: M.parsing_mask(lib, st, lgt[:n], rm, (40, 56), (16, 16))
    xbc, k2 = d(torch.randn(nb, 2, 8, 16) + 3.0), d(bicubic_taps(2))
    g["bicubic_down"] = lambda n: M.bicubic_down(lib, st, xbc[:n], k2, 2)
    msk = d((torch.rand(nb, 1, 17, 23) > 0.7).float())
    g["dilate_erode"] = lambda n: torch.cat(M.dilate_erode(lib, st, msk[:n], 2), 1)
    # feature-major operators: the tokens of an image are columns i * seq .. (i + 1) * seq - 1
    seq = 17
    xc, gc, bc = torch.randn(1040, nb, seq) * 2 + 5, d(torch.rand(1040) + 0.5), d(torch.randn(1040))
    tok = lambda t, n: d(t[:, :n].reshape(t.shape[0], n * seq).contiguous())  # noqa: E731
    back = lambda y, n: y.reshape(y.shape[0], n, seq).transpose(0, 1)  # noqa: E731
    g["channel_layernorm (re-reading form)"] = lambda n: back(M.channel_layernorm(lib, st, tok(xc, n), gc, bc), n)
    g["channel_layernorm"] = lambda n: back(M.channel_layernorm(lib, st, tok(xc[:768], n), gc[:768], bc[:768]), n)
    qkv = torch.randn(3 * 128, nb, seq)
    g["mha_small"] = lambda n: back(M.mha_small(lib, st, tok(qkv, n), n, seq, 2), n)
    g["quick_gelu"] = lambda n: M.quick_gelu(lib, st, xm[:n])
    g["tanh"] = lambda n: M.tanh(lib, st, xm[:n])
    xr, lab = _region_inputs((nb, 5, 19, 25), 1)
    xr, lab = d(xr), d(lab)
    g["region_mean"] = lambda n: M.region_mean(lib, st, xr[:n], lab[:n], 1, True)
    return g


def _big_batch_runs(lib, st, dev):
    """Grid-stride kernels: five samples cross 524288 elements (outputs), three do not."""
    torch.manual_seed(131)
    g = {}
    d = lambda t: t.to(dev)  # noqa: E731
    nb, m = 5, BIG[1]
    pl = (nb,) + BIG_PLANES[1:]
    a, b2, c2 = d(torch.randn(nb, m)), d(torch.randn(nb, m)), d(torch.randn(nb, m))
    bv = d(torch.randn(49))
    g["modulate"] = lambda n: M.modulate(lib, st, a[:n], b2[:n], c2[:n], True)
    g["axpby"] = lambda n: M.axpby(lib, st, a[:n], 0.75, bv, -1.25)
    g["add_bcast"] = lambda n: M.add_bcast(lib, st, a[:n], bv)
    lg = d(torch.randn(nb, 1))
    g["gate"] = lambda n: M.gate(lib, st, a[:n].view((n,) + pl[1:]), lg[:n], b2[:n].view((n,) + pl[1:]), lg[:n], 1.0)
    g["scale_shortcut_add"] = lambda n: M.scale_shortcut_add(lib, st, a[:n].view((n,) + pl[1:]), lg[:n], b2[:n].view((n,) + pl[1:]), 1)
    xu, yu = d(torch.randn(nb, 7, 16, 16)), d(torch.randn(nb, 7, 128, 128))  # 7 * 16384 outputs per sample
    g["upsample_bilinear_add"] = lambda n: M.upsample_bilinear_add(lib, st, xu[:n], yu[:n])
    g["upsample_nearest"] = lambda n: M.upsample_nearest(lib, st, xu[:n], 128, 128)
    xd2 = d(torch.randn(nb, 7, 256, 256))
    g["downscale2x"] = lambda n: M.downscale2x(lib, st, xd2[:n])
    g["maxpool3x3s2"] = lambda n: M.maxpool3x3s2(lib, st, xd2[:n])
    lgt = d(torch.randn(nb, 19, 8, 10))
    g["parsing_mask"] = lambda n: M.parsing_mask(lib, st, lgt[:n], None, (330, 330), (330, 330))  # 108900 pixels per image
    msk = d((torch.rand(nb, 1, 330, 330) > 0.7).float())
    g["dilate_erode"] = lambda n: torch.cat(M.dilate_erode(lib, st, msk[:n], 2), 1)
    return g


BATCH_OPS = ["plane_mean", "plane_mean (block form)", "se_gate", "scale_shortcut_add", "scale_shortcut_add_split",
             "upsample_bilinear_add", "adaptive_avgpool_into", "downscale2x", "linear", "linear (K-split)", "equal_linear",
             "pixel_norm", "pixel_norm_dim1", "layernorm", "sample_layernorm", "modulate", "gate", "axpby", "add_bcast",
             "maxpool3x3s2", "upsample_nearest", "parsing_mask", "bicubic_down", "dilate_erode", "channel_layernorm",
             "channel_layernorm (re-reading form)", "mha_small", "quick_gelu", "tanh", "region_mean"]
BIG_BATCH_OPS = ["modulate", "axpby", "add_bcast", "gate", "scale_shortcut_add", "upsample_bilinear_add", "upsample_nearest",
                 "downscale2x", "maxpool3x3s2", "parsing_mask", "dilate_erode"]


def check_batch_invariance(lib, st, dev, op):
    invariant(op, _batch_runs(lib, st, dev)[op])


def check_big_batch_invariance(lib, st, dev, op):
    assert 5 * BIG[1] > GRID >= 3 * BIG[1]
    invariant(op, _big_batch_runs(lib, st, dev)[op], pairs=((5, 3),))


def check_size_refusals(lib):
    """Size arguments outside the documented ranges are refused before any launch (valid pointers, nothing runs)."""
    t = torch.zeros(64)
    p = t.data_ptr()
    assert lib.hf_plane_mean_f32(p, p, 0, 4, None) != 0
    assert lib.hf_downscale2x_f32(p, p, 1, 3, 4, None) != 0              # odd height
    assert lib.hf_mha_small_f32(p, p, 1, 65, 1, 64, None) != 0           # beyond the sequence limit
    assert lib.hf_mha_small_f32(p, p, 1, 4, 1, 32, None) != 0            # head dim other than 64
    assert lib.hf_dilate_erode_f32(p, p, p, 1, 4, 4, 65, None) != 0      # beyond the radius limit
    assert lib.hf_bicubic_down_f32(p, p, p, 1, 6, 8, 2, None) != 0       # fewer rows than taps
    assert lib.hf_layernorm_grouped_f32(p, p, p, p, 4, 8, 3, 1e-5, 0, 0.0, None) != 0  # rows % groups
    assert lib.hf_scale_shortcut_add_f32(p, p, p, p, 2, 1, 1, 3, 3, 4, 4, None) != 0   # shortcut too small for the stride
    assert lib.hf_sample_layernorm_f32(p, p, None, None, 1, 1, 1, 0, 1e-5, 1.0, p, 64, None) != 0  # n < 2
