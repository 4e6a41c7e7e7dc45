"""TEST INFRASTRUCTURE - direct checks of the generator's glue kernels (csrc/upfirdn2d.hip, torgb.hip, style.hip,
elementwise.hip) and of every conv route that contains the 4x4 filter, shared by the hipsim tests
(tests/test_sim_generator_ops.py) and the GPU tests (tests/test_gpu_generator_ops.py).  Built like tests/small_ops_checks.py,
whose rules (accuracy, exact, sentinels, batch invariance) are imported, not copied.

Every reference is restated here from the operation's definition, in torch fp64 on the CPU; a filter is: zero-insert per axis,
F.pad per side (negative crops), F.conv2d with the flipped kernel, then every down-th sample.  Inputs come from
torch.manual_seed on the CPU; whatever is summed carries a DC offset.

Filters.  Every 4x4 kernel the rest of the suite passes is [1,3,3,1] x [1,3,3,1]: equal to its flip and its transpose.  Here
KA = randn(4, 4) (non-separable) and KS = outer([0.3,1.1,0.7,-0.2], [0.9,-0.4,1.3,0.5]) (for the routes that factor the kernel)
are neither; each check that takes a filter also runs once with the product's symmetric kernel."""
import types

import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from oracle import ref_stylegan2 as O
from tests.conv_kernel_checks import presplit, styled_layer
from tests.small_ops_checks import ROWS, SENTINEL, Case, _c, _guard_ok, _guarded, _offset_view, _sync, accuracy, exact, invariant  # noqa: F401

ALPHA = float(torch.tensor(0.2, dtype=torch.float32))        # the fp32 values the kernels receive
SQRT2 = float(torch.tensor(2.0 ** 0.5, dtype=torch.float32))
HSENT = -12344.0             # fp16 sentinel (exactly representable)
TOL = 2e-5                   # conv routes on the interpreter: of max(1, |ref|max), as tests/test_sim_kernels.py
REL = 1e-4                   # conv routes on the GPU: close() of tests/test_gpu_parity.py


def filt(kind):
    if kind == "KA":
        torch.manual_seed(200)
        return torch.randn(4, 4)
    if kind == "KS":
        return torch.outer(torch.tensor([0.3, 1.1, 0.7, -0.2]), torch.tensor([0.9, -0.4, 1.3, 0.5]))
    assert kind == "sym"
    k = torch.tensor([1.0, 3.0, 3.0, 1.0])
    return torch.outer(k, k) / 16.0  # blur_kernel_1d_to_2d(gain=4)


def upfirdn_ref(x, k, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    """upfirdn2d from its definition, in x's dtype."""
    n, c, h, w = x.shape
    kh, kw = k.shape
    u = x.new_zeros(n * c, 1, h * up_y, w * up_x)
    u[:, :, ::up_y, ::up_x] = x.reshape(n * c, 1, h, w)
    z = F.conv2d(F.pad(u, [px0, px1, py0, py1]), torch.flip(k, [0, 1]).reshape(1, 1, kh, kw).to(x.dtype))
    z = z[:, :, ::down_y, ::down_x]
    return z.reshape(n, c, z.shape[2], z.shape[3])


def lrelu(v):
    return F.leaky_relu(v, ALPHA) * SQRT2


def _dd(t):
    return None if t is None else t.double()


def _dv(t, dev):
    return None if t is None else t.to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------------------------------------
# upfirdn2d.hip: the generic FIR
# --------------------------------------------------------------------------------------------------------------------
def check_upfirdn2d(lib, st, dev, case):
    shape, kshape, up, down, pad, sym = case.args
    torch.manual_seed(201)
    x = torch.randn(shape) + 1.0
    k = filt("sym") if sym else torch.randn(kshape)
    args = (up[0], up[1], down[0], down[1]) + tuple(pad)
    xd, kd = x.to(dev), k.to(dev)
    got = M.upfirdn2d(lib, st, xd, kd, *args)
    accuracy("upfirdn2d", case.label, got, upfirdn_ref(x.double(), k.double(), *args), upfirdn_ref(x, k, *args))
    n = got.numel()
    buf = _guarded(n, dev)
    rc = lib.hf_upfirdn2d_f32(buf.data_ptr(), xd.data_ptr(), kd.data_ptr(), shape[0] * shape[1], shape[2], shape[3],
                              k.shape[0], k.shape[1], *args, st)
    _guard_ok("upfirdn2d", case.label, buf, n, rc)


# --------------------------------------------------------------------------------------------------------------------
# upfirdn2d.hip: blur 4x4 pad (1,1) + noise + bias + lrelu, fp32 and split outputs
# --------------------------------------------------------------------------------------------------------------------
def _blur_inputs(b, c, in_h, in_w, pitch, noise, bias, seed):
    torch.manual_seed(seed)
    tmp = torch.randn(b, c, in_h, pitch) + 1.0
    nz = None if noise == "none" else torch.randn(b if noise == "per" else 1, 1, in_h - 1, in_w - 1)
    return tmp, nz, torch.tensor([0.3]), torch.randn(c) if bias else None


def _blur_restated(tmp, in_w, k, nz, nw, bv):
    y = upfirdn_ref(tmp[..., :in_w], k.to(tmp.dtype), 1, 1, 1, 1, 1, 1, 1, 1)
    if nz is not None:
        y = y + nw.to(y.dtype) * nz.to(y.dtype)
    return y if bv is None else lrelu(y + bv.to(y.dtype).view(1, -1, 1, 1))  # no bias: the plain blur


def _blur_call(lib, st, dev, tmp, in_w, k, nz, nw, bv, out_floats=0):
    """hf_blur_noise_bias_act_f32 into a guarded buffer that starts out_floats floats into its storage."""
    b, c, in_h, pitch = tmp.shape
    oh, ow = in_h - 1, in_w - 1
    n = b * c * oh * ow
    buf = _guarded(n + out_floats, dev)
    nbs = oh * ow if nz is not None and nz.shape[0] == b and b > 1 else 0
    rc = lib.hf_blur_noise_bias_act_f32(buf.data_ptr() + 4 * out_floats, tmp.data_ptr(), k.data_ptr(), _ptr(nz), nw.data_ptr() if nz is not None else None,
                                        nbs, _ptr(bv), b, c, in_h, in_w, pitch, ALPHA, SQRT2, st)
    return buf, buf[out_floats:out_floats + n].view(b, c, oh, ow), rc


def check_blur_f32(lib, st, dev, case):
    b, c, in_h, in_w, pitch, noise, bias, offset, kind = case.args
    tmp, nz, nw, bv = _blur_inputs(b, c, in_h, in_w, pitch, noise, bias, 202)
    k = filt(kind)
    tmp_d, k_d, nw_d, bv_d = tmp.to(dev), k.to(dev), nw.to(dev), _dv(bv, dev)
    nz_d = _offset_view(nz, dev) if offset == "noise" else _dv(nz, dev)
    off = 1 if offset == "out" else 0
    buf, out, rc = _blur_call(lib, st, dev, tmp_d, in_w, k_d, nz_d, nw_d, bv_d, off)
    _guard_ok("blur_f32", case.label, buf, out.numel() + off, rc)
    assert off == 0 or float(buf[0]) == SENTINEL
    accuracy("blur_f32", case.label, out, _blur_restated(tmp.double(), in_w, k.double(), _dd(nz), nw.double(), _dd(bv)),
             _blur_restated(tmp, in_w, k, nz, nw, bv))
    if offset:  # a pointer one float off takes the scalar kernel: the same fmaf chain per output as the vector form
        _, aligned, rc = _blur_call(lib, st, dev, tmp_d, in_w, k_d, _dv(nz, dev), nw_d, bv_d)
        assert rc == 0
        _sync(dev)
        exact("blur_f32", case.label + " == aligned call", out, aligned.cpu())


def check_blur_split(lib, st, dev, case):
    b, c, oh, ow, extra, noise, bias, snext, lo, kind = case.args
    in_h, in_w = oh + 1, ow + 1
    tmp, nz, nw, bv = _blur_inputs(b, c, in_h, in_w, in_w + extra, noise, bias, 203)
    s2 = torch.rand(b, c) + 0.5 if snext else None
    k = filt(kind)
    tmp_d, k_d, nz_d, nw_d, bv_d, s2_d = tmp.to(dev), k.to(dev), _dv(nz, dev), nw.to(dev), _dv(bv, dev), _dv(s2, dev)
    # the fp32 blur of the same case: checked against fp64 here, then the yardstick of the split's bits
    buf, out, rc = _blur_call(lib, st, dev, tmp_d, in_w, k_d, nz_d, nw_d, bv_d)
    _guard_ok("blur_split", case.label, buf, out.numel(), rc)
    accuracy("blur_split (its fp32 blur)", case.label, out, _blur_restated(tmp.double(), in_w, k.double(), _dd(nz), nw.double(), _dd(bv)),
             _blur_restated(tmp, in_w, k, nz, nw, bv))
    n = b * c * oh * ow  # halves per part
    hbuf = torch.full((2 * n + 512,), HSENT, dtype=torch.float16, device=dev)  # hi | lo | guard
    nbs = oh * ow if noise == "per" and b > 1 else 0
    rc = lib.hf_blur_noise_bias_act_split_f16(hbuf.data_ptr(), hbuf.data_ptr() + 2 * n if lo else None, tmp_d.data_ptr(), k_d.data_ptr(),
                                              _ptr(nz_d), nw_d.data_ptr() if nz is not None else None, nbs, _ptr(bv_d), _ptr(s2_d), b, c,
                                              in_h, in_w, in_w + extra, ALPHA, SQRT2, st)
    _sync(dev)
    assert rc == 0, ("blur_split", case.label, rc)
    eh, el = M.split_activation_reference(out.cpu(), s2)
    h = hbuf.cpu()
    exact("blur_split", case.label + " hi", h[:n].view(eh.shape), eh)
    if lo:
        exact("blur_split", case.label + " lo", h[n:2 * n].view(el.shape), el)
    assert bool((h[(2 if lo else 1) * n:] == HSENT).all()), ("blur_split", case.label, "write behind the output" if lo else "lo written")


# --------------------------------------------------------------------------------------------------------------------
# torgb.hip
# --------------------------------------------------------------------------------------------------------------------
def _torgb_restated(x, wt, s, bias, skip, k):
    y = torch.einsum("bihw,ic->bchw", x if s is None else x * s[:, :, None, None], wt[0])
    if bias is not None:
        y = y + bias.view(1, 3, 1, 1)
    return y if skip is None else y + upfirdn_ref(skip, k.to(x.dtype), 2, 2, 1, 1, 2, 1, 2, 1)


def _torgb_inputs(b, cin, h, w, skip, seed=204):
    torch.manual_seed(seed)
    x, wt = torch.randn(b, cin, h, w) + 0.5, torch.randn(1, cin, 3) + 0.5
    return x, wt, torch.rand(b, cin) + 0.5, torch.randn(3), torch.randn(b, 3, h // 2, w // 2) + 1.0 if skip else None


def check_torgb(lib, st, dev, case):
    b, cin, h, w, skip, kind, form = case.args
    x, wt, s, bias, sk = _torgb_inputs(b, cin, h, w, skip)
    if form == "finish":  # the finishing pass of a fused ToRGB: no style, no bias
        s = bias = None
    k = filt(kind) if skip else None
    xd = _offset_view(x, dev) if form == "offset" else x.to(dev)
    rest = (wt.to(dev), _dv(s, dev), _dv(bias, dev), _dv(sk, dev), _dv(k, dev))
    got = M.torgb(lib, st, xd, *rest)
    accuracy("torgb", case.label, got, _torgb_restated(x.double(), wt.double(), _dd(s), _dd(bias), _dd(sk), _dd(k)),
             _torgb_restated(x, wt, s, bias, sk, k))
    if form == "offset":  # VEC 1 with a skip: the per-pixel form states the products of the four-pixel form in the same order
        exact("torgb", case.label + " == aligned call", got, M.torgb(lib, st, x.to(dev), *rest).cpu())


# --------------------------------------------------------------------------------------------------------------------
# elementwise.hip
# --------------------------------------------------------------------------------------------------------------------
def check_fused_bias_act(lib, st, dev, case):
    shape, bias, offset = case.args
    torch.manual_seed(205)
    x = torch.randn(shape)
    bv = torch.randn(shape[1]) if bias else None
    bshape = [1, -1] + [1] * (len(shape) - 2)
    re = lambda x_, b_: lrelu(x_ if b_ is None else x_ + b_.view(bshape))  # noqa: E731
    xd, bd = x.to(dev), _dv(bv, dev)
    got = M.fused_bias_act(lib, st, _offset_view(x, dev) if offset else xd, bd, ALPHA, SQRT2)
    accuracy("fused_bias_act", case.label, got, re(x.double(), _dd(bv)), re(x, bv))
    if offset:
        exact("fused_bias_act", case.label + " == aligned call", got, M.fused_bias_act(lib, st, xd, bd, ALPHA, SQRT2).cpu())
    n = x.numel()
    buf = _guarded(n, dev)
    step_b = 1
    for d in shape[2:]:
        step_b *= d
    rc = lib.hf_fused_bias_act_f32(buf.data_ptr(), xd.data_ptr(), _ptr(bd), n, shape[1] if bias else 1, step_b, ALPHA, SQRT2, st)
    _guard_ok("fused_bias_act", case.label, buf, n, rc)


def check_noise_bias_act(lib, st, dev, case):
    shape, noise, bias, offset = case.args
    torch.manual_seed(206)
    b, c, h, w = shape
    x = torch.randn(shape)
    nz = None if noise == "none" else torch.randn(b if noise == "per" else 1, 1, h, w)
    nw, bv = torch.tensor([0.3]), torch.randn(c) if bias else None

    def re(x_, nz_, nw_, b_):  # the activation is applied with or without a bias
        y = x_ if nz_ is None else x_ + nw_ * nz_
        return lrelu(y if b_ is None else y + b_.view(1, -1, 1, 1))

    rest = (_dv(nz, dev), nw.to(dev) if nz is not None else None, _dv(bv, dev), ALPHA, SQRT2)
    got = M.noise_bias_act(lib, st, _offset_view(x, dev) if offset else x.to(dev), *rest)
    accuracy("noise_bias_act", case.label, got, re(x.double(), _dd(nz), nw.double(), _dd(bv)), re(x, nz, nw, bv))
    if offset:  # scalar kernel: fmaf(nw, z, x), + bias, activation - the vector kernel's statements
        exact("noise_bias_act", case.label + " == aligned call", got, M.noise_bias_act(lib, st, x.to(dev), *rest).cpu())


# --------------------------------------------------------------------------------------------------------------------
# style.hip
# --------------------------------------------------------------------------------------------------------------------
def _mod_restated(lat, w, bv):
    return F.linear(lat, w * (1.0 / w.shape[1] ** 0.5), bv)


def _demod_restated(s, wsq):
    return torch.rsqrt((wsq[None] * (s * s)[:, None, :]).sum(2) + 1e-8)


def check_modulation_demod(lib, st, dev, case):
    b, cin, sd, cout, strided = case.args
    torch.manual_seed(207)
    latent = torch.randn(b, 7, sd) + 0.5
    mw, mb, wsq = torch.randn(cin, sd) + 0.25, torch.randn(cin) + 1.0, torch.rand(cout, cin) + 0.1
    lat = latent[:, 4]
    style = latent.to(dev)[:, 4] if strided else lat.contiguous().to(dev)
    mwd, mbd, wsqd = mw.to(dev), mb.to(dev), wsq.to(dev)
    s = M.modulation(lib, st, style, mwd, mbd)
    accuracy("modulation", case.label, s, _mod_restated(lat.double(), mw.double(), mb.double()), _mod_restated(lat, mw, mb))
    buf = _guarded(b * cin, dev)
    rc = lib.hf_modulation_f32(buf.data_ptr(), style.data_ptr(), style.stride(0) if b > 1 else sd, mwd.data_ptr(), mbd.data_ptr(), b, cin, sd, st)
    _guard_ok("modulation", case.label, buf, b * cin, rc)
    s_in = _mod_restated(lat, mw, mb)  # demod's input: ATen's fp32 modulation, not the kernel's
    sd_in = s_in.to(dev)
    d = M.demod(lib, st, sd_in, wsqd)
    accuracy("demod", case.label, d, _demod_restated(s_in.double(), wsq.double()), _demod_restated(s_in, wsq))
    buf = _guarded(b * cout, dev)
    rc = lib.hf_demod_f32(buf.data_ptr(), sd_in.data_ptr(), wsqd.data_ptr(), b, cin, cout, st)
    _guard_ok("demod", case.label, buf, b * cout, rc)


def check_prepare_weights(lib, st, dev, case):
    cout, cin, k = case.args
    torch.manual_seed(208)
    weight = torch.randn(1, cout, cin, k, k) + 0.5
    wt, wsq = M.prepare_weights(lib, st, weight.to(dev))
    scale = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(cin * k * k))))  # 1.0f / sqrtf((float)(cin k k))
    v = weight[0] * scale  # one rounding per element
    exact("prepare_weights", case.label + " wt", wt, v.permute(2, 3, 1, 0).reshape(k * k, cin, cout).contiguous())
    accuracy("prepare_weights wsq", case.label, wsq, (v.double() ** 2).sum((2, 3)), (v * v).sum((2, 3)))


def _style_convs(dev, sd, seed=209):
    """The three jobs: (cin -> cout, demodulated, latent row)."""
    torch.manual_seed(seed)
    convs, rows = [], []
    for cin, cout, demod, row in ((6, 300, True, 0), (70, 3, False, 4), (264, 8, True, 2)):
        wsq = (torch.rand(cout, cin) + 0.1).to(dev)
        convs.append(types.SimpleNamespace(in_channel=cin, out_channel=cout, demodulate=demod,
                                           modulation=types.SimpleNamespace(weight=(torch.randn(cin, sd) + 0.25).to(dev),
                                                                            bias=(torch.randn(cin) + 1.0).to(dev)),
                                           prepared=lambda wsq=wsq: (None, wsq)))
        rows.append(row)
    return convs, rows


def _style_batch(lib, st, dev, latent, convs, rows):
    table, layout, total = M.style_job_table(convs, rows, latent.shape[0], dev)
    res = M.style_batch(lib, st, latent, table, layout, total, 264, 300)
    _sync(dev)  # the table must outlive the launches
    return res


def check_style_batch(lib, st, dev, case):
    b, sd = case.args
    convs, rows = _style_convs(dev, sd)
    torch.manual_seed(210)
    latent = torch.randn(b, 7, sd) + 0.5
    lat_d = latent.to(dev)
    res = _style_batch(lib, st, dev, lat_d, convs, rows)
    for i, (c, row, (s, d)) in enumerate(zip(convs, rows, res)):
        mw, mb = c.modulation.weight.cpu(), c.modulation.bias.cpu()
        s1 = M.modulation(lib, st, lat_d[:, row], c.modulation.weight, c.modulation.bias)
        lat = latent[:, row]
        accuracy("style_batch (per-layer modulation)", f"{case.label} job {i}", s1, _mod_restated(lat.double(), mw.double(), mb.double()),
                 _mod_restated(lat, mw, mb))
        if not c.demodulate:
            exact("style_batch", f"{case.label} job {i} s", s, s1.cpu())
            assert d is None
            continue
        wsq = c.prepared()[1]
        d1 = M.demod(lib, st, s1, wsq)
        s_in = s1.cpu()
        accuracy("style_batch (per-layer demod)", f"{case.label} job {i}", d1, _demod_restated(s_in.double(), wsq.cpu().double()),
                 _demod_restated(s_in, wsq.cpu()))
        M.style_normalize(lib, st, s1, d1)
        exact("style_batch", f"{case.label} job {i} s", s, s1.cpu())
        exact("style_batch", f"{case.label} job {i} d", d, d1.cpu())
        m = s.cpu().abs().amax(1)
        assert float(m.min()) >= 1.0 and float(m.max()) < 2.0


def _normalize_expected(s, d):
    m = s.abs().amax(1)
    e = torch.frexp(m).exponent - 1                       # floor(log2 max|s|)
    acts = (m > 0) & (e > -120) & (e < 120) & (e != 0)
    e = torch.where(acts, e, torch.zeros_like(e))
    return torch.ldexp(s, -e[:, None]), torch.ldexp(d, e[:, None]), acts


def check_style_normalize(lib, st, dev, case):
    cin, cout = case.args
    torch.manual_seed(211)
    peaks = [0.0, 4.0, 1.5, 3.9999998, 1e-30, 1e-37]
    s = torch.rand(len(peaks), cin) * 0.9 * torch.where(torch.rand(len(peaks), cin) < 0.5, -1.0, 1.0)
    s[:, cin - 1] = 1.0  # the row maximum sits in the last element: the last trip of the loop
    s = s * torch.tensor(peaks, dtype=torch.float32)[:, None]
    d = torch.rand(len(peaks), cout) + 0.5
    assert [float(v) for v in s.abs().amax(1)] == [float(torch.tensor(p, dtype=torch.float32)) for p in peaks]
    want_s, want_d, acts = _normalize_expected(s, d)
    assert acts.tolist() == [False, True, False, True, True, False]
    sbuf, dbuf = _guarded(s.numel(), dev), _guarded(d.numel(), dev)
    sbuf[:s.numel()] = s.flatten().to(dev)
    dbuf[:d.numel()] = d.flatten().to(dev)
    rc = lib.hf_style_normalize_f32(sbuf.data_ptr(), dbuf.data_ptr(), len(peaks), cin, cout, st)
    _guard_ok("style_normalize", case.label, sbuf, s.numel(), rc)
    _guard_ok("style_normalize", case.label, dbuf, d.numel(), rc)
    got_s, got_d = sbuf[:s.numel()].view(s.shape), dbuf[:d.numel()].view(d.shape)
    exact("style_normalize", case.label + " s", got_s, want_s)
    exact("style_normalize", case.label + " d", got_d, want_d)
    assert torch.equal(want_s[~acts], s[~acts]) and torch.equal(want_d[~acts], d[~acts])  # the leave-alone rows
    m = got_s.cpu().abs().amax(1)[acts]
    assert bool((m >= 1.0).all()) and bool((m < 2.0).all())
    assert float(m[0]) == 1.0 and float(got_d.cpu()[1, 0]) == 4.0 * float(d[1, 0])


# --------------------------------------------------------------------------------------------------------------------
# KS through every conv route that contains a filter
# --------------------------------------------------------------------------------------------------------------------
def close(lib_is_sim, what, got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err, scale = float((got - ref).abs().max()), max(1.0, float(ref.abs().max()))
    print(f"generator_ops {what}: max-abs {err:.2e}, scale {scale:.2f}")
    if lib_is_sim:
        assert err < TOL * scale, (what, err, scale)
    else:
        assert err <= REL * scale, (what, err, scale)
        assert float(((got - ref) ** 2).mean()) <= 1e-8 * max(1.0, float(ref.var())), what


def check_conv_route(lib, st, dev, case):
    route, shape, kind = case.args
    B, cin, cout, H, W = shape
    sim = dev.type == "cpu"
    L = styled_layer(lib, st, dev, shape, 212, True)
    c, k = L.cpu, filt(kind)
    full = O.fused_leaky_relu(O.modulated_conv2d(c.x.double(), c.sty.double(), c.wgt.double(), c.mw.double(), c.mb.double(), True, True,
                                                 blur_kernel=k.double()) + c.nw.double() * c.nz.double(), c.bias.double())
    kd, tail = k.to(dev), (L.nz, L.nw, L.bias)
    M.style_normalize(lib, st, L.s, L.dm)
    if route == "fp32_up":
        y = M.modconv3x3_up(lib, st, L.x, L.wt, L.s, L.dm, kd, *tail)
    elif route == "two_pass_f16":
        assert M.modconv3x3_up_f16_supported(cin, cout, H, W)
        y = M.modconv3x3_up(lib, st, L.x, L.wt, L.s, L.dm, kd, *tail, f16=(L.hi, L.lo, 3))
        assert lib.hf_debug_last_path() == 563
    elif route == "fused":
        fac = M.blur_factors(k)
        assert fac is not None and M.modconv3x3_up_fused_supported(cin, cout, H, W)
        y = M.modconv3x3_up_fused(lib, st, L.x, L.hi, L.lo, L.s, L.dm, fac, *tail)
        assert lib.hf_debug_last_path() == 573
        s2 = (torch.rand(B, cout) + 0.5).to(dev)
        sp = M.modconv3x3_up_fused(lib, st, L.x, L.hi, L.lo, L.s, L.dm, fac, *tail, split_for=s2)
        _sync(dev)
        eh, el = M.split_activation_reference(y.cpu(), s2.cpu())
        exact("conv_route", case.label + " split hi", sp.hi, eh)
        exact("conv_route", case.label + " split lo", sp.lo, el)
    else:
        assert route == "small_up_blur"
        w9 = M.split_weights_small(lib, st, L.wt)
        assert M.small_up_blur_supported(H, W)
        y = M.modconv3x3_small_up_blur(lib, st, L.x, w9, 3, L.s, L.dm, kd, *tail, cout)
        assert lib.hf_debug_last_path() == 705
    _sync(dev)
    close(sim, f"conv_route {case.label}", y, full)


def check_rows_image(lib, st, dev, case):
    """The row pipeline's image epilogue (skip ring): hf_modconv3x3_f16_pre_image_f32 with the filter equals the raw product plus
    hf_torgb_f32's finishing pass with the same filter (itself checked against fp64 by check_torgb), bit for bit."""
    (B, H, W), kind = case.args
    L = styled_layer(lib, st, dev, (B, 32, 32, H, W), 213, False, rgb=True)
    skip, rgb_bias, k = L.skip + 1.0, L.brgb.view(1, 3, 1, 1), filt(kind).to(dev)
    conv = (presplit(L), L.hi, L.lo, 3, L.dm, L.nz, L.nw, L.bias)
    _, raw = M.modconv3x3_f16_pre(lib, st, *conv, rgb=(L.wtr, L.sr))
    want = M.torgb(lib, st, raw, torch.eye(3).reshape(1, 3, 3).to(dev), None, rgb_bias, skip, k)
    img = M.modconv3x3_f16_pre_image(lib, st, *conv, (L.wtr, L.sr), rgb_bias, skip, k)
    assert img is not None and lib.hf_debug_last_path() == 579
    _sync(dev)
    exact("rows_image", case.label, img, want.cpu())
    # the finishing pass it is compared with, against the definition
    ref = raw.cpu().double() + rgb_bias.cpu().double() + upfirdn_ref(skip.cpu().double(), k.cpu().double(), 2, 2, 1, 1, 2, 1, 2, 1)
    t32 = raw.cpu() + rgb_bias.cpu() + upfirdn_ref(skip.cpu(), k.cpu(), 2, 2, 1, 1, 2, 1, 2, 1)
    accuracy("rows_image (finishing pass)", case.label, want, ref, t32)


# --------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes that reach each branch (size classes as in small_ops_checks)
# --------------------------------------------------------------------------------------------------------------------
_BLUR_BASE = (2, 3, 9, 9, 12, "per", True)
CASES = {
    "upfirdn2d": [
        _c("2x3x7x9 k3x5 up 2,1 down 1,2", (2, 3, 7, 9), (3, 5), (2, 1), (1, 2), (2, 1, 0, 3), False),
        _c("1x2x6x5 k8x8 up 3,2 down 2,3: tap limit", (1, 2, 6, 5), (8, 8), (3, 2), (2, 3), (7, 4, 5, 6), False),
        _c("1x1x5x5 k1x1", (1, 1, 5, 5), (1, 1), (1, 1), (1, 1), (0, 0, 0, 0), False),
        _c("1x2x9x9 k4x4 negative pads", (1, 2, 9, 9), (4, 4), (1, 1), (1, 1), (-1, 2, 3, -2), False),
        _c("1x2x9x9 symmetric kernel, negative pads", (1, 2, 9, 9), (4, 4), (1, 1), (1, 1), (-1, 2, 3, -2), True),
        _c("3x5x33x47 k4x2 up 2,2", (3, 5, 33, 47), (4, 2), (2, 2), (1, 1), (2, 1, 1, 0), False),
        _c("1x3x600x600 k4x4: past the grid cap", (1, 3, 600, 600), (4, 4), (1, 1), (1, 1), (1, 1, 1, 1), False, size=1),
    ],
    # (B, C, in_h, in_w, pitch, noise, bias, offset pointer, filter)
    "blur_f32": [
        _c("2x3x9x9 pitch 12: vec4, cq 2, rpt shrunk, plane % channels", *_BLUR_BASE, None, "KA"),
        _c("2x3x9x9 pitch 12, symmetric kernel", *_BLUR_BASE, None, "sym"),
        _c("1x2x5x5 pitch 5: out_w 4, cq 1, plain blur", 1, 2, 5, 5, 5, "none", False, None, "KA"),
        _c("2x2x131x261 pitch 264 shared noise: vec4, second block column of one quad, second block row", 2, 2, 131, 261, 264,
           "shared", True, None, "KA"),
        _c("1x1x7x13 pitch 16: vec4, last quad of the block inactive", 1, 1, 7, 13, 16, "per", True, None, "KA"),
        _c("1x1x8x66 pitch 66: scalar, out 7x65, column block of one, out_h % 4 = 3", 1, 1, 8, 66, 66, "per", True, None, "KA"),
        _c("1x2x131x66 pitch 68: scalar, second block row", 1, 2, 131, 66, 68, "per", True, None, "KA"),
        _c("1x1x3x5 pitch 8: out 2x4", 1, 1, 3, 5, 8, "none", True, None, "KA"),
        _c("2x1x2x2 pitch 2: 1x1 outputs", 2, 1, 2, 2, 2, "per", True, None, "KA"),
        _c("2x3x9x9 pitch 12, out offset: scalar kernel", *_BLUR_BASE, "out", "KA"),
        _c("2x3x9x9 pitch 12, noise offset: scalar kernel", *_BLUR_BASE, "noise", "KA"),
    ],
    # (B, C, out_h, out_w, extra pitch, noise, bias, s_next, lo, filter)
    "blur_split": [
        _c("1x8x5x61: exactly one wave", 1, 8, 5, 61, 0, "per", True, True, True, "KA"),
        _c("1x8x5x61 symmetric kernel", 1, 8, 5, 61, 0, "per", True, True, True, "sym"),
        _c("1x8x9x62 pitch +3: second wave of one column, no s_next, no lo", 1, 8, 9, 62, 3, "none", True, False, False, "KA"),
        _c("2x16x70x123 pitch +1 shared noise: three waves, strips, no bias", 2, 16, 70, 123, 1, "shared", False, True, True, "KA"),
        _c("1x8x1x1: the smallest plane", 1, 8, 1, 1, 0, "per", True, True, True, "KA"),
        _c("1x8x33x489: nine waves, a second block of waves", 1, 8, 33, 489, 0, "per", True, True, True, "KA"),
    ],
    # (B, cin, h, w, skip, filter, form)
    "torgb": [
        _c("2x5x6x8 skip: VEC 4 fast skip path", 2, 5, 6, 8, True, "KA", "plain"),
        _c("2x5x6x8 skip, symmetric kernel", 2, 5, 6, 8, True, "sym", "plain"),
        _c("1x7x2x6 skip: VEC 4, w % 4 = 2, per-pixel skip", 1, 7, 2, 6, True, "KA", "plain"),
        _c("2x3x3x5: VEC 1", 2, 3, 3, 5, False, "KA", "plain"),
        _c("2x5x6x8 skip, x offset: VEC 1 with skip", 2, 5, 6, 8, True, "KA", "offset"),
        _c("1x70x6x10 skip: small-plane kernel, part-filled block, two empty groups", 1, 70, 6, 10, True, "KA", "plain"),
        _c("1x64x64x64 skip: the last small-plane size", 1, 64, 64, 64, True, "KA", "plain"),
        _c("2x9x66x64 skip: streaming, five blocks, unroll remainder", 2, 9, 66, 64, True, "KA", "plain"),
        _c("1x12x4x4 no style, no bias: finishing-pass form", 1, 12, 4, 4, False, "KA", "finish"),
    ],
    # (shape, bias, offset)
    "fused_bias_act": [
        _c("2x7x5x5 step 25: scalar", (2, 7, 5, 5), True, False),
        _c("3x512 step 1", (3, 512), True, False),
        _c("1x32x16x16 step 256: vector", (1, 32, 16, 16), True, False),
        _c("1x32x16x16 no bias", (1, 32, 16, 16), False, False),
        _c("1x32x16x16 offset view: scalar", (1, 32, 16, 16), True, True),
        _c("1x5x196x2141: 524288+257 float4, ragged second trip", (1, 5, 196, 2141), True, False, size=1),
    ],
    # (shape, noise, bias, offset)
    "noise_bias_act": [
        _c("2x7x5x5 per-sample noise: hw % 4 = 1, scalar", (2, 7, 5, 5), "per", True, False),
        _c("1x32x16x16 shared noise", (1, 32, 16, 16), "shared", True, False),
        _c("3x5x4x8 per-sample noise", (3, 5, 4, 8), "per", True, False),
        _c("3x5x4x8 no noise", (3, 5, 4, 8), "none", True, False),
        _c("3x5x4x8 no bias", (3, 5, 4, 8), "per", False, False),
        _c("3x5x4x8 offset view: scalar", (3, 5, 4, 8), "per", True, True),
        _c("1x5x196x2141 shared noise: 524288+257 float4, ragged second trip", (1, 5, 196, 2141), "shared", True, False, size=1),
    ],
    # (B, cin, style_dim, cout of the demod, strided latent row)
    "modulation_demod": [
        _c("1,5,1 -> 3", 1, 5, 1, 3, False),
        _c("3,70,70 -> 9", 3, 70, 70, 9, False),
        _c("9,16,513 -> 130", 9, 16, 513, 130, False),
        _c("2,260,1024 -> 7", 2, 260, 1024, 7, False),
        _c("17,6,64 -> 6", 17, 6, 64, 6, False),
        _c("3,70,70 -> 9 strided latent row", 3, 70, 70, 9, True),
    ],
    "prepare_weights": [_c("8,5 k3", 8, 5, 3), _c("3,16 k1", 3, 16, 1), _c("1025,512 k1: 524800 pairs", 1025, 512, 1, size=1)],
    "style_batch": [_c("batch 9, style_dim 70", 9, 70), _c("batch 17, style_dim 513", 17, 513), _c("batch 8, style_dim 512", 8, 512)],
    "style_normalize": [_c("cin 5, cout 3", 5, 3), _c("cin 600, cout 300: later trips of both loops", 600, 300)],
    # (route, (B, cin, cout, H, W), filter)
    "conv_route": [_c(f"{r} {kind}", r, shp, kind)
                   for r, shp in (("fp32_up", (1, 8, 8, 4, 4)), ("two_pass_f16", (1, 16, 32, 16, 32)), ("fused", (1, 16, 32, 16, 32)),
                                  ("small_up_blur", (2, 64, 64, 8, 8))) for kind in ("KS", "sym")],
    "rows_image": [_c("1x16x64 KS", (1, 16, 64), "KS"), _c("1x16x64 symmetric kernel", (1, 16, 64), "sym")],
}
CHECKS = {op: globals()["check_" + op] for op in CASES}


def cases(gpu):
    return [(op, c) for op, cs in CASES.items() for c in cs if gpu or c.size < 2]


def case_id(v):
    return v.label.replace(" ", "_") if isinstance(v, Case) else str(v)


# --------------------------------------------------------------------------------------------------------------------
# batch invariance: run(n) = the operator on the first n samples of one input, batch-major
# --------------------------------------------------------------------------------------------------------------------
STYLE_PAIRS = ((6, 3), (9, 1), (17, 9), (9, 8))  # the last two cross kStyleBC = 8


def _batch_runs(lib, st, dev):
    torch.manual_seed(230)
    g = {}
    d = lambda t: t.to(dev)  # noqa: E731
    nb = 9
    ka = d(filt("KA"))

    xu, ku = d(torch.randn(nb, 3, 7, 9) + 1.0), d(torch.randn(3, 5))
    g["upfirdn2d"] = lambda n: M.upfirdn2d(lib, st, xu[:n], ku, 2, 1, 1, 2, 2, 1, 0, 3)
    tmp, nzb = d(torch.randn(nb, 3, 9, 12) + 1.0), d(torch.randn(nb, 1, 8, 8))
    nw, b3 = d(torch.tensor([0.3])), d(torch.randn(3))
    g["blur_f32"] = lambda n: _blur_call(lib, st, dev, tmp[:n], 9, ka, nzb[:n], nw, b3)[1]
    tmp8, b8, s8 = d(torch.randn(nb, 8, 10, 63) + 1.0), d(torch.randn(8)), d(torch.rand(nb, 8) + 0.5)
    nz8 = d(torch.randn(nb, 1, 9, 62))

    def blur_split(n):
        sp = M.SplitActivation.empty(n, 8, 9, 62, dev)
        rc = lib.hf_blur_noise_bias_act_split_f16(sp.hi.data_ptr(), sp.lo.data_ptr(), tmp8[:n].data_ptr(), ka.data_ptr(), nz8[:n].data_ptr(),
                                                  nw.data_ptr(), 9 * 62 if n > 1 else 0, b8.data_ptr(), s8[:n].data_ptr(), n, 8, 10, 63, 63,
                                                  ALPHA, SQRT2, st)
        assert rc == 0
        return torch.cat([sp.hi.reshape(n, -1), sp.lo.reshape(n, -1)], 1)

    g["blur_split"] = blur_split
    xt, wtt, stt, bt, skt = (d(t) for t in _torgb_inputs(nb, 5, 6, 8, True, 231))
    g["torgb"] = lambda n: M.torgb(lib, st, xt[:n], wtt, stt[:n], bt, skt[:n], ka)
    xs, wts, sts, bs, sks = (d(t) for t in _torgb_inputs(nb, 70, 6, 10, True, 232))
    g["torgb (small planes)"] = lambda n: M.torgb(lib, st, xs[:n], wts, sts[:n], bs, sks[:n], ka)
    xa, ba, nza = d(torch.randn(nb, 5, 4, 8)), d(torch.randn(5)), d(torch.randn(nb, 1, 4, 8))
    g["fused_bias_act"] = lambda n: M.fused_bias_act(lib, st, xa[:n], ba, ALPHA, SQRT2)
    g["noise_bias_act"] = lambda n: M.noise_bias_act(lib, st, xa[:n], nza[:n], nw, ba, ALPHA, SQRT2)
    lat, mw, mb = d(torch.randn(nb, 7, 70) + 0.5), d(torch.randn(70, 70) + 0.25), d(torch.randn(70) + 1.0)
    wsq, s_in = d(torch.rand(9, 70) + 0.1), d(torch.randn(nb, 70) + 1.0)
    g["modulation"] = lambda n: M.modulation(lib, st, lat[:n, 4], mw, mb)
    g["demod"] = lambda n: M.demod(lib, st, s_in[:n], wsq)
    convs, rows = _style_convs(dev, 70)
    lat17 = d(torch.randn(17, 7, 70) + 0.5)

    def style_batch(n):
        res = _style_batch(lib, st, dev, lat17[:n], convs, rows)
        return torch.cat([t.reshape(n, -1) for pair in res for t in pair if t is not None], 1)

    g["style_batch"] = style_batch
    return g


BATCH_OPS = ["upfirdn2d", "blur_f32", "blur_split", "torgb", "torgb (small planes)", "fused_bias_act", "noise_bias_act", "modulation",
             "demod", "style_batch"]


def check_batch_invariance(lib, st, dev, op):
    run = _batch_runs(lib, st, dev)[op]
    if op == "style_batch":
        invariant(op, run, pairs=STYLE_PAIRS)
    else:
        invariant(op, run)


def check_size_refusals(lib):
    """Sizes outside the documented ranges are refused before any launch (valid pointers, nothing runs)."""
    t = torch.zeros(64)
    p = t.data_ptr()
    assert lib.hf_upfirdn2d_f32(p, p, p, 1, 4, 4, 9, 4, 1, 1, 1, 1, 0, 0, 0, 0, None) != 0   # 9 taps
    assert lib.hf_upfirdn2d_f32(p, p, p, 1, 4, 4, 4, 9, 1, 1, 1, 1, 0, 0, 0, 0, None) != 0
    assert lib.hf_upfirdn2d_f32(p, p, p, 1, 2, 4, 4, 4, 1, 1, 1, 1, 0, 0, 1, 0, None) != 0   # full_h = 2 + 1 - 4 < 0
    # the blur passes put the planes on gridDim.z: at most 65535
    assert lib.hf_blur_noise_bias_act_f32(p, p, p, None, None, 0, None, 65536, 1, 2, 2, 2, 0.2, 1.0, None) != 0
    assert lib.hf_blur_noise_bias_act_f32(p, p, p, None, None, 0, None, 256, 256, 2, 2, 2, 0.2, 1.0, None) != 0
    assert lib.hf_blur_noise_bias_act_split_f16(p, p, p, p, None, None, 0, None, None, 65536, 8, 2, 2, 2, 0.2, 1.0, None) != 0
    assert lib.hf_blur_noise_bias_act_split_f16(p, p, p, p, None, None, 0, None, None, 1, 12, 2, 2, 2, 0.2, 1.0, None) != 0  # channels % 8
    assert lib.hf_torgb_f32(p, p, p, p, p, p, p, 1, 2, 3, 4, None) != 0                       # odd h with a skip
    assert lib.hf_torgb_f32(p, p, p, p, p, None, None, 1, 5462, 2, 2, None) != 0              # 3 * 5462 floats of LDS
    assert lib.hf_modulation_f32(p, p, 1025, p, p, 1, 1, 1025, None) != 0                     # style_dim above 64 * 16
    assert lib.hf_style_batch_f32(p, p, 1025, 1025, p, 1, 1, 1025, 1, 1, None) != 0
