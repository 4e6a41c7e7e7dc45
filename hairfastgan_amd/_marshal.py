"""Argument marshalling between torch tensors and the C ABI (include/hairfast_hip.h).

Pure plumbing: shape arithmetic, output allocation through torch's caching
allocator, ``data_ptr()`` extraction and error-code checking.  There is no
arithmetic here and no alternative code path: every function ends in exactly one
(or, for the upsampling conv, two) calls into the shared library it is given.
The public ops in ``hairfastgan_amd.op`` / ``hairfastgan_amd.stylegan2`` call
these with the HIP library and the current HIP stream after checking that all
tensors live on the GPU.
"""
import functools
import os

import torch
import torch.nn.functional as F

from ._lib import check
from ._runtime import CANON_BATCH, plan_batch

SQRT2 = 2 ** 0.5

# bench.py sets this to a list to bracket every modulated-conv launch with HIP events
# recorded on the launch stream: entries are (kernel label, algorithmic flops, start, end).
PROFILE = None


KERNEL_NAMES = {  # hf_debug_last_path() code -> kernel instantiation (csrc/modconv.hip dispatch)
    211: "conv_mfma_pipe<2,2,2,4>", 212: "conv_mfma_pipe<2,2,1,4>", 213: "conv_mfma_pipe<1,2,1,4>",
    214: "conv_mfma_pipe<2,2,2,2>", 215: "conv_mfma_pipe<1,1,2,2>", 216: "conv_mfma_pipe<1,4,1,4>",
    231: "conv_mfma_dma<2,2,2,4>", 232: "conv_mfma_dma<2,2,1,4>", 233: "conv_mfma_dma<1,2,1,4>", 234: "conv_mfma_dma<2,2,2,2>",
    244: "conv_mfma_pipe<2,2,2,2,stride2>", 245: "conv_mfma_pipe<1,1,2,2,stride2>",
    221: "conv_mfma_pipe<1,2,2,2,up>", 222: "conv_mfma_pipe<1,2,1,4,up>", 223: "conv_mfma_pipe<1,1,2,2,up>",
    224: "conv_mfma_pipe<1,2,2,4,up>", 225: "conv_mfma_pipe<1,1,1,4,up>", 300: "conv_mfma<1,1,2,2> split-K",
    # csrc/convh.hip (fp16 matrix cores; <CT_TILES,PG,WAVES_CO,WAVES_PX>)
    581: "conv_mfma_h<1,2,2,4,up,pre>", 583: "conv_mfma_h<1,2,1,8,up,pre>",
    571: "conv_mfma_h<1,2,2,4,pre>", 572: "conv_mfma_h<2,2,1,8,pre>", 575: "conv_mfma_h<1,2,1,8,tw128,pre>",
    579: "conv_rows_h<32->32,strip64,pre>",
    551: "conv_mfma_h<1,2,2,4>", 552: "conv_mfma_h<2,2,1,8>", 553: "conv_mfma_h<1,2,1,8>", 555: "conv_mfma_h<1,2,1,8,tw128>",
    561: "conv_mfma_h<1,2,2,4,up>", 563: "conv_mfma_h<1,2,1,8,up>",
    # (the library reports 573 for two forms: this one and "conv_mfma_h<1,2,1,8,pre>")
    573: "conv_mfma_h<1,2,1,8,up,fuse>", 593: "conv_mfma_h<1,2,1,8,up,pre,fuse>",
    # csrc/convh_enc.hip (encoder convs on the fp16 matrix cores)
    601: "conv_enc_h<64x256>", 602: "conv_enc_h<64x128,stride2>", 603: "conv_enc_h<64x128>", 604: "conv_enc_h<64x512>",
    605: "conv_enc_h<64x128,stride2,x4 tiles>",
    606: "conv_enc_h<64x128,stride2,x2 tiles>",
}


def _launch_profiled(lib, flops, fn, label=None, nbytes=0.0, tag=""):
    """bench.py only: brackets one launch with HIP events on the launch stream.  Entries are
    (kernel label, algorithmic flops, start, end, algorithmic bytes); `label` None = a modulated /
    plain conv whose instantiation hf_debug_last_path reports."""
    if PROFILE is None:
        return fn()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    if label is None:
        code = lib.hf_debug_last_path()
        label = KERNEL_NAMES.get(code, f"conv_mfma (general, code {code})")
        if tag and label.endswith(">"):
            label = label[:-1] + tag + ">"
    PROFILE.append((label, flops, e0, e1, nbytes))
    return r


def _p(t):
    return None if t is None else t.data_ptr()


def _c(t):
    """fp32 + contiguous (the reference takes .contiguous() copies defensively too,
    fused_bias_act_kernel.cu:58-60, upfirdn2d_kernel.cu:219-220)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"hairfastgan_amd kernels are fp32; got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


class SplitActivation:
    """An activation handed from a producer to a 3x3 conv on the fp16 matrix cores without an fp32
    round trip: s_next * y split into fp16 (hi, lo) and K-blocked [B, C/8, H, W, 8] (csrc/convh.hip)."""

    def __init__(self, hi, lo, key):
        self.hi, self.lo, self.key = hi, lo, key
        b, cb, h, w, _ = hi.shape
        self.shape = (b, cb * 8, h, w)

    @classmethod
    def empty(cls, b, c, h, w, device, want_lo=True, key=None):
        """Uninitialised storage for a producer kernel to fill; want_lo=False: plain fp16 operands, no lo part."""
        hi = torch.empty((b, c // 8, h, w, 8), dtype=torch.float16, device=device)
        return cls(hi, torch.empty_like(hi) if want_lo else None, key)


def _hl(split):
    """(hi, lo) data pointers of a SplitActivation, (None, None) for None."""
    return (None, None) if split is None else (_p(split.hi), _p(split.lo))


def upfirdn2d(lib, st, x, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    x, kernel = _c(x), _c(kernel)
    n, c, h, w = x.shape
    kh, kw = kernel.shape
    out_h = (h * up_y + pad_y0 + pad_y1 - kh) // down_y + 1
    out_w = (w * up_x + pad_x0 + pad_x1 - kw) // down_x + 1
    out = x.new_empty((n, c, out_h, out_w))
    if out.numel():
        check(lib, lib.hf_upfirdn2d_f32(_p(out), _p(x), _p(kernel), n * c, h, w, kh, kw, up_x, up_y, down_x,
                                        down_y, pad_x0, pad_x1, pad_y0, pad_y1, st), "hf_upfirdn2d_f32")
    return out


def fused_bias_act(lib, st, x, bias, alpha, scale):
    x, bias = _c(x), _c(bias)
    out = torch.empty_like(x)
    n = x.numel()
    if n == 0:
        return out
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    n_bias = bias.numel() if bias is not None else 0
    if bias is not None and x.ndim >= 2 and n_bias != x.shape[1]:
        raise ValueError("bias must have one entry per channel (dim 1)")
    check(lib, lib.hf_fused_bias_act_f32(_p(out), _p(x), _p(bias), n, max(n_bias, 1), step_b, alpha, scale, st),
          "hf_fused_bias_act_f32")
    return out


def _noise_args(noise, batch, hw):
    if noise is None:
        return None, 0
    noise = _c(noise)
    if noise.numel() == hw:
        return noise, 0
    if noise.numel() == batch * hw:
        return noise, hw
    raise ValueError(f"noise must be [1,1,H,W] or [B,1,H,W]; got {tuple(noise.shape)}")


def noise_bias_act(lib, st, x, noise, noise_w, bias, alpha=0.2, scale=SQRT2):
    x, bias, noise_w = _c(x), _c(bias), _c(noise_w)
    b, c, h, w = x.shape
    noise, nbs = _noise_args(noise, b, h * w)
    out = torch.empty_like(x)
    check(lib, lib.hf_noise_bias_act_f32(_p(out), _p(x), _p(noise), _p(noise_w), _p(bias), b, c, h * w, nbs,
                                         alpha, scale, st), "hf_noise_bias_act_f32")
    return out


def prepare_weights(lib, st, weight):
    """weight [1,cout,cin,k,k] -> (wt [k*k,cin,cout], wsq [cout,cin])."""
    weight = _c(weight)
    _, cout, cin, k, _ = weight.shape
    wt = weight.new_empty((k * k, cin, cout))
    wsq = weight.new_empty((cout, cin))
    check(lib, lib.hf_modconv_prepare_f32(_p(wt), _p(wsq), _p(weight), cout, cin, k, st), "hf_modconv_prepare_f32")
    return wt, wsq


def modulation(lib, st, style, mod_w, mod_b):
    """style: [B, style_dim], possibly a strided row view of W+ (latent[:, i])."""
    if style.dtype != torch.float32:
        raise TypeError("style must be fp32")
    if style.stride(-1) != 1:
        style = style.contiguous()
    b, sd = style.shape
    mod_w, mod_b = _c(mod_w), _c(mod_b)
    cin = mod_w.shape[0]
    s = style.new_empty((b, cin))
    check(lib, lib.hf_modulation_f32(_p(s), _p(style), style.stride(0) if b > 1 else sd, _p(mod_w), _p(mod_b),
                                     b, cin, sd, st), "hf_modulation_f32")
    return s


def style_job_table(convs, rows, batch, device):
    """Device job table (hf_style_job records, 7 int64 = 56 bytes each) + output layout for hf_style_batch_f32.
    convs: ModulatedConv2d-like objects with .modulation.weight/.bias, .in_channel, .out_channel,
    .demodulate and .prepared(); rows: latent row of each.  Offsets depend on the batch size."""
    recs, layout, ofs = [], [], 0
    for conv, row in zip(convs, rows):
        _, wsq = conv.prepared()
        cin, cout = conv.in_channel, conv.out_channel
        s_ofs = ofs
        ofs += batch * cin
        d_ofs = -1
        if conv.demodulate:
            d_ofs = ofs
            ofs += batch * cout
        mw, mb = conv.modulation.weight.detach(), conv.modulation.bias.detach()
        recs.append([mw.data_ptr(), mb.data_ptr(), wsq.data_ptr() if conv.demodulate else 0, cin | (cout << 32), row,
                     s_ofs, max(d_ofs, 0)])
        layout.append((s_ofs, cin, d_ofs, cout))
    table = torch.tensor(recs, dtype=torch.int64).to(device)
    return table, layout, ofs


def style_batch(lib, st, latent, table, layout, total, max_cin, max_cout):
    """All (s, d) pairs of a forward in two launches; returns [(s, d|None)] views per job."""
    if latent.dtype != torch.float32 or latent.stride(-1) != 1:
        latent = latent.float().contiguous()
    b, _, sd = latent.shape
    out = latent.new_empty(total)
    check(lib, lib.hf_style_batch_f32(_p(out), _p(latent), latent.stride(0), latent.stride(1), _p(table), len(layout), b, sd,
                                      max_cin, max_cout, st), "hf_style_batch_f32")
    res = []
    for s_ofs, cin, d_ofs, cout in layout:
        s = out[s_ofs:s_ofs + b * cin].view(b, cin)
        d = out[d_ofs:d_ofs + b * cout].view(b, cout) if d_ofs >= 0 else None
        res.append((s, d))
    return res


def demod(lib, st, s, wsq):
    b, cin = s.shape
    cout = wsq.shape[0]
    d = s.new_empty((b, cout))
    check(lib, lib.hf_demod_f32(_p(d), _p(s), _p(wsq), b, cin, cout, st), "hf_demod_f32")
    return d


def style_normalize(lib, st, s, d):
    """In-place power-of-two range normalisation of a layer's (s, d) pair (hf_style_normalize_f32)."""
    b, cin = s.shape
    check(lib, lib.hf_style_normalize_f32(_p(s), _p(d), b, cin, d.shape[1], st), "hf_style_normalize_f32")


def f16_overflow_count(lib, reset=False):
    """Elements the fp16 (hi, lo) split clamped since the last reset (synchronises the device)."""
    return int(lib.hf_f16_overflow_count(1 if reset else 0))


def _workspace(lib, like, b, cin, cout, h, w, up):
    """Split-K scratch for the small-plane layers (size dictated by the library)."""
    n = lib.hf_modconv_workspace_floats(b, cin, cout, h, w, 1 if up else 0)
    if n <= 0:
        return None, 0
    return like.new_empty((n,)), n


def modconv3x3(lib, st, x, wt, s, d, noise, noise_w, bias, alpha=0.2, scale=SQRT2):
    x = _c(x)
    b, cin, h, w = x.shape
    cout = wt.shape[2]
    noise, nbs = _noise_args(noise, b, h * w)
    out = x.new_empty((b, cout, h, w))
    noise_w, bias = _c(noise_w), _c(bias)
    ws, ws_n = _workspace(lib, x, b, cin, cout, h, w, False)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_f32(_p(out), _p(x), _p(wt), _p(s), _p(d), _p(noise), _p(noise_w), nbs, _p(bias),
                                      b, cin, cout, h, w, alpha, scale, _p(ws), ws_n, st))
    check(lib, code, "hf_modconv3x3_f32")
    return out


def split_weights_f16(lib, st, wt):
    """Prepared fp32 weights [9, cin, cout] -> (hi, lo) fp16 tensors in the K-contiguous
    layout of csrc/convh.hip ([cin/16][tap][2][cout][8])."""
    wt = _c(wt)
    taps, cin, cout = wt.shape
    if taps != 9 or cin % 16:
        raise ValueError(f"f16 MFMA path needs 3x3 weights with cin % 16 == 0; got {tuple(wt.shape)}")
    n = 9 * cin * cout
    # wt_hi carries a 16-byte trailer behind its n halves (2^-k of the power-of-two pre-scale)
    hi = torch.empty(n + 8, dtype=torch.float16, device=wt.device)[:n].view(cin // 16, 9, 2, cout, 8)
    lo = torch.empty((cin // 16, 9, 2, cout, 8), dtype=torch.float16, device=wt.device)
    check(lib, lib.hf_conv_split_weights_f16(_p(hi), _p(lo), _p(wt), cin, cout, st), "hf_conv_split_weights_f16")
    return hi, lo


def split_weights_unscale(wt_hi):
    """The 2^-k of the power-of-two pre-scale, read from the trailer behind wt_hi's halves (tests)."""
    n = wt_hi.numel()
    flat = torch.empty(0, dtype=torch.float16, device=wt_hi.device).set_(wt_hi.untyped_storage(), wt_hi.storage_offset(), (n + 8,))
    return float(flat[n:n + 2].view(torch.float32)[0])


def modconv3x3_f16_supported(cin, cout, h, w, batch=None):
    """Shapes hf_modconv3x3_f16_f32 takes (include/hairfast_hip.h).  batch given: also whether it PAYS - a launch of
    fewer than 2048 pixels in total (a batch-1 32^2 layer: 4 tiles x 8 channel tiles) leaves the chip to 32 blocks that
    each walk the whole K loop (94 us); the fp32 kernels split K over the CUs instead (70 us; tools/probes/tower.py)."""
    if batch is not None and plan_batch(batch) * h * w < 2048:
        return False
    return cin % 16 == 0 and w >= 32 and (h >= 8 if cout % 64 == 0 else (cout % 32 == 0 and h >= 16))


def torgb_fusable(cin, cout, h, w):
    """Layers whose ToRGB hf_modconv3x3_f16_rgb_f32 computes in the conv epilogue."""
    if not (cout % 32 == 0 and modconv3x3_f16_supported(cin, cout, h, w)):
        return False
    # one slab (cout 32 / 64) from 512 pixels; several slabs need the 64-channel-per-wave tile shape, which only
    # fills the chip from 64^2 planes (a 32^2 layer on it measured 2x slower than on its own tile shape)
    return h * w >= (512 if cout in (32, 64) else 4096)


IMAGE_FUSE = os.environ.get("HAIRFAST_IMAGE_FUSE", "1") != "0"  # 0: the last layer as conv + ToRGB finishing pass (A/B, tests)


def image_fusable(cin, cout, h, w):
    """The generator's last StyledConv whose epilogue finishes ToRGB (hf_modconv3x3_f16_pre_image_f32: the row pipeline's
    shapes).  The library may still decline (debug dispatch / tuning switches): modconv3x3_f16_pre_image then returns None."""
    return cin == 32 and cout == 32 and w % 64 == 0 and h % 8 == 0 and IMAGE_FUSE


def modconv3x3_f16_pre_image(lib, st, act, wt_hi, wt_lo, nterms, d, noise, noise_w, bias, rgb, rgb_bias, skip, up_kernel,
                             alpha=0.2, scale=SQRT2):
    """hf_modconv3x3_f16_pre_image_f32: same-resolution 3x3 conv on a SplitActivation + its complete ToRGB (1x1 modulated conv
    + bias + upsampled skip) in one launch - the image [B,3,H,W], or None when the library does not take the shape (the caller
    runs modconv3x3_f16_pre(rgb=...) + torgb: the same bits)."""
    b, cin, h, w = act.shape
    cout = wt_hi.shape[3]
    skip = _c(skip)
    if tuple(skip.shape) != (b, 3, h // 2, w // 2):
        raise ValueError(f"skip must be [B,3,H/2,W/2]; got {tuple(skip.shape)} for a {h}x{w} layer")
    noise, nbs = _noise_args(noise, b, h * w)
    image = torch.empty((b, 3, h, w), dtype=torch.float32, device=act.hi.device)
    rgb_wt, rgb_s = _c(rgb[0]), _c(rgb[1])
    nparts = 2 if nterms == 3 else 1
    nb = float(b) * h * w * (2.0 * nparts * cin + 12.0 + 3.0) + 2.0 * nparts * 9 * cin * cout  # split input, image, skip, weights: once
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_f16_pre_image_f32(_p(image), _p(act.hi), _p(act.lo), _p(wt_hi), _p(wt_lo), nterms, _p(d), _p(noise),
                                                    _p(_c(noise_w)), nbs, _p(_c(bias)), b, cin, cout, h, w, alpha, scale, _p(rgb_wt),
                                                    _p(rgb_s), _p(_c(rgb_bias)), _p(skip), _p(_c(up_kernel)), st), nbytes=nb)
    if code == -1:  # HF_E_INVALID: not a row-pipeline launch
        return None
    check(lib, code, "hf_modconv3x3_f16_pre_image_f32")
    return image


def torgb_slabs(cout):
    """Slabs of the fused ToRGB's raw tensor [B, 3*slabs, H, W] (hf_modconv3x3_f16_rgb_slabs)."""
    return cout // 64 if cout % 64 == 0 else cout // 32


def modconv3x3_f16(lib, st, x, wt_hi, wt_lo, nterms, s, d, noise, noise_w, bias, alpha=0.2, scale=SQRT2, rgb=None):
    """hf_modconv3x3_f32 on the fp16 matrix cores (nterms 3: split operands, fp32-class
    accuracy; nterms 1: fp16 operands); fp32 tensors and accumulation.
    rgb = (rgb_wt [1,cout,3], rgb_s [B,cout]): also returns ToRGB's raw 1x1 modulated conv of the
    output, computed in the epilogue (hf_modconv3x3_f16_rgb_f32)."""
    x = _c(x)
    b, cin, h, w = x.shape
    cout = wt_hi.shape[3]
    noise, nbs = _noise_args(noise, b, h * w)
    out = x.new_empty((b, cout, h, w))
    noise_w, bias = _c(noise_w), _c(bias)
    if rgb is not None:
        rgb_wt, rgb_s = _c(rgb[0]), _c(rgb[1])
        raw = x.new_empty((b, 3 * torgb_slabs(cout), h, w))
        code = _launch_profiled(
            lib, 2.0 * cin * cout * 9 * h * w * b,
            lambda: lib.hf_modconv3x3_f16_rgb_f32(_p(out), _p(x), _p(wt_hi), _p(wt_lo), nterms, _p(s), _p(d), _p(noise),
                                                  _p(noise_w), nbs, _p(bias), b, cin, cout, h, w, alpha, scale,
                                                  _p(raw), _p(rgb_wt), _p(rgb_s), st))
        check(lib, code, "hf_modconv3x3_f16_rgb_f32")
        return out, raw
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_f16_f32(_p(out), _p(x), _p(wt_hi), _p(wt_lo), nterms, _p(s), _p(d), _p(noise),
                                          _p(noise_w), nbs, _p(bias), b, cin, cout, h, w, alpha, scale, st))
    check(lib, code, "hf_modconv3x3_f16_f32")
    return out


def split_activation_reference(x, s):
    """torch statement of the producer-side split (tests / tools): s*x -> (hi, lo) K-blocked."""
    b, c, h, w = x.shape
    v = x if s is None else x * s[:, :, None, None]
    hi = v.half()
    lo = (v - hi.float()).half()
    blk = lambda t: t.reshape(b, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()  # noqa: E731
    return blk(hi), blk(lo)


def _modconv3x3_f16_pre(lib, st, act, wt_hi, wt_lo, nterms, d, noise, noise_w, bias, alpha=0.2, scale=SQRT2, rgb=None,
                        want_out=True, split_for=None):
    """modconv3x3_f16_pre with the fixed return form (out | None, raw | None, split | None)."""
    b, cin, h, w = act.shape
    cout = wt_hi.shape[3]
    dev = act.hi.device
    noise, nbs = _noise_args(noise, b, h * w)
    if not want_out and rgb is None and split_for is None:
        raise ValueError("want_out=False needs another consumer (rgb= or split_for=)")
    out = torch.empty((b, cout, h, w), dtype=torch.float32, device=dev) if want_out else None
    noise_w, bias = _c(noise_w), _c(bias)
    raw = rgb_wt = rgb_s = split = s_next = None
    if rgb is not None:
        rgb_wt, rgb_s = _c(rgb[0]), _c(rgb[1])
        raw = torch.empty((b, 3 * torgb_slabs(cout), h, w), dtype=torch.float32, device=dev)
    if split_for is not None:
        s_next = _c(split_for)
        split = SplitActivation.empty(b, cout, h, w, dev, want_lo=nterms == 3)  # plain fp16 consumer: no lo part
    # algorithmic HBM bytes (bench.py: traffic / algorithmic): the split input once, every output form once, the weights once
    nparts = 2 if nterms == 3 else 1
    nb = (float(b) * h * w * (2.0 * nparts * cin + (4.0 * cout if want_out else 0.0) + (2.0 * nparts * cout if split_for is not None else 0.0)
                              + (12.0 * torgb_slabs(cout) if rgb is not None else 0.0)) + 2.0 * nparts * 9 * cin * cout)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_f16_pre_f32(_p(out), _p(act.hi), _p(act.lo), _p(wt_hi), _p(wt_lo), nterms, _p(d), _p(noise),
                                              _p(noise_w), nbs, _p(bias), b, cin, cout, h, w, alpha, scale, _p(raw),
                                              _p(rgb_wt), _p(rgb_s), *_hl(split), _p(s_next), st), nbytes=nb)
    check(lib, code, "hf_modconv3x3_f16_pre_f32")
    return out, raw, split


def modconv3x3_f16_pre(lib, st, act, wt_hi, wt_lo, nterms, d, noise, noise_w, bias, alpha=0.2, scale=SQRT2, rgb=None,
                       want_out=True, split_for=None):
    """hf_modconv3x3_f16_pre_f32: same-resolution 3x3 conv on the fp16 matrix cores whose input is a
    SplitActivation (modulation already applied by the producer).
    rgb = (rgb_wt, rgb_s): fused ToRGB raw product (see modconv3x3_f16);
    split_for = s_next [B,cout]: the epilogue also writes a SplitActivation of s_next*out for the next
    layer's transposed conv; want_out=False: the fp32 activation itself is not written.
    Returns out, or (out, raw), (out, split), (out, raw, split) in that order of optional parts."""
    out, raw, split = _modconv3x3_f16_pre(lib, st, act, wt_hi, wt_lo, nterms, d, noise, noise_w, bias, alpha, scale, rgb, want_out,
                                          split_for)
    res = (out,) + (() if rgb is None else (raw,)) + (() if split_for is None else (split,))
    return res[0] if len(res) == 1 else res


def split_weights_small(lib, st, wt):
    """Prepared weights wt [9, cin, cout] -> the (hi, lo) blobs hf_modconv3x3_small_f16_f32 takes: the nine taps as the
    rows of ONE 1x1 GEMM, [1][cin][tap*cout + co], split by hf_conv_split_weights_f16_taps(taps = 1)."""
    taps, cin, cout = wt.shape
    w1 = _c(wt).permute(1, 0, 2).reshape(1, cin, taps * cout).contiguous()
    return conv_split_weights_f16(lib, st, w1)


def modconv3x3_small_supported(cin, cout, h, w, batch, upsample=False):
    """Shapes hf_modconv3x3_small_f16_f32 takes AND pays for (tools/probes/tower.py, 512 -> 512 channels, batch 1 / 3 / 8):
    same resolution: 256 < batch*h*w <= 2048 pixels per launch (below, the three launches of the tap-GEMM form cost more than
    the fp32 split-K kernel's two; above, the tiled fp16-core conv fills the chip) - 8^2 at batch 8: 43 -> 30 us, 16^2: 98 ->
    81 us, 32^2 at batch 1: 70 -> 56 us; transposed: inputs up to 8^2 at any batch (4 -> 8: 72 -> 56 us, 8 -> 16: 141 -> 58 us
    at batch 8; 62 -> 38 / 68 -> 43 us at batch 1) and 16^2 inputs up to 1024 pixels per launch (batch 3: 110 -> 88 us)."""
    if cin % 32 or cout % 64 or h * w > 1024:
        return False
    n = plan_batch(batch) * h * w  # batch-invariant mode: the dispatch of ONE sample (_runtime.plan_batch)
    if upsample:
        return h * w <= 64 or (h * w <= 256 and n <= 1024)
    # n = 256 from tiny planes (4^2 at batch 16, 8^2 at batch 4): the fp32 split-K kernel takes 180 us there, the tap GEMM 60
    # 8^2 planes from n = CANON_BATCH * 64 = the canonical batch 3 of the batch-invariant plans (round 6: at batch 8 the fp32 split-K family that
    # batch 3 alone would take costs 53 us, the tap GEMM 29; at batch 3 itself 29 vs 31 - tools/probes/tower.py, profiles/r06an_*)
    return 256 < n <= 2048 or (n == 256 and h * w <= 64) or (h * w == 64 and CANON_BATCH * 64 <= n <= 2048)


def conv3x3_small_supported(cin, cout, h, w, batch):
    """Plain (unmodulated) 3x3 convs worth the tap-GEMM form: planes the tiled fp16 kernel does not take, weights of 1 MB
    and more (below, the fp32 split-K kernel's two launches win), at most 4096 pixels per launch."""
    return cin % 32 == 0 and cout % 64 == 0 and h * w <= 256 and plan_batch(batch) * h * w <= 4096 and cin * cout >= 512 * 512


def modconv3x3_small(lib, st, x, w9, nterms, s, d, noise, noise_w, bias, cout, alpha=0.2, scale=SQRT2, upsample=False):
    """hf_modconv3x3_small_f16_f32.  upsample: returns the (2h+1) x pitch intermediate [B,cout,2h+1,pitch] (demodulated)."""
    x = _c(x)
    b, cin, h, w = x.shape
    hi, lo = w9
    n = lib.hf_modconv3x3_small_workspace_floats(b, cin, cout, h, w)
    ws = x.new_empty((max(n, 1),))
    if upsample:
        pitch = lib.hf_modconv_up_pitch(w)
        out = x.new_empty((b, cout, 2 * h + 1, pitch))
        noise = bias = noise_w = None
        nbs = 0
    else:
        pitch = 0
        out = x.new_empty((b, cout, h, w))
        noise, nbs = _noise_args(noise, b, h * w)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_small_f16_f32(_p(out), _p(x), _p(hi), _p(lo), nterms, _p(_c(s)), _p(_c(d)), _p(noise),
                                                _p(_c(noise_w)), nbs, _p(_c(bias)), b, cin, cout, h, w, alpha, scale,
                                                1 if upsample else 0, pitch, _p(ws), n, st),
        label="gemm_h tap-GEMM (small planes)")
    check(lib, code, "hf_modconv3x3_small_f16_f32")
    return out


SMALL_UP_FUSED = os.environ.get("HAIRFAST_SMALL_UP_FUSED", "1") != "0"  # 0: tap GEMM, combine pass, blur pass (A/B, tests)


def small_up_blur_supported(h, w):
    """hf_modconv3x3_small_up_blur_f16_f32's LDS bound: 8 channels x ((2h+3) x (2w+3) + 9 h w) floats."""
    return (8 * (2 * h + 3) * (2 * w + 3) + 72 * h * w) * 4 <= 150 * 1024


def modconv3x3_small_up_blur(lib, st, x, w9, nterms, s, d, blur_kernel, noise, noise_w, bias, cout, alpha=0.2, scale=SQRT2,
                             split_for=None):
    """hf_modconv3x3_small_up_blur_f16_f32: the small-plane upsampling StyledConv as tap GEMM + one combine / blur / tail kernel.
    split_for as in modconv3x3_up: None -> the fp32 activation [B,cout,2h,2w]; (key, s_next[, want_lo]) -> SplitActivation."""
    x = _c(x)
    b, cin, h, w = x.shape
    hi, lo = w9
    n = lib.hf_modconv3x3_small_workspace_floats(b, cin, cout, h, w)
    ws = x.new_empty((max(n, 1),))
    noise, nbs = _noise_args(noise, b, 4 * h * w)
    out = split = s_next = None
    if split_for is not None:
        s_next = _c(split_for[1])
        split = SplitActivation.empty(b, cout, 2 * h, 2 * w, x.device, want_lo=split_for[2] if len(split_for) > 2 else True,
                                      key=split_for[0])
    else:
        out = x.new_empty((b, cout, 2 * h, 2 * w))
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_small_up_blur_f16_f32(_p(out), *_hl(split), _p(x), _p(hi), _p(lo), nterms, _p(_c(s)), _p(_c(d)),
                                                        _p(_c(blur_kernel)), _p(noise), _p(_c(noise_w)), nbs, _p(_c(bias)),
                                                        _p(s_next), b, cin, cout, h, w, alpha, scale, _p(ws), n, st),
        label="gemm_h tap-GEMM (small planes)")
    check(lib, code, "hf_modconv3x3_small_up_blur_f16_f32")
    return out if split_for is None else split


def modconv3x3_up_f16_supported(cin, cout, h, w, batch=None):
    """Shapes hf_modconv3x3_up_f16_f32 takes (include/hairfast_hip.h); batch: see modconv3x3_f16_supported (a batch-1
    16^2 -> 32^2 layer: 84 us on the fp32 split-K kernels, 106 us here)."""
    if batch is not None and plan_batch(batch) * h * w < 512:
        return False
    return cin % 16 == 0 and cout % 32 == 0 and h * w >= (256 if cout % 64 == 0 else 512) and min(h, w) >= 2


def modconv3x3_up(lib, st, x, wt, s, d, blur_kernel, noise, noise_w, bias, alpha=0.2, scale=SQRT2, f16=None,
                  split_for=None, small=None):
    """conv_transpose(stride 2) -> [B,cout,2h+1,2w+1] scratch -> blur+noise+bias+act -> [B,cout,2h,2w].
    f16 = (wt_hi, wt_lo, nterms): part 1 on the fp16 matrix cores (hf_modconv3x3_up_f16_f32).
    split_for = (key, s_next [B,cout]): part 2 writes a SplitActivation for the conv whose modulation
    is s_next instead of the fp32 tensor (hf_blur_noise_bias_act_split_f16).
    small = (w9, nterms): part 1 as the small-plane tap-GEMM (hf_modconv3x3_small_f16_f32, upsample form)."""
    pre = isinstance(x, SplitActivation)
    if not pre:
        x = _c(x)
    b, cin, h, w = x.shape
    cout = wt.shape[2]
    pitch = lib.hf_modconv_up_pitch(w)  # rows padded to a multiple of 4 floats (aligned 16 B loads in the blur)
    if pre or small is None:
        tmp = torch.empty((b, cout, 2 * h + 1, pitch), dtype=torch.float32, device=(x.hi if pre else x).device)
    if pre:  # pre-split input (modulation already applied by the producer): hf_modconv3x3_up_f16_pre_f32
        hi, lo, nterms = f16
        code = _launch_profiled(
            lib, 2.0 * cin * cout * 9 * h * w * b,
            lambda: lib.hf_modconv3x3_up_f16_pre_f32(_p(tmp), _p(x.hi), _p(x.lo), _p(hi), _p(lo), nterms, _p(d), b, cin, cout,
                                                     h, w, pitch, st))
        check(lib, code, "hf_modconv3x3_up_f16_pre_f32")
    elif small is not None and SMALL_UP_FUSED and small_up_blur_supported(h, w):
        # round 6: tap GEMM + ONE combine / blur / tail kernel (the (2h+1)^2 intermediate stays in LDS) - same bits
        return modconv3x3_small_up_blur(lib, st, x, small[0], small[1], s, d, blur_kernel, noise, noise_w, bias, cout, alpha, scale,
                                        split_for=split_for)
    elif small is not None:
        tmp = modconv3x3_small(lib, st, x, small[0], small[1], s, d, None, None, None, cout, upsample=True)
    elif f16 is not None:
        hi, lo, nterms = f16
        code = _launch_profiled(
            lib, 2.0 * cin * cout * 9 * h * w * b,
            lambda: lib.hf_modconv3x3_up_f16_f32(_p(tmp), _p(x), _p(hi), _p(lo), nterms, _p(s), _p(d), b, cin, cout, h, w,
                                                 pitch, st))
        check(lib, code, "hf_modconv3x3_up_f16_f32")
    else:
        ws, ws_n = _workspace(lib, x, b, cin, cout, h, w, True)
        code = _launch_profiled(
            lib, 2.0 * cin * cout * 9 * h * w * b,
            lambda: lib.hf_modconv3x3_up_f32(_p(tmp), _p(x), _p(wt), _p(s), _p(d), b, cin, cout, h, w, pitch, _p(ws),
                                             ws_n, st))
        check(lib, code, "hf_modconv3x3_up_f32")
    noise, nbs = _noise_args(noise, b, 4 * h * w)
    if split_for is not None:
        s_next = split_for[1]
        want_lo = split_for[2] if len(split_for) > 2 else True  # False: consumer with plain fp16 operands
        split = SplitActivation.empty(b, cout, 2 * h, 2 * w, tmp.device, want_lo, key=split_for[0])
        # algorithmic bytes: the (2h+1)(2w+1) fp32 intermediate read once, one 2-byte value per part written
        nb = float(b * cout) * (4.0 * (2 * h + 1) * (2 * w + 1) + (4.0 if want_lo else 2.0) * 4 * h * w)
        code = _launch_profiled(
            lib, 0.0,
            lambda: lib.hf_blur_noise_bias_act_split_f16(*_hl(split), _p(tmp), _p(_c(blur_kernel)), _p(noise),
                                                         _p(_c(noise_w)), nbs, _p(_c(bias)), _p(_c(s_next)), b, cout,
                                                         2 * h + 1, 2 * w + 1, pitch, alpha, scale, st),
            label="blur4x4_split8", nbytes=nb)
        check(lib, code, "hf_blur_noise_bias_act_split_f16")
        return split
    out = tmp.new_empty((b, cout, 2 * h, 2 * w))
    nb = float(b * cout) * 4.0 * ((2 * h + 1) * (2 * w + 1) + 4 * h * w)
    code = _launch_profiled(
        lib, 0.0,
        lambda: lib.hf_blur_noise_bias_act_f32(_p(out), _p(tmp), _p(_c(blur_kernel)), _p(noise), _p(_c(noise_w)),
                                               nbs, _p(_c(bias)), b, cout, 2 * h + 1, 2 * w + 1, pitch, alpha, scale, st),
        label="blur4x4_noise_bias_act", nbytes=nb)
    check(lib, code, "hf_blur_noise_bias_act_f32")
    return out


def blur_factors(kernel4x4):
    """(kx, ky): the 1-D factors of a rank-1 4x4 blur kernel (k[r][j] = ky[r]*kx[j]) as ctypes float[4] arrays,
    or None when the kernel is not separable.  Reads the kernel on the host (synchronises): callers cache it."""
    import ctypes

    k = kernel4x4.detach().double().cpu()
    if tuple(k.shape) != (4, 4) or float(k[0, 0]) == 0.0:
        return None
    kx, ky = k[0, :].clone(), k[:, 0] / k[0, 0]
    if not torch.allclose(torch.outer(ky, kx), k, rtol=1e-6, atol=1e-12):
        return None
    arr = ctypes.c_float * 4
    return arr(*[float(v) for v in kx]), arr(*[float(v) for v in ky])


def modconv3x3_up_fused_supported(cin, cout, h, w):
    """Shapes hf_modconv3x3_up_blur_f16_f32 takes."""
    return cin % 16 == 0 and cout % 32 == 0 and h >= 16 and w >= 32


def modconv3x3_up_fused(lib, st, x, wt_hi, wt_lo, s, d, factors, noise, noise_w, bias, alpha=0.2, scale=SQRT2, split_for=None,
                        nterms=3):
    """hf_modconv3x3_up_blur_f16_f32: transposed conv + blur + noise + bias + lrelu in one kernel (nterms 3: f16x3; 1: plain
    fp16 operands - wt_lo is then not passed, a split output has no lo part).
    x: fp32 tensor (with s) or SplitActivation.  Returns the fp32 activation, or - split_for = s_next [B,cout] -
    the SplitActivation of s_next * activation for a pre-split consumer (one output form per launch)."""
    pre = isinstance(x, SplitActivation)
    if not pre:
        x = _c(x)
    b, cin, h, w = x.shape
    cout = wt_hi.shape[3]
    dev = x.hi.device if pre else x.device
    noise, nbs = _noise_args(noise, b, 4 * h * w)
    out = split = s_next = None
    if split_for is not None:
        s_next = _c(split_for)
        split = SplitActivation.empty(b, cout, 2 * h, 2 * w, dev, want_lo=nterms == 3)
    else:
        out = torch.empty((b, cout, 2 * h, 2 * w), dtype=torch.float32, device=dev)
    kx, ky = factors
    nb_alg = float(b) * (4.0 * cin * h * w + 4.0 * cout * 4 * h * w + 4.0 * 4 * h * w) + 4.0 * 9 * cin * cout  # input, output, noise, weights
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * h * w * b,
        lambda: lib.hf_modconv3x3_up_blur_f16_f32(_p(out), *_hl(split), None if pre else _p(x), _p(x.hi) if pre else None,
                                                  _p(x.lo) if (pre and nterms == 3) else None, _p(wt_hi),
                                                  _p(wt_lo) if nterms == 3 else None, None if pre else _p(s), _p(d),
                                                  kx, ky, _p(noise), _p(_c(noise_w)), nbs, _p(_c(bias)), _p(s_next), b, cin, cout,
                                                  h, w, alpha, scale, st), nbytes=nb_alg)
    check(lib, code, "hf_modconv3x3_up_blur_f16_f32")
    return out if split_for is None else split


def torgb(lib, st, x, wt, s, bias, skip, up_kernel):
    x = _c(x)
    b, cin, h, w = x.shape
    skip = _c(skip)
    if skip is not None and tuple(skip.shape) != (b, 3, h // 2, w // 2):
        raise ValueError(f"skip must be [B,3,H/2,W/2]; got {tuple(skip.shape)} for x {tuple(x.shape)}")
    out = x.new_empty((b, 3, h, w))
    nb = float(b) * 4.0 * h * w * (cin + 3 + (0.75 if skip is not None else 0.0))  # x read, rgb written, skip read
    code = _launch_profiled(
        lib, 0.0,
        lambda: lib.hf_torgb_f32(_p(out), _p(x), _p(wt), _p(s), _p(_c(bias)), _p(skip), _p(_c(up_kernel)), b, cin, h, w, st),
        label="torgb_kernel" if h * w > 4096 else "torgb_small_kernel", nbytes=nb)
    check(lib, code, "hf_torgb_f32")
    return out


# ----------------------------------------------------------------------------------------
# encoders
# ----------------------------------------------------------------------------------------
ACT_NONE, ACT_LRELU, ACT_PRELU, ACT_QGELU = 0, 1, 2, 3
ACT_RESIDUAL_FIRST = 16  # OR-ed into act: residual added before the activation (HF_ACT_RESIDUAL_FIRST)


def conv_prepare(lib, st, weight, scale=1.0):
    """Conv2d weight [cout,cin,k,k] -> wt [k*k,cin,cout]."""
    weight = _c(weight)
    cout, cin, k, _ = weight.shape
    wt = weight.new_empty((k * k, cin, cout))
    check(lib, lib.hf_conv_prepare_f32(_p(wt), _p(weight), cout, cin, k, scale, st), "hf_conv_prepare_f32")
    return wt


def bn_fold(lib, st, gamma, beta, mean, var, eps, conv_bias=None):
    gamma, beta, mean, var, conv_bias = _c(gamma), _c(beta), _c(mean), _c(var), _c(conv_bias)
    n = gamma.numel()
    scale, shift = gamma.new_empty(n), gamma.new_empty(n)
    check(lib, lib.hf_bn_fold_f32(_p(scale), _p(shift), _p(gamma), _p(beta), _p(mean), _p(var), _p(conv_bias),
                                  float(eps), n, st), "hf_bn_fold_f32")
    return scale, shift


def _enc_conv_io(lib, x, cout, stride, in_scale, in_shift, residual, groups=1, x_shared=True, ws_floats=None, taps=9, nterms=3,
                 want_f32=True, split_out=False):
    """What the four encoder conv wrappers share.  Parses x - fp32 [B,cin,H,W], grouped [G,B,cin,H,W] (groups > 1, not
    x_shared), or a SplitActivation of B (grouped: G*B) images that carries its affine already -, allocates the fp32 output
    (want_f32) and the workspace that ws_floats = (size query's name, arguments it takes between w and stride...) asks for,
    checks the residual against the output shape and models the algorithmic HBM bytes (bench.py: traffic / algorithmic): the
    pixels read (a shared input of a grouped launch once), every output form, a residual and the weights - each once.
    Returns (x, (b, cin, h, w, oh, ow), x_gstride, out, residual, ws, floats in ws, nbytes)."""
    pre = isinstance(x, SplitActivation)
    own = groups > 1 and not x_shared  # every group reads its own input
    if pre:
        if in_scale is not None or in_shift is not None:
            raise ValueError("a pre-split input carries its affine already")
        n_img, cin, h, w = x.shape
        b = n_img // groups if own else n_img
        x_gstride = 1 if own else 0
        dev = x.hi.device
    else:
        x = _c(x)
        dev = x.device
        if own:
            g_, b, cin, h, w = x.shape
            if g_ != groups:
                raise ValueError("x must be [groups, B, cin, H, W]")
            x_gstride = b * cin * h * w
        else:
            b, cin, h, w = x.shape
            x_gstride = 0
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    shape = (groups, b, cout, oh, ow) if groups > 1 else (b, cout, oh, ow)
    out = torch.empty(shape, dtype=torch.float32, device=dev) if want_f32 else None
    if residual is not None:
        residual = _c(residual)
        if tuple(residual.shape) != shape:
            raise ValueError(f"residual {tuple(residual.shape)} != output {shape}")
    n = 0 if ws_floats is None else getattr(lib, ws_floats[0])(b, cin, cout, h, w, *ws_floats[1:], stride, groups)
    ws = torch.empty((n,), dtype=torch.float32, device=dev) if n > 0 else None
    nparts = 2 if nterms == 3 else 1
    nb = (float(b * (groups if own else 1)) * cin * (h * w if taps == 9 else oh * ow) * (2.0 * nparts if pre else 4.0)
          + float(b) * groups * cout * oh * ow * ((2.0 * nparts if split_out else 0.0) + (4.0 if want_f32 else 0.0)
                                                  + (4.0 if residual is not None else 0.0))
          + 2.0 * nparts * taps * cin * cout * groups)
    return x, (b, cin, h, w, oh, ow), x_gstride, out, residual, ws, max(n, 0), nb


def conv2d(lib, st, x, wt, k, stride=1, in_scale=None, in_shift=None, out_scale=None, bias=None, act=ACT_NONE,
           slope=None, alpha=0.0, residual=None, groups=1, x_shared=True):
    """groups == 1: x [B,cin,H,W], wt [k*k,cin,cout] -> [B,cout,oh,ow].
    groups  > 1: wt [G,k*k,cin,cout], bias/out_scale/slope [G,cout]; x [B,cin,H,W] shared by all
    groups (x_shared) or [G,B,cin,H,W]; returns [G,B,cout,oh,ow]."""
    cout = wt.shape[-1]
    x, (b, cin, h, w, oh, ow), x_gstride, out, residual, ws, n, _ = _enc_conv_io(
        lib, x, cout, stride, None, None, residual, groups, x_shared, ("hf_conv2d_workspace_floats", k))
    code = _launch_profiled(
        lib, 2.0 * cin * cout * k * k * oh * ow * b * groups,
        lambda: lib.hf_conv2d_f32(_p(out), _p(x), _p(_c(wt)), _p(in_scale), _p(in_shift), _p(_c(out_scale)), _p(_c(bias)),
                                  act, _p(_c(slope)), float(alpha), _p(residual), b, cin, cout, h, w, k, stride, groups,
                                  x_gstride, _p(ws), n, st))
    check(lib, code, "hf_conv2d_f32")
    return out


def _pow2_ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


@functools.lru_cache(maxsize=4096)  # (asked ~700 times per swap with ~60 distinct shapes: host time of a host-bound call sequence)
def conv2d_f16_supported(cin, cout, h, w, k, stride):
    """Shapes hf_conv2d_f16_f32 takes (include/hairfast_hip.h; mirrors launch_enc's tile geometry)."""
    if k != 3 or cin % 16 or cout % 64 or stride not in (1, 2):
        return False
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    tw = min(32, _pow2_ceil(ow))
    return tw >= 16 and _pow2_ceil(oh) >= 128 // tw


def conv_split_weights_f16(lib, st, wt):
    """Prepared conv weights [taps,cin,cout] or [G,taps,cin,cout] (taps 9 or 1) -> (hi, lo) fp16 blobs in the layout
    hf_conv2d_f16_f32 / hf_conv1x1_f16_f32 take: per group [taps*cin*cout halves | 16-byte trailer] (hi) and
    taps*cin*cout halves (lo)."""
    wt = _c(wt)
    w4 = wt if wt.ndim == 4 else wt.unsqueeze(0)
    g, taps, cin, cout = w4.shape
    if taps not in (9, 1) or cin % 16:
        raise ValueError(f"f16 MFMA path needs 3x3 or 1x1 weights with cin % 16 == 0; got {tuple(wt.shape)}")
    n = taps * cin * cout
    hi = torch.empty(g * (n + 8), dtype=torch.float16, device=wt.device)
    lo = torch.empty(g * n, dtype=torch.float16, device=wt.device)
    for i in range(g):
        check(lib, lib.hf_conv_split_weights_f16_taps(hi[i * (n + 8):].data_ptr(), lo[i * n:].data_ptr(), w4[i].data_ptr(), cin, cout,
                                                     taps, st), "hf_conv_split_weights_f16_taps")
    return hi, lo


def conv1x1_f16_supported(cin, cout):
    """Shapes hf_conv1x1_f16_f32 takes (include/hairfast_hip.h)."""
    return cin % 32 == 0 and cout % 64 == 0


def conv1x1_f16(lib, st, x, wt_hi, wt_lo, nterms, cout, stride=1, in_scale=None, in_shift=None, out_scale=None, bias=None,
                act=ACT_NONE, slope=None, alpha=0.0, residual=None, groups=1, x_shared=True):
    """hf_conv1x1_f16_f32: a 1x1 conv / Linear layer as a GEMM on the fp16 matrix cores; argument meaning as conv2d().
    x may be a SplitActivation (stride 1, no groups, affine already applied)."""
    pre = isinstance(x, SplitActivation)
    x, (b, cin, h, w, oh, ow), x_gstride, out, residual, ws, n, nb = _enc_conv_io(
        lib, x, cout, stride, in_scale, in_shift, residual, groups, x_shared, ("hf_conv1x1_f16_workspace_floats",), taps=1, nterms=nterms)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * oh * ow * b * groups,
        lambda: lib.hf_conv1x1_f16_f32(_p(out), None if pre else _p(x), _p(x.hi) if pre else None, _p(x.lo) if pre else None,
                                       _p(wt_hi), _p(wt_lo), nterms, _p(_c(in_scale)), _p(_c(in_shift)),
                                       _p(_c(out_scale)), _p(_c(bias)), act, _p(_c(slope)), float(alpha), _p(residual), b, cin, cout,
                                       h, w, stride, groups, x_gstride, _p(ws), n, st),
        label="gemm_h", nbytes=nb)
    check(lib, code, "hf_conv1x1_f16_f32")
    return out


def split_activation_f16(lib, st, x, in_scale=None, in_shift=None, want_lo=True):
    """hf_split_activation_f16: x [..., C, H, W] fp32 -> SplitActivation of in_scale*x + in_shift
    (fp16 hi/lo pairs, K-blocked [images, C/8, H, W, 8]); leading dims are flattened into images."""
    x = _c(x)
    c, h, w = x.shape[-3:]
    images = x.numel() // (c * h * w)
    split = SplitActivation.empty(images, c, h, w, x.device, want_lo)
    check(lib, lib.hf_split_activation_f16(*_hl(split), _p(x), _p(_c(in_scale)), _p(_c(in_shift)), images, c, h, w, st),
          "hf_split_activation_f16")
    return split


def conv2d_f16(lib, st, x, wt_hi, wt_lo, nterms, cout, stride=1, in_scale=None, in_shift=None, out_scale=None, bias=None,
               act=ACT_NONE, slope=None, alpha=0.0, residual=None, groups=1, x_shared=True):
    """hf_conv2d_f16_f32: conv2d(k=3) on the fp16 matrix cores; argument meaning as conv2d().
    x may be a SplitActivation (split_activation_f16 of the input, any in_scale / in_shift already applied):
    [B] images, or [groups*B] images with x_shared=False."""
    pre = isinstance(x, SplitActivation)
    x, (b, cin, h, w, oh, ow), x_gstride, out, residual, ws, n, nb = _enc_conv_io(
        lib, x, cout, stride, in_scale, in_shift, residual, groups, x_shared, ("hf_conv2d_f16_workspace_floats",), nterms=nterms)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * oh * ow * b * groups,
        lambda: lib.hf_conv2d_f16_f32(_p(out), None if pre else _p(x), _p(x.hi) if pre else None, _p(x.lo) if pre else None,
                                      _p(wt_hi), _p(wt_lo), nterms, _p(in_scale), _p(in_shift), _p(_c(out_scale)),
                                      _p(_c(bias)), act, _p(_c(slope)), float(alpha), _p(residual), b, cin, cout, h, w, stride,
                                      groups, x_gstride, _p(ws), n, st), tag=",pre" if pre else "", nbytes=nb)
    check(lib, code, "hf_conv2d_f16_f32")
    return out


def conv2d_f16_split_supported(lib, b, cin, cout, h, w, stride, nterms=3, pre=False):
    """hf_conv2d_f16_split_f32 takes the launch: groups 1 and no K split spread over the grid (the split output is written by
    the conv kernel's own epilogue; hf_conv2d_f16_split_output_ok).  pre: the input arrives pre-split (SplitActivation)."""
    return cout % 8 == 0 and lib.hf_conv2d_f16_split_output_ok(b, cin, cout, h, w, stride, nterms, 1 if pre else 0) == 1


def conv2d_f16_split(lib, st, x, wt_hi, wt_lo, nterms, cout, stride=1, in_scale=None, in_shift=None, out_scale=None, bias=None,
                     act=ACT_NONE, slope=None, alpha=0.0, residual=None, next_scale=None, next_shift=None, want_f32=False):
    """hf_conv2d_f16_split_f32: conv2d_f16 whose result leaves as a SplitActivation (next_scale * y + next_shift, fp16 hi / lo,
    K-blocked) for the next fp16-core conv; want_f32: also the fp32 tensor -> (SplitActivation, out | None)."""
    pre = isinstance(x, SplitActivation)
    x, (b, cin, h, w, oh, ow), _, out, residual, _, _, nb = _enc_conv_io(
        lib, x, cout, stride, in_scale, in_shift, residual, nterms=nterms, want_f32=want_f32, split_out=True)
    split = SplitActivation.empty(b, cout, oh, ow, (x.hi if pre else x).device, want_lo=nterms == 3)
    code = _launch_profiled(
        lib, 2.0 * cin * cout * 9 * oh * ow * b,
        lambda: lib.hf_conv2d_f16_split_f32(_p(out), *_hl(split), _p(_c(next_scale)), _p(_c(next_shift)), None if pre else _p(x),
                                            _p(x.hi) if pre else None, _p(x.lo) if pre else None, _p(wt_hi), _p(wt_lo), nterms,
                                            _p(in_scale), _p(in_shift), _p(_c(out_scale)), _p(_c(bias)), act, _p(_c(slope)),
                                            float(alpha), _p(residual), b, cin, cout, h, w, stride, st),
        tag=",pre,split-out" if pre else ",split-out", nbytes=nb)
    check(lib, code, "hf_conv2d_f16_split_f32")
    return split, out


def plane_mean(lib, st, x):
    x = _c(x)
    b, c, h, w = x.shape
    out = x.new_empty((b, c))
    check(lib, lib.hf_plane_mean_f32(_p(out), _p(x), b * c, h * w, st), "hf_plane_mean_f32")
    return out


def se_gate(lib, st, pooled, fc1, fc2):
    b, c = pooled.shape
    cr = fc1.shape[0]
    gate = pooled.new_empty((b, c))
    check(lib, lib.hf_se_gate_f32(_p(gate), _p(pooled), _p(_c(fc1)), _p(_c(fc2)), b, c, cr, st), "hf_se_gate_f32")
    return gate


def scale_shortcut_add(lib, st, r, gate, shortcut, sc_stride=1):
    r, shortcut = _c(r), _c(shortcut)
    b, c, oh, ow = r.shape
    sh, sw = shortcut.shape[2], shortcut.shape[3]
    out = torch.empty_like(r)
    check(lib, lib.hf_scale_shortcut_add_f32(_p(out), _p(r), _p(gate), _p(shortcut), sc_stride, b, c, oh, ow, sh, sw,
                                             st), "hf_scale_shortcut_add_f32")
    return out


def scale_shortcut_add_split(lib, st, r, gate, shortcut, sc_stride=1, next_scale=None, next_shift=None, want_lo=True):
    """hf_scale_shortcut_add_split_f16: scale_shortcut_add whose result also leaves as the SplitActivation of
    next_scale * out + next_shift (the next unit's first conv input) -> (out fp32, SplitActivation)."""
    r, shortcut = _c(r), _c(shortcut)
    b, c, oh, ow = r.shape
    sh, sw = shortcut.shape[2], shortcut.shape[3]
    out = torch.empty_like(r)
    split = SplitActivation.empty(b, c, oh, ow, r.device, want_lo)
    check(lib, lib.hf_scale_shortcut_add_split_f16(_p(out), *_hl(split), _p(_c(next_scale)), _p(_c(next_shift)), _p(r), _p(gate),
                                                   _p(shortcut), sc_stride, b, c, oh, ow, sh, sw, st), "hf_scale_shortcut_add_split_f16")
    return out, split


def upsample_bilinear_add(lib, st, x, y):
    x, y = _c(x), _c(y)
    b, c, h, w = x.shape
    oh, ow = y.shape[2], y.shape[3]
    out = torch.empty_like(y)
    check(lib, lib.hf_upsample_bilinear_add_f32(_p(out), _p(x), _p(y), b * c, h, w, oh, ow, st),
          "hf_upsample_bilinear_add_f32")
    return out


def adaptive_avgpool_into(lib, st, out, x, c_off):
    """AdaptiveAvgPool2d(out.shape[2:]) of x written into out[:, c_off:c_off+C]."""
    x = _c(x)
    b, c, h, w = x.shape
    check(lib, lib.hf_adaptive_avgpool_f32(_p(out), _p(x), b, c, h, w, out.shape[2], out.shape[3], out.shape[1], c_off,
                                           st), "hf_adaptive_avgpool_f32")


def downscale2x(lib, st, x):
    x = _c(x)
    b, c, h, w = x.shape
    out = x.new_empty((b, c, h // 2, w // 2))
    check(lib, lib.hf_downscale2x_f32(_p(out), _p(x), b * c, h, w, st), "hf_downscale2x_f32")
    return out


def linear(lib, st, x, weight, bias, scale=1.0):
    """x [B,in] (row stride may exceed in), weight [out,in] -> [B,out]; B <= 8 per launch."""
    if x.stride(-1) != 1:
        x = x.contiguous()
    b, k = x.shape
    weight = _c(weight)
    n = weight.shape[0]
    out = x.new_empty((b, n))
    check(lib, lib.hf_linear_f32(_p(out), _p(x), x.stride(0) if b > 1 else k, _p(weight), _p(_c(bias)), b, k, n, float(scale), st),
          "hf_linear_f32")
    return out


def equal_linear(lib, st, x, weight, bias, lr_mul=1.0, fused_lrelu=False, alpha=0.2, act_scale=SQRT2):
    """EqualLinear.forward (model.py:153-163) in one launch per <= 8 rows: x [..., in] -> [..., out]."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if x2.dtype != torch.float32:
        raise TypeError("hairfastgan_amd kernels are fp32")
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    b, k = x2.shape
    weight = _c(weight)
    n = weight.shape[0]
    out = x2.new_empty((b, n))
    check(lib, lib.hf_equal_linear_f32(_p(out), _p(x2), x2.stride(0) if b > 1 else k, _p(weight), _p(_c(bias)), b, k, n,
                                       float(lr_mul), 1 if fused_lrelu else 0, float(alpha), float(act_scale), st),
          "hf_equal_linear_f32")
    return out.reshape(*lead, n)


def pixel_norm(lib, st, x):
    """PixelNorm over dim 1 of [B, dim] (model.py:16-21)."""
    x = _c(x)
    if x.ndim != 2:
        raise ValueError("pixel_norm expects [B, dim] (the mapping network's z)")
    out = torch.empty_like(x)
    check(lib, lib.hf_pixel_norm_f32(_p(out), _p(x), x.shape[0], x.shape[1], st), "hf_pixel_norm_f32")
    return out


def bicubic_down(lib, st, x, k1d, factor):
    """BicubicDownSample.forward (utils/bicubic.py): x [B,C,H,W] -> [B,C,H/factor,W/factor]."""
    x, k1d = _c(x), _c(k1d)
    b, c, h, w = x.shape
    out = x.new_empty((b, c, h // factor, w // factor))
    check(lib, lib.hf_bicubic_down_f32(_p(out), _p(x), _p(k1d), b * c, h, w, factor, st), "hf_bicubic_down_f32")
    return out


def dilate_erode(lib, st, mask, radius):
    """DilateErosion.mask on a binary float mask [..., H, W] -> (dilated, eroded)."""
    mask = _c(mask)
    h, w = mask.shape[-2:]
    dil, ero = torch.empty_like(mask), torch.empty_like(mask)
    check(lib, lib.hf_dilate_erode_f32(_p(dil), _p(ero), _p(mask), mask.numel() // (h * w), h, w, radius, st), "hf_dilate_erode_f32")
    return dil, ero


def stem_prepare(w):
    """[cout,3,7,7] conv weight -> (w_hi, w_lo, w_unscale) of hf_stem7x7s2_f16_f32: fp16 (hi, lo) parts of W * 2^k in
    [cout/64][22 K groups][64][8] - group (ci, ky), eight halves = kx 0..6 + a zero; the 22nd group zero - with 2^k placing
    max|W| in [2^13, 2^14) (the lo parts of small weights would otherwise be fp16 subnormals, csrc/convh.hip split_weights)."""
    cout = w.shape[0]
    if tuple(w.shape[1:]) != (3, 7, 7) or cout % 64:
        raise ValueError(f"stem weight must be [64n,3,7,7]; got {tuple(w.shape)}")
    w = w.detach().float()
    amax = w.abs().max().clamp_min(1e-30)
    k = torch.floor(13.0 - torch.log2(amax))
    scale = torch.exp2(k)
    ws = F.pad(w * scale, (0, 1)).reshape(cout, 21, 8)                           # kx padded to 8
    ws = torch.cat([ws, ws.new_zeros(cout, 1, 8)], 1)                            # the zero group
    ws = ws.reshape(cout // 64, 64, 22, 8).permute(0, 2, 1, 3).contiguous()      # [tiles][22][64][8]
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return hi.contiguous(), lo.contiguous(), torch.exp2(-k).reshape(1).float().contiguous()


def stem7x7s2(lib, st, x, w3, out_scale=None, bias=None, alpha=0.0, pool=True):
    """hf_stem7x7s2_f16_f32: 7x7 stride-2 conv of a 3-channel image + per-channel affine + leaky ReLU (+ 3x3/2 max pool)."""
    x = _c(x)
    b, cin, h, w = x.shape
    hi, lo, unscale = w3
    cout = hi.shape[0] * 64
    if cin != 3:
        raise ValueError("stem input must have 3 channels")
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if pool:
        oh, ow = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    out = x.new_empty((b, cout, oh, ow))
    code = _launch_profiled(
        lib, 2.0 * 3 * 49 * cout * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * b,
        lambda: lib.hf_stem7x7s2_f16_f32(_p(out), _p(x), _p(hi), _p(lo), _p(unscale), _p(_c(out_scale)), _p(_c(bias)), float(alpha),
                                         b, h, w, cout, 1 if pool else 0, st),
        label="stem 7x7/2 (+pool)")
    check(lib, code, "hf_stem7x7s2_f16_f32")
    return out


def maxpool3x3s2(lib, st, x):
    x = _c(x)
    b, c, h, w = x.shape
    out = x.new_empty((b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    check(lib, lib.hf_maxpool3x3s2_f32(_p(out), _p(x), b * c, h, w, st), "hf_maxpool3x3s2_f32")
    return out


def gate(lib, st, x, logit, add_plane=None, add_bcast=None, plus_one=0.0):
    """x * (sigmoid(logit[b,c]) + plus_one) + add_plane + add_bcast[b,c] (hf_gate_f32)."""
    x = _c(x)
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    check(lib, lib.hf_gate_f32(_p(out), _p(x), _p(_c(logit)), _p(_c(add_plane)), _p(_c(add_bcast)), float(plus_one), b * c, h * w, st),
          "hf_gate_f32")
    return out


def upsample_nearest(lib, st, x, oh, ow):
    x = _c(x)
    b, c, h, w = x.shape
    out = x.new_empty((b, c, oh, ow))
    check(lib, lib.hf_upsample_nearest_f32(_p(out), _p(x), b * c, h, w, oh, ow, st), "hf_upsample_nearest_f32")
    return out


def parsing_mask(lib, st, logits, remap, full_hw, out_hw):
    """hf_parsing_mask_i64: class logits [B,C,h,w] -> int64 mask [B,1,oh,ow] (bilinear up to full_hw, nearest resize
    to out_hw, first-max argmax, label permutation remap int32 [C])."""
    logits = _c(logits)
    b, c, h, w = logits.shape
    out = torch.empty((b, 1, out_hw[0], out_hw[1]), dtype=torch.int64, device=logits.device)
    check(lib, lib.hf_parsing_mask_i64(_p(out), _p(logits), _p(remap), b, c, h, w, full_hw[0], full_hw[1], out_hw[0], out_hw[1], st),
          "hf_parsing_mask_i64")
    return out


def layernorm(lib, st, x, dim, gamma=None, beta=None, eps=1e-5, lrelu=False, alpha=0.01, groups=1):
    """F.layer_norm over the trailing `dim` elements (x viewed as [rows, dim]), optional affine + LeakyReLU.
    groups > 1 (hf_layernorm_grouped_f32): gamma / beta [groups, dim], row r of the [rows, dim] view takes group r % groups."""
    x = _c(x)
    if x.numel() % dim:
        raise ValueError("dim must divide the tensor")
    out = torch.empty_like(x)
    if groups > 1:
        rows = x.numel() // dim
        if rows % groups or gamma is None or tuple(gamma.shape) != (groups, dim) or (beta is not None and tuple(beta.shape) != (groups, dim)):
            raise ValueError("grouped layernorm: rows % groups == 0 and gamma / beta [groups, dim]")
        check(lib, lib.hf_layernorm_grouped_f32(_p(out), _p(x), _p(_c(gamma)), _p(_c(beta)), rows, dim, groups, float(eps),
                                                1 if lrelu else 0, float(alpha), st), "hf_layernorm_grouped_f32")
        return out
    check(lib, lib.hf_layernorm_f32(_p(out), _p(x), _p(_c(gamma)), _p(_c(beta)), x.numel() // dim, dim, float(eps),
                                    1 if lrelu else 0, float(alpha), st), "hf_layernorm_f32")
    return out


def sample_layernorm(lib, st, x, gamma=None, beta=None, eps=1e-5, slope=1.0, channels=None):
    """hf_sample_layernorm_f32: per-sample LayerNorm over C*H*W with the unbiased std and eps added to it, per-channel
    affine, LeakyReLU(slope) - the CtrlHair shape adaptor's norm.  channels < x.shape[1]: only the first `channels`
    planes of every sample are normalised and returned (x came out of a conv with a padded channel count)."""
    x = _c(x)
    b, c_all = x.shape[0], x.shape[1]
    c = c_all if channels is None else channels
    hw = x.numel() // (b * c_all)
    out = x.new_empty((b, c) + tuple(x.shape[2:]))
    n = lib.hf_sample_layernorm_workspace_floats(b, c, hw)
    ws = x.new_empty((max(n, 1),))
    check(lib, lib.hf_sample_layernorm_f32(_p(out), _p(x), _p(_c(gamma)), _p(_c(beta)), b, c, hw, c_all * hw, float(eps),
                                           float(slope), _p(ws), n, st), "hf_sample_layernorm_f32")
    return out


def modulate(lib, st, x, gamma, beta, lrelu=False, alpha=0.01):
    x, gamma, beta = _c(x), _c(gamma), _c(beta)
    if gamma.shape != x.shape or beta.shape != x.shape:
        raise ValueError("gamma / beta must have x's shape")
    out = torch.empty_like(x)
    check(lib, lib.hf_modulate_f32(_p(out), _p(x), _p(gamma), _p(beta), x.numel(), 1 if lrelu else 0, float(alpha), st),
          "hf_modulate_f32")
    return out


def pixel_norm_dim1(lib, st, x):
    x = _c(x)
    b, layers, d = x.shape
    out = torch.empty_like(x)
    check(lib, lib.hf_pixel_norm_dim1_f32(_p(out), _p(x), b, layers, d, st), "hf_pixel_norm_dim1_f32")
    return out


def axpby(lib, st, a, alpha, bvec, beta=1.0):
    """alpha * a + beta * bvec, bvec broadcast periodically over a (hf_axpby_bcast_f32)."""
    a, bvec = _c(a), _c(bvec)
    out = torch.empty_like(a)
    check(lib, lib.hf_axpby_bcast_f32(_p(out), _p(a), float(alpha), _p(bvec), float(beta), a.numel(), bvec.numel(), st),
          "hf_axpby_bcast_f32")
    return out


def add_bcast(lib, st, a, bvec):
    a, bvec = _c(a), _c(bvec)
    out = torch.empty_like(a)
    check(lib, lib.hf_add_bcast_f32(_p(out), _p(a), _p(bvec), a.numel(), bvec.numel(), st), "hf_add_bcast_f32")
    return out


# ----------------------------------------------------------------------------------------
# SEAN (csrc/sean.hip)
# ----------------------------------------------------------------------------------------
def label_conv3x3(lib, st, labels, table, bias, channels, batch=None, cols_per_sample=0, group=1, relu=False):
    """hf_label_conv3x3_f32: 3x3 conv of a per-label-constant input as nine table lookups per output.
    labels int32 [B/group, H, W]; table [9*channels, table_cols] -> [B, channels, H, W]."""
    if labels.dtype != torch.int32 or not labels.is_contiguous():
        raise TypeError("labels must be contiguous int32 [B/group, H, W]")
    table = _c(table)
    nb, h, w = labels.shape
    b = nb * group if batch is None else batch
    if table.shape[0] != 9 * channels or (cols_per_sample and table.shape[1] < b * cols_per_sample):
        raise ValueError(f"table {tuple(table.shape)} does not fit {channels} channels / {b} samples")
    out = table.new_empty((b, channels, h, w))
    # interior fast path (one lookup of the tap sum instead of nine) where planes are large enough to have interiors
    tsum = table.new_empty((channels, table.shape[1])) if h * w >= 1024 else None
    check(lib, lib.hf_label_conv3x3_f32(_p(out), _p(labels), _p(table), _p(_c(bias)), b, channels, h, w, table.shape[1],
                                        cols_per_sample, group, 1 if relu else 0, _p(tsum), st), "hf_label_conv3x3_f32")
    return out


def ace_modulate(lib, st, x, noise, noise_var, bn_scale, bn_shift, avg, sp, blend, group=1, slope=1.0, x_up=False):
    """hf_ace_modulate_f32: the tail of ACE.forward; x [B,C,H,W], noise [B,H,W] | None, avg [B,2C,H,W] | None,
    sp [B/group,2C,H,W], blend = device tensor (blending_gamma, blending_beta).  x_up: x is [B,C,H/2,W/2] and its nearest
    x2 up-sampling is read in place."""
    x, sp = _c(x), _c(sp)
    b, c = x.shape[:2]
    h, w = sp.shape[-2:]
    if tuple(x.shape[-2:]) != ((h // 2, w // 2) if x_up else (h, w)):
        raise ValueError(f"x {tuple(x.shape)} does not match the {h} x {w} planes of sp (x_up={x_up})")
    if tuple(sp.shape) != (b // group, 2 * c, h, w) or (avg is not None and tuple(avg.shape) != (b, 2 * c, h, w)):
        raise ValueError("sp / avg must be [B/group | B, 2C, H, W]")
    if noise is not None and noise.numel() != b * h * w:
        raise ValueError("noise must be [B, H, W]")
    out = x.new_empty((b, c, h, w))
    check(lib, lib.hf_ace_modulate_f32(_p(out), _p(x), _p(_c(noise)), _p(_c(noise_var)), _p(_c(bn_scale)), _p(_c(bn_shift)),
                                       _p(_c(avg)), _p(sp), _p(_c(blend)), b, c, h * w, group, float(slope), w if x_up else 0, st),
          "hf_ace_modulate_f32")
    return out


def ace_modulate_table(lib, st, x, noise, noise_var, bn_scale, bn_shift, labels, table, avg_bias, sp, blend, group=1, slope=1.0,
                       x_up=False):
    """hf_ace_modulate_table_f32: label_conv3x3(labels, table, avg_bias, 2C, batch=B, cols_per_sample=19, group) fused into
    ace_modulate (the [B,2C,H,W] avg planes never exist).  table [9*2C, >= B*19]; labels int32 [B/group,H,W]."""
    x, sp, table = _c(x), _c(sp), _c(table)
    b, c = x.shape[:2]
    h, w = sp.shape[-2:]
    if tuple(x.shape[-2:]) != ((h // 2, w // 2) if x_up else (h, w)):
        raise ValueError(f"x {tuple(x.shape)} does not match the {h} x {w} planes of sp (x_up={x_up})")
    if labels.dtype != torch.int32 or not labels.is_contiguous() or tuple(labels.shape) != (b // group, h, w):
        raise TypeError("labels must be contiguous int32 [B/group, H, W]")
    if tuple(sp.shape) != (b // group, 2 * c, h, w) or table.shape[0] != 9 * 2 * c or table.shape[1] < b * 19:
        raise ValueError("sp must be [B/group, 2C, H, W] and table [9*2C, >= 19*B]")
    if noise is not None and noise.numel() != b * h * w:
        raise ValueError("noise must be [B, H, W]")
    out = x.new_empty((b, c, h, w))
    check(lib, lib.hf_ace_modulate_table_f32(_p(out), _p(x), _p(_c(noise)), _p(_c(noise_var)), _p(_c(bn_scale)), _p(_c(bn_shift)),
                                             _p(labels), _p(table), _p(_c(avg_bias)), _p(sp), _p(_c(blend)), b, c, h, w,
                                             table.shape[1], 19, group, float(slope), 1 if h * w >= 1024 else 0, 1 if x_up else 0, st),
          "hf_ace_modulate_table_f32")
    return out


def ace_modulate_table_supported(h, w):
    return w % 4 == 0 and h * w >= 1024


def region_mean(lib, st, x, labels, crop=0, act_tanh=False):
    """hf_region_mean_f32: per-label mean of (tanh of) x [B,C,H+2*crop,W+2*crop] over its interior, labels int32
    [B,H,W] -> [B,19,C]."""
    x = _c(x)
    b, c, hp, wp = x.shape
    h, w = hp - 2 * crop, wp - 2 * crop
    if labels.dtype != torch.int32 or tuple(labels.shape) != (b, h, w) or not labels.is_contiguous():
        raise TypeError("labels must be contiguous int32 [B, H, W] of the cropped size")
    out = x.new_empty((b, 19, c))
    base = x.data_ptr() + 4 * (crop * wp + crop)
    check(lib, lib.hf_region_mean_f32(_p(out), base, _p(labels), b, c, h, w, 19, c * hp * wp, hp * wp, wp, 1 if act_tanh else 0, st),
          "hf_region_mean_f32")
    return out


def tanh(lib, st, x):
    x = _c(x)
    out = torch.empty_like(x)
    check(lib, lib.hf_tanh_f32(_p(out), _p(x), x.numel(), st), "hf_tanh_f32")
    return out


# ----------------------------------------------------------------------------------------
# CLIP ViT image tower (csrc/vit.hip): feature-major activations [C, T]
# ----------------------------------------------------------------------------------------
def channel_layernorm(lib, st, x, gamma, beta, eps=1e-5):
    """LayerNorm over the feature axis of x [C, ...tokens] or [1, C, ...tokens] (the NCHW view the 1x1-conv GEMMs use)."""
    x = _c(x)
    c = x.shape[1] if (x.ndim == 4 and x.shape[0] == 1) else x.shape[0]
    out = torch.empty_like(x)
    check(lib, lib.hf_channel_layernorm_f32(_p(out), _p(x), _p(_c(gamma)), _p(_c(beta)), c, x.numel() // c, float(eps), st),
          "hf_channel_layernorm_f32")
    return out


def mha_small(lib, st, qkv, images, seq, heads):
    """qkv [3E, images*seq] (or [1, 3E, images, seq]) feature-major -> attention output [E, images*seq] (same form)."""
    qkv = _c(qkv)
    lead = 1 if (qkv.ndim == 4 and qkv.shape[0] == 1) else 0
    e = qkv.shape[lead] // 3
    if qkv.numel() != 3 * e * images * seq:
        raise ValueError("qkv must be [3E, images*seq]")
    out = qkv.new_empty(tuple(qkv.shape[:lead]) + (e,) + tuple(qkv.shape[lead + 1:]))
    check(lib, lib.hf_mha_small_f32(_p(out), _p(qkv), images, seq, heads, e // heads, st), "hf_mha_small_f32")
    return out


def quick_gelu(lib, st, x):
    x = _c(x)
    out = torch.empty_like(x)
    check(lib, lib.hf_quick_gelu_f32(_p(out), _p(x), x.numel(), st), "hf_quick_gelu_f32")
    return out


# ---- Poisson image blending (csrc/poisson.h; hairfastgan_amd.image_utils chains these) ----
POISSON_TBLOCKS = (1, 2, 4, 8, 16)  # the sweep depths hf_poisson_jacobi_f32 is instantiated for


def _u8(t):
    if t.dtype != torch.uint8:
        raise TypeError(f"expected a uint8 tensor; got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _poisson_dims(img, mask):
    """img [N,C,H,W], mask [N,1,H,W] or [N,H,W] of the same N, H, W -> (N, C, H, W)."""
    if img.ndim != 4 or mask.numel() != img.shape[0] * img.shape[2] * img.shape[3] or tuple(mask.shape[-2:]) != tuple(img.shape[-2:]):
        raise ValueError(f"images must be [N,C,H,W] and the mask [N,1,H,W] of the same N, H, W; got {tuple(img.shape)}, {tuple(mask.shape)}")
    return tuple(img.shape)


def quantize_u8(lib, st, x):
    """torchvision save_image's bytes of a float tensor (any shape): uint8(trunc(clamp(fl(fl(x*255) + 0.5), 0, 255)))."""
    x = _c(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib, lib.hf_quantize_u8_f32(_p(out), _p(x), x.numel(), st), "hf_quantize_u8_f32")
    return out


def poisson_setup(lib, st, src, tgt, mask):
    """u8 source / target [N,C,H,W] and mask [N,1,H,W] -> (B, X_0) fp32 [N,C,H,W] of the Jacobi solve."""
    src, tgt, mask = _u8(src), _u8(tgt), _u8(mask)
    n, c, h, w = _poisson_dims(tgt, mask)
    if src.shape != tgt.shape:
        raise ValueError(f"source {tuple(src.shape)} and target {tuple(tgt.shape)} differ in shape")
    b = torch.empty(tgt.shape, dtype=torch.float32, device=tgt.device)
    x0 = torch.empty_like(b)
    check(lib, lib.hf_poisson_setup_u8(_p(b), _p(x0), _p(src), _p(tgt), _p(mask), n, c, h, w, st), "hf_poisson_setup_u8")
    return b, x0


def poisson_jacobi_into(lib, st, x_out, x_in, b, mask, sweeps, tblock):
    """`sweeps` (1..tblock) Jacobi sweeps x_in -> x_out in one launch blocked `tblock` sweeps deep."""
    x_in, b, mask = _c(x_in), _c(b), _u8(mask)
    n, c, h, w = _poisson_dims(b, mask)
    if x_out.shape != b.shape or x_in.shape != b.shape or not x_out.is_contiguous() or x_out.dtype != torch.float32:
        raise ValueError("x_in, x_out and b must be contiguous fp32 tensors of one shape")
    check(lib, lib.hf_poisson_jacobi_f32(_p(x_out), _p(x_in), _p(b), _p(mask), n, c, h, w, sweeps, tblock, st),
          "hf_poisson_jacobi_f32")
    return x_out


def poisson_finish(lib, st, x, tgt, mask):
    """out = Omega ? uint8(trunc(clamp(X, 0, 255))) : target, u8 [N,C,H,W]."""
    x, tgt, mask = _c(x), _u8(tgt), _u8(mask)
    n, c, h, w = _poisson_dims(tgt, mask)
    if x.shape != tgt.shape:
        raise ValueError(f"X {tuple(x.shape)} and target {tuple(tgt.shape)} differ in shape")
    out = torch.empty_like(tgt)
    check(lib, lib.hf_poisson_finish_u8(_p(out), _p(x), _p(tgt), _p(mask), n, c, h, w, st), "hf_poisson_finish_u8")
    return out


# ---- FFHQ face alignment (csrc/align.h; hairfastgan_amd.face_align chains these).  Images: planar uint8 [C,H,W] ----
def _planes(img):
    img = _u8(img)
    if img.ndim != 3:
        raise ValueError(f"expected a planar uint8 image [C,H,W]; got {tuple(img.shape)}")
    return img


def _table(pair):
    """(bounds int32 [n,2], kk int32 [n,ksize]) of one Lanczos pass, or None -> (pointers, ksize)."""
    if pair is None:
        return None, None, 0
    bounds, kk = pair
    if bounds.dtype != torch.int32 or kk.dtype != torch.int32 or bounds.ndim != 2 or bounds.shape[1] != 2 or kk.ndim != 2 \
            or kk.shape[0] != bounds.shape[0] or not bounds.is_contiguous() or not kk.is_contiguous():
        raise ValueError("a Lanczos table is (bounds int32 [n,2], kk int32 [n,ksize]), contiguous")
    return bounds, kk, kk.shape[1]


def _coef8(coef):
    import ctypes

    if len(coef) != 8:
        raise ValueError("the quad transform takes 8 coefficients a0..a7")
    return (ctypes.c_double * 8)(*[float(v) for v in coef])


def resize_lanczos_u8(lib, st, img, out_h, out_w, table_x, table_y):
    """PIL's 8-bit Lanczos resize: table_x / table_y = face_align.lanczos_coeffs of the axis on the device (None for an
    axis whose size does not change)."""
    img = _planes(img)
    c, h, w = img.shape
    bx, kx, nx = _table(table_x)
    by, ky, ny = _table(table_y)
    if (bx is None) != (out_w == w) or (by is None) != (out_h == h) or (bx is not None and bx.shape[0] != out_w) \
            or (by is not None and by.shape[0] != out_h):
        raise ValueError("one table per axis whose size changes, with one row per output sample")
    out = torch.empty((c, out_h, out_w), dtype=torch.uint8, device=img.device)
    mid = torch.empty((c, h, out_w), dtype=torch.uint8, device=img.device) if bx is not None and by is not None else None
    check(lib, lib.hf_resize_lanczos_u8(_p(out), _p(mid), _p(img), c, h, w, out_h, out_w, _p(bx), _p(kx), nx, _p(by), _p(ky), ny, st),
          "hf_resize_lanczos_u8")
    return out


def quad_bilinear_u8(lib, st, img, coef, out_h, out_w):
    """PIL's transform(QUAD, BILINEAR) with the coefficients a0..a7 of face_align.quad_coefficients."""
    img = _planes(img)
    c, h, w = img.shape
    out = torch.empty((c, out_h, out_w), dtype=torch.uint8, device=img.device)
    check(lib, lib.hf_quad_bilinear_u8(_p(out), _p(img), _coef8(coef), c, h, w, out_h, out_w, st), "hf_quad_bilinear_u8")
    return out


def quad_lanczos4_u8(lib, st, img, coef, out_size, table):
    """quad_bilinear_u8 to (4 out_size)^2 and resize_lanczos_u8 to out_size^2 in one launch; table = the 4 out_size ->
    out_size pass."""
    img = _planes(img)
    c, h, w = img.shape
    b, k, n = _table(table)
    if b is None or b.shape[0] != out_size:
        raise ValueError("the table must have one row per output sample")
    out = torch.empty((c, out_size, out_size), dtype=torch.uint8, device=img.device)
    check(lib, lib.hf_quad_lanczos4_u8(_p(out), _p(img), _coef8(coef), c, h, w, out_size, _p(b), _p(k), n, st), "hf_quad_lanczos4_u8")
    return out


def align_pad_blur(lib, st, img, weights, radius, mask_x, mask_y, pad):
    """Reflect pad by pad = (left, top, right, bottom), Gaussian (2 radius + 1 float64 weights) and the blur fade -> fp32
    [C,H,W]; mask_x fp32 [W], mask_y fp32 [H]."""
    img = _planes(img)
    c, h, w = img.shape
    left, top, right, bottom = (int(v) for v in pad)
    H, W = h + top + bottom, w + left + right
    if weights.dtype != torch.float64 or weights.numel() != 2 * radius + 1 or not weights.is_contiguous():
        raise ValueError("weights: 2 * radius + 1 contiguous float64 values")
    mask_x, mask_y = _c(mask_x), _c(mask_y)
    if mask_x.numel() != W or mask_y.numel() != H:
        raise ValueError(f"mask_x / mask_y must have {W} / {H} elements")
    out = torch.empty((c, H, W), dtype=torch.float32, device=img.device)
    tmp = torch.empty_like(out)
    check(lib, lib.hf_align_pad_blur_f32(_p(out), _p(tmp), _p(img), _p(weights), radius, _p(mask_x), _p(mask_y), c, h, w, left, top,
                                         right, bottom, st), "hf_align_pad_blur_f32")
    return out


def align_pad_finish(lib, st, img, median, mask_x, mask_y, return_float=False):
    """The median fade, rint, clip -> (uint8 [C,H,W], the fp32 image before rint or None)."""
    img, median, mask_x, mask_y = _c(img), _c(median), _c(mask_x), _c(mask_y)
    c, h, w = img.shape
    if median.numel() != c or mask_x.numel() != w or mask_y.numel() != h:
        raise ValueError("median [C], mask_x [W] and mask_y [H] must match the image")
    out = torch.empty((c, h, w), dtype=torch.uint8, device=img.device)
    pre = torch.empty_like(img) if return_float else None
    check(lib, lib.hf_align_pad_finish_u8(_p(out), _p(pre), _p(img), _p(median), _p(mask_x), _p(mask_y), c, h, w, st),
          "hf_align_pad_finish_u8")
    return out, pre


def u8_to_unit(lib, st, img):
    """float32 byte / 255 (ToTensor)."""
    img = _u8(img)
    out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
    check(lib, lib.hf_u8_to_unit_f32(_p(out), _p(img), img.numel(), st), "hf_u8_to_unit_f32")
    return out


# ---- the aligned result pasted back into the photograph (csrc/paste.h; hairfastgan_amd.face_align.paste_back) ----
def paste_quad_u8(lib, st, photo, src, mask, coef, roi):
    """In place on photo u8 [C,H,W]: PIL's transform(QUAD, BILINEAR) of src u8 [C,n,n] and of mask u8 [n,n] onto the region
    roi = (x0, y0, x1, y1) with the coefficients a0..a7 of face_align.quad_coefficients, composited through the warped
    mask.  -> photo."""
    if not photo.is_contiguous():
        raise ValueError("paste works in place: the photograph must be contiguous")
    photo, src, mask = _planes(photo), _planes(src), _u8(mask)
    c, h, w = photo.shape
    n = src.shape[1]
    if src.shape != (c, n, n) or mask.shape != (n, n):
        raise ValueError(f"paste: source [C,n,n] and mask [n,n] for a photograph of {c} planes; got {tuple(src.shape)}, {tuple(mask.shape)}")
    x0, y0, x1, y1 = (int(v) for v in roi)
    check(lib, lib.hf_paste_quad_u8(_p(photo), _p(src), _p(mask), _coef8(coef), c, h, w, n, x0, y0, x1, y1, st), "hf_paste_quad_u8")
    return photo


def multiply_u8(lib, st, a, b):
    """PIL's ImageChops.multiply of two uint8 tensors of one shape: a * b / 255, rounded down."""
    a, b = _u8(a), _u8(b)
    if a.shape != b.shape:
        raise ValueError(f"multiply: {tuple(a.shape)} and {tuple(b.shape)} differ in shape")
    out = torch.empty_like(a)
    check(lib, lib.hf_multiply_u8(_p(out), _p(a), _p(b), a.numel(), st), "hf_multiply_u8")
    return out


# ---- the PNG bytes of --save_all (csrc/export.h; hairfastgan_amd.image_utils has the public forms) ----
def image_to_bytes(lib, st, images, lo, hi, round_half, interleaved):
    """fp32 [B,3,H,W] -> uint8 [B,H,W,3] (interleaved) or [B,3,H,W]: t = (x - lo) / (hi - lo), then trunc(clamp(t, 0, 1) * 255)
    or, round_half, trunc(clamp(t * 255 + 0.5, 0, 255))."""
    images = _c(images)
    if images.ndim != 4 or images.shape[1] != 3 or images.numel() == 0:
        raise ValueError(f"expected images [B,3,H,W] with B, H, W > 0; got {tuple(images.shape)}")
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        raise ValueError(f"value range needs lo < hi; got ({lo}, {hi})")
    b, _, h, w = images.shape
    out = torch.empty((b, h, w, 3) if interleaved else (b, 3, h, w), dtype=torch.uint8, device=images.device)
    check(lib, lib.hf_image_to_bytes_f32(_p(out), _p(images), b, h, w, lo, hi, int(bool(round_half)), int(bool(interleaved)), st),
          "hf_image_to_bytes_f32")
    return out


def labels_to_rgb(lib, st, labels, palette, unknown_label=255):
    """int64 labels (any shape) -> uint8 labels.shape + (3,): palette uint8 [n_colors,3] on the labels' device; a label
    outside the table is black, `unknown_label` white."""
    if labels.dtype != torch.int64:
        raise TypeError(f"expected int64 labels; got {labels.dtype}")
    if palette.dtype != torch.uint8 or palette.ndim != 2 or palette.shape[1] != 3 or palette.shape[0] == 0:
        raise ValueError(f"the palette is uint8 [n_colors,3]; got {palette.dtype} {tuple(palette.shape)}")
    if palette.device != labels.device:
        raise ValueError(f"palette on {palette.device}, labels on {labels.device}")
    if labels.numel() == 0:
        raise ValueError("empty label map")
    labels = labels if labels.is_contiguous() else labels.contiguous()
    palette = palette if palette.is_contiguous() else palette.contiguous()
    out = torch.empty(tuple(labels.shape) + (3,), dtype=torch.uint8, device=labels.device)
    check(lib, lib.hf_labels_to_rgb_i64(_p(out), _p(labels), labels.numel(), _p(palette), palette.shape[0], int(unknown_label), st),
          "hf_labels_to_rgb_i64")
    return out


PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "adaptive": 3}


def _check_encode_images(images):
    if images.dtype != torch.uint8:
        raise TypeError(f"expected uint8 images; got {images.dtype}")
    if images.ndim != 4 or images.shape[3] not in (1, 3) or images.numel() == 0:
        raise ValueError(f"expected images [B,H,W,1] or [B,H,W,3] with B, H, W > 0; got {tuple(images.shape)}")


def _encode_buffers(images, bound, ws_bytes, name, limits):
    """What png_encode and jpeg_encode allocate for checked images, the library's `bound` and workspace size: -> (contiguous
    images, files [B,stride], stride >= bound, sizes [B], workspace).  `name`, `limits`: the entry point and what it takes."""
    b, h, w, c = images.shape
    if bound <= 0:
        raise ValueError(f"{name} does not take images of {h}x{w}x{c}: {limits}")
    images = images if images.is_contiguous() else images.contiguous()
    stride = (bound + 15) // 16 * 16
    files = torch.empty((b, stride), dtype=torch.uint8, device=images.device)
    sizes = torch.empty((b,), dtype=torch.int64, device=images.device)
    ws = torch.empty((ws_bytes + 15) // 16 * 2, dtype=torch.int64, device=images.device)
    return images, files, stride, sizes, ws


def png_encode(lib, st, images, filter_mode=3):
    """uint8 [B,H,W,C] (C = 1 or 3, interleaved) -> (files uint8 [B,stride], sizes int64 [B]) on the images' device: image b's
    PNG file is files[b, :sizes[b]] (csrc/png.h).  Nothing is synchronised; stride >= hf_png_bound."""
    _check_encode_images(images)
    if filter_mode not in (0, 1, 2, 3):
        raise ValueError(f"filter mode must be 0..3; got {filter_mode}")
    b, h, w, c = images.shape
    images, files, stride, sizes, ws = _encode_buffers(images, lib.hf_png_bound(h, w, c), lib.hf_png_workspace_bytes(b, h, w, c),
                                                       "hf_png_encode_u8", "a row of at most 24639 bytes, a file below 2 GiB")
    check(lib, lib.hf_png_encode_u8(_p(files), stride, _p(sizes), _p(images), b, h, w, c, int(filter_mode), _p(ws), ws.numel() * 8, st),
          "hf_png_encode_u8")
    return files, sizes


JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def jpeg_encode(lib, st, images, quality=75, subsampling=2):
    """uint8 [B,H,W,C] (C = 1 or 3, interleaved) -> (files uint8 [B,stride], sizes int64 [B]) on the images' device: image b's
    JPEG file is files[b, :sizes[b]] (csrc/jpeg.h).  Nothing is synchronised; stride >= hf_jpeg_bound."""
    _check_encode_images(images)
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"quality must be an integer in 1..100; got {quality!r}")
    if subsampling not in (0, 1, 2):
        raise ValueError(f"subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0); got {subsampling!r}")
    b, h, w, c = images.shape
    images, files, stride, sizes, ws = _encode_buffers(images, lib.hf_jpeg_bound(h, w, c, subsampling),
                                                       lib.hf_jpeg_workspace_bytes(b, h, w, c, subsampling),
                                                       "hf_jpeg_encode_u8", "dimensions of at most 65535, a file below 2 GiB")
    check(lib, lib.hf_jpeg_encode_u8(_p(files), stride, _p(sizes), _p(images), b, h, w, c, quality, subsampling, _p(ws), ws.numel() * 8,
                                     st), "hf_jpeg_encode_u8")
    return files, sizes


JPEG_TABLE_BYTES = 2048  # per file: quantisation tables uint16 [3][64], six Huffman tables of 16 counts + 256 symbols
JPEG_DECODE_ERRORS = {1: "truncated scan (fewer MCUs than the header implies, or no marker ends it)",
                      2: "an unexpected marker in the scan", 3: "a block of more than 64 coefficients",
                      4: "a code that is not in the Huffman table", 5: "a DC difference of more than 11 bits"}


def jpeg_decode(lib, st, scans, offsets, max_scan_bytes, tables, h, w, components, hs, vs, restart_interval, out_channels=3,
                u8=True, f32=False, sub_bytes=0):
    """The scans of B files of one geometry (csrc/jpeg_decode.h) -> (uint8 [B,H,W,out_channels] or None, float32
    [B,out_channels,H,W] or None, status int32 [B,2]) on the scans' device.  scans: uint8 [N]; offsets: int64 [B+1];
    tables: uint8 [B,2048] (the layout include/hairfast_hip.h states).  Nothing is synchronised: the caller reads status."""
    if scans.dtype != torch.uint8 or tables.dtype != torch.uint8 or offsets.dtype != torch.int64:
        raise TypeError(f"expected uint8 scans and tables, int64 offsets; got {scans.dtype}, {tables.dtype}, {offsets.dtype}")
    if tables.ndim != 2 or tables.shape[1] != JPEG_TABLE_BYTES or offsets.ndim != 1 or offsets.numel() != tables.shape[0] + 1:
        raise ValueError(f"expected tables [B,{JPEG_TABLE_BYTES}] and offsets [B+1]; got {tuple(tables.shape)}, {tuple(offsets.shape)}")
    if not (u8 or f32):
        raise ValueError("one of u8 and f32 must be asked for")
    if not (scans.is_contiguous() and tables.is_contiguous() and offsets.is_contiguous()) or scans.numel() == 0:
        raise ValueError("scans, offsets and tables must be contiguous and not empty")
    b, dev = tables.shape[0], scans.device
    ws_bytes = lib.hf_jpeg_decode_workspace_bytes(b, h, w, components, hs, vs, restart_interval, int(max_scan_bytes))
    if ws_bytes <= 0:
        raise ValueError(f"hf_jpeg_decode_u8 does not take {b} files of {h}x{w}, {components} components, sampling {hs}x{vs}")
    out = torch.empty((b, h, w, out_channels), dtype=torch.uint8, device=dev) if u8 else None
    outf = torch.empty((b, out_channels, h, w), dtype=torch.float32, device=dev) if f32 else None
    status = torch.empty((b, 2), dtype=torch.int32, device=dev)
    ws = torch.empty((ws_bytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
    check(lib, lib.hf_jpeg_decode_u8(_p(out) if u8 else None, _p(outf) if f32 else None, _p(status), _p(scans), scans.numel(), _p(offsets),
                                     int(max_scan_bytes), _p(tables), b, h, w, components, hs, vs, restart_interval, out_channels,
                                     int(sub_bytes), _p(ws), ws.numel() * 8, st), "hf_jpeg_decode_u8")
    return out, outf, status


PNG_COLOR_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}  # colour type -> samples per pixel in the file
PNG_DECODE_ERRORS = {1: "truncated stream", 2: "block type 3", 3: "a stored block whose LEN is not the complement of NLEN",
                     4: "an invalid set of code lengths (over-subscribed, incomplete, a repeat past the end, or no end-of-block code)",
                     5: "repeat code 16 with no previous length", 6: "more than 286 literal/length or 30 distance codes",
                     7: "a code that is not in the Huffman table", 8: "length symbol 286 or 287", 9: "distance symbol 30 or 31",
                     10: "a match distance beyond the bytes produced", 11: "more bytes than the image holds",
                     12: "fewer bytes than the image holds", 13: "a filter type above 4", 14: "the Adler-32 does not match",
                     15: "a bad zlib header"}


def png_decode(lib, st, streams, offsets, max_stream_bytes, palettes, h, w, color_type, out_channels=3, u8=True, f32=False,
               token_cap=0):
    """The zlib streams of B PNG files of one geometry (csrc/png_decode.h) -> (uint8 [B,H,W,out_channels] or None, float32
    [B,out_channels,H,W] or None, status int32 [B,2]) on the streams' device.  streams: uint8 [N]; offsets: int64 [B+1];
    palettes: uint8 [B,256,3] for colour type 3, else None.  Nothing is synchronised: the caller reads status."""
    if streams.dtype != torch.uint8 or offsets.dtype != torch.int64 or (palettes is not None and palettes.dtype != torch.uint8):
        raise TypeError(f"expected uint8 streams and palettes, int64 offsets; got {streams.dtype}, {offsets.dtype}")
    if offsets.ndim != 1 or offsets.numel() < 2:
        raise ValueError(f"expected offsets [B+1]; got {tuple(offsets.shape)}")
    b, dev = offsets.numel() - 1, streams.device
    if color_type == 3 and (palettes is None or tuple(palettes.shape) != (b, 256, 3)):
        raise ValueError(f"colour type 3 needs palettes [B,256,3]; got {None if palettes is None else tuple(palettes.shape)}")
    if not (u8 or f32):
        raise ValueError("one of u8 and f32 must be asked for")
    if not (streams.is_contiguous() and offsets.is_contiguous() and (palettes is None or palettes.is_contiguous())) or streams.numel() == 0:
        raise ValueError("streams, offsets and palettes must be contiguous and not empty")
    ws_bytes = lib.hf_png_decode_workspace_bytes(b, h, w, color_type, int(max_stream_bytes))
    if ws_bytes <= 0:
        raise ValueError(f"hf_png_decode_u8 does not take {b} files of {h}x{w}, colour type {color_type}")
    out = torch.empty((b, h, w, out_channels), dtype=torch.uint8, device=dev) if u8 else None
    outf = torch.empty((b, out_channels, h, w), dtype=torch.float32, device=dev) if f32 else None
    status = torch.empty((b, 2), dtype=torch.int32, device=dev)
    ws = torch.empty((ws_bytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
    check(lib, lib.hf_png_decode_u8(_p(out) if u8 else None, _p(outf) if f32 else None, _p(status), _p(streams), streams.numel(), _p(offsets),
                                    int(max_stream_bytes), _p(palettes) if color_type == 3 else None, b, h, w, color_type, out_channels,
                                    int(token_cap), _p(ws), ws.numel() * 8, st), "hf_png_decode_u8")
    return out, outf, status


# ---- Frechet distance (csrc/frechet.h; hairfastgan_amd.metrics chains these).  Everything fp64, row-major ----
def _f64(t, shape, name):
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float64 tensor of shape {tuple(shape)}; got {t.dtype} {tuple(t.shape)}")
    return t


def frechet_accumulate_into(lib, st, total, cov_sum, feats):
    """total[d] += sum_n feats[n], cov_sum[d,d] += sum_n outer(feats[n], feats[n]) in fp64, samples in ascending n; feats
    [n,d] fp32 or fp16 (upcast exactly)."""
    if feats.ndim != 2 or feats.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"features must be [n,d] float32 or float16; got {feats.dtype} {tuple(feats.shape)}")
    n, d = feats.shape
    _f64(total, (d,), "sum")
    _f64(cov_sum, (d, d), "cov_sum")
    if n == 0:
        return
    feats = feats if feats.is_contiguous() else feats.contiguous()
    fn = lib.hf_frechet_accumulate_f64 if feats.dtype == torch.float32 else lib.hf_frechet_accumulate_f16_f64
    check(lib, fn(_p(total), _p(cov_sum), _p(feats), n, d, st), fn.__name__)


def frechet_stats(lib, st, total, cov_sum, n):
    """(mu [d], cov [d,d]) = (sum / n, (cov_sum - n mu mu^T) / (n - 1))."""
    d = total.numel()
    _f64(total, (d,), "sum")
    _f64(cov_sum, (d, d), "cov_sum")
    mu, cov = torch.empty_like(total), torch.empty_like(cov_sum)
    check(lib, lib.hf_frechet_stats_f64(_p(mu), _p(cov), _p(total), _p(cov_sum), int(n), d, st), "hf_frechet_stats_f64")
    return mu, cov


def sym_eigh_f64(lib, st, a, vectors=True, max_sweeps=30, info=None):
    """Eigenvalues (in the solver's order) and, with `vectors`, eigenvectors (columns) of the symmetric fp64 matrix a [d,d]
    by the Jacobi solver: (w [d], V [d,d] or None).  RuntimeError if `max_sweeps` sweeps do not converge.  `info`: a dict
    that receives sweeps and off_norm.  Synchronises the stream once per sweep."""
    import ctypes

    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"expected a square matrix; got {tuple(a.shape)}")
    d = a.shape[0]
    _f64(a, (d, d), "the matrix")
    w = torch.empty(d, dtype=torch.float64, device=a.device)
    v = torch.empty_like(a) if vectors else None
    work = torch.empty(lib.hf_sym_eig_jacobi_work_doubles(d, 1 if vectors else 0), dtype=torch.float64, device=a.device)
    sweeps, off = ctypes.c_int(0), ctypes.c_double(0.0)
    check(lib, lib.hf_sym_eig_jacobi_f64(_p(w), _p(v), _p(a), _p(work), d, int(max_sweeps), ctypes.byref(sweeps), ctypes.byref(off), st),
          "hf_sym_eig_jacobi_f64")
    if info is not None:
        info.update(sweeps=sweeps.value, off_norm=off.value)
    if sweeps.value < 0:
        raise RuntimeError(f"hf_sym_eig_jacobi_f64: no convergence in {max_sweeps} sweeps at d = {d} (off-diagonal norm {off.value:.3e})")
    return w, v


def frechet_congruence(lib, st, w, v, s2):
    """B s2 B^T with B = diag(sqrt(max(w, 0))) v^T, symmetrised."""
    d = w.numel()
    _f64(w, (d,), "w")
    _f64(v, (d, d), "V")
    _f64(s2, (d, d), "sigma2")
    out = torch.empty_like(s2)
    work = torch.empty(2 * d * d, dtype=torch.float64, device=s2.device)
    check(lib, lib.hf_frechet_congruence_f64(_p(out), _p(w), _p(v), _p(s2), _p(work), d, st), "hf_frechet_congruence_f64")
    return out


def frechet_distance_from_stats(lib, st, mu1, sigma1, mu2, sigma2, max_sweeps=30, info=None):
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr((sigma1 sigma2)^(1/2)) as a 0-d fp64 tensor on the device: the
    spectrum of sigma1 sigma2 is taken from sigma1^(1/2) sigma2 sigma1^(1/2) (two symmetric eigenproblems)."""
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError(f"the two sides differ in dimension: {tuple(mu1.shape)} / {tuple(mu2.shape)}")
    d = mu1.numel()
    for t, shape, name in ((mu1, (d,), "mu1"), (mu2, (d,), "mu2"), (sigma1, (d, d), "sigma1"), (sigma2, (d, d), "sigma2")):
        _f64(t, shape, name)
    i1, i2 = {}, {}
    w, v = sym_eigh_f64(lib, st, sigma1, True, max_sweeps, i1)
    m = frechet_congruence(lib, st, w, v, sigma2)
    ev, _ = sym_eigh_f64(lib, st, m, False, max_sweeps, i2)
    if info is not None:
        info.update(sweeps=(i1["sweeps"], i2["sweeps"]), off_norm=(i1["off_norm"], i2["off_norm"]))
    out = torch.empty(1, dtype=torch.float64, device=mu1.device)
    check(lib, lib.hf_frechet_finish_f64(_p(out), _p(mu1), _p(mu2), _p(sigma1), _p(sigma2), _p(ev), d, st), "hf_frechet_finish_f64")
    return out.reshape(())


# ---- LPIPS and L2 / PSNR (csrc/lpips.h; hairfastgan_amd.lpips chains these) ----
def conv2d_direct(lib, st, x, weight, stride=1, pad=0, in_scale=None, in_shift=None, bias=None, act=ACT_NONE, alpha=0.0):
    """hf_conv2d_direct_f32: x [N,cin,H,W] (cin <= 4), weight [cout,cin,k,k] in torch's layout -> [N,cout,oh,ow]; the input
    affine touches real pixels only (the padding stays zero)."""
    x, weight = _c(x), _c(weight)
    n, cin, h, w = x.shape
    cout, cin_w, k, k2 = weight.shape
    if cin_w != cin or k2 != k:
        raise ValueError(f"weight {tuple(weight.shape)} does not fit an input of {cin} channels")
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = x.new_empty((n, cout, max(oh, 0), max(ow, 0)))
    check(lib, lib.hf_conv2d_direct_f32(_p(out), _p(x), _p(weight), _p(_c(in_scale)), _p(_c(in_shift)), _p(_c(bias)), act,
                                        float(alpha), n, cin, cout, h, w, k, stride, pad, st), "hf_conv2d_direct_f32")
    return out


def maxpool2d(lib, st, x, k, stride):
    """nn.MaxPool2d(k, stride): no padding, floor mode."""
    x = _c(x)
    b, c, h, w = x.shape
    out = x.new_empty((b, c, max((h - k) // stride + 1, 0), max((w - k) // stride + 1, 0)))
    check(lib, lib.hf_maxpool2d_f32(_p(out), _p(x), b * c, h, w, k, stride, st), "hf_maxpool2d_f32")
    return out


def lpips_layer_into(lib, st, dist, fx, fy, lin_w, accumulate=False):
    """dist [N] float64 = (or +=) the LPIPS distance of one layer's feature maps fx, fy [N,C,H,W] under lin_w [C]."""
    fx, fy, lin_w = _c(fx), _c(fy), _c(lin_w).reshape(-1)
    n, c, h, w = fx.shape
    if fy.shape != fx.shape or lin_w.numel() != c:
        raise ValueError(f"feature maps {tuple(fx.shape)} / {tuple(fy.shape)} and {lin_w.numel()} weights do not fit")
    _f64(dist, (n,), "dist")
    work = torch.empty(max(int(lib.hf_lpips_layer_work_doubles(n, h, w)), 1), dtype=torch.float64, device=fx.device)
    check(lib, lib.hf_lpips_layer_f64(_p(dist), _p(fx), _p(fy), _p(lin_w), _p(work), n, c, h, w, 1 if accumulate else 0, st),
          "hf_lpips_layer_f64")
    return dist


def sq_err_sum(lib, st, a, b):
    """[N] float64: sum (a - b)^2 over everything but the first axis; a, b both uint8 or both fp32."""
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (torch.uint8, torch.float32) or a.ndim < 2:
        raise ValueError(f"two uint8 or two fp32 tensors [N, ...] of one shape; got {a.dtype} {tuple(a.shape)}, {b.dtype} {tuple(b.shape)}")
    a, b = a.contiguous(), b.contiguous()
    n = a.shape[0]
    per_image = a.numel() // max(n, 1)
    out = torch.empty(n, dtype=torch.float64, device=a.device)
    work = torch.empty(max(int(lib.hf_sq_err_sum_work_doubles(n, per_image)), 1), dtype=torch.float64, device=a.device)
    check(lib, lib.hf_sq_err_sum_f64(_p(out), _p(a), _p(b), _p(work), n, per_image, 1 if a.dtype == torch.uint8 else 0, st),
          "hf_sq_err_sum_f64")
    return out


SSIM_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}


def ssim_planes(lib, st, x, y, taps, c1, c2, cn, mask=None, want_cs=False, want_map=False, want_next=False):
    """hf_ssim_planes_f64 (csrc/ssim.h) of images x, y [N,C,H,W], both uint8, fp32 or fp64; taps: the 1-D window, float64 on the
    device.  -> {"s": [N,C] float64 sums of S over the valid region} plus, on request, "cs" (sums of cs), "map" [N,C,oh,ow],
    "next" (the 2x2 means of x and of y, float64 [N,C,H//2,W//2]).  mask: fp32 [N,oh,ow] weights shared by an image's
    channels; then "s" holds the sums of m S and "m" those of m (want_cs is not available with a mask)."""
    if x.shape != y.shape or x.dtype != y.dtype or x.dtype not in SSIM_DTYPES or x.ndim != 4:
        raise ValueError(f"two uint8, fp32 or fp64 images [N,C,H,W] of one shape; got {x.dtype} {tuple(x.shape)}, {y.dtype} {tuple(y.shape)}")
    if mask is not None and want_cs:
        raise ValueError("the second sum is the mask's with a mask: no cs sums")
    x, y = x.contiguous(), y.contiguous()
    n, c, h, w = x.shape
    win = taps.numel()
    _f64(taps, (win,), "taps")
    oh, ow = h - win + 1, w - win + 1
    if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != (n, oh, ow) or not mask.is_contiguous() or
                             mask.device != x.device):
        raise ValueError(f"mask must be a contiguous fp32 tensor of shape {(n, oh, ow)} on {x.device}; got {mask.dtype} "
                         f"{tuple(mask.shape)} on {mask.device}")
    if y.device != x.device or taps.device != x.device:
        raise ValueError(f"x, y and taps must share a device; got {x.device}, {y.device}, {taps.device}")

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=x.device)

    out = {"s": f64(n, c)}
    aux = f64(n, c) if want_cs or mask is not None else None
    if aux is not None:
        out["m" if mask is not None else "cs"] = aux
    if want_map:
        out["map"] = f64(n, c, max(oh, 0), max(ow, 0))
    if want_next:
        out["next"] = (f64(n, c, h // 2, w // 2), f64(n, c, h // 2, w // 2))
    nx, ny = out.get("next", (None, None))
    work = f64(max(int(lib.hf_ssim_work_doubles(n * c, h, w, win)), 1))
    check(lib, lib.hf_ssim_planes_f64(_p(out["s"]), _p(aux), _p(out.get("map")), _p(nx), _p(ny), _p(x), _p(y), _p(mask), _p(taps), _p(work),
                                      SSIM_DTYPES[x.dtype], n * c, c, h, w, win, float(c1), float(c2), float(cn), st), "hf_ssim_planes_f64")
    return out


# ---- identity similarity (csrc/identity.h; hairfastgan_amd.identity chains these) ----
def crop_avgpool(lib, st, x, y0, x0, ch, cw, oh, ow, scale=None, shift=None):
    """hf_crop_avgpool_f32: AdaptiveAvgPool2d((oh, ow)) of x[:, :, y0:y0+ch, x0:x0+cw], the window read in place;
    scale / shift [C]: a per-channel affine of the means."""
    x = _c(x)
    n, c, h, w = x.shape
    out = x.new_empty((n, c, max(oh, 0), max(ow, 0)))
    check(lib, lib.hf_crop_avgpool_f32(_p(out), _p(x), _p(_c(scale)), _p(_c(shift)), n, c, h, w, y0, x0, ch, cw, oh, ow, st),
          "hf_crop_avgpool_f32")
    return out


def l2_normalize_rows(lib, st, x, want_norms=False):
    """hf_l2_normalize_rows_f32: x [R,D] -> x / |x|_2 per row (-> (unit rows, norms [R]) with want_norms)."""
    x = _c(x)
    rows, d = x.shape
    out = torch.empty_like(x)
    norms = x.new_empty(rows) if want_norms else None
    check(lib, lib.hf_l2_normalize_rows_f32(_p(out), _p(norms), _p(x), rows, d, st), "hf_l2_normalize_rows_f32")
    return (out, norms) if want_norms else out


def row_similarity(lib, st, a, b, paired=True):
    """hf_row_similarity_f64: fp32 rows a [N,D], b [M,D] -> float64 [N] (paired, N == M) or [N,M]."""
    a, b = _c(a), _c(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or (paired and a.shape[0] != b.shape[0]):
        raise ValueError(f"rows {tuple(a.shape)} and {tuple(b.shape)} do not fit{' pairwise' if paired else ''}")
    n, m = a.shape[0], b.shape[0]
    out = torch.empty((n,) if paired else (n, m), dtype=torch.float64, device=a.device)
    check(lib, lib.hf_row_similarity_f64(_p(out), _p(a), _p(b), n, m, a.shape[1], 1 if paired else 0, st), "hf_row_similarity_f64")
    return out


# ---- FID Inception-v3 (csrc/conv_rect.h, csrc/inception.h; hairfastgan_amd.inception chains these) ----
class RectWeights:
    """A rectangular conv's weights prepared once: `w` [cout,cin,kh,kw] fp32 (the exact-fp32 form reads it) and, derived on
    first use, the fp16 (hi, lo) split of the zero-padded table [tap*cinp + ci][co] for the matrix-core form."""

    def __init__(self, w):
        self.w = _c(w.detach())
        self.cout, self.cin, self.kh, self.kw = self.w.shape
        self._f16 = None

    def f16(self, lib, st):
        if self._f16 is None:
            cinp, coutp = -(-self.cin // 32) * 32, -(-self.cout // 64) * 64
            table = self.w.new_zeros((self.kh * self.kw, cinp, coutp))
            table[:, :self.cin, :self.cout] = self.w.permute(2, 3, 1, 0).reshape(self.kh * self.kw, self.cin, self.cout)
            self._f16 = conv_split_weights_f16(lib, st, table.reshape(1, -1, coutp))
        return self._f16


def conv_out_size(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def conv2d_rect_into(lib, st, out, oc0, x, xc0, wts, nterms, stride=1, pad=(0, 0), out_scale=None, bias=None, relu=False):
    """hf_conv2d_rect_f16_f32: channels oc0 .. oc0+cout-1 of out [N,Co,oh,ow] = the conv of channels xc0 .. xc0+cin-1 of
    x [N,Cx,H,W] with `wts` (a RectWeights), torch's symmetric padding pad = (rows, columns); nterms 3 / 1 / 0."""
    if x.dtype != torch.float32 or out.dtype != torch.float32 or not x.is_contiguous() or not out.is_contiguous():
        raise TypeError("conv2d_rect_into takes contiguous fp32 tensors")
    n, xct, h, w = x.shape
    oh, ow = conv_out_size(h, wts.kh, stride, pad[0]), conv_out_size(w, wts.kw, stride, pad[1])
    if out.ndim != 4 or out.shape[0] != n or out.shape[2] != oh or out.shape[3] != ow or oc0 < 0 or oc0 + wts.cout > out.shape[1]:
        raise ValueError(f"output {tuple(out.shape)} does not hold channels {oc0}..{oc0 + wts.cout - 1} of [{n},*,{oh},{ow}]")
    hi, lo = wts.f16(lib, st) if nterms else (None, None)
    check(lib, lib.hf_conv2d_rect_f16_f32(_p(out), _p(x), _p(wts.w), _p(hi), _p(lo), nterms, _p(_c(out_scale)), _p(_c(bias)),
                                          1 if relu else 0, n, wts.cin, wts.cout, h, w, wts.kh, wts.kw, stride, pad[0], pad[1], oh, ow,
                                          xc0, xct, oc0, out.shape[1], st), "hf_conv2d_rect_f16_f32")
    return out


def pool3x3_into(lib, st, out, oc0, x, xc0, c, mode, stride):
    """hf_pool3x3_f32: mode "max" / "avg" (padding not counted); stride 1 (pad 1) or 2 (pad 0, floor)."""
    if x.dtype != torch.float32 or out.dtype != torch.float32 or not x.is_contiguous() or not out.is_contiguous():
        raise TypeError("pool3x3_into takes contiguous fp32 tensors")
    n, xct, h, w = x.shape
    oh, ow = (h, w) if stride == 1 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    if out.ndim != 4 or out.shape[0] != n or out.shape[2] != oh or out.shape[3] != ow or oc0 < 0 or oc0 + c > out.shape[1]:
        raise ValueError(f"output {tuple(out.shape)} does not hold channels {oc0}..{oc0 + c - 1} of [{n},*,{oh},{ow}]")
    check(lib, lib.hf_pool3x3_f32(_p(out), _p(x), {"max": 0, "avg": 1}[mode], n, c, h, w, stride, xc0, xct, oc0, out.shape[1], st),
          "hf_pool3x3_f32")
    return out


def resize_bilinear_tf1(lib, st, x, oh, ow, mul=None, add=None):
    """hf_resize_bilinear_tf1_f32: x [N,C,H,W] uint8 or fp32 -> fp32 [N,C,oh,ow]; mul / add: v * mul + add of the result."""
    if x.dtype not in (torch.uint8, torch.float32) or x.ndim != 4:
        raise TypeError(f"resize_bilinear_tf1 takes uint8 or fp32 [N,C,H,W]; got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    n, c, h, w = x.shape
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    affine = mul is not None or add is not None
    check(lib, lib.hf_resize_bilinear_tf1_f32(_p(out), _p(x), 1 if x.dtype == torch.uint8 else 0, n, c, h, w, oh, ow, 1 if affine else 0,
                                              1.0 if mul is None else float(mul), 0.0 if add is None else float(add), st),
          "hf_resize_bilinear_tf1_f32")
    return out
