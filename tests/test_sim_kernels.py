"""CPU tests: the HIP kernel SOURCES interpreted by tests/hipsim vs the oracle and the
golden vectors produced by the real reference.  They validate index arithmetic, LDS
layouts, the MFMA fragment maps and tile geometry before any GPU time is spent; the
numerical parity proper is re-established on the GPU by the -m gpu tests.  The conv-kernel checks that also run on the GPU
(tests/test_gpu_parity.py) are stated once, in tests/conv_kernel_checks.py; their tests here are one call each."""
import numpy as np
import pytest
import torch

from hairfastgan_amd import _marshal as M
from oracle import cases as C
from oracle import ref_stylegan2 as O
from tests import conv_kernel_checks as K

TOL = 2e-5
CPU = torch.device("cpu")


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("name", list(C.UPFIRDN_CASES))
def test_upfirdn2d(simlib, golden, name):
    c = C.UPFIRDN_CASES[name]
    x, k = C.upfirdn_input(name), C.blur_kernel4()
    y = M.upfirdn2d(simlib, None, x, k, c["up"], c["up"], c["down"], c["down"], c["pad"][0], c["pad"][1],
                    c["pad"][0], c["pad"][1])
    ref = torch.from_numpy(golden("upfirdn2d.npz")[name])
    assert y.shape == ref.shape
    assert maxdiff(y, ref) < TOL


@pytest.mark.parametrize("name", list(C.ACT_CASES))
def test_fused_bias_act(simlib, golden, name):
    x, b = C.act_inputs(name)
    y = M.fused_bias_act(simlib, None, x, b, 0.2, 2 ** 0.5)
    assert maxdiff(y, torch.from_numpy(golden("fused_act.npz")[name])) < 1e-6


def test_noise_bias_act(simlib):
    x = torch.randn(2, 5, 6, 6)
    nz = torch.randn(1, 1, 6, 6)
    nw = torch.tensor([0.3])
    b = torch.randn(5)
    y = M.noise_bias_act(simlib, None, x, nz, nw, b)
    assert maxdiff(y, O.fused_leaky_relu(x + nw * nz, b)) < 1e-6
    nzb = torch.randn(2, 1, 6, 6)
    y = M.noise_bias_act(simlib, None, x, nzb, nw, b)
    assert maxdiff(y, O.fused_leaky_relu(x + nw * nzb, b)) < 1e-6
    x = torch.randn(2, 3, 5, 3)  # hw not a multiple of 4 -> scalar kernel
    nz = torch.randn(2, 1, 5, 3)
    y = M.noise_bias_act(simlib, None, x, nz, nw, b[:3].contiguous())
    assert maxdiff(y, O.fused_leaky_relu(x + nw * nz, b[:3])) < 1e-6


def _style(simlib, P, w):
    wt, wsq = M.prepare_weights(simlib, None, P["L.conv.weight"])
    s = M.modulation(simlib, None, w, P["L.conv.modulation.weight"], P["L.conv.modulation.bias"])
    return wt, wsq, s


@pytest.mark.parametrize("name", [c[0] for c in C.MODCONV_SMALL])
def test_style_and_demod(simlib, name):
    d = C.modconv_small_inputs(name)
    P = d["P_up0"]
    wt, wsq, s = _style(simlib, P, d["w"])
    s_ref = O.equal_linear(d["w"], P["L.conv.modulation.weight"], P["L.conv.modulation.bias"])
    assert maxdiff(s, s_ref) < 1e-5
    cin = d["cin"]
    wref = P["L.conv.weight"][0] / (cin * 9) ** 0.5
    assert maxdiff(wt, wref.permute(2, 3, 1, 0).reshape(9, cin, -1)) < 1e-7
    dm = M.demod(simlib, None, s, wsq)
    dref = torch.rsqrt(((wref[None] * s_ref[:, None, :, None, None]) ** 2).sum([2, 3, 4]) + 1e-8)
    assert maxdiff(dm, dref) / float(dref.abs().max()) < 1e-5


@pytest.mark.parametrize("name", [c[0] for c in C.MODCONV_SMALL])
@pytest.mark.parametrize("up", [False, True])
def test_styled_conv(simlib, golden, name, up):
    d = C.modconv_small_inputs(name)
    P = d[f"P_up{int(up)}"]
    wt, wsq, s = _style(simlib, P, d["w"])
    dm = M.demod(simlib, None, s, wsq)
    G = golden("modconv_small.npz")
    if up:
        y_conv = M.modconv3x3_up(simlib, None, d["x"], wt, s, dm, P["L.conv.blur.kernel"], None, None, None)
        y = M.modconv3x3_up(simlib, None, d["x"], wt, s, dm, P["L.conv.blur.kernel"], d["noise_up1"],
                            P["L.noise.weight"], P["L.activate.bias"])
    else:
        y_conv = M.modconv3x3(simlib, None, d["x"], wt, s, dm, None, None, None)
        y = M.modconv3x3(simlib, None, d["x"], wt, s, dm, d["noise_up0"], P["L.noise.weight"], P["L.activate.bias"])
    ref_conv = torch.from_numpy(G[f"{name}_up{int(up)}_conv"])
    ref = torch.from_numpy(G[f"{name}_up{int(up)}_styled"])
    assert y_conv.shape == ref_conv.shape
    assert maxdiff(y_conv, ref_conv) < TOL * max(1.0, float(ref_conv.abs().max()))
    assert maxdiff(y, ref) < TOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("name", [c[0] for c in C.MODCONV_SMALL])
@pytest.mark.parametrize("use_skip", [False, True])
def test_torgb(simlib, golden, name, use_skip):
    d = C.modconv_small_inputs(name)
    P = d["P_rgb"]
    wt, _ = M.prepare_weights(simlib, None, P["L.conv.weight"])
    s = M.modulation(simlib, None, d["w"], P["L.conv.modulation.weight"], P["L.conv.modulation.bias"])
    y = M.torgb(simlib, None, d["x_rgb"], wt, s, P["L.bias"], d["skip"] if use_skip else None,
                P["L.upsample.kernel"])
    ref = torch.from_numpy(golden("modconv_small.npz")[f"{name}_rgb_skip{int(use_skip)}"])
    assert maxdiff(y, ref) < TOL * max(1.0, float(ref.abs().max()))


def test_modconv_tile_geometries(simlib):
    K.run_all("tile_geometries", simlib, None, CPU)


@pytest.mark.parametrize("case", K.params("pipelined", gpu=False))
def test_modconv_pipelined_configs(simlib, case):
    K.check_pipelined(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("f16_matrix_cores", gpu=False))
def test_modconv_f16_matrix_cores(simlib, case):
    K.check_f16_matrix_cores(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("up_f16_matrix_cores", gpu=False))
def test_modconv_up_f16_matrix_cores(simlib, case):
    K.check_up_f16_matrix_cores(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("persistent_tile_walk", gpu=False))
def test_modconv_f16_persistent_tile_walk(simlib, case):
    K.check_persistent_tile_walk(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("fused_torgb", gpu=False))
def test_modconv_f16_fused_torgb(simlib, case):
    K.check_fused_torgb(simlib, None, CPU, case)


@pytest.mark.parametrize("shape", [(2, 16, 6, 5), (1, 8, 9, 40), (1, 24, 33, 70)])
def test_blur_split_output_is_the_split_of_the_fp32_blur(simlib, shape):
    """hf_blur_noise_bias_act_split_f16 == hf_blur_noise_bias_act_f32 followed by *s, fp16 (hi, lo)
    split and K-blocking, bit for bit (odd sizes, edges, strips shorter than the plane)."""
    B, C, h, w = shape
    torch.manual_seed(13)
    pitch = simlib.hf_modconv_up_pitch(w)
    tmp = torch.randn(B, C, 2 * h + 1, pitch)
    k4 = O.blur_kernel_1d_to_2d(gain=4.0)
    nz, nw, bias, s_next = torch.randn(B, 1, 2 * h, 2 * w), torch.tensor([0.3]), torch.randn(C), torch.rand(B, C) + 0.5
    out = torch.empty(B, C, 2 * h, 2 * w)
    M.check(simlib, simlib.hf_blur_noise_bias_act_f32(M._p(out), M._p(tmp), M._p(k4), M._p(nz), M._p(nw), 4 * h * w, M._p(bias),
                                                      B, C, 2 * h + 1, 2 * w + 1, pitch, 0.2, 2 ** 0.5, None), "blur")
    hi = torch.empty(B, C // 8, 2 * h, 2 * w, 8, dtype=torch.float16)
    lo = torch.empty_like(hi)
    M.check(simlib, simlib.hf_blur_noise_bias_act_split_f16(M._p(hi), M._p(lo), M._p(tmp), M._p(k4), M._p(nz), M._p(nw), 4 * h * w,
                                                            M._p(bias), M._p(s_next), B, C, 2 * h + 1, 2 * w + 1, pitch, 0.2,
                                                            2 ** 0.5, None), "blur split")
    v = out * s_next[:, :, None, None]
    eh = v.half()
    el = (v - eh.float()).half()
    blocked = lambda t: t.reshape(B, C // 8, 8, 2 * h, 2 * w).permute(0, 1, 3, 4, 2).contiguous()  # noqa: E731
    assert torch.equal(hi, blocked(eh))
    assert torch.equal(lo, blocked(el))


@pytest.mark.parametrize("case", K.params("presplit_input", gpu=False))
def test_modconv_f16_presplit_input(simlib, case):
    K.check_presplit_input(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("presplit_chain", gpu=False))
def test_presplit_chain_same_res_to_transposed(simlib, case):
    K.check_presplit_chain(simlib, None, CPU, case)


def test_style_batch_equals_per_layer_launches(simlib):
    """hf_style_batch_f32 (every layer's modulation + demodulation in two launches) against
    hf_modulation_f32 / hf_demod_f32 per layer: identical values, strided W+ rows, a job without
    demodulation (ToRGB), different channel counts per job."""
    import types

    torch.manual_seed(29)
    B, sd = 3, 48
    latent = torch.randn(B, 7, sd)
    convs, rows = [], []
    for cin, cout, demod, row in [(16, 24, True, 0), (40, 3, False, 5), (8, 8, True, 2)]:
        w = torch.randn(1, cout, cin, 3 if demod else 1, 3 if demod else 1)
        wt, wsq = M.prepare_weights(simlib, None, w)
        c = types.SimpleNamespace(in_channel=cin, out_channel=cout, demodulate=demod,
                                  modulation=types.SimpleNamespace(weight=torch.randn(cin, sd), bias=torch.randn(cin)),
                                  prepared=lambda wt=wt, wsq=wsq: (wt, wsq))
        convs.append(c)
        rows.append(row)
    table, layout, total = M.style_job_table(convs, rows, B, "cpu")
    res = M.style_batch(simlib, None, latent, table, layout, total, 40, 24)
    for c, row, (s, d) in zip(convs, rows, res):
        s_ref = M.modulation(simlib, None, latent[:, row], c.modulation.weight, c.modulation.bias)
        if c.demodulate:
            d_ref = M.demod(simlib, None, s_ref, c.prepared()[1])
            # the batch applies hf_style_normalize_f32: per sample s * 2^-e, d * 2^e (exact), max|s| in [1, 2)
            e = torch.floor(torch.log2(s_ref.abs().amax(1, keepdim=True)))
            assert torch.equal(s, s_ref * torch.exp2(-e)) and torch.equal(d, d_ref * torch.exp2(e))
            assert float(s.abs().amax(1).min()) >= 1.0 and float(s.abs().amax(1).max()) < 2.0
            M.style_normalize(simlib, None, s_ref, d_ref)  # the per-layer entry point does the same, in place
            assert torch.equal(s, s_ref) and torch.equal(d, d_ref)
        else:
            assert torch.equal(s, s_ref)  # no demodulation (ToRGB): nothing could absorb the factor
            assert d is None


def test_f16_split_range(simlib):
    K.run_all("f16_split_range", simlib, None, CPU)
    K.run_all("f16_split_saturates", simlib, None, CPU)


@pytest.mark.parametrize("shape,use_skip", [((2, 64, 4, 4), False), ((3, 136, 8, 12), True), ((1, 512, 16, 16), True)])
def test_torgb_small_plane_kernel(simlib, shape, use_skip):
    """hf_torgb_f32's small-plane kernel (channels split over 16 waves, LDS reduction) against a
    direct torch statement of ToRGB (model.py:356-365): ragged pixel counts, cin not a multiple of 16."""
    B, cin, H, W = shape
    torch.manual_seed(31)
    x, wt, s, bias = torch.randn(B, cin, H, W), torch.randn(1, cin, 3), torch.rand(B, cin) + 0.5, torch.randn(3)
    skip = torch.randn(B, 3, H // 2, W // 2) if use_skip else None
    k4 = O.blur_kernel_1d_to_2d(gain=4.0)
    y = M.torgb(simlib, None, x, wt, s, bias, skip, k4 if use_skip else None)
    ref = torch.einsum("bihw,ic,bi->bchw", x, wt[0], s) + bias.view(1, 3, 1, 1)
    if use_skip:
        ref = ref + O.upfirdn2d(skip, k4, up=2, pad=(2, 1))
    assert maxdiff(y, ref) < 1e-4 * max(1.0, float(ref.abs().max()))


def test_mapping_network_kernels(simlib, golden):
    """Row a11: PixelNorm + 8 x EqualLinear(lr_mul 0.01, fused_lrelu) through hf_pixel_norm_f32 /
    hf_equal_linear_f32 against the reference's golden w (and the oracle), 3 and 11 rows (> 8: two launches)."""
    size, cm, n_mlp, _, _ = C.GENERATOR_CASES["g64"]
    P = C.generator_params(O.generator_param_shapes(size, 512, n_mlp, cm))
    for B in (3, 11):
        z = C.mapping_inputs(B)
        x = M.pixel_norm(simlib, None, z)
        for i in range(1, n_mlp + 1):
            x = M.equal_linear(simlib, None, x, P[f"style.{i}.weight"], P[f"style.{i}.bias"], 0.01, True)
        ref = O.mapping_network(P, z, n_mlp=n_mlp)
        assert maxdiff(x, ref) < 1e-5 * max(1.0, float(ref.abs().max()))
        if B == 3:
            assert maxdiff(x, torch.from_numpy(golden("generator_64.npz")["g64_mapping_w"])) < 1e-5
    # no activation, no bias, strided input rows
    xx = torch.randn(5, 40)[:, :24]
    w = torch.randn(7, 24)
    y = M.equal_linear(simlib, None, xx, w, None, 1.0, False)
    assert maxdiff(y, xx @ w.t() / 24 ** 0.5) < 1e-5


@pytest.mark.parametrize("case", K.params("up_fused_blur", gpu=False))
def test_modconv_up_fused_blur(simlib, case):
    K.check_up_fused_blur(simlib, None, CPU, case)


def test_modconv_up_fused_blur_plain_fp16_operands(simlib):
    K.run_all("up_fused_blur_plain_fp16", simlib, None, CPU)


@pytest.mark.parametrize("case", K.params("up_fused_blur_persistent", gpu=False))
def test_modconv_up_fused_blur_persistent_walk(simlib, case):
    K.check_up_fused_blur_persistent(simlib, None, CPU, case)


@pytest.mark.parametrize("case", K.params("conv_rows", gpu=False))
def test_conv_rows_pipeline_equals_tiled_kernel(simlib, case):
    K.check_conv_rows(simlib, None, CPU, case)


@pytest.mark.parametrize("nterms", [3, 1])
def test_modconv_f16_tile_forms_51_and_52_give_equal_bits(simlib, nterms):
    """The two same-resolution tile forms of csrc/convh.hip (51: 64 co x 256 px, 2 x 4 waves of 1 x 2 MFMA tiles; 52: 64 co x
    512 px, 8 waves of 2 x 2 tiles) walk K in the same order - chunk, tap, (hi*hi, hi*lo, lo*hi) - so a sample's bits do
    not depend on which one a launch takes: the choice follows the whole launch also under batch-invariant plans.  Ragged
    plane, odd chunk count, fp32 and pre-split input, noise + bias + lrelu epilogue."""
    L = K.styled_layer(simlib, None, CPU, (2, 48, 64, 36, 40), 23, False)
    act = K.presplit(L)
    out = {}
    for cfg in (51, 52):
        with K.debug(simlib, "dispatch", cfg, 0):
            out[cfg] = K.conv_f16(simlib, None, L, nterms)
            assert simlib.hf_debug_last_path() == 500 + cfg
            out[cfg, "pre"] = M.modconv3x3_f16_pre(simlib, None, act, L.hi, L.lo, nterms, L.dm, *K.tail(L))
            assert simlib.hf_debug_last_path() == 520 + cfg
    assert torch.equal(out[51], out[52]) and torch.equal(out[51, "pre"], out[52, "pre"]) and torch.equal(out[51], out[51, "pre"])


def test_small_plane_tap_gemm_virtual_split_k(simlib):
    """hf_modconv3x3_small_f16_f32 (the tap GEMM of the generator's small planes + small_combine) under batch-invariant
    plans: a batch that fills "the chip" keeps the canonical K partition inside its blocks (one slab instead of `splits`) -
    the bits of the one-sample launches."""
    B, cin, cout, H, W = shape = 4, 256, 64, 8, 8
    L = K.styled_layer(simlib, None, CPU, shape, 29, False)
    x, s, dm, nz, nw, bias = L.x, L.s, L.dm, L.nz, L.nw, L.bias
    w9 = M.split_weights_small(simlib, None, L.wt)
    prev = simlib.hf_set_batch_invariant(1)
    try:
        ref = torch.cat([M.modconv3x3_small(simlib, None, x[b:b + 1], w9, 3, s[b:b + 1], dm[b:b + 1], nz[b:b + 1], nw, bias, cout)
                         for b in range(B)])
        n1 = simlib.hf_modconv3x3_small_workspace_floats(B, cin, cout, H, W)
        # canonical batch 3: 2 pixel tiles (two 8 x 8 images each) x 9 channel tiles = 18 blocks -> splits; batch 4: 18 too...
        simlib.hf_debug_set_tuning(18 << 24)
        y = M.modconv3x3_small(simlib, None, x, w9, 3, s, dm, nz, nw, bias, cout)
        n2 = simlib.hf_modconv3x3_small_workspace_floats(B, cin, cout, H, W)
    finally:
        simlib.hf_debug_set_tuning(0)
        simlib.hf_set_batch_invariant(prev)
    assert torch.equal(y, ref)
    assert n2 < n1  # one slab instead of `splits`: the virtual form ran


@pytest.mark.parametrize("up", [False, True])
def test_modconv_f16_block_order_does_not_change_results(simlib, up):
    """csrc/convh.hip launches (tile walkers, cout tiles) or - ConvParams::swap_xy, forced here by hf_debug_set_tuning bit 3 -
    (cout tiles, tile walkers): which of the input tile and the cout tile's weights stays in an XCD's L2.  Identical results:
    same-resolution conv with split output and the transposed conv, several cout tiles, a persistent tile walk."""
    L = K.styled_layer(simlib, None, CPU, (2, 32, 128, 16, 32), 37, up)
    s2, act = torch.rand(2, 128) + 0.5, K.presplit(L)
    outs = []
    try:
        for tune in (0, 8):
            simlib.hf_debug_set_tuning(tune)
            simlib.hf_debug_set_persistent_blocks(4)  # 4 resident blocks over 2 cout tiles: every block walks several tiles
            if up:
                outs.append(M.modconv3x3_up(simlib, None, act, L.wt, None, L.dm, L.k4, *K.tail(L), f16=(L.hi, L.lo, 3)))
            else:
                y = M.modconv3x3_f16_pre(simlib, None, act, L.hi, L.lo, 3, L.dm, *K.tail(L), split_for=s2)
                parts = y if isinstance(y, (tuple, list)) else (y,)
                flat = []
                for t_ in parts:
                    flat += [t_.hi.float().flatten(), t_.lo.float().flatten()] if isinstance(t_, M.SplitActivation) else ([t_.flatten()] if torch.is_tensor(t_) else [])
                outs.append(torch.cat(flat))
    finally:
        simlib.hf_debug_set_tuning(0)
        simlib.hf_debug_set_persistent_blocks(0)
    assert outs[0].numel() > 0 and torch.equal(outs[0], outs[1])
