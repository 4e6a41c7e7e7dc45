"""GPU parity tests (-m gpu): the HIP path, called through the product API and hence the
C ABI, against (a) the committed golden vectors produced by the real reference and
(b) the CPU oracle on the same seeded inputs.

Tolerance: fp32 everywhere.  The HIP path reassociates the contraction (MFMA k-order,
modulation applied to activations, demodulation to outputs), so results differ from the
reference's ATen kernels at fp32 round-off: we require max-abs <= 1e-4 * max(1, |ref|max)
and MSE <= 1e-8 * max(1, var) (SURVEY.md section 8c measured the reference's own
fp32-vs-fp64 noise floor at 8.9e-6 max-abs); north_star's pixel-MSE bar is 1e-4.

The kernel-level conv checks are stated once, in tests/conv_kernel_checks.py, for this file and for
tests/test_sim_kernels.py; their tests here are one call each.
"""
import numpy as np
import pytest
import torch

from oracle import cases as C
from oracle import ref_stylegan2 as O
from tests import conv_kernel_checks as K

pytestmark = pytest.mark.gpu

REL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def _native():
    """(library, stream, device) of the checks in tests/conv_kernel_checks.py."""
    dev = _dev()
    from hairfastgan_amd._runtime import lib, stream

    return lib(), stream(), dev


def close(y, ref, rel=REL):
    y = y.detach().cpu().double()
    ref = ref.detach().cpu().double() if torch.is_tensor(ref) else torch.from_numpy(np.asarray(ref)).double()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    scale = max(1.0, float(ref.abs().max()))
    err = float((y - ref).abs().max())
    mse = float(((y - ref) ** 2).mean())
    assert err <= rel * scale, f"max-abs {err:.3e} > {rel * scale:.3e}"
    assert mse <= 1e-8 * max(1.0, float(ref.var())), f"mse {mse:.3e}"
    # scale-free: the RMS error relative to the RMS of the reference (max-abs relative to the LARGEST value is loose
    # for feature maps whose typical magnitude is far below their maximum)
    rms_ref = float((ref ** 2).mean()) ** 0.5
    if rms_ref > 1e-6:
        assert mse ** 0.5 <= 0.3 * rel * rms_ref, f"relative RMS error {mse ** 0.5 / rms_ref:.3e} > {0.3 * rel:.1e}"
    return err


def test_native_library_is_loaded():
    from hairfastgan_amd import _lib

    lib = _lib.load()
    assert lib.hf_abi_version() == 13
    maps = open("/proc/self/maps").read()
    assert "libhairfast_hip.so" in maps


@pytest.mark.parametrize("name", list(C.UPFIRDN_CASES))
def test_upfirdn2d(golden, name):
    from hairfastgan_amd.stylegan2.op import upfirdn2d

    dev = _dev()
    c = C.UPFIRDN_CASES[name]
    y = upfirdn2d(C.upfirdn_input(name).to(dev), C.blur_kernel4().to(dev), up=c["up"], down=c["down"], pad=c["pad"])
    close(y, golden("upfirdn2d.npz")[name], 1e-5)


@pytest.mark.parametrize("name", list(C.ACT_CASES))
def test_fused_leaky_relu(golden, name):
    from hairfastgan_amd.stylegan2.op import FusedLeakyReLU, fused_leaky_relu

    dev = _dev()
    x, b = C.act_inputs(name)
    close(fused_leaky_relu(x.to(dev), b.to(dev)), golden("fused_act.npz")[name], 1e-6)
    m = FusedLeakyReLU(b.numel()).to(dev)
    m.bias.data.copy_(b)
    close(m(x.to(dev)), golden("fused_act.npz")[name], 1e-6)
    # empty input
    assert fused_leaky_relu(x[:0].to(dev), b.to(dev)).shape == x[:0].shape


def _load_small(mod, P, dev):
    mod.load_state_dict({k[2:]: v for k, v in P.items()})
    return mod.to(dev).eval()


@pytest.mark.parametrize("name", [c[0] for c in C.MODCONV_SMALL])
def test_small_modules_vs_reference_golden(golden, name):
    import hairfastgan_amd.stylegan2.model as model

    dev = _dev()
    d = C.modconv_small_inputs(name)
    G = golden("modconv_small.npz")
    x, w = d["x"].to(dev), d["w"].to(dev)
    with torch.inference_mode():
        for up in (False, True):
            m = _load_small(model.StyledConv(d["cin"], d["cout"], 3, d["sdim"], upsample=up), d[f"P_up{int(up)}"], dev)
            close(m.conv(x, w), G[f"{name}_up{int(up)}_conv"])
            close(m(x, w, noise=d[f"noise_up{int(up)}"].to(dev)), G[f"{name}_up{int(up)}_styled"])
        m = _load_small(model.ToRGB(d["cout"], d["sdim"]), d["P_rgb"], dev)
        close(m(d["x_rgb"].to(dev), w, None), G[f"{name}_rgb_skip0"])
        close(m(d["x_rgb"].to(dev), w, d["skip"].to(dev)), G[f"{name}_rgb_skip1"])


def test_modconv_tile_geometries_vs_oracle():
    K.run_all("tile_geometries", *_native())


def _gpu_generator(tag, dev):
    import hairfastgan_amd.stylegan2.model as model

    size, cm, n_mlp, batches, ranges = C.GENERATOR_CASES[tag]
    g = model.Generator(size, 512, n_mlp, channel_multiplier=cm).eval()
    shapes = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    g.load_state_dict(C.generator_params(shapes))
    return g.to(dev), shapes, size, batches, ranges


def _run_range(g, shapes, size, B, s, e, dev):
    cin = shapes[f"convs.{2 * s - 2}.conv.weight"][2] if s > 0 else None
    lat, nz, layer_in = C.generator_inputs(size, B, s, cin)
    with torch.inference_mode():
        return g([lat.to(dev)], input_is_latent=True, noise=[n.to(dev) for n in nz],
                 layer_in=None if layer_in is None else layer_in.to(dev), start_layer=s, end_layer=e)


def _strided(y, n=1024):
    f = y.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n]


def _check_against_golden(G, key, y, sk):
    scale = max(1.0, abs(float(G[f"{key}_stats"][2])), abs(float(G[f"{key}_stats"][3])))
    st = G[f"{key}_stats"]
    yd = y.double()
    got = np.array([yd.mean().item(), yd.std().item(), yd.min().item(), yd.max().item()])
    assert np.allclose(got, st, rtol=0, atol=REL * scale), (got, st)
    close(_strided(y), G[f"{key}_samples"])
    if f"{key}_full" in G:
        close(y, G[f"{key}_full"])
    if f"{key}_crop" in G:
        c0 = y.shape[-1] // 2 - 32
        close(y[:, :, c0:c0 + 64, c0:c0 + 64], G[f"{key}_crop"])
    if f"{key}_edges" in G:  # four corners + the middle of each edge: tile-edge bugs away from the centre
        for nm, (sy, sx) in C.edge_crops(y.shape[-1]).items():
            close(y[:, :, sy, sx], G[f"{key}_edges_{nm}"])
    if f"{key}_chan16" in G:
        close(y[:, ::16], G[f"{key}_chan16"])
    if f"{key}_skip_samples" in G:
        close(_strided(sk), G[f"{key}_skip_samples"])
    else:
        assert sk is None


def test_generator64_all_ranges_vs_reference_golden(golden):
    dev = _dev()
    g, shapes, size, batches, ranges = _gpu_generator("g64", dev)
    G = golden("generator_64.npz")
    for B in batches:
        for (s, e) in ranges:
            y, sk = _run_range(g, shapes, size, B, s, e, dev)
            _check_against_golden(G, f"g64_B{B}_r{s}to{e}", y, sk)


def test_generator1024_all_ranges_vs_reference_golden(golden):
    """BASELINE.json configs[0]/[2] shapes: every layer range HairFast uses
    (0->8, 0->3, 3->3, 4->8, 5->8; Embedding.py:52,78,90, Alignment.py:63, Blending.py:62,68)."""
    dev = _dev()
    g, shapes, size, batches, ranges = _gpu_generator("g1024", dev)
    G = golden("generator_1024.npz")
    for B in batches:
        for (s, e) in ranges:
            y, sk = _run_range(g, shapes, size, B, s, e, dev)
            _check_against_golden(G, f"g1024_B{B}_r{s}to{e}", y, sk)


def test_generator1024_intermediates_localise(golden):
    """Per-layer checkpoints of the full forward (stats + 16 samples per module output)."""
    dev = _dev()
    g, shapes, size, batches, _ = _gpu_generator("g1024", dev)
    G = golden("generator_1024.npz")
    B = batches[0]
    got = {}
    hooks = []
    for nm, mod in g.named_modules():
        if nm in ("conv1", "to_rgb1") or (nm.count(".") == 1 and nm.split(".")[0] in ("convs", "to_rgbs")):
            hooks.append(mod.register_forward_hook(lambda _m, _i, o, nm=nm: got.__setitem__(nm, o)))
    _run_range(g, shapes, size, B, 0, 8, dev)
    for h in hooks:
        h.remove()
    assert len(got) == 2 + 16 + 8
    for nm, o in got.items():
        ref = G[f"g1024_B{B}_r0to8_inter_{nm}"]
        od = o.double()
        stats = np.array([od.mean().item(), od.std().item(), od.min().item(), od.max().item()])
        scale = max(1.0, abs(ref[2]), abs(ref[3]))
        assert np.allclose(stats, ref[:4], rtol=0, atol=REL * scale), (nm, stats, ref[:4])
        close(_strided(o, 16), ref[4:], REL)


def test_full_size_properties_batch8():
    """BASELINE.json configs[1] size (batch 8, 1024^2), no oracle needed:
    batch independence (sample i of a batch == the same sample alone, bit-exact since the
    kernels share weights across the batch), determinism, and linearity of ToRGB in its bias."""
    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g1024", dev)
    lat8, nz, _ = C.generator_inputs(size, 8, 0)
    nz = [n.to(dev) for n in nz]
    lat8 = lat8.to(dev)
    with torch.inference_mode():
        y8, _ = g([lat8], input_is_latent=True, noise=nz)
        y8b, _ = g([lat8], input_is_latent=True, noise=nz)
        assert torch.equal(y8, y8b)
        assert torch.isfinite(y8).all()
        for i in (0, 5):
            yi, _ = g([lat8[i:i + 1]], input_is_latent=True, noise=nz)
            # not bit-exact: the split-K plan of the small-plane layers depends on the batch size
            assert float((yi[0] - y8[i]).abs().max()) <= 1e-5 * max(1.0, float(y8[i].abs().max()))
        old = g.to_rgbs[7].bias.data.clone()
        g.to_rgbs[7].bias.data += 0.5
        y_shift, _ = g([lat8[:1]], input_is_latent=True, noise=nz)
        g.to_rgbs[7].bias.data.copy_(old)
        y_base, _ = g([lat8[:1]], input_is_latent=True, noise=nz)
        assert float((y_shift - y_base - 0.5).abs().max()) < 1e-5
    assert y8.shape == (8, 3, 1024, 1024)


def test_random_noise_path_statistics():
    """noise=None draws fresh N(0,1) maps (model.py:289-291): two calls differ, and the
    difference has the scale predicted by the noise weights."""
    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g64", dev)
    lat, _, _ = C.generator_inputs(size, 2, 0)
    with torch.inference_mode():
        torch.manual_seed(0)
        a, _ = g([lat.to(dev)], input_is_latent=True)
        b, _ = g([lat.to(dev)], input_is_latent=True)
        torch.manual_seed(0)
        a2, _ = g([lat.to(dev)], input_is_latent=True)
    assert not torch.equal(a, b)
    assert torch.equal(a, a2)


@pytest.mark.parametrize("case", K.params("pipelined", gpu=True))
def test_every_pipelined_instantiation_vs_oracle(case):
    K.check_pipelined(*_native(), case)


@pytest.mark.parametrize("case", K.params("f16_matrix_cores", gpu=True))
def test_modconv_f16_matrix_cores(case):
    K.check_f16_matrix_cores(*_native(), case)


@pytest.mark.parametrize("case", K.params("up_f16_matrix_cores", gpu=True))
def test_modconv_up_f16_matrix_cores(case):
    K.check_up_f16_matrix_cores(*_native(), case)


@pytest.mark.parametrize("case", K.params("persistent_tile_walk", gpu=True))
def test_modconv_f16_persistent_tile_walk(case):
    K.check_persistent_tile_walk(*_native(), case)


@pytest.mark.parametrize("case", K.params("fused_torgb", gpu=True))
def test_modconv_f16_fused_torgb(case):
    K.check_fused_torgb(*_native(), case)


def test_generator1024_fuses_torgb_of_the_top_layers(monkeypatch):
    """The 512^2 (64 ch) and 1024^2 (32 ch) ToRGBs ride in their producer's epilogue in the
    default mode - and only when the ToRGB is called with the style it was fused for."""
    from hairfastgan_amd import _marshal as M

    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g1024", dev)
    lat, nz, _ = C.generator_inputs(size, 2, 0)  # batch 2: the smallest batch whose 32^2 layers take the fp16-core kernels
    lat, nz = lat.to(dev), [n.to(dev) for n in nz]
    fused, plain_rgb, presplit = [], [], []
    real_conv, real_rgb, real_pre = M.modconv3x3_f16, M.torgb, M._modconv3x3_f16_pre  # (the fixed-triple form the generator calls)

    def conv(*a, **k):
        if k.get("rgb") is not None:
            fused.append(a[2].shape[2])
        return real_conv(*a, **k)

    def pre(*a, **k):
        presplit.append(a[2].shape[2])
        if k.get("rgb") is not None:
            fused.append(a[2].shape[2])
        return real_pre(*a, **k)

    monkeypatch.setattr(M, "_modconv3x3_f16_pre", pre)
    image, real_image = [], M.modconv3x3_f16_pre_image

    def pre_image(*a, **k):  # round 6: the last layer's epilogue finishes ToRGB (no raw product, no finishing launch)
        image.append(a[2].shape[2])
        return real_image(*a, **k)

    monkeypatch.setattr(M, "modconv3x3_f16_pre_image", pre_image)
    up_pre, real_up = [], M.modconv3x3_up

    def up(lib, st, x, *a, **k):
        if isinstance(x, M.SplitActivation):
            up_pre.append(x.shape[2])
        return real_up(lib, st, x, *a, **k)

    monkeypatch.setattr(M, "modconv3x3_up", up)
    up_fused, real_fused = [], M.modconv3x3_up_fused

    def fusedup(lib, st, x, *a, **k):
        assert isinstance(x, M.SplitActivation) and k.get("split_for") is not None  # pre-split in, split out
        up_fused.append(x.shape[2])
        return real_fused(lib, st, x, *a, **k)

    monkeypatch.setattr(M, "modconv3x3_up_fused", fusedup)

    def rgb(lib, st, x, *a):
        plain_rgb.append(x.shape[1])
        return real_rgb(lib, st, x, *a)

    monkeypatch.setattr(M, "modconv3x3_f16", conv)
    monkeypatch.setattr(M, "torgb", rgb)
    with torch.inference_mode():
        y, _ = g([lat], input_is_latent=True, noise=nz)
        assert fused == [64, 128, 256, 512] and image == [1024]  # ToRGB's 1x1 conv in the conv epilogue from 64^2 upward (partial sums per 64 channels); the 1024^2 layer writes the image
        assert presplit == [32, 64, 128, 256, 512]  # blur -> conv hand-over without an fp32 activation
        # conv epilogue -> next block's transposed conv, pre-split: two-pass up to 64^2 inputs, then the one-kernel
        # form (transposed conv + blur + noise + bias + lrelu, no (2h+1)^2 intermediate) from 128^2 inputs upward
        assert up_pre == [32, 64] and up_fused == [128, 256, 512]
        # finishing passes on the raw slabs (8, 4, 2, 1, 1 slabs of 3 channels); the layers below 64^2 run the stand-alone ToRGB
        assert plain_rgb == [512, 512, 512, 512, 24, 12, 6, 3], plain_rgb
        # ... and the two-launch form of the last layer (HAIRFAST_IMAGE_FUSE=0) gives the same image, bit for bit
        image.clear()
        with monkeypatch.context() as two_launch:
            two_launch.setattr(M, "IMAGE_FUSE", False)
            y2, _ = g([lat], input_is_latent=True, noise=nz)
        assert image == [] and torch.equal(y, y2)
        # batch 1 under batch-invariant plans (the default): the kernel families of the canonical batch-3 launch - the same chain
        fused.clear(); presplit.clear(); up_pre.clear(); up_fused.clear(); plain_rgb.clear()
        g([lat[:1]], input_is_latent=True, noise=nz)
        assert presplit == [32, 64, 128, 256, 512] and up_pre == [32, 64] and up_fused == [128, 256, 512], (presplit, up_pre)
        # ... and with plans from the whole launch (HAIRFAST_DETERMINISTIC=0): the 32^2 block of a batch-1 forward (1024 pixels per
        # launch: 32 blocks that would each walk the whole K loop) stays on the fp32 split-K kernels
        # (M.modconv3x3_f16_supported(batch=)), the hand-over chain starts at 64^2
        from hairfastgan_amd import _runtime
        prev_mode = _runtime.set_batch_invariant(False)
        try:
            fused.clear(); presplit.clear(); up_pre.clear(); up_fused.clear(); plain_rgb.clear()
            g([lat[:1]], input_is_latent=True, noise=nz)
            assert presplit == [64, 128, 256, 512] and up_pre == [64] and up_fused == [128, 256, 512], (presplit, up_pre)
        finally:
            _runtime.set_batch_invariant(prev_mode)
        # module API: forward_rgb's explicit (out, raw) pair finished by ToRGB.finish equals the stand-alone ToRGB
        x32 = torch.randn(1, 32, 1024, 1024, device=dev)
        l1 = lat[:1]
        out, raw = g.convs[15].forward_rgb(x32, l1[:, 16], nz[16], g.to_rgbs[7].coefficients(l1[:, 17]))
        a = g.to_rgbs[7].finish(raw, None)
        b = g.to_rgbs[7](out, l1[:, 17])
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))
        assert torch.equal(out, g.convs[15](x32, l1[:, 16], noise=nz[16])) and not hasattr(out, "_hf_fused_rgb")
    assert y.shape == (2, 3, 1024, 1024)


@pytest.mark.parametrize("mode,bar", [("f16", 1e-4), ("f32", 1e-8)])
def test_generator1024_other_precision_modes(golden, mode, bar):
    """BASELINE.json configs[4] (fp16 operands, fp32 accumulate / demodulation) and the exact-fp32
    mode against the reference's golden 1024^2 output: pixel MSE below north_star's 1e-4 bar for
    fp16, below the fp32 bar for f32 (the default f16x3 mode is what every other test runs in)."""
    from hairfastgan_amd import _runtime

    dev = _dev()
    g, shapes, size, batches, _ = _gpu_generator("g1024", dev)
    G = golden("generator_1024.npz")
    B = batches[0]
    prev = _runtime.set_conv_precision(mode)
    try:
        y, _ = _run_range(g, shapes, size, B, 0, 8, dev)
    finally:
        _runtime.set_conv_precision(prev)
    key = f"g1024_B{B}_r0to8"
    ref = torch.from_numpy(np.asarray(G[f"{key}_crop"])).double()
    c0 = y.shape[-1] // 2 - 32
    got = y[:, :, c0:c0 + 64, c0:c0 + 64].cpu().double()
    mse = float(((got - ref) ** 2).mean())
    assert mse < bar * max(1.0, float(ref.var())), (mode, mse)
    smp = torch.from_numpy(np.asarray(G[f"{key}_samples"])).double()
    mse_s = float(((_strided(y).cpu().double() - smp) ** 2).mean())
    assert mse_s < bar * max(1.0, float(smp.var())), (mode, mse_s)
    print(f"{mode}: crop mse {mse:.3e}, strided-sample mse {mse_s:.3e}")


@pytest.mark.parametrize("case", K.params("presplit_input", gpu=True))
def test_modconv_f16_presplit_pipeline(case):
    K.check_presplit_input(*_native(), case)


@pytest.mark.parametrize("case", K.params("presplit_chain", gpu=True))
def test_presplit_chain_same_res_to_transposed(case):
    K.check_presplit_chain(*_native(), case)


def test_generator1024_fast_paths_equal_the_module_by_module_path():
    """Generator's fused hand-overs (pre-split blur output, ToRGB in the conv epilogue) against the
    same forward with a forward hook registered (which makes every module run on plain tensors):
    the conv inputs are bit-identical by construction, so the images are too."""
    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g1024", dev)
    lat, nz, _ = C.generator_inputs(size, 2, 0)
    lat, nz = lat.to(dev), [n.to(dev) for n in nz]
    with torch.inference_mode():
        fast, _ = g([lat], input_is_latent=True, noise=nz)
        seen = []
        hooks = [m.register_forward_hook(lambda _m, _i, o: seen.append(type(o))) for m in g.convs]
        slow, _ = g([lat], input_is_latent=True, noise=nz)
        for h in hooks:
            h.remove()
    assert len(seen) == 16 and all(t is torch.Tensor for t in seen)
    # the conv inputs are bit-identical by construction (pre-split hand-over == in-kernel split); the images differ only
    # through the two top ToRGBs, which the hooked path runs stand-alone (a hook on the StyledConv must see the module
    # being called, so its epilogue cannot also produce the ToRGB product) instead of in the conv epilogue
    assert float((fast - slow).abs().max()) <= 2e-6 * max(1.0, float(slow.abs().max()))


# ------------------------------------------------------------------------------------------------
# Range of the fp16 (hi, lo) operand split (round-1 verdict / advisor: the default f16x3 mode must
# not depend on tame O(1) tensors)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.params("f16_split_range", gpu=True))
def test_f16_split_range(case):
    K.check_f16_split_range(*_native(), case)


def test_f16_split_saturates_and_counts():
    K.run_all("f16_split_saturates", *_native())


@pytest.mark.parametrize("scale", [1e3, 1e-3])
def test_generator1024_scaled_activations_f16x3_vs_f32(scale):
    """The whole 1024^2 generator with every additive term (constant input, noise weights, biases)
    scaled by 1e+-3 - activations 1e+-3 times their usual size in every layer - and styles scaled by
    the inverse: the default f16x3 mode stays within the fp32 tolerance of the exact-fp32 mode and
    nothing clamps."""
    from hairfastgan_amd import _marshal as M, _runtime
    from hairfastgan_amd._runtime import lib as _lib_fn

    dev = _dev()
    import hairfastgan_amd.stylegan2.model as model

    size, cm, n_mlp, _, _ = C.GENERATOR_CASES["g1024"]
    g = model.Generator(size, 512, n_mlp, channel_multiplier=cm).eval()
    shapes = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    P = C.generator_params(shapes)
    for k in P:
        if k == "input.input" or k.endswith(".noise.weight") or k.endswith(".activate.bias") or (k.startswith("to_rgb") and k.endswith(".bias") and "conv" not in k):
            P[k] = P[k] * scale
        if k.endswith("conv.modulation.weight") or k.endswith("conv.modulation.bias"):
            if not k.startswith("to_rgb"):
                P[k] = P[k] / scale  # demodulation makes the 3x3 layers invariant to the style's magnitude
    g.load_state_dict(P)
    g = g.to(dev)
    lat, nz, _ = C.generator_inputs(size, 1, 0)
    nz = [n.to(dev) for n in nz]
    M.f16_overflow_count(_lib_fn(), reset=True)
    with torch.inference_mode():
        y, _ = g([lat.to(dev)], input_is_latent=True, noise=nz)
        prev = _runtime.set_conv_precision("f32")
        try:
            ref, _ = g([lat.to(dev)], input_is_latent=True, noise=nz)
        finally:
            _runtime.set_conv_precision(prev)
    assert torch.isfinite(y).all()
    assert M.f16_overflow_count(_lib_fn()) == 0
    ref_scale = float(ref.abs().max())
    assert ref_scale > 0.05 * scale  # the image really is ~scale times the usual one
    err = float((y - ref).abs().max())
    # fp32 tolerance for ordinary and large activations; with activations of size 1e-3 the split's
    # absolute floor (2^-25 per operand, include/hairfast_hip.h) shows: + ~6e-8 / |activation| relative
    tol = REL + 6e-8 / min(1.0, scale)
    assert err <= tol * ref_scale, (err, ref_scale, tol)


# ------------------------------------------------------------------------------------------------
# BASELINE.json configs[4] at its own batch size (16), configs[1] rows against the goldens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,bar", [("f16", 16, 1e-4), ("f16x3", 8, 1e-8)])
def test_generator1024_full_batch_rows_vs_reference_golden(golden, mode, B, bar):
    """configs[4] (fp16 operands, batch 16) and configs[1] (batch 8) at their real batch sizes: the
    first two rows use the latents of the B=2 golden case, so they are checked against the reference's
    golden crop / samples; every row is finite and rows with equal latents are equal (batch
    independence: the kernels share weights across the batch)."""
    from hairfastgan_amd import _runtime

    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g1024", dev)
    G = golden("generator_1024.npz")
    lat2, nz, _ = C.generator_inputs(size, 2, 0)
    lat = lat2.repeat(B // 2, 1, 1).to(dev)  # rows 0,1 = golden rows; rows 2k, 2k+1 repeat them
    nz = [n.to(dev) for n in nz]
    prev = _runtime.set_conv_precision(mode)
    try:
        with torch.inference_mode():
            y, _ = g([lat], input_is_latent=True, noise=nz)
    finally:
        _runtime.set_conv_precision(prev)
    assert y.shape == (B, 3, 1024, 1024) and torch.isfinite(y).all()
    for k in range(2, B, 2):
        assert torch.equal(y[k:k + 2], y[0:2]), f"rows {k},{k + 1} differ from rows 0,1"
    key = "g1024_B2_r0to8"
    ref = torch.from_numpy(np.asarray(G[f"{key}_crop"])).double()
    c0 = y.shape[-1] // 2 - 32
    got = y[:2, :, c0:c0 + 64, c0:c0 + 64].cpu().double()
    mse = float(((got - ref) ** 2).mean())
    assert mse < bar * max(1.0, float(ref.var())), (mode, mse)
    smp = torch.from_numpy(np.asarray(G[f"{key}_samples"])).double()
    mse_s = float(((_strided(y[:2]).cpu().double() - smp) ** 2).mean())
    assert mse_s < bar * max(1.0, float(smp.var())), (mode, mse_s)
    if f"{key}_edges" in G:  # four corner crops + edge strips (tile-edge coverage away from the centre)
        for name, (sy, sx) in C.edge_crops(1024).items():
            close_fn = close if mode != "f16" else (lambda a, b: None)  # fp16 operands: judged by the MSE bar above
            close_fn(y[:2, :, sy, sx], G[f"{key}_edges_{name}"])
    print(f"{mode} B={B}: crop mse {mse:.3e}, strided-sample mse {mse_s:.3e}")


# ------------------------------------------------------------------------------------------------
# the z -> w mapping network (PixelNorm + n_mlp x EqualLinear/fused_lrelu)
# ------------------------------------------------------------------------------------------------
def test_mapping_network_vs_reference_golden(golden):
    """Generator.style (model.py:16-21, 384-393) and a forward entered through z
    (input_is_latent=False), on the HIP library: hf_linear_f32 + hf_fused_bias_act_f32."""
    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g64", dev)
    G = golden("generator_64.npz")
    z = C.mapping_inputs(3).to(dev)
    with torch.inference_mode():
        w = g.get_latent(z)
        close(w, G["g64_mapping_w"], 1e-5)
        assert g.mean_latent(16).shape == (1, 512)
        _, nz, _ = C.generator_inputs(size, 3, 0)
        y, _ = g([z], input_is_latent=False, noise=[n.to(dev) for n in nz])
    close(y, G["g64_from_z_full"])
    g1024, _, _, _, _ = _gpu_generator("g1024", dev)
    with torch.inference_mode():
        close(g1024.style(z), golden("generator_1024.npz")["g1024_mapping_w"], 1e-5)


def test_ops_refuse_autograd():
    """Forward-only kernels: an input that requires grad raises instead of returning a silently
    detached result (the reference's ops are differentiable)."""
    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g64", dev)
    lat, nz, _ = C.generator_inputs(size, 1, 0)
    lat = lat.to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        g([lat], input_is_latent=True, noise=[n.to(dev) for n in nz])
    with torch.no_grad():
        g([lat], input_is_latent=True, noise=[n.to(dev) for n in nz])


# ------------------------------------------------------------------------------------------------
# The upsampling StyledConv as ONE kernel (transposed conv + blur + noise + bias + lrelu; no (2h+1)^2 intermediate)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.params("up_fused_blur", gpu=True))
def test_modconv_up_fused_blur(case):
    K.check_up_fused_blur(*_native(), case)


def test_modconv_up_fused_blur_plain_fp16_operands():
    K.run_all("up_fused_blur_plain_fp16", *_native())


@pytest.mark.parametrize("case", K.params("up_fused_blur_persistent", gpu=True))
def test_modconv_up_fused_blur_persistent_walk(case):
    K.check_up_fused_blur_persistent(*_native(), case)


def test_auto_precision_reruns_clamped_forward_in_f32():
    """HAIRFAST_CONV_PRECISION=auto (the real-checkpoint safety net): a forward whose activations leave the fp16-pair
    range (|s*x| > 131008: the split saturates and counts) is repeated on the exact fp32 kernels - the result equals the
    f32 mode's bit for bit; a forward that stays in range is not repeated and equals the f16x3 mode's."""
    from hairfastgan_amd import _runtime
    from hairfastgan_amd.stylegan2.model import Generator

    dev = _dev()
    g = Generator(64, 512, 2).eval()
    shapes = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    g.load_state_dict(C.generator_params(shapes))
    g = g.to(dev)
    lat, nz, _ = C.generator_inputs(64, 2, 0)
    lat, nz = lat.to(dev), [n.to(dev) for n in nz]

    def run(mode):
        prev = _runtime.set_conv_precision(mode)
        try:
            with torch.inference_mode():
                return g([lat], input_is_latent=True, noise=nz)[0]
        finally:
            _runtime.set_conv_precision(prev)

    n0 = _runtime.auto_reruns
    assert torch.equal(run("auto"), run("f16x3")) and _runtime.auto_reruns == n0          # in range: one pass
    with torch.no_grad():
        g.input.input.mul_(1e7)                                                            # learned constant far out of range
    y32, y16, ya = run("f32"), run("f16x3"), run("auto")
    assert _runtime.auto_reruns == n0 + 1
    assert torch.equal(ya, y32)
    assert not torch.equal(y16, y32)
    assert _runtime.configured_conv_precision() != "auto" and _runtime.conv_precision() in ("f16x3", "f32", "f16")


@pytest.mark.parametrize("case", K.params("conv_rows", gpu=True))
def test_conv_rows_pipeline_equals_tiled_kernel_on_hardware(case):
    K.check_conv_rows(*_native(), case)


def test_generator1024_block_order_does_not_change_the_image():
    """The cout-tiles-fastest block order of the generator's fp16-core kernels (ConvParams::swap_xy; by default only from 128 MB of
    layer input, i.e. in a batched swap's batch-64 calls) forced on a batch-8 forward through hf_debug_set_tuning bit 3: the
    image - every layer form: same-resolution, fused upsampling, two-pass upsampling, fused ToRGB slabs - is bit-identical."""
    from hairfastgan_amd._runtime import lib

    dev = _dev()
    g, shapes, size, _, _ = _gpu_generator("g1024", dev)
    lat2, nz, _ = C.generator_inputs(size, 2, 0)
    lat = torch.cat([lat2, lat2.flip(0), lat2 * 0.5, lat2 * 0.25]).to(dev)
    nz = [n.to(dev) for n in nz]
    L = lib()
    try:
        with torch.inference_mode():
            ref, _ = g([lat], input_is_latent=True, noise=nz)
            L.hf_debug_set_tuning(8)
            y, _ = g([lat], input_is_latent=True, noise=nz)
    finally:
        L.hf_debug_set_tuning(0)
    assert torch.isfinite(ref).all() and torch.equal(y, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B,h", [(8, 4), (8, 8), (8, 16), (3, 16), (1, 8)])
def test_small_plane_upsampling_in_two_launches_equals_three(B, h, monkeypatch):
    """hf_modconv3x3_small_up_blur_f16_f32 on the hardware: the generator's 4^2 / 8^2 / 16^2 upsampling StyledConvs (512 -> 512) as
    tap GEMM + one combine / blur / tail kernel against tap GEMM + small_combine + blur pass, fp32 and split outputs: equal bits."""
    from hairfastgan_amd import _marshal as M
    from hairfastgan_amd._runtime import lib, stream

    dev = _dev()
    L, st = lib(), stream()
    lay = K.styled_layer(L, st, dev, (B, 512, 512, h, h), h, True)
    x, wt, s, d, k4, nz, nw, bias = lay.x, lay.wt, lay.s, lay.dm, lay.k4, lay.nz, lay.nw, lay.bias
    s2 = (torch.rand(B, 512) + 0.5).to(dev)
    w9 = M.split_weights_small(L, st, wt)
    for split_for in (None, (None, s2, True)):
        res = {}
        for fused in (False, True):
            monkeypatch.setattr(M, "SMALL_UP_FUSED", fused)
            res[fused] = M.modconv3x3_up(L, st, x, wt, s, d, k4, nz, nw, bias, split_for=split_for, small=(w9, 3))
        if split_for is None:
            assert torch.equal(res[False], res[True])
        else:
            assert torch.equal(res[False].hi, res[True].hi) and torch.equal(res[False].lo, res[True].lo)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 3])
def test_small_plane_tap_gemm_pixel_tile_forms_agree(B):
    """The 16^2 layers' tap GEMM (512 -> 512) in its 128-pixel tile form (taken when the last round of the 256-pixel form would
    be under half full: batch 8 = 576 blocks on 512 slots) against the 256-pixel form (hf_debug_set_tuning bit 1): equal bits,
    same resolution and transposed; and against the fp32 kernel."""
    from hairfastgan_amd import _marshal as M
    from hairfastgan_amd._runtime import lib, stream

    dev = _dev()
    L, st = lib(), stream()
    c, h = 512, 16
    lay = K.styled_layer(L, st, dev, (B, c, c, h, h), B, False)
    x, wt, s, d, nz, nw, bias = lay.x, lay.wt, lay.s, lay.dm, lay.nz, lay.nw, lay.bias
    w9 = M.split_weights_small(L, st, wt)
    same, up = {}, {}
    try:
        for never in (0, 2):
            L.hf_debug_set_tuning(never)
            same[never] = M.modconv3x3_small(L, st, x, w9, 3, s, d, nz, nw, bias, c)
            up[never] = M.modconv3x3_small(L, st, x, w9, 3, s, d, None, None, None, c, upsample=True)
    finally:
        L.hf_debug_set_tuning(0)
    assert torch.equal(same[0], same[2]) and torch.equal(up[0][..., :2 * h + 1], up[2][..., :2 * h + 1])
    ref = M.modconv3x3(L, st, x, wt, s, d, nz, nw, bias)
    assert float((same[0] - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
