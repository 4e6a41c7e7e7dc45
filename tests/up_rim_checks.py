"""The checks of the two-pass upsampling conv's edge kernel (csrc/convh.hip, conv_up_rim_h), shared by the hipsim tests
(tests/test_sim_up_rim.py) and the GPU tests (tests/test_gpu_up_rim.py).

With pre-split input hf_modconv3x3_up_f16_pre_f32 launches conv_mfma_h over the interior h x w of the (h+1) x (w+1) phase
domain and conv_up_rim_h over the row Y = h and the column X = w; hf_debug_set_tuning bit 5 keeps the edge as rim tile
families of the main launch (the form before the edge kernel existed).  The edge kernel issues the three taps that read the
image, in the main kernel's order, and leaves out the six that multiply zero padding: the two forms must agree in every bit
of the whole output."""
import torch

from hairfastgan_amd import _marshal as M
from tests.conv_kernel_checks import oracle, presplit, styled_layer

RIM_FAMILIES = 32  # hf_debug_set_tuning bit 5

# (B, cin, cout, h, w)
CASES = [
    (2, 32, 64, 16, 16),   # form 61; row of 17 and column of 16 positions, both shorter than one 32-position tile
    (1, 48, 128, 20, 70),  # no multiple of anything: 71 row positions = three tiles, the last ragged; two cout tiles; 3 chunks
    (3, 64, 32, 16, 32),   # form 63 (cout % 64 != 0); three images: the image stride of both tensors
    (2, 512, 64, 16, 16),  # 32 chunks, the hot path's K depth, at the smallest plane that takes the route
    (1, 32, 64, 40, 16),   # a column of 40 positions: a second column tile (as on the 64^2 -> 128^2 layer), ragged
]


def check_case(lib, st, dev, shape, nterms, with_split=True):
    B, cin, cout, H, W = shape
    L = styled_layer(lib, st, dev, shape, 11, True)
    s_next = (torch.rand(B, cout) + 1.0).to(dev)
    wt, dm, hi, lo, k4, nz, nw, bias = L.wt, L.dm, L.hi, L.lo, L.k4, L.nz, L.nw, L.bias
    assert M.modconv3x3_up_f16_supported(cin, cout, H, W)
    act = presplit(L)
    want_path = 583 if cout % 64 else 581
    res = {}
    try:
        for bits in (0, RIM_FAMILIES):
            lib.hf_debug_set_tuning(bits)
            y = M.modconv3x3_up(lib, st, act, wt, None, dm, k4, nz, nw, bias, f16=(hi, lo, nterms))
            assert lib.hf_debug_last_path() == want_path
            sp = None
            if with_split:
                sp = M.modconv3x3_up(lib, st, act, wt, None, dm, k4, nz, nw, bias, f16=(hi, lo, nterms),
                                     split_for=(None, s_next, nterms == 3))
            if dev.type == "cuda":
                torch.cuda.synchronize()
            res[bits] = (y, sp)
    finally:
        lib.hf_debug_set_tuning(0)
    y, sp = res[0]
    y_old, sp_old = res[RIM_FAMILIES]
    assert y.shape == (B, cout, 2 * H, 2 * W)
    assert torch.equal(y, y_old)  # every element
    if with_split:
        assert torch.equal(sp.hi, sp_old.hi)
        if nterms == 3:
            assert torch.equal(sp.lo, sp_old.lo)
    if cin <= 64:
        full = oracle(L)
        scale = max(1.0, float(full.abs().max()))
        err = float((y.cpu() - full).abs().max())
        print(f"up_rim {shape} nterms {nterms}: max-abs vs oracle {err:.3e} (bound {(1e-5 if nterms == 3 else 4e-3) * scale:.3e})")
        assert err < (1e-5 if nterms == 3 else 4e-3) * scale
