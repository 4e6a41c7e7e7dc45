"""TEST INFRASTRUCTURE - checks of the FID Inception-v3 path (csrc/conv_rect.h, csrc/inception.h, hairfastgan_amd.inception,
the --fid column of hairfastgan_amd.metrics), shared by the hipsim tests (tests/test_sim_inception.py) and the GPU tests
(tests/test_gpu_inception.py).  Every check takes (lib, st, dev, ...); the rules of tests/small_ops_checks.py and
tests/gemm_checks.py (accuracy, exact, sentinels) are imported, not copied.  The yardstick is tests/inception_ref.py, never
the device code.

Rect conv, accuracy rule per element (gemm_checks' rule with the taps inside the sums): with
    A = |out_scale| * conv(|x|, |W|),   S = |out_scale| * sum_{ci,ky,kx} |W|,
    |y - ref64| <= c * A + 2^-25 * S + FACTOR * E_t + 4 * 2^-23 * max |ref64|,
c = 3 * 2^-22 (f16x3), 2 * 2^-11 (f16), 0 (the exact-fp32 form); E_t: ATen fp32 on the CPU against ref64.  ReLU is 1-Lipschitz.

Network thresholds.  E32[kind][tap]: the largest error of torch fp32 ON THE CPU against fp64 for the same case, as
tests/inception_ref.py computes both - the MEASURED figures (8 threads, oneDNN), rounded up in the third digit.
threshold(tap) = max(8 * E32, 3 * 2^-24 * max |truth|): at the 2048 tap 5.5e-6 (tiny) and 2.2e-5 (full).  Another CPU's summation
order may move the fp32 error a little; that headroom (1.5 x) stands only in check_fp32_yardstick's own assertion, never in a
device threshold.  Measured on the device: see the README row.
"""
import csv
import functools
import os

import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import _runtime
from hairfastgan_amd import metrics as MT
from hairfastgan_amd.inception import InceptionV3
from tests import frechet_ref as FR
from tests import inception_ref as R
from tests.frechet_checks import dist_threshold, write_images
from tests.gemm_checks import C_F16, C_F16X3, LO_FLOOR
from tests.metric_common import inject, raises
from tests.small_ops_checks import SENTINEL, _guard_ok, _guarded, _sync, accuracy, exact

E32 = {"tiny": {64: 1.22e-7, 192: 6.63e-7, 768: 7.29e-7, 2048: 6.85e-7},
       "full": {64: 1.84e-7, 192: 2.73e-7, 768: 9.36e-7, 2048: 2.76e-6}}
YARDSTICK_HEADROOM = 1.5  # of check_fp32_yardstick alone
KINDS = {"tiny": dict(channel_div=8, size=75, resize=False), "full": dict(channel_div=1, size=64, resize=True)}
MODES = ("f16x3", "f16", "f32")       # the kernel's operand modes
NET_MODES = MODES + ("auto",)         # every _runtime.CONV_PRECISIONS mode; the network runs "f16" and "auto" with f16x3 operands
NTERMS = {"f16x3": 3, "f16": 1, "f32": 0}
HF_E_INVALID = -1

# ---- the rect conv kernel ------------------------------------------------------------------------------------------------
# label -> (B, cin, cout, H, W, (kh, kw), stride, (ph, pw)): one case per tap shape of the network; planes 9 x 7 (189 flat
# pixels at batch 3: two 128-pixel tiles, the first crosses two image boundaries) and 17 x 17 (867: seven tiles), the 3 x 3 ->
# 1 x 1 stride-2 plane (3 pixels), cin 3 / 16 / 48 / 80 (below one 32-channel stage, half a stage, two and three stages with a
# ragged last one), cout 32 / 80 / 96 / 192 (half a 64-channel tile, ragged second tile, three tiles)
RECT_CASES = {
    "1x1": (3, 80, 192, 9, 7, (1, 1), 1, (0, 0)),
    "3x3_p0": (3, 16, 32, 9, 7, (3, 3), 1, (0, 0)),
    "3x3_p0_s2": (3, 48, 96, 17, 17, (3, 3), 2, (0, 0)),
    "3x3_p0_s2_to_1x1": (3, 3, 80, 3, 3, (3, 3), 2, (0, 0)),
    "3x3_p1": (3, 3, 80, 9, 7, (3, 3), 1, (1, 1)),
    "5x5_p2": (3, 48, 32, 9, 7, (5, 5), 1, (2, 2)),
    "1x7": (3, 16, 192, 17, 17, (1, 7), 1, (0, 3)),
    "7x1": (3, 80, 96, 9, 7, (7, 1), 1, (3, 0)),
    "1x3": (3, 48, 80, 9, 7, (1, 3), 1, (0, 1)),
    "3x1": (3, 16, 32, 17, 17, (3, 1), 1, (1, 0)),
}
XC0, XPAD, OC0, OPAD = 3, 5, 5, 7  # the slices start at odd channels of tensors that hold XPAD / OPAD channels more


@functools.lru_cache(maxsize=None)
def rect_operands(label):
    """Seeded CPU operands, what is summed carries a DC offset (x = randn + 3, w = (randn + 0.5) / sqrt(K)); the weights differ
    in every tap, so a 1x7 / 7x1 transpose, a flipped tap or a shifted pad moves every output.  -> x, w, osc, bias, ref64, t32, A, S"""
    b, cin, cout, h, w_, (kh, kw), stride, pad = RECT_CASES[label]
    g = torch.Generator().manual_seed(9000 + sorted(RECT_CASES).index(label))
    x = torch.randn(b, cin, h, w_, generator=g) + 3.0
    w = (torch.randn(cout, cin, kh, kw, generator=g) + 0.5) / (cin * kh * kw) ** 0.5
    osc, bias = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)

    def run(dt):
        v = F.conv2d(x.to(dt), w.to(dt), None, stride, pad)
        return F.relu(v * osc.to(dt).view(1, -1, 1, 1) + bias.to(dt).view(1, -1, 1, 1))

    a = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad) * osc.double().view(1, -1, 1, 1)
    s = (w.double().abs().sum((1, 2, 3)) * osc.double()).view(1, -1, 1, 1).expand_as(a)
    return x, w, osc, bias, run(torch.float64), run(torch.float32), a, s


def _rect_launch(lib, st, dev, label, nterms, images=None):
    """-> the output slice [B,cout,oh,ow] of a launch into a sentinel-filled, guarded tensor; the input's other channels are NaN."""
    b, cin, cout, h, w_, (kh, kw), stride, pad = RECT_CASES[label]
    x, w, osc, bias = rect_operands(label)[:4]
    if images is not None:
        x = x[images]
        b = x.shape[0]
    xt = torch.full((b, cin + XPAD, h, w_), float("nan"))
    xt[:, XC0:XC0 + cin] = x
    oh, ow = M.conv_out_size(h, kh, stride, pad[0]), M.conv_out_size(w_, kw, stride, pad[1])
    n = b * (cout + OPAD) * oh * ow
    buf = _guarded(n, dev)
    out = buf[:n].view(b, cout + OPAD, oh, ow)
    wts = M.RectWeights(w.to(dev))
    M.conv2d_rect_into(lib, st, out, OC0, xt.to(dev), XC0, wts, nterms, stride, pad, osc.to(dev), bias.to(dev), relu=True)
    _guard_ok("conv2d_rect", label, buf, n, 0)
    host = out.cpu()
    assert bool((host[:, :OC0] == SENTINEL).all()) and bool((host[:, OC0 + cout:] == SENTINEL).all()), (label, "write outside the slice")
    return out[:, OC0:OC0 + cout]


def check_rect(lib, st, dev, label, mode):
    nterms = NTERMS[mode]
    _, _, _, _, ref64, t32, a, s = rect_operands(label)
    got = _rect_launch(lib, st, dev, label, nterms)
    c = {3: C_F16X3, 1: C_F16, 0: 0.0}[nterms]
    accuracy("conv2d_rect", f"{label} {mode}", got, ref64, t32, extra=(c * a + LO_FLOOR * s) if nterms else 0.0, tag="inception")
    for i in range(ref64.shape[0]):  # a row's bits are those of its single-image call
        exact("conv2d_rect", f"{label} {mode} image {i}", _rect_launch(lib, st, dev, label, nterms, images=[i])[0], got[i])


def check_rect_refusals(lib, st, dev):
    x = torch.zeros(1, 8, 5, 5, device=dev)
    out = torch.zeros(1, 8, 5, 5, device=dev)
    w = torch.zeros(4, 4, 3, 3, device=dev)
    hi, lo = M.RectWeights(w).f16(lib, st)

    def rc(nterms=0, act=0, cin=4, cout=4, kh=3, kw=3, stride=1, pt=1, pl=1, oh=5, ow=5, xc0=0, xct=8, oc0=0, oct=8, weight=w, whi=hi, wlo=lo):
        return lib.hf_conv2d_rect_f16_f32(out.data_ptr(), x.data_ptr(), None if weight is None else weight.data_ptr(),
                                          None if whi is None else whi.data_ptr(), None if wlo is None else wlo.data_ptr(), nterms, None,
                                          None, act, 1, cin, cout, 5, 5, kh, kw, stride, pt, pl, oh, ow, xc0, xct, oc0, oct, st)

    assert rc() == 0 and rc(nterms=3) == 0 and rc(nterms=1, wlo=None) == 0
    for bad in (dict(nterms=2), dict(act=2), dict(kh=8), dict(kw=0), dict(stride=3), dict(pt=3), dict(pl=-1), dict(xc0=5), dict(oc0=5),
                dict(xc0=-1), dict(oh=0), dict(oh=7), dict(ow=7), dict(weight=None), dict(nterms=3, whi=None), dict(nterms=3, wlo=None),
                dict(cin=0), dict(cout=0)):
        assert rc(**bad) == HF_E_INVALID, bad
    _sync(dev)


# ---- pool and resize ---------------------------------------------------------------------------------------------------
POOL_CASES = [(mode, stride, plane) for mode in ("max", "avg") for stride in (1, 2) for plane in ((7, 5), (3, 3))]


def check_pool(lib, st, dev, mode, stride, plane):
    """Small-integer data: the sums are exact in fp32 and one correctly rounded division remains, so the result equals the
    fp64 restatement rounded to fp32, bit for bit (the maximum is exact anyway)."""
    h, w = plane
    g = torch.Generator().manual_seed(300 + 10 * h + stride)
    x = torch.randint(-40, 41, (2, 3, h, w), generator=g).float()
    xt = torch.full((2, 3 + XPAD, h, w), float("nan"))
    xt[:, XC0:XC0 + 3] = x
    want = R.pool3x3(x.double(), mode, stride).float()
    n = 2 * (3 + OPAD) * want.shape[2] * want.shape[3]
    buf = _guarded(n, dev)
    out = buf[:n].view(2, 3 + OPAD, want.shape[2], want.shape[3])
    M.pool3x3_into(lib, st, out, OC0, xt.to(dev), XC0, 3, mode, stride)
    _guard_ok("pool3x3", f"{mode} s{stride} {plane}", buf, n, 0)
    host = out.cpu()
    assert bool((host[:, :OC0] == SENTINEL).all()) and bool((host[:, OC0 + 3:] == SENTINEL).all())
    exact("pool3x3", f"{mode} s{stride} {plane}", out[:, OC0:OC0 + 3], want)
    if mode == "avg" and stride == 1:  # the look-alike that counts padding differs on the rim
        assert not torch.equal(R.pool3x3(x.double(), "avg", 1, count_include_pad=True).float(), want)


def check_pool_refusals(lib, st, dev):
    x = torch.zeros(1, 4, 2, 5, device=dev)

    def rc(mode=0, stride=1, c=4, xc0=0, oc0=0):
        return lib.hf_pool3x3_f32(x.data_ptr(), x.data_ptr(), mode, 1, c, 2, 5, stride, xc0, 4, oc0, 4, st)

    for bad in (dict(mode=2), dict(stride=3), dict(stride=2), dict(c=0), dict(xc0=1), dict(oc0=1)):  # stride 2 needs 3 rows
        assert rc(**bad) == HF_E_INVALID, bad


# The bound of the general resize cases.  The source coordinates are fp32 by definition and the restatement uses the same
# ones, so what remains are the roundings of the lerps.  Every rounded value (a difference of two bytes, its product with
# t in [0,1), a lerp result) is below 256 in magnitude: each rounding errs by at most half an ulp there, u = 2^-17.
# top = a + (b - a) * tx takes three roundings, bot three as well, and v = top + (bot - top) * ty = (1 - ty) top + ty bot
# carries at most max(err top, err bot) = 3 u of them plus three roundings of its own: 6 u.  With fp32 inputs the pixel values
# are arbitrary fp32 numbers in [0, 255] and the same count holds.
RESIZE_BOUND = 6 * 2.0 ** -17
RESIZE_CASES = {"identity_299": (299, 299, "u8"), "half_598": (598, 598, "u8"), "up_64": (64, 64, "u8"), "up_64_f32": (64, 64, "f32"),
                "up_75x53": (75, 53, "u8"), "down_400x350": (400, 350, "f32")}


def check_resize(lib, st, dev, label):
    h, w, kind = RESIZE_CASES[label]
    g = torch.Generator().manual_seed(400 + h + w)
    x = torch.randint(0, 256, (2, 3, h, w), generator=g).to(torch.uint8)
    if kind == "f32":
        x = x.float() * torch.rand(2, 3, h, w, generator=g)
    got = M.resize_bilinear_tf1(lib, st, x.to(dev), 299, 299)
    _sync(dev)
    assert got.shape == (2, 3, 299, 299) and got.dtype == torch.float32
    if label == "identity_299":
        exact("resize", label, got, x.float())
        scaled = M.resize_bilinear_tf1(lib, st, x.to(dev), 299, 299, mul=1.0 / 128, add=-1.0)
        exact("resize", label + " affine", scaled, (x.float() - 128) / 128)
        return
    if label == "half_598":
        exact("resize", label, got, x.float()[:, :, ::2, ::2])  # every t is 0
        return
    truth = R.resize_tf1(x.double(), 299, 299)
    err = float((got.cpu().double() - truth).abs().max())
    miss = float((R.resize_tf1(x.double(), 299, 299, half_pixel=True) - truth).abs().max())
    print(f"inception resize {label}: E_k {err:.2e} bound {RESIZE_BOUND:.2e}; the half-pixel variant differs by {miss:.2e}")
    assert err <= RESIZE_BOUND, (label, err)
    assert miss > RESIZE_BOUND, (label, miss)  # the look-alike misses the bound on the same input


def check_resize_refusals(lib, st, dev):
    x = torch.zeros(1, 1, 4, 4, device=dev)
    out = torch.zeros(1, 1, 8, 8, device=dev)
    assert lib.hf_resize_bilinear_tf1_f32(out.data_ptr(), x.data_ptr(), 0, 1, 1, 4, 4, 8, 8, 0, 1.0, 0.0, st) == 0
    assert lib.hf_resize_bilinear_tf1_f32(out.data_ptr(), x.data_ptr(), 0, 1, 1, 4, 4, 0, 8, 0, 1.0, 0.0, st) == HF_E_INVALID
    assert lib.hf_resize_bilinear_tf1_f32(None, x.data_ptr(), 0, 1, 1, 4, 4, 8, 8, 0, 1.0, 0.0, st) == HF_E_INVALID
    assert lib.hf_resize_bilinear_tf1_f32(out.data_ptr(), x.data_ptr(), 0, 0, 1, 4, 4, 8, 8, 0, 1.0, 0.0, st) == HF_E_INVALID
    _sync(dev)


# ---- the network -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(kind, dtype=torch.float64, **variant):
    k = KINDS[kind]
    return R.forward(R.discriminating_state(k["channel_div"]), R.byte_images(k["size"]), dtype, k["channel_div"], k["resize"], **variant)


def threshold(kind, tap):
    return max(8 * E32[kind][tap], 3 * 2.0 ** -24 * float(truth(kind)[tap].abs().max()))


def check_conditions(kind):
    """On the CPU: the inputs tell the cases apart by far more than the threshold.  At 75^2 (tiny) Mixed_7c's plane is a single
    pixel, where the maximum and the average that does not count padding coincide, and there is no resize: those two variants
    are conditions of `full` only."""
    t = truth(kind)
    for tap in R.TAPS:
        thr = threshold(kind, tap)
        assert float((t[tap][0] - t[tap][1]).abs().max()) >= 100 * thr, (kind, tap, "near-duplicate pair")
        assert float((t[tap] == 0).double().mean()) <= 0.75, (kind, tap, "dead features")
    variants = [("count_include_pad", (768, 2048))] + ([("avg_in_7c", (2048,)), ("half_pixel", R.TAPS)] if kind == "full" else [])
    for name, taps in variants:
        v = truth(kind, **{name: True})
        for tap in taps:
            assert float((v[tap] - t[tap]).abs().max()) >= 100 * threshold(kind, tap), (kind, name, tap)


def check_fp32_yardstick(kind):
    t, t32 = truth(kind), truth(kind, torch.float32)
    for tap in R.TAPS:
        e = float((t32[tap].double() - t[tap]).abs().max())
        print(f"inception {kind} tap {tap}: torch fp32 on the CPU against fp64 {e:.3e} (recorded {E32[kind][tap]:.1e})")
        assert e <= YARDSTICK_HEADROOM * E32[kind][tap], (kind, tap, e)


def model(kind, dev, L, feature=2048):
    k = KINDS[kind]
    net = InceptionV3(feature, weights=R.discriminating_state(k["channel_div"]), resize_input=k["resize"], channel_div=k["channel_div"],
                      lib=inject(L, dev))
    return net.to(dev)


def check_network(lib, st, dev, kind, mode, every_row=True):
    images = R.byte_images(KINDS[kind]["size"]).to(dev)
    with _runtime.conv_precision_scope(mode):
        net = model(kind, dev, lib)
        got = net.taps(images)
        again = net.taps(images)
        rows = [net.taps(images[i:i + 1]) for i in (range(images.shape[0]) if every_row else (1,))]
        called = net(images)
    _sync(dev)
    t = truth(kind)
    for tap in R.TAPS:
        err = float((got[tap].cpu().double() - t[tap]).abs().max())
        thr = threshold(kind, tap)
        print(f"inception {kind} {mode} tap {tap}: E_k {err:.3e} threshold {thr:.3e} ({err / E32[kind][tap]:.2f} x the recorded fp32 CPU error)")
        assert got[tap].shape == t[tap].shape and got[tap].dtype == torch.float32
        assert err <= thr, (kind, mode, tap, err, thr)
        exact("inception", f"{kind} {mode} tap {tap} twice", again[tap], got[tap])
        for i, r in zip(range(images.shape[0]) if every_row else (1,), rows):
            exact("inception", f"{kind} {mode} tap {tap} row {i}", r[tap][0], got[tap][i])
    assert torch.equal(called, got[2048])


# ---- the front end -----------------------------------------------------------------------------------------------------
def check_state_dict():
    """The module tree carries the reference class's keys (94 layers x 5 tensors) and shapes; the published file's `fc.*` and
    batch counters are tolerated, anything else is not."""
    net = InceptionV3(2048, channel_div=8)
    keys = R.key_list()
    assert len(keys) == 470 and list(net.state_dict().keys()) == keys
    for name, cin, cout, (kh, kw), stride, pad in R.layer_table(8):
        m = net.get_submodule(name)
        assert tuple(m.conv.weight.shape) == (cout, cin, kh, kw) and m.conv.stride == (stride, stride) and tuple(m.conv.padding) == pad, name
        assert m.bn.eps == 0.001 and m.conv.bias is None
    assert [tuple(v.shape) for v in InceptionV3(2048).state_dict().values()][:2] == [(32, 3, 3, 3), (32,)]
    sd = R.discriminating_state(8)
    published = dict(sd)
    published["fc.weight"], published["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    published["Mixed_7c.branch_pool.bn.num_batches_tracked"] = torch.tensor(0)
    net.load_state_dict(published)
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    missing = dict(sd)
    del missing["Mixed_6e.branch7x7dbl_5.bn.running_var"]
    raises(RuntimeError, lambda: net.load_state_dict(missing), "Mixed_6e.branch7x7dbl_5.bn.running_var")
    raises(RuntimeError, lambda: net.load_state_dict(dict(sd, **{"AuxLogits.conv0.conv.weight": torch.zeros(1)})), "AuxLogits")
    assert "Mixed_5b.branch1x1.conv.weight" not in InceptionV3(192, channel_div=8).state_dict()


def check_refusals(lib, st, dev):
    for bad in (0, 100, 1008, 2047, "2048", True, 64.0):
        raises(ValueError, lambda: InceptionV3(bad, channel_div=8))
    raises(ValueError, lambda: InceptionV3(64, channel_div=0))
    for width in R.TAPS:
        raises(NotImplementedError, lambda: MT.FrechetDistance(width), "Inception")
    raises(NotImplementedError, lambda: MT.FrechetDistance(2048), "InceptionV3(2048")
    net = model("tiny", dev, lib, feature=64)
    raises(ValueError, lambda: net(torch.zeros(2, 1, 75, 75, dtype=torch.uint8, device=dev)))
    raises(ValueError, lambda: net(torch.zeros(3, 75, 75, dtype=torch.uint8, device=dev)))
    raises(ValueError, lambda: net(torch.zeros(1, 3, 74, 80, dtype=torch.uint8, device=dev)))
    raises(TypeError, lambda: net(torch.zeros(1, 3, 75, 75, dtype=torch.int32, device=dev)))
    # [0,1] floats become trunc(255 x) as a byte
    images = R.byte_images(75)[:2]
    floats = (images.float() + 0.25) / 255
    assert torch.equal(net(floats.to(dev)), net(images.to(dev)))


def check_frechet(lib, st, dev, feature):
    """FrechetDistance(InceptionV3(feature)) on seeded images against tests/frechet_ref.py fed with the fp64 features of the
    restatement.  Bound: the distance's own sensitivity to fp32 features - 8 x the change of the reference distance when it is
    fed torch's fp32 CPU features instead - plus the Frechet kernels' threshold for a full-rank problem of that dimension."""
    k = KINDS["tiny"]
    d = R.cdiv(feature, k["channel_div"])
    n = 2 * d + 4  # more samples than dimensions: full-rank covariances
    sd = R.discriminating_state(k["channel_div"])
    real, fake = R.byte_images(75, n, 1), R.byte_images(75, n, 2)
    net = model("tiny", dev, lib, feature)
    fid = MT.FrechetDistance(net, lib=inject(lib, dev))
    for s in range(0, n, 7):
        fid.update(real[s:s + 7].to(dev), real=True)
        fid.update(fake[s:s + 7].to(dev), real=False)
    got = float(fid.compute())

    def ref(dtype):
        fr = R.forward(sd, real, dtype, k["channel_div"], False, upto=feature)[feature].double().numpy()
        ff = R.forward(sd, fake, dtype, k["channel_div"], False, upto=feature)[feature].double().numpy()
        return FR.fid_symmetric(*FR.gaussian(fr), *FR.gaussian(ff))

    want, want32 = ref(torch.float64), ref(torch.float32)
    bound = 8 * abs(want32 - want) + dist_threshold("full", d) * max(1.0, abs(want))
    print(f"inception frechet d={d}: got {got:.9g} want {want:.9g} (fp32 CPU features {want32:.9g}) bound {bound:.2e}")
    assert want > 100 * bound, "the two image sets must differ by far more than the bound"
    assert abs(got - want) <= bound, (got, want, bound)


def check_cli(lib, st, dev, root, feature=64):
    """The command line with --fid and an injected InceptionV3 at channel_div = 8: the reference's column order, FID then
    FID_CLIP, both columns equal to compute_fid_datasets with the same modules; without --fid the file is what it was."""
    dirs = {name: os.path.join(root, name) for name in ("real", "method_a", "method_b")}
    for k, d in enumerate(dirs.values()):
        write_images(d, seed=k)
    g = torch.Generator().manual_seed(9)
    proj = torch.randn(3 * 16, 6, generator=g).to(dev) / 255

    def clip(images):  # [N,3,299,299] uint8 -> [N,6]
        return F.adaptive_avg_pool2d(images.float(), 4).reshape(images.shape[0], -1) @ proj

    net = InceptionV3(feature, weights=R.discriminating_state(8), channel_div=8, lib=inject(lib, dev)).to(dev)
    out = os.path.join(root, "logs", "metric.csv")
    argv = ["--source_dataset", dirs["real"], "--methods_dataset", f"A,{dirs['method_a']}", f"B,{dirs['method_b']}", "--output", out,
            "--batch", "2"]
    plain = MT.main(argv, feature=clip, lib=inject(lib, dev), device=dev)
    with open(out, newline="") as f:
        before = f.read()
    assert list(csv.reader(before.splitlines())) == [["", "FID_CLIP"]] + [[name, str(round(plain[name], 2))] for name in ("A", "B")]
    both = MT.main(argv + ["--fid"], feature=clip, inception=net, lib=inject(lib, dev), device=dev)
    assert set(both) == {"FID", "FID_CLIP"} and both["FID_CLIP"] == plain
    datasets = {name: MT.load_images_299(d, MT.list_image_files(d), device=dev, lib=inject(lib, dev)) for name, d in dirs.items()}
    want = MT.compute_fid_datasets({"real": datasets["real"], "A": datasets["method_a"], "B": datasets["method_b"]}, "real", net, 2,
                                   inject(lib, dev))
    assert both["FID"] == want and all(v > 0 for v in want.values())
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [["", "FID", "FID_CLIP"]] + [[name, str(round(both["FID"][name], 2)), str(round(plain[name], 2))] for name in ("A", "B")]
    # against the restatement: five images a side give a rank-deficient problem; the bound is check_frechet's with that family
    sd = R.discriminating_state(8)

    def ref(dtype, key):
        fr, ff = (R.forward(sd, datasets[k].cpu(), dtype, 8, True, upto=feature)[feature].double().numpy() for k in ("real", key))
        return FR.fid_symmetric(*FR.gaussian(fr), *FR.gaussian(ff))

    for name, key in (("A", "method_a"), ("B", "method_b")):
        r64, r32 = ref(torch.float64, key), ref(torch.float32, key)
        bound = 8 * abs(r32 - r64) + dist_threshold("deficient", net.feature_width) * max(1.0, abs(r64))
        print(f"inception cli {name}: got {both['FID'][name]:.9g} want {r64:.9g} (fp32 CPU features {r32:.9g}) bound {bound:.2e}")
        assert abs(both["FID"][name] - r64) <= bound, (name, both["FID"][name], r64, bound)
    MT.main(argv, feature=clip, lib=inject(lib, dev), device=dev)
    with open(out, newline="") as f:
        assert f.read() == before
