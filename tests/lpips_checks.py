"""TEST INFRASTRUCTURE - the checks of the LPIPS and L2 / PSNR path (csrc/lpips.h, hairfastgan_amd.lpips) against the torch /
numpy restatements (tests/lpips_ref.py), shared by the hipsim tests (tests/test_sim_lpips.py) and the GPU tests
(tests/test_gpu_lpips.py): every function takes the library, the stream and the device to run on.

Rules.
  max pool     bit equality with F.max_pool2d on the CPU.
  resize       byte equality with Pillow's Image.resize(size, BILINEAR).
  direct conv  |y - truth| <= (K + 4) 2^-24 (sum |w x^| + |b|) per output, K = cin k^2, truth = an fp64 conv: one rounding of
               the affine, K fused multiply-adds, the bias add (+ 1 spare).  Derived; nothing measured.
  LPIPS layer  |dev - truth| <= max(8 x the error of the same formula evaluated in fp32 torch on the CPU, floor) per sample;
               the 8 x allows for a different but equally valid summation order.  floor = lpips_ref.lpips_layer_floor: the
               first-order bound of ANY fp32 evaluation from the operation count, u sum_c |w_c| (C + 6) (|d_c| (|x^_c| +
               |y^_c|) + d_c^2) per pixel (derivation in its docstring), evaluated on the fp64 values of the case.
               fp32 errors of torch on the CPU, absolute, largest over LAYER_SHAPES (LAYER_MEASURED adds a third: torch's
               summation order follows its thread count and vector width):
                 independent 3.15e-8, noise 1e-2 2.22e-11, noise 1e-4 2.67e-13, zeroed pixels 9.03e-9, negative weights 4.61e-9
               The floor is a worst-case bound and 10 to 300 times these figures: it decides in most cases.
  whole LPIPS  the same rule with the fp32 evaluation of the whole metric (tower and distance) on the CPU; the floor is the sum
               of the layer floors on the true features (the error of the last stage alone).  fp32 errors, absolute, largest
               over the sizes of a tower (LPIPS_MEASURED rounds them up; the relative ones are about 1e-7, 5e-7 and 1e-4 at
               noise 0.5, 1e-2 and 1e-4 against distances of 6.8e-3, 5.5e-6 and 5.5e-10):
                 alex (64, 95, 272)  8.7e-10 1.1e-9 4.3e-10 | 5.3e-12 6.3e-12 3.1e-12 | 2.4e-13 5.4e-14 5.7e-15
                 vgg (32, 48)        4.6e-10 2.1e-10        | 3.6e-12 2.9e-12         | 5.4e-14 6.4e-15
               The floors are 1.6e-7, 4e-9 and 4e-11 at the three noise levels and decide here too.
  L2 / PSNR    uint8: the bits of numpy's integer sum (every term and every partial sum is an integer below 2^53); fp32:
               relative n 2^-52 against numpy's fp64 sum (n terms, one rounding of the square and one of the add each, all
               terms non-negative).  PSNR: 10 log10(range^2 / mse) within 4 fp64 eps relative of numpy's (one division, one
               log10, one product each side) plus the relative error of the mse inside the logarithm.
tests/test_lpips_ref.py measures the recorded fp32 errors again and fails if one exceeds what is recorded here.
"""
import functools
import os

import numpy as np
import PIL.Image
import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import face_align as FA
from hairfastgan_amd import lpips as LP
from tests import lpips_ref as R
from tests.metric_common import bits, inject, raises, read_scores

EPS64 = 2.0 ** -52

POOL_CASES = ((3, 2, 15, 15), (3, 2, 8, 9), (2, 2, 7, 6), (2, 2, 2, 2))                    # (k, stride, h, w)
RESIZE_CASES = ((37, 53, 16, 16), (64, 64, 256, 256), (1024, 1024, 256, 256), (300, 200, 256, 256))  # (w, h) -> (w, h)
CONV_CASES = ((3, 64, 11, 4, 2, 35, 39), (3, 64, 3, 1, 1, 9, 17), (1, 5, 5, 1, 2, 6, 7), (4, 7, 3, 2, 0, 8, 8))  # cin cout k s p h w
CONV_VARIANTS = ("affine_bias_relu", "bias", "affine", "relu")
LAYER_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (3, 64, 15, 15), (2, 192, 7, 9), (1, 512, 2, 2), (2, 64, 63, 63))
LAYER_FAMILIES = ("independent", "noise_1e-2", "noise_1e-4", "zeroed", "negative_w")
LAYER_MEASURED = {"independent": 4.2e-8, "noise_1e-2": 3.0e-11, "noise_1e-4": 3.6e-13, "zeroed": 1.2e-8, "negative_w": 6.2e-9}
LPIPS_SIM = (("alex", 64), ("alex", 95), ("vgg", 32), ("vgg", 48))
LPIPS_GPU = (("alex", 272),)
NOISES = (0.5, 1e-2, 1e-4)
LPIPS_MEASURED = {("alex", 0.5): 1.5e-9, ("alex", 1e-2): 8.4e-12, ("alex", 1e-4): 3.2e-13,
                  ("vgg", 0.5): 6.2e-10, ("vgg", 1e-2): 4.8e-12, ("vgg", 1e-4): 7.2e-14}


def _seed(*key):
    s = 17
    for v in key:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---- max pool -----------------------------------------------------------------------------------------------------
def check_maxpool(L, st, device, k, stride, h, w):
    g = _seed(1, k, stride, h, w)
    x = torch.randn(2, 3, h, w, generator=g)
    x[0, 0, 0, 0], x[0, 0, 0, 1] = 0.0, -0.0
    for name, t in (("mixed", x), ("negative", -x.abs() - 0.1)):
        got = M.maxpool2d(L, st, t.to(device), k, stride)
        want = F.max_pool2d(t, k, stride)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32)), name
    bad = torch.zeros(1, 1, 4, 4, device=device)
    for args in ((4, 2), (1, 1), (3, 0), (3, 4)):
        assert L.hf_maxpool2d_f32(bad.data_ptr(), bad.data_ptr(), 1, 4, 4, *args, st) == -1, args
    assert L.hf_maxpool2d_f32(bad.data_ptr(), bad.data_ptr(), 1, 2, 4, 3, 2, st) == -1


# ---- bilinear resize ----------------------------------------------------------------------------------------------
def check_resize_bilinear(L, st, device, w, h, ow, oh):
    rng = np.random.default_rng(7 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // w, yy * 255 // h, (xx + 2 * yy) % 256], -1) + rng.integers(-60, 60, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    want = np.asarray(PIL.Image.fromarray(img, "RGB").resize((ow, oh), PIL.Image.BILINEAR))
    got = FA.resize_bilinear(L, st, torch.from_numpy(img).permute(2, 0, 1).contiguous().to(device), ow, oh)
    assert got.shape == (3, oh, ow) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy().transpose(1, 2, 0), want), int(np.abs(got.cpu().numpy().transpose(1, 2, 0).astype(int) - want).max())


# ---- direct conv --------------------------------------------------------------------------------------------------
def check_conv_direct(L, st, device, cin, cout, k, stride, pad, h, w, variant):
    g = _seed(2, cin, cout, k, stride, pad, h, w)
    x = torch.randn(2, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g)
    scale, shift = 1.0 / (0.4 + 0.1 * torch.rand(cin, generator=g)), torch.randn(cin, generator=g)
    affine, has_bias, relu = "affine" in variant, "bias" in variant, "relu" in variant
    args = dict(in_scale=scale if affine else None, in_shift=shift if affine else None, bias=bias if has_bias else None)
    got = M.conv2d_direct(L, st, x.to(device), wt.to(device), stride, pad, act=M.ACT_LRELU if relu else M.ACT_NONE, alpha=0.0,
                          **{n: (None if v is None else v.to(device)) for n, v in args.items()})
    want, mag = R.conv_direct(x, wt, stride, pad, relu=relu, **args)
    assert got.shape == want.shape and got.dtype == torch.float32, (got.shape, want.shape)
    err = (got.cpu().double() - want).abs()
    bound = (cin * k * k + 4) * R.U32 * mag
    assert bool((err <= bound).all()), (variant, float((err / bound.clamp_min(1e-300)).max()))
    assert float(want.abs().max()) > 0.1


def check_conv_direct_refusals(L, st, device):
    """cin > 4, k > 11, stride outside 1..4, pad outside [0, k) and an input smaller than the filter return HF_E_INVALID."""
    buf = torch.zeros(1 << 16, device=device)
    p = buf.data_ptr()

    def call(cin=3, cout=8, k=3, stride=1, pad=1, h=8, w=8, out=p, x=p, wt=p, act=0):
        return L.hf_conv2d_direct_f32(out, x, wt, None, None, None, act, 0.0, 1, cin, cout, h, w, k, stride, pad, st)

    assert call() == 0
    for kw in (dict(cin=5), dict(cin=0), dict(k=12, pad=0, h=16, w=16), dict(k=0), dict(stride=0), dict(stride=5), dict(pad=3),
               dict(pad=-1), dict(k=5, pad=0, h=4), dict(cout=0), dict(out=None), dict(x=None), dict(wt=None), dict(x=p + 2),
               dict(act=2)):
        assert call(**kw) == -1, kw


# ---- LPIPS layer --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_case(shape, family):
    """-> (fx, fy, lin_w) fp32 CPU tensors, read-only by agreement."""
    n, c, h, w = shape
    g = _seed(3, n, c, h, w, LAYER_FAMILIES.index(family))
    fx = torch.randn(n, c, h, w, generator=g)
    lin_w = torch.rand(c, generator=g) * (2.0 / c)
    if family == "independent":
        fy = torch.randn(n, c, h, w, generator=g)
    elif family.startswith("noise"):
        fy = fx + float(family.split("_")[1]) * torch.randn(n, c, h, w, generator=g)
    elif family == "zeroed":  # ReLU-like maps; whole pixels zeroed in fx (index % 4 == 1), in fy (== 2) and in both (== 3)
        fx, fy = fx.clamp_min(0.0), torch.randn(n, c, h, w, generator=g).clamp_min(0.0)
        idx = torch.arange(h * w).reshape(1, 1, h, w)
        fx = torch.where((idx % 4 == 1) | (idx % 4 == 3), torch.zeros(()), fx)
        fy = torch.where((idx % 4 == 2) | (idx % 4 == 3), torch.zeros(()), fy)
    else:
        fy = torch.randn(n, c, h, w, generator=g)
        lin_w = (torch.rand(c, generator=g) * 2.0 - 1.0) / c
    return fx.contiguous(), fy.contiguous(), lin_w


@functools.lru_cache(maxsize=None)
def layer_truth(shape, family):
    fx, fy, lin_w = layer_case(shape, family)
    return R.lpips_layer(fx, fy, lin_w), R.lpips_layer_floor(fx, fy, lin_w)


def layer_fp32_error(shape, family):
    fx, fy, lin_w = layer_case(shape, family)
    return float((R.lpips_layer(fx, fy, lin_w, torch.float32).double() - layer_truth(shape, family)[0]).abs().max())


def _layer(L, st, device, fx, fy, lin_w, into=None):
    dist = torch.empty(fx.shape[0], dtype=torch.float64, device=device) if into is None else into
    return M.lpips_layer_into(L, st, dist, fx.to(device), fy.to(device), lin_w.to(device), accumulate=into is not None)


def check_layer(L, st, device, shape, family):
    fx, fy, lin_w = layer_case(shape, family)
    truth, floor = layer_truth(shape, family)
    got = _layer(L, st, device, fx, fy, lin_w).cpu()
    assert bool(torch.isfinite(got).all())
    thr = torch.maximum(torch.full_like(floor, 8.0 * LAYER_MEASURED[family]), floor)
    err = (got - truth).abs()
    print(f"lpips layer {shape} {family}: err {float(err.max()):.3e} thr {float(thr.min()):.3e} floor {float(floor.min()):.3e} "
          f"truth {float(truth.abs().max()):.3e}")
    assert bool((err <= thr).all()), (shape, family, err.tolist(), thr.tolist())
    if family == "zeroed":  # both maps all zero: 0 / 1e-10 - 0 / 1e-10
        z = torch.zeros_like(fx)
        assert bits(_layer(L, st, device, z, z, lin_w)).tolist() == [0] * shape[0]


def check_layer_conditions(L, st, device, shape):
    """d(x, x) = 0 exactly; d(x, y) and d(y, x) have equal bits; a sample's bits depend neither on the batch size nor on its
    position; two runs give equal bits; accumulate adds to the output."""
    fx, fy, lin_w = layer_case(shape, "independent")
    n = shape[0]
    d = _layer(L, st, device, fx, fy, lin_w)
    assert bits(_layer(L, st, device, fx, fx, lin_w)).tolist() == [0] * n
    assert np.array_equal(bits(_layer(L, st, device, fy, fx, lin_w)), bits(d))
    assert np.array_equal(bits(_layer(L, st, device, fx, fy, lin_w)), bits(d))
    for i in range(n):
        assert np.array_equal(bits(_layer(L, st, device, fx[i:i + 1], fy[i:i + 1], lin_w)), bits(d[i:i + 1])), i
    big = _layer(L, st, device, torch.cat([fy, fx.flip(0), fx]), torch.cat([fx, fy.flip(0), fy]), lin_w)
    assert np.array_equal(bits(big), np.concatenate([bits(d), bits(d.flip(0)), bits(d)]))
    start = torch.linspace(0.25, 1.75, n, dtype=torch.float64).to(device)
    acc = _layer(L, st, device, fx, fy, lin_w, into=start.clone())
    assert np.array_equal(bits(acc), bits(start + d))


def check_layer_refusals(L, st, device):
    buf = torch.zeros(256, dtype=torch.float64, device=device)
    p = buf.data_ptr()
    assert L.hf_lpips_layer_work_doubles(2, 5, 7) == 2 and L.hf_lpips_layer_work_doubles(1, 63, 63) == 63 and L.hf_lpips_layer_work_doubles(0, 1, 1) == 0
    assert L.hf_lpips_layer_f64(p, p, p, p, p, 1, 3, 2, 2, 0, st) == 0
    for args in ((None, p, p, p, p, 1, 3, 2, 2), (p + 4, p, p, p, p, 1, 3, 2, 2), (p, None, p, p, p, 1, 3, 2, 2), (p, p, p + 2, p, p, 1, 3, 2, 2),
                 (p, p, p, None, p, 1, 3, 2, 2), (p, p, p, p, None, 1, 3, 2, 2), (p, p, p, p, p, 0, 3, 2, 2), (p, p, p, p, p, 1, 0, 2, 2),
                 (p, p, p, p, p, 1, 3, 0, 2)):
        assert L.hf_lpips_layer_f64(*args, 0, st) == -1, args


# ---- whole LPIPS --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lpips_images(net_type, size, noise):
    g = _seed(4, size, 0 if net_type == "alex" else 1)
    x = torch.rand(2, 3, size, size, generator=g) * 2.0 - 1.0
    gn = _seed(5, size, NOISES.index(noise))
    return x, (x + noise * torch.randn(2, 3, size, size, generator=gn)).contiguous()


@functools.lru_cache(maxsize=None)
def lpips_truth(net_type, size, noise):
    x, y = lpips_images(net_type, size, noise)
    sd = R.random_weights(net_type)
    return R.lpips(sd, net_type, x, y), R.lpips_floor(sd, net_type, x, y)


def lpips_fp32_error(net_type, size, noise):
    x, y = lpips_images(net_type, size, noise)
    return float((R.lpips(R.random_weights(net_type), net_type, x, y, torch.float32).double() - lpips_truth(net_type, size, noise)[0]).abs().max())


def make_model(L, device, net_type):
    model = LP.LPIPS(net_type, lib=inject(L, device))
    model.load_state_dict(R.random_weights(net_type))
    return model.to(device).eval()


def _per_sample_shared_x(model, L, st, x, ys):
    """per_sample's own steps with the features of x taken ONCE for all of ys (the interpreter spends minutes on a VGG pass)."""
    fx = model.features(x)
    fy = model.features(ys)
    dist = torch.empty(ys.shape[0], dtype=torch.float64, device=ys.device)
    for j, (a, b) in enumerate(zip(fx, fy)):
        M.lpips_layer_into(L, st, dist, a.expand_as(b), b, model.lin[j][1].weight.detach().reshape(-1), accumulate=j > 0)
    return dist


def check_lpips(L, st, device, net_type, size, whole_batch=False, shared_x=False, models={}):
    """per_sample against the fp64 truth in ONE call of batch 4 - the first image against its three noisy versions and against
    itself (exactly 0).  whole_batch: also both images of the noise 0.5 pair, and forward = per_sample.sum() / N.
    shared_x: the same distances from `features` and the layer kernel, with x's features computed once."""
    key = (net_type, device.type)
    if key not in models:
        models[key] = make_model(L, device, net_type)
    model = models[key]
    x = lpips_images(net_type, size, NOISES[0])[0][:1]
    ys = [lpips_images(net_type, size, noise)[1][:1] for noise in NOISES]
    if shared_x:
        got = _per_sample_shared_x(model, L, st, x.to(device), torch.cat(ys).to(device))
    else:
        got = model.per_sample(torch.cat([x] * 4).to(device), torch.cat(ys + [x]).to(device))
    assert got.shape == (3 if shared_x else 4,) and got.dtype == torch.float64 and got.device.type == device.type
    assert bits(got[3:]).tolist() == [0] * (got.numel() - 3)
    for k, noise in enumerate(NOISES):
        truth, floor = (float(t[0]) for t in lpips_truth(net_type, size, noise))
        thr = max(8.0 * LPIPS_MEASURED[(net_type, noise)], floor)
        err = abs(float(got[k]) - truth)
        print(f"lpips {net_type} {size} noise {noise}: truth {truth:.6e} err {err:.3e} thr {thr:.3e} floor {floor:.3e}")
        assert err <= thr, (net_type, size, noise, err, thr, truth)
    if whole_batch:
        xb, yb = (t.to(device) for t in lpips_images(net_type, size, NOISES[0]))
        both = model.per_sample(xb, yb)
        truth, floor = lpips_truth(net_type, size, NOISES[0])
        thr = torch.maximum(torch.full_like(floor, 8.0 * LPIPS_MEASURED[(net_type, NOISES[0])]), floor)
        assert bool(((both.cpu() - truth).abs() <= thr).all()), (both.tolist(), truth.tolist())
        fwd = model(xb, yb)
        assert fwd.ndim == 0 and fwd.dtype == torch.float32 and torch.equal(fwd, (both.sum() / 2).float())


# ---- L2 / PSNR ----------------------------------------------------------------------------------------------------
def check_psnr(L, st, device):
    lib = inject(L, device)
    rng = np.random.default_rng(11)
    for shape in ((3, 3, 17, 23), (2, 3, 64, 65), (1, 1, 1, 1)):
        a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
        per = a[0].size
        ta, tb = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
        sums = M.sq_err_sum(L, st, ta, tb)
        want = R.sq_err_sum(a, b)
        assert np.array_equal(bits(sums), want.astype(np.float64).view(np.uint64)), shape
        assert np.array_equal(bits(LP.mse(ta, tb, lib=lib)), (want.astype(np.float64) / per).view(np.uint64))
        got = LP.psnr(ta, tb, lib=lib).cpu().numpy()
        ref = R.psnr(a, b, 255)
        assert np.all(np.abs(got - ref) <= 4 * EPS64 * np.abs(ref) + 10 * EPS64), (got, ref)
        assert np.all(np.isinf(LP.psnr(ta, ta, lib=lib).cpu().numpy()))
        for i in range(shape[0]):  # batch invariance
            assert np.array_equal(bits(M.sq_err_sum(L, st, ta[i:i + 1], tb[i:i + 1])), bits(sums[i:i + 1]))
        fa, fb = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        fta, ftb = torch.from_numpy(fa).to(device), torch.from_numpy(fb).to(device)
        fs = M.sq_err_sum(L, st, fta, ftb)
        fw = R.sq_err_sum(fa, fb)
        assert np.all(np.abs(fs.cpu().numpy() - fw) <= per * EPS64 * fw), shape
        for i in range(shape[0]):
            assert np.array_equal(bits(M.sq_err_sum(L, st, fta[i:i + 1], ftb[i:i + 1])), bits(fs[i:i + 1]))
        assert np.all(np.isinf(LP.psnr(fta, fta, data_range=2.0, lib=lib).cpu().numpy()))
        p2 = LP.psnr(fta, ftb, data_range=2.0, lib=lib).cpu().numpy()
        r2 = R.psnr(fa, fb, 2.0)
        assert np.all(np.abs(p2 - r2) <= 4 * EPS64 * np.abs(r2) + 10 * (per + 1) * EPS64)
    raises(ValueError, lambda: LP.psnr(fta, ftb, lib=lib), "data_range")
    raises(ValueError, lambda: M.sq_err_sum(L, st, ta, ftb))
    buf = torch.zeros(64, dtype=torch.float64, device=device)
    p = buf.data_ptr()
    assert L.hf_sq_err_sum_work_doubles(2, 12480) == 8 and L.hf_sq_err_sum_work_doubles(1, 1) == 1
    for args in ((None, p, p, p, 1, 4, 0), (p + 4, p, p, p, 1, 4, 0), (p, None, p, p, 1, 4, 1), (p, p + 1, p, p, 1, 4, 0), (p, p, p, None, 1, 4, 0),
                 (p, p, p, p, 0, 4, 0), (p, p, p, p, 1, 0, 0)):
        assert L.hf_sq_err_sum_f64(*args, st) == -1, args


# ---- command line -------------------------------------------------------------------------------------------------
CLI_FILES = (("a.png", (70, 64)), ("b.png", (64, 64)), ("c.png", (96, 80)), ("d.png", (33, 47)), ("e.png", (128, 128)), ("f.png", (65, 66)))


def write_pairs(root):
    rng = np.random.default_rng(21)
    data, gt = os.path.join(root, "results"), os.path.join(root, "gt_images")
    os.makedirs(data), os.makedirs(gt)
    for k, (name, (w, h)) in enumerate(CLI_FILES):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 // w, yy * 255 // h, (3 * xx + yy) % 256], -1) + rng.integers(-30, 30, (h, w, 3))
        other = base + rng.integers(-(4 + 10 * k), 5 + 10 * k, (h, w, 3))
        for folder, img in ((gt, base), (data, other)):
            PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(os.path.join(folder, name))
    return data, gt


def check_cli(L, st, device, root, decoder="pil"):
    """Six small PNGs: the JSON keys are the file names, the values equal direct calls, the stat text has the reference's format."""
    data, gt = write_pairs(root)
    lib = inject(L, device)
    names = [n for n, _ in CLI_FILES]
    model = make_model(L, device, "alex")
    res, truth = LP.load_pairs(data, gt, names, 64, decoder, device, lib)
    for k, name in enumerate(names):
        ref = np.asarray(PIL.Image.open(os.path.join(data, name)).convert("RGB").resize((64, 64), PIL.Image.BILINEAR))
        assert np.array_equal(res[k].cpu().numpy().transpose(1, 2, 0), ref), name
    x, y = (res.float() / 255 - 0.5) / 0.5, (truth.float() / 255 - 0.5) / 0.5
    want = {"lpips": torch.cat([model.per_sample(x[:4], y[:4]), model.per_sample(x[4:], y[4:])]),  # the command line's batches
            "l2": LP.mse(x, y, lib), "psnr": LP.psnr(res, truth, lib=lib)}
    for mode in ("lpips", "l2", "psnr"):
        scores = LP.main(["--mode", mode, "--data_path", data, "--gt_path", gt, "--size", "64", "--batch", "4", "--image_decoder", decoder],
                         model=model, lib=lib, device=device)
        saved, stat = read_scores(root, mode)
        assert list(saved) == names == list(scores)
        values = want[mode].cpu().tolist()
        assert [saved[n] for n in names] == values, mode
        assert stat == "Average loss is {:.2f}+-{:.2f}".format(np.mean(values), np.std(values))
    assert want["lpips"].min() > 0 and len(set(want["lpips"].tolist())) == 6
