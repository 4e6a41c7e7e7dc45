"""TEST INFRASTRUCTURE - the checks of the SSIM / MS-SSIM path (csrc/ssim.h, hairfastgan_amd.ssim) against the two fp64
restatements of tests/ssim_ref.py, shared by the hipsim tests (tests/test_sim_ssim.py) and the GPU tests
(tests/test_gpu_ssim.py): every function takes the library, the stream and the device to run on.

Rule for values.  |device - truth| <= max(8 x d, floor) per sample, per pixel for the map.
  truth  the conv form of ssim_ref in float64.
  d      the disagreement of the two CPU fp64 restatements (scipy form, conv form) on the same case, largest over KERNEL_SHAPES,
         recorded per family below with a margin of up to two (the filters' summation order follows the library build):
         D_MEAN for the plane means of S and cs, D_MAP for single pixels.  The factor 8 allows for a different but equally
         valid summation order, as in tests/lpips_checks.py.  Measured (absolute):
           plane means  independent 7.0e-16, noise 4 / 24 / 64 3.8e-15 2.7e-15 1.9e-15, constant 1.6e-13 (scipy's uniform
                        filter is a running sum), checker 3.9e-16, inverted 3.6e-14, unit 7.1e-15, offset 2.9e-9
           pixels       independent 9.9e-15, noise 3.1e-13 2.4e-13 9.8e-14, constant 1.6e-13, checker 9.2e-16, inverted 2.0e-13,
                        unit 4.9e-14, offset 4.6e-8
         tests/test_ssim_ref.py measures them again and fails when one exceeds what is recorded.
  floor  ssim_ref.ssim_floor: the first-order bound of any fp64 evaluation from the operation count, on the fp64 values of the
         case (derivation in its docstring).  It scales with (uxx + uyy) / (vx + vy + C2).  On the plane means it is 2e-14 to
         1e-12 for the 8-bit families (8e-12 for constant planes), 5e-14 to 2e-13 for floats in [-1, 1] and 1.2e-7 to 2.1e-7 in
         the offset family (floats in [1000, 1001], data range 1).  It is a worst-case bound, 10 to 100 times what the
         restatements differ by, and at or above 8 d in most cases.
  MS-SSIM  the same rule; d between ssim_ref.ms_ssim and its scipy twin (at most 5.6e-16 over MS_CASES; MS_D), floor = value x
         (sum_j w_j floor_j / v_j + 4 M u): the first-order error of prod v_j^w_j from the level floors and M pow / product
         roundings; 1e-13 to 2e-12 here.
The fp32 evaluation of the same formula misses the rule by five orders of magnitude (1e-8 to 1e-6 on the plane means of the
8-bit and unit families, 3 to 4 in the offset family; test_ssim_ref.py asserts it), so an fp32 kernel would be noticed.
Everything stated as "equal" is compared as bits.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import lpips as LP
from hairfastgan_amd import ssim as SS
from tests import lpips_checks as LK
from tests import ssim_ref as R
from tests.metric_common import bits, inject, raises, read_scores

TILE_H, TILE_W = 16, 32  # csrc/ssim.h kSsTileH, kSsTileW; check_tile_constants compares them with hf_ssim_tile
# (planes, H, W, win): one output pixel (narrowest / widest window), one output row, one output column, ragged, general, the
# smallest window; then two full tiles plus a ragged remainder in each direction (seams, the halo of an inner tile) at each of
# the five window widths the kernel is instantiated for (3, 5, 7, 9, 11)
KERNEL_SHAPES = ((1, 7, 7, 7), (3, 11, 11, 11), (2, 7, 40, 7), (2, 40, 7, 7), (3, 33, 47, 7), (6, 70, 64, 11), (1, 5, 9, 3),
                 (2, 2 * TILE_H + 5 + 6, 2 * TILE_W + 9 + 6, 7), (1, 2 * TILE_H + 3 + 10, 2 * TILE_W + 7 + 10, 11),
                 (1, 2 * TILE_H + 1 + 2, 2 * TILE_W + 3 + 2, 3), (1, 2 * TILE_H + 3 + 4, 2 * TILE_W + 5 + 4, 5),
                 (1, 2 * TILE_H + 7 + 8, 2 * TILE_W + 3 + 8, 9))
# One window per width.  The asymmetric ones (3, 5) catch a flipped window and swapped passes; 9 is the Gaussian of sigma 1.2,
# as ssim(win_size=9, sigma=1.2) builds it.
WINDOWS = {7: "uniform", 11: "gaussian", 3: (0.1, 0.2, 0.7), 5: (0.05, 0.1, 0.15, 0.3, 0.4),
           9: tuple(float(v) for v in np.exp(-0.5 * (np.arange(-4, 5) / 1.2) ** 2) / np.exp(-0.5 * (np.arange(-4, 5) / 1.2) ** 2).sum())}
U8_FAMILIES = ("independent", "noise4", "noise24", "noise64", "constant", "checker", "inverted")
FLOAT_FAMILIES = ("unit", "offset")
FAMILIES = U8_FAMILIES + FLOAT_FAMILIES
DATA_RANGE = {"unit": 2.0, "offset": 1.0}
DTYPES = {"uint8": torch.uint8, "fp32": torch.float32, "fp64": torch.float64}
D_MEAN = {"independent": 1.5e-15, "noise4": 8e-15, "noise24": 6e-15, "noise64": 4e-15, "constant": 3.2e-13, "checker": 1e-15,
          "inverted": 7e-14, "unit": 1.5e-14, "offset": 6e-9}
D_MAP = {"independent": 2e-14, "noise4": 6e-13, "noise24": 5e-13, "noise64": 2e-13, "constant": 3.2e-13, "checker": 2e-15,
         "inverted": 4e-13, "unit": 1e-13, "offset": 1e-7}
HOST_SHAPES = ((33, 47), (2 * TILE_H + 5 + 6, 2 * TILE_W + 9 + 6))
MS_CASES = (((176, 177), R.MS_WEIGHTS, "gaussian"), ((176, 176), R.MS_WEIGHTS, "gaussian"), ((28, 29), (0.3, 0.3, 0.4), "uniform"),
            ((44, 45), (0.5, 0.5), "gaussian"))
MS_NOISES = (4, 64)
MS_D = 1.2e-15


def _rng(*key):
    return np.random.default_rng([23] + [int(v) for v in key])


def structured(rng, planes, h, w):
    """[planes,h,w] int64 in 0..255: the channels of lpips_checks.write_pairs, which differ along rows and columns."""
    yy, xx = np.mgrid[0:h, 0:w]
    chans = np.stack([xx * 255 // w, yy * 255 // h, (3 * xx + yy) % 256])
    base = chans[np.arange(planes) % 3] + rng.integers(-30, 30, (planes, h, w))
    return np.clip(base, 0, 255)


@functools.lru_cache(maxsize=None)
def plane_case(planes, h, w, family):
    """-> (x, y) CPU tensors [planes,h,w]: uint8 for the 8-bit families, fp32 for the float ones; read-only by agreement."""
    rng = _rng(planes, h, w, FAMILIES.index(family))
    base = structured(rng, planes, h, w)
    if family == "independent":
        x, y = rng.integers(0, 256, (planes, h, w)), rng.integers(0, 256, (planes, h, w))
    elif family.startswith("noise"):
        k = int(family[5:])
        x, y = base, np.clip(base + rng.integers(-k, k + 1, base.shape), 0, 255)
    elif family == "constant":
        x = np.broadcast_to((100 + 7 * np.arange(planes))[:, None, None], base.shape)
        y = np.broadcast_to((140 - 33 * (np.arange(planes) % 2))[:, None, None], base.shape)  # plane 1: equal constants
    elif family == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        x = np.broadcast_to(255 * ((yy + xx) % 2), base.shape)
        y = np.stack([255 * ((yy + xx // 2 + p) % 2) for p in range(planes)])
    elif family == "inverted":
        x, y = base, 255 - base
    elif family == "unit":
        x = (base / 127.5 - 1.0).astype(np.float32)
        y = (np.clip(base + rng.integers(-24, 25, base.shape), 0, 255) / 127.5 - 1.0).astype(np.float32)
        return torch.from_numpy(x), torch.from_numpy(y)
    else:  # offset: the mean is a thousand data ranges
        x = (1000.0 + rng.random(base.shape)).astype(np.float32)
        y = np.clip(x + 0.1 * rng.standard_normal(base.shape), 1000.0, 1001.0).astype(np.float32)
        return torch.from_numpy(x), torch.from_numpy(y)
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.uint8)), torch.from_numpy(np.ascontiguousarray(y).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def plane_truth(shape, family):
    """-> (S, cs, floor of S, floor of cs) float64 [planes,oh,ow] of the conv form."""
    planes, h, w, win = shape
    x, y = plane_case(planes, h, w, family)
    rng_ = DATA_RANGE.get(family, 255.0)
    s, cs = R.conv_maps(x, y, WINDOWS[win], rng_)
    return (s, cs) + R.ssim_floor(x, y, WINDOWS[win], rng_)


def restatement_gap(shape, family):
    """(largest |scipy form - conv form| of the plane means of S and cs, of single pixels)."""
    planes, h, w, win = shape
    x, y = plane_case(planes, h, w, family)
    s, cs = plane_truth(shape, family)[:2]
    s2, cs2 = (torch.from_numpy(a) for a in R.scipy_maps(x.numpy(), y.numpy(), WINDOWS[win], DATA_RANGE.get(family, 255.0)))
    mean = max(float((s.mean((1, 2)) - s2.mean((1, 2))).abs().max()), float((cs.mean((1, 2)) - cs2.mean((1, 2))).abs().max()))
    return mean, max(float((s - s2).abs().max()), float((cs - cs2).abs().max()))


def fp32_misses(shape, family):
    """Does the fp32 evaluation of the same formula miss the rule of the plane means?"""
    planes, h, w, win = shape
    x, y = plane_case(planes, h, w, family)
    s, _, fs, _ = plane_truth(shape, family)
    s32 = R.conv_maps(x, y, WINDOWS[win], DATA_RANGE.get(family, 255.0), dtype=torch.float32)[0].double()
    err = (s32.mean((1, 2)) - s.mean((1, 2))).abs()
    return bool((err > torch.clamp_min(fs.mean((1, 2)), 8.0 * D_MEAN[family])).any()), float(err.max())


def _taps(win, device):
    taps, cn = R.window(WINDOWS[win])
    return torch.from_numpy(np.ascontiguousarray(taps)).to(device), cn


def families_of(dtype):
    """The 8-bit families run in every element type (their values are exact in each), the float ones in fp32 and fp64."""
    return U8_FAMILIES if dtype == "uint8" else FAMILIES


# ---- the kernel through the C ABI -----------------------------------------------------------------------------------
def check_tile_constants(L):
    assert (L.hf_ssim_tile(0), L.hf_ssim_tile(1)) == (TILE_H, TILE_W)
    assert L.hf_ssim_work_doubles(3, 33, 47, 7) == 2 * 3 * 2 * 2 and L.hf_ssim_work_doubles(1, 7, 7, 7) == 2
    assert L.hf_ssim_work_doubles(1, 6, 7, 7) == 0 and L.hf_ssim_work_doubles(0, 7, 7, 7) == 0 and L.hf_ssim_work_doubles(1, 9, 9, 4) == 0


def check_kernel(L, st, device, shape, dtype):
    """Sums of S and cs, the map and the next level of every family the element type holds, against the truth by the rule; the
    sums' bits do not depend on which optional outputs are requested."""
    planes, h, w, win = shape
    taps, cn = _taps(win, device)
    pixels = (h - win + 1) * (w - win + 1)
    for family in families_of(dtype):
        x, y = (t.to(DTYPES[dtype])[None].to(device) for t in plane_case(planes, h, w, family))
        c1, c2 = R.constants(DATA_RANGE.get(family, 255.0))
        out = M.ssim_planes(L, st, x, y, taps, c1, c2, cn, want_cs=True, want_map=True, want_next=True)
        s, cs, fs, fcs = plane_truth(shape, family)
        got_map = out["map"][0].cpu()
        assert bool(torch.isfinite(got_map).all()) and got_map.shape == s.shape
        err_map = (got_map - s).abs()
        thr_map = torch.clamp_min(fs, 8.0 * D_MAP[family])
        for name, got, truth, floor in (("S", out["s"], s, fs), ("cs", out["cs"], cs, fcs)):
            err = (got[0].cpu() / pixels - truth.mean((1, 2))).abs()
            thr = torch.clamp_min(floor.mean((1, 2)), 8.0 * D_MEAN[family])
            print(f"ssim {shape} {dtype} {family} {name}: mean {float(truth.mean()):+.4f} err {float(err.max()):.3e} thr {float(thr.min()):.3e} "
                  f"floor {float(floor.mean((1, 2)).min()):.3e}; map err {float(err_map.max()):.3e}")
            assert bool((err <= thr).all()), (shape, dtype, family, name, err.tolist(), thr.tolist())
        assert bool((err_map <= thr_map).all()), (shape, dtype, family, float((err_map / thr_map).max()))
        # the score is the map's mean (the kernel adds the same values in its own order)
        assert bool(((got_map.mean((1, 2)) - out["s"][0].cpu() / pixels).abs() <= torch.clamp_min(fs.mean((1, 2)), 8.0 * D_MEAN[family])).all())
        plain = M.ssim_planes(L, st, x, y, taps, c1, c2, cn, want_cs=True)
        assert np.array_equal(bits(plain["s"]), bits(out["s"])) and np.array_equal(bits(plain["cs"]), bits(out["cs"])), (shape, family)
        again = M.ssim_planes(L, st, x, y, taps, c1, c2, cn, want_cs=True, want_map=True, want_next=True)
        for key in ("s", "cs", "map"):
            assert np.array_equal(bits(again[key]), bits(out[key])), key
        a, b = x[0].cpu().double().numpy(), y[0].cpu().double().numpy()
        for got, src in zip(out["next"], (a, b)):
            e = src[:, :h // 2 * 2, :w // 2 * 2]
            want = (((e[:, 0::2, 0::2] + e[:, 0::2, 1::2]) + e[:, 1::2, 0::2]) + e[:, 1::2, 1::2]) * 0.25
            assert got.shape == (1, planes, h // 2, w // 2)
            assert np.array_equal(bits(got[0]), want.view(np.uint64)), (shape, dtype, family)
        if dtype == "uint8":  # integer sums / 4
            xi = x[0].cpu().numpy().astype(np.int64)[:, :h // 2 * 2, :w // 2 * 2]
            want = (xi[:, 0::2, 0::2] + xi[:, 0::2, 1::2] + xi[:, 1::2, 0::2] + xi[:, 1::2, 1::2]) / 4
            assert np.array_equal(out["next"][0][0].cpu().numpy(), want)
        if family == "inverted":
            assert float(out["s"].max()) < 0 and float(out["cs"].max()) < 0


def check_next_level_f64(L, st, device):
    """The next level of an fp64 level with fractional values equals the fp64 2x2 mean exactly, for odd and even H and W."""
    for h, w in ((12, 14), (13, 14), (12, 15), (2 * TILE_H + 9, 2 * TILE_W + 7)):
        rng = _rng(h, w, 99)
        x, y = (torch.from_numpy(rng.random((2, 3, h, w)) * 255.0).to(device) for _ in range(2))
        taps, cn = _taps(3, device)
        out = M.ssim_planes(L, st, x, y, taps, *R.constants(255.0), cn, want_next=True)
        for got, src in zip(out["next"], (x, y)):
            e = src.cpu().numpy()[:, :, :h // 2 * 2, :w // 2 * 2]
            want = (((e[..., 0::2, 0::2] + e[..., 0::2, 1::2]) + e[..., 1::2, 0::2]) + e[..., 1::2, 1::2]) * 0.25
            assert np.array_equal(bits(got), np.ascontiguousarray(want).view(np.uint64)), (h, w)
            assert float((got.cpu() - F.avg_pool2d(src.cpu(), 2)).abs().max()) <= 255 * 4 * R.U64


def check_kernel_refusals(L, st, device):
    """Every HF_E_INVALID condition of include/hairfast_hip.h."""
    buf = torch.zeros(1 << 14, dtype=torch.float64, device=device)
    p = buf.data_ptr()

    def call(sum_s=p, aux=None, smap=None, nx=None, ny=None, x=p, y=p, mask=None, taps=p, work=p, dtype=1, planes=3, channels=3, h=9, w=9,
             win=7):
        return L.hf_ssim_planes_f64(sum_s, aux, smap, nx, ny, x, y, mask, taps, work, dtype, planes, channels, h, w, win, 1.0, 1.0, 1.0, st)

    assert call() == 0 and call(aux=p, smap=p, nx=p, ny=p, mask=p) == 0
    for kw in (dict(sum_s=None), dict(x=None), dict(y=None), dict(taps=None), dict(work=None), dict(sum_s=p + 4), dict(aux=p + 4),
               dict(smap=p + 4), dict(nx=p + 4, ny=p), dict(nx=p, ny=p + 4), dict(x=p + 2), dict(y=p + 2), dict(x=p + 4, dtype=2),
               dict(mask=p + 2), dict(taps=p + 4), dict(work=p + 4), dict(dtype=3), dict(dtype=-1), dict(win=6), dict(win=1), dict(win=13, h=16, w=16),
               dict(h=6), dict(w=6), dict(planes=0), dict(planes=-3), dict(nx=p), dict(ny=p), dict(mask=p, planes=4), dict(mask=p, channels=0)):
        assert call(**kw) == -1, kw
    assert call(x=p + 1, y=p + 3, dtype=0) == 0  # bytes need no alignment


# ---- the host functions ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image_case(n, h, w, family):
    """-> (x, y) [n,3,h,w] CPU tensors."""
    x, y = plane_case(3 * n, h, w, family)
    return x.reshape(n, 3, h, w), y.reshape(n, 3, h, w)


def _rule(family, floor):
    return torch.clamp_min(floor, 8.0 * D_MEAN[family])


def check_ssim(L, st, device, hw, window):
    """ssim / dssim / full against the truth for both conventions; a float image with its data range."""
    lib = inject(L, device)
    h, w = hw
    for family in ("noise4", "noise24", "noise64", "inverted", "unit"):
        x, y = image_case(3, h, w, family)
        rng_ = DATA_RANGE.get(family, 255.0)
        kw = {} if x.dtype == torch.uint8 else {"data_range": rng_}
        truth = R.ssim(x, y, window, rng_)
        floor = R.ssim_floor(x.reshape(9, h, w), y.reshape(9, h, w), window, rng_)[0].mean((1, 2)).reshape(3, 3).mean(1)
        got, smap = SS.ssim(x.to(device), y.to(device), window=window, full=True, lib=lib, **kw)
        win = len(R.window(window)[0])
        assert got.shape == (3,) and got.dtype == torch.float64 and got.device.type == device.type
        assert smap.shape == (3, 3, h - win + 1, w - win + 1) and smap.dtype == torch.float64
        err = (got.cpu() - truth).abs()
        print(f"ssim {hw} {window} {family}: {truth.tolist()} err {float(err.max()):.3e} thr {float(_rule(family, floor).min()):.3e}")
        assert bool((err <= _rule(family, floor)).all()), (hw, window, family, err.tolist())
        assert bool(((smap.cpu().mean((2, 3)).mean(1) - got.cpu()).abs() <= _rule(family, floor)).all())
        assert np.array_equal(bits(SS.ssim(x.to(device), y.to(device), window=window, lib=lib, **kw)), bits(got))
        if window == "uniform":
            assert np.array_equal(bits(SS.dssim(x.to(device), y.to(device), lib=lib, **kw)), bits((1.0 - got) / 2.0))
            pop = SS.ssim(x.to(device), y.to(device), window=window, use_sample_covariance=False, lib=lib, **kw)
            assert bool(((pop.cpu() - R.ssim(x, y, window, rng_, cn=1.0)).abs() <= _rule(family, floor)).all())
    x, y = image_case(3, h, w, "noise24")
    assert 0.7 < float(R.ssim(x, y, "uniform", 255.0).mean()) < 0.9  # noise 24 gives about 0.8


def check_conditions(L, st, device, hw, window):
    """ssim(x, x) = 1 and dssim(x, x) = 0 exactly; ssim(x, y) = ssim(y, x); a sample's bits depend neither on the batch size nor
    on its position (batch 1 against 3 against a permuted 9); two runs are equal."""
    lib = inject(L, device)
    h, w = hw
    for family in ("noise24", "independent", "unit"):
        x, y = (t.to(device) for t in image_case(3, h, w, family))
        kw = {} if x.dtype == torch.uint8 else {"data_range": DATA_RANGE[family]}
        f = lambda a, b: SS.ssim(a, b, window=window, lib=lib, **kw)  # noqa: E731
        d = f(x, y)
        assert bits(f(x, x)).tolist() == bits(torch.ones(3, dtype=torch.float64)).tolist()
        assert bits(SS.dssim(x, x, lib=lib, **kw)).tolist() == [0, 0, 0]
        assert np.array_equal(bits(f(y, x)), bits(d)) and np.array_equal(bits(f(x, y)), bits(d))
        for i in range(3):
            assert np.array_equal(bits(f(x[i:i + 1], y[i:i + 1])), bits(d[i:i + 1])), i
        perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]
        xb, yb = torch.cat([x, y, x])[perm], torch.cat([y, x, y])[perm]
        assert np.array_equal(bits(f(xb, yb)), bits(torch.cat([d, d, d])[perm]))


def check_mask(L, st, device, hw, window):
    lib = inject(L, device)
    h, w = hw
    x, y = image_case(3, h, w, "noise64")
    win = len(R.window(window)[0])
    p = (win - 1) // 2
    xd, yd = x.to(device), y.to(device)
    score, smap = SS.ssim(xd, yd, window=window, full=True, lib=lib)
    floor = R.ssim_floor(x.reshape(9, h, w), y.reshape(9, h, w), window, 255.0)[0].reshape(3, 3, h - 2 * p, w - 2 * p)
    truth_map = R.conv_maps(x.reshape(9, h, w), y.reshape(9, h, w), window, 255.0)[0].reshape(3, 3, h - 2 * p, w - 2 * p)
    rng = _rng(h, w, 7)
    binary = torch.from_numpy((rng.random((3, 1, h, w)) < 0.4).astype(np.float32))
    frac = torch.from_numpy(rng.random((3, h, w)).astype(np.float32))
    for mask in (binary, binary.bool(), frac, torch.ones(3, 1, h, w)):
        got = SS.ssim(xd, yd, window=window, mask=mask.to(device), lib=lib).cpu()
        crop = mask.reshape(3, h, w)[:, p:h - p, p:w - p].float()
        thr = _rule("noise64", R.masked_mean(floor, crop))
        assert bool(((got - R.masked_mean(truth_map, crop)).abs() <= thr).all()), (got.tolist(), R.masked_mean(truth_map, crop).tolist())
        assert bool(((got - R.masked_mean(smap.cpu(), crop)).abs() <= thr).all())  # the device map's own mean over the kept pixels
    ones = SS.ssim(xd, yd, window=window, mask=torch.ones(3, h, w, device=device), lib=lib)
    assert bool(((ones - score).abs().cpu() <= _rule("noise64", floor.mean((2, 3)).mean(1))).all())
    zero = binary.clone()
    zero[1] = 0.0
    got = SS.ssim(xd, yd, window=window, mask=zero.to(device), lib=lib).cpu()
    assert bool(torch.isnan(got[1])) and bool(torch.isfinite(got[[0, 2]]).all())
    one = SS.ssim(xd[2:], yd[2:], window=window, mask=zero[2:].to(device), lib=lib)  # batch invariance with a mask
    assert np.array_equal(bits(one), bits(got[2:]))


def check_host_refusals(L, st, device):
    lib = inject(L, device)
    x, y = (t.to(device) for t in image_case(3, 33, 47, "noise24"))
    xf, yf = (t.to(device) for t in image_case(3, 33, 47, "unit"))
    raises(ValueError, lambda: SS.ssim(xf, yf, lib=lib), "data_range")
    raises(ValueError, lambda: SS.dssim(xf, yf, lib=lib), "data_range")
    raises(ValueError, lambda: SS.ms_ssim(xf, yf, lib=lib), "data_range")
    raises(ValueError, lambda: SS.ssim(x, y[:2], lib=lib))
    raises(ValueError, lambda: SS.ssim(x, y[:, :, :32], lib=lib))
    raises(ValueError, lambda: SS.ssim(x, yf, lib=lib))
    raises(ValueError, lambda: SS.ssim(x.double(), y.double(), data_range=255.0, lib=lib))
    raises(ValueError, lambda: SS.ssim(x[:, :, :9], y[:, :, :9], lib=lib), "window")
    raises(ValueError, lambda: SS.ssim(x, y, win_size=8, lib=lib), "win_size")
    raises(ValueError, lambda: SS.ssim(x, y, win_size=13, lib=lib), "win_size")
    raises(ValueError, lambda: SS.ssim(x, y, window="box", lib=lib), "window")
    raises(ValueError, lambda: SS.ssim(x, y, mask=torch.ones(3, 33, 46, device=device), lib=lib), "mask")
    raises(ValueError, lambda: SS.ssim(x, y, mask=torch.ones(3, 3, 33, 47, device=device), lib=lib), "mask")
    elsewhere = torch.device("cpu" if device.type != "cpu" else "meta")  # a mask on another device is refused before any launch
    raises(ValueError, lambda: SS.ssim(x, y, mask=torch.ones(3, 33, 47, device=elsewhere), lib=lib), "mask is on")
    raises(ValueError, lambda: M.ssim_planes(L, st, x, y, torch.ones(7, dtype=torch.float64, device=device) / 7, 1.0, 1.0, 1.0,
                                             mask=torch.ones(3, 27, 41, device=elsewhere)), "mask must be")
    raises(ValueError, lambda: SS.ms_ssim(x, y, lib=lib), "too small")
    raises(ValueError, lambda: SS.ms_ssim(x, y, weights=(0.3, 0.3, 0.4), lib=lib), "too small")  # 33 // 4 = 8 < 11
    assert SS.ms_ssim(x, y, weights=(0.3, 0.3, 0.4), window="uniform", lib=lib).shape == (3,)    # 8 >= 7
    raises(ValueError, lambda: SS.ms_ssim(x, y, weights=(0.5, 0.5), mask=torch.ones(3, 33, 47, device=device), lib=lib), "mask")


# ---- MS-SSIM --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ms_case(hw, noise):
    h, w = hw
    rng = _rng(h, w, noise, 5)
    base = structured(rng, 3, h, w)
    other = np.clip(base + rng.integers(-noise, noise + 1, base.shape), 0, 255)
    return torch.from_numpy(base.astype(np.uint8))[None], torch.from_numpy(other.astype(np.uint8))[None]


def ms_ssim_scipy(x, y, kind, weights):
    """The scipy twin of ssim_ref.ms_ssim: scipy_maps per scale, numpy 2x2 means between."""
    n, c, h, w = x.shape
    a, b = x.reshape(n * c, h, w).double().numpy(), y.reshape(n * c, h, w).double().numpy()
    prod = np.ones(n * c)
    for j, wt in enumerate(weights):
        s, cs = R.scipy_maps(a, b, kind, 255.0)
        prod = prod * np.maximum((s if j == len(weights) - 1 else cs).mean((1, 2)), 0.0) ** wt
        a, b = (t[:, :t.shape[1] // 2 * 2, :t.shape[2] // 2 * 2] for t in (a, b))
        a, b = ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]) / 4 for t in (a, b))
    return torch.from_numpy(prod.reshape(n, c).mean(1))


@functools.lru_cache(maxsize=None)
def ms_truth(hw, weights, kind, noise):
    """-> (value [1], floor [1])."""
    x, y = ms_case(hw, noise)
    value = R.ms_ssim(x, y, kind, 255.0, weights)
    a, b = x[0].double()[:, None], y[0].double()[:, None]
    rel = torch.zeros(3, dtype=torch.float64)
    for j, wt in enumerate(weights):
        last = j == len(weights) - 1
        v = R.conv_maps(a[:, 0], b[:, 0], kind, 255.0)[0 if last else 1].mean((1, 2))
        fl = R.ssim_floor(a[:, 0], b[:, 0], kind, 255.0)[0 if last else 1].mean((1, 2))
        rel = rel + wt * fl / v.clamp_min(1e-300)
        a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return value, value * (float(rel.max()) + 4 * len(weights) * R.U64)


def check_ms_ssim(L, st, device, hw, weights, kind):
    lib = inject(L, device)
    for noise in MS_NOISES:
        x, y = ms_case(hw, noise)
        truth, floor = ms_truth(hw, weights, kind, noise)
        got = SS.ms_ssim(x.to(device), y.to(device), weights=weights, window=kind, lib=lib)
        assert got.shape == (1,) and got.dtype == torch.float64
        err, thr = float((got.cpu() - truth).abs()), max(8.0 * MS_D, float(floor))
        print(f"ms_ssim {hw} {len(weights)} scales {kind} noise {noise}: {float(truth):.6f} err {err:.3e} thr {thr:.3e}")
        assert err <= thr, (hw, noise, err, thr)
    xd, yd = (t.to(device) for t in ms_case(hw, MS_NOISES[1]))
    f = lambda a, b: SS.ms_ssim(a, b, weights=weights, window=kind, lib=lib)  # noqa: E731
    assert bits(f(xd, xd)).tolist() == bits(torch.ones(1, dtype=torch.float64)).tolist()
    assert bits(f(xd, 255 - xd)).tolist() == [0]  # negative cs: the clamp is taken
    if hw[0] <= 64:  # batch invariance: 1 against 3 against a permuted 9
        d = f(torch.cat([xd, yd, xd]), torch.cat([yd, xd, 255 - xd]))
        assert np.array_equal(bits(d[:1]), bits(f(xd, yd))) and np.array_equal(bits(d[1:2]), bits(d[:1])) and bits(d[2:]).tolist() == [0]
        perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]
        xb, yb = torch.cat([xd, yd, xd] * 3)[perm], torch.cat([yd, xd, 255 - xd] * 3)[perm]
        assert np.array_equal(bits(f(xb, yb)), bits(torch.cat([d, d, d])[perm]))


# ---- command line ---------------------------------------------------------------------------------------------------
def check_cli(L, st, device, root, decoder="pil"):
    """--mode ssim with both windows on the six PNGs of lpips_checks.write_pairs at --size 64, --mode ms_ssim at --size 176 on
    two of them: keys in file order, values equal to direct calls at the command line's batches, the stat text's format; the
    lpips / l2 / psnr outputs as before (lpips_checks.check_cli, run first: it writes the files)."""
    LK.check_cli(L, st, device, root, decoder)
    lib = inject(L, device)
    data, gt = os.path.join(root, "results"), os.path.join(root, "gt_images")
    names = [n for n, _ in LK.CLI_FILES]
    common = ["--data_path", data, "--gt_path", gt, "--batch", "4", "--image_decoder", decoder]
    res, truth = LP.load_pairs(data, gt, names, 64, decoder, device, lib)
    seen = {}
    for window in ("gaussian", "uniform"):
        scores = LP.main(["--mode", "ssim", "--ssim_window", window, "--size", "64"] + common, lib=lib, device=device)
        want = torch.cat([SS.ssim(res[:4], truth[:4], window=window, lib=lib), SS.ssim(res[4:], truth[4:], window=window, lib=lib)]).cpu().tolist()
        saved, stat = read_scores(root, "ssim")
        assert list(saved) == names == list(scores) and [saved[n] for n in names] == want, window
        assert stat == "Average ssim is {:.4f}+-{:.4f}".format(np.mean(want), np.std(want))
        assert all(0.2 < v < 1.0 for v in want) and len(set(want)) == 6
        seen[window] = want
    assert seen["gaussian"] != seen["uniform"]
    assert LP.main(["--mode", "ssim", "--size", "64"] + common, lib=lib, device=device) == dict(zip(names, seen["gaussian"]))  # the default
    two = os.path.join(root, "two")
    for folder in ("results", "gt_images"):
        os.makedirs(os.path.join(two, folder))
        for name in names[:2]:
            with open(os.path.join(root, folder, name), "rb") as src, open(os.path.join(two, folder, name), "wb") as dst:
                dst.write(src.read())
    data2, gt2 = os.path.join(two, "results"), os.path.join(two, "gt_images")
    scores = LP.main(["--mode", "ms_ssim", "--size", "176", "--data_path", data2, "--gt_path", gt2, "--image_decoder", decoder], lib=lib, device=device)
    res2, truth2 = LP.load_pairs(data2, gt2, names[:2], 176, decoder, device, lib)
    want = SS.ms_ssim(res2, truth2, lib=lib).cpu().tolist()
    saved, stat = read_scores(two, "ms_ssim")
    assert list(saved) == names[:2] == list(scores) and [saved[n] for n in names[:2]] == want
    assert stat == "Average ms_ssim is {:.4f}+-{:.4f}".format(np.mean(want), np.std(want))
    assert all(0.5 < v < 1.0 for v in want)
