"""TEST INFRASTRUCTURE - the checks of the Frechet-distance path (csrc/frechet.h, hairfastgan_amd.metrics) against the numpy
and mpmath restatements (tests/frechet_ref.py), shared by the hipsim tests (tests/test_sim_frechet.py) and the GPU tests
(tests/test_gpu_frechet.py): every function takes the library, the stream and the device to run on.

Rules.
  statistics   bit equality with the sequential fp64 loops (every output has one owner that adds in ascending n; the
               product of two fp32 values is exact in fp64, so a fused multiply-add rounds like multiply-then-add).
  eigenvalues  max |w - truth| (both sorted) <= thr * |A|_2; truth = mpmath at 60 digits for d <= 40, numpy eigvalsh above.
               thr = max(8 * the largest error of numpy's eigvalsh against mpmath in the matrix family, 64 d eps); the second
               term is the solver's own rounding: about 10 sweeps of d - 1 rotations per element, a few eps each.
               Measured numpy errors (d = 1, 2, 3, 24, 37; EIG_MEASURED rounds them up): diagonal 0, spread 4.5e-16,
               rank_deficient 5.1e-16, cluster 1.2e-15, zero_row 4.8e-16 - the floor 64 d eps (1.4e-14 at d = 1, 5.3e-13 at
               d = 37) decides everywhere.  max |V diag(w) V^T - A| <= 64 d eps |A|_2 and max |V^T V - I| <= 64 d eps by the
               same count of rotations.
  distance     |device - truth| <= thr * max(1, |truth|); truth = mpmath for d <= 40, above it the symmetric fp64 route
               (the two fp64 routes' disagreement stands in for the error of numpy there).
               thr = max(8 * the largest error of the two numpy routes in the family, 64 d eps).  Measured (a, b) and (b, a):
                 full rank       (24,67,130) 0.2 - 1.3e-15, (37,130,67) 2.1 - 7.7e-15          -> 8 x 7.8e-15 < floor: thr =
                                 3.4e-13 (d = 24), 5.3e-13 (d = 37); sanity cap 1e-11
                 rank deficient  (40,5,67) 0.80 - 1.52e-8; routes differ by 1.36e-8 at (130,67,40) and 1.07e-8 at
                                 (512,300,700)                                                   -> thr = 1.22e-7; cap 1e-6
               (the square root of noise-level eigenvalues limits every fp64 method there).  tests/test_frechet_ref.py
               measures these again and fails if one exceeds what is recorded here.
"""
import csv
import ctypes
import functools
import os

import numpy as np
import PIL.Image
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import metrics as MT
from tests import frechet_ref as R
from tests.metric_common import bits, inject, raises

EPS = R.EPS
MAX_SWEEPS = 30

ACCUMULATE_SHAPES = ((1, 1), (5, 3), (67, 24), (130, 37), (3, 130), (16, 512))  # (n, d)
EIG_SIZES = (1, 2, 3, 24, 37, 130)
EIG_MEASURED = {"diagonal": 0.0, "spread": 4.6e-16, "rank_deficient": 5.1e-16, "cluster": 1.2e-15, "zero_row": 4.8e-16}
DIST_CASES = {(24, 67, 130): "full", (37, 130, 67): "full", (40, 5, 67): "deficient", (130, 67, 40): "deficient"}
DIST_CASE_GPU = ((512, 300, 700), "deficient")
DIST_MEASURED = {"full": 7.8e-15, "deficient": 1.53e-8}
DIST_CAP = {"full": 1e-11, "deficient": 1e-6}


def eig_threshold(family, d):
    return max(8.0 * EIG_MEASURED[family], 64.0 * d * EPS)


def dist_threshold(family, d):
    thr = max(8.0 * DIST_MEASURED[family], 64.0 * d * EPS)
    assert thr <= DIST_CAP[family]
    return thr


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)  # a copy: the references are read-only


def _same_bits(t, ref):
    return np.array_equal(bits(t), np.ascontiguousarray(ref).view(np.uint64))


# ---- statistics ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stat_features(n, d):
    f = np.random.default_rng(100 * n + d).standard_normal((n, d)).astype(np.float32) * 3.0 + 0.5
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def stat_reference(n, d):
    total, cov_sum = R.stats(stat_features(n, d))
    return total, cov_sum


def _accumulate(L, st, device, slices):
    d = slices[0].shape[1]
    total = torch.zeros(d, dtype=torch.float64, device=device)
    cov_sum = torch.zeros((d, d), dtype=torch.float64, device=device)
    for f in slices:
        M.frechet_accumulate_into(L, st, total, cov_sum, f)
    return total, cov_sum


def check_accumulate(L, st, device, n, d):
    """One update against the sequential loops, bit for bit; cov_sum symmetric; then mu / cov of hf_frechet_stats_f64."""
    f = stat_features(n, d)
    ref_total, ref_cov = stat_reference(n, d)
    total, cov_sum = _accumulate(L, st, device, [_dev(f, device)])
    assert _same_bits(total, ref_total), (n, d)
    assert _same_bits(cov_sum, ref_cov), (n, d, float((cov_sum.cpu() - torch.from_numpy(ref_cov)).abs().max()))
    assert torch.equal(cov_sum, cov_sum.t())
    if n >= 2:
        mu, cov = M.frechet_stats(L, st, total, cov_sum, n)
        ref_mu, ref_s = R.moments(ref_total, ref_cov, n)
        assert _same_bits(mu, ref_mu) and _same_bits(cov, ref_s), (n, d)
        assert torch.equal(cov, cov.t())


def check_accumulate_split(L, st, device):
    """Updates of 64 and 66 samples give the bits of one update of 130; a non-contiguous slice is taken too."""
    f = _dev(stat_features(130, 37), device)
    whole = _accumulate(L, st, device, [f])
    parts = _accumulate(L, st, device, [f[:64], f[64:]])
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    assert _same_bits(parts[1], stat_reference(130, 37)[1])
    wide = torch.cat([f, f], dim=1)[:, :37]  # a view with a row stride of 74
    assert not wide.is_contiguous()
    again = _accumulate(L, st, device, [wide])
    assert torch.equal(again[1], whole[1])


def check_accumulate_f16(L, st, device):
    """fp16 features give the bits of their fp32 upcast."""
    h = _dev(stat_features(67, 24), device).half()
    a = _accumulate(L, st, device, [h])
    b = _accumulate(L, st, device, [h.float()])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert _same_bits(a[1], R.stats(h.cpu().numpy())[1])


def check_reset(L, st, device):
    """The real side survives reset() under reset_real_features=False only."""
    f = _dev(stat_features(67, 24), device)
    for keep in (False, True):
        fid = MT.FrechetDistance(lambda x: x, reset_real_features=not keep, lib=inject(L, device))
        assert fid.to(device) is fid and fid.eval() is fid
        fid.update(f, real=True)  # through the feature callable
        fid.update_features(f[:5], real=False)
        total, cov_sum, n = fid.state(True)
        assert _same_bits(cov_sum, stat_reference(67, 24)[1]) and int(n) == 67 and n.device.type == device.type
        assert total.dtype == torch.float64 and cov_sum.dtype == torch.float64
        fid.reset()
        assert fid.state(False) is None
        assert (fid.state(True) is not None) == keep
        if keep:
            assert torch.equal(fid.state(True)[1], cov_sum)


# ---- eigensolver --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eig_truth(family, d):
    a = R.eig_matrix(family, d)
    return R.eigh_truth(a) if d <= R.MP_MAX_D else np.linalg.eigvalsh(a)


def check_eigh(L, st, device, family, d):
    a = R.eig_matrix(family, d)
    truth = eig_truth(family, d)
    norm2 = float(np.abs(truth).max()) or 1.0
    thr = eig_threshold(family, d)
    info = {}
    w, v = M.sym_eigh_f64(L, st, _dev(a, device), True, MAX_SWEEPS, info)
    w, v = w.cpu().numpy(), v.cpu().numpy()
    err = float(np.abs(np.sort(w) - truth).max()) / norm2
    resid = float(np.abs((v * w) @ v.T - a).max()) / norm2
    ortho = float(np.abs(v.T @ v - np.eye(d)).max())
    print(f"eigh {family} d={d}: sweeps {info['sweeps']} err {err:.3e} resid {resid:.3e} ortho {ortho:.3e} thr {thr:.3e}")
    assert 0 <= info["sweeps"] < MAX_SWEEPS, info
    if family == "diagonal":
        assert info["sweeps"] == 0 and np.array_equal(w, np.diag(a)) and np.array_equal(v, np.eye(d))  # no rotation is taken
    assert err <= thr, (family, d, err, thr)
    assert resid <= 64.0 * d * EPS and ortho <= 64.0 * d * EPS, (family, d, resid, ortho)
    w0, none = M.sym_eigh_f64(L, st, _dev(a, device), False, MAX_SWEEPS)  # without vectors: the same rotations
    assert none is None and np.array_equal(w0.cpu().numpy(), w)
    ws, vs = MT.sym_eigh(_dev(a, device), lib=inject(L, device))  # the public form: ascending, columns permuted alike
    assert np.array_equal(ws.cpu().numpy(), np.sort(w)) and np.array_equal(vs.cpu().numpy(), v[:, np.argsort(w, kind="stable")])


# ---- distance -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dist_reference(d, n1, n2, pair):
    """pair 'ab' / 'ba' / 'aa' -> (truth, fp64 symmetric route, fp64 eigvals route); truth is None above d = 40."""
    f1, f2 = R.features(d, n1, n2)
    g = {"a": R.gaussian(f1), "b": R.gaussian(f2)}
    args = (*g[pair[0]], *g[pair[1]])
    return (R.fid_truth(*args) if d <= R.MP_MAX_D else None), R.fid_symmetric(*args), R.fid_eigvals(*args)


def _distance(L, st, device, fa, fb, chunk=64):
    fid = MT.FrechetDistance(lambda x: x, lib=inject(L, device))
    for side, f in ((True, fa), (False, fb)):
        t = _dev(f, device)
        for k in range(0, t.shape[0], chunk):
            fid.update_features(t[k:k + chunk], real=side)
    out = fid.compute()
    assert out.dtype == torch.float64 and out.ndim == 0 and out.device.type == device.type
    assert all(0 <= s < MAX_SWEEPS for s in fid.last_info["sweeps"]), fid.last_info
    return float(out), fid


def check_distance(L, st, device, d, n1, n2, family):
    """FID(a, b) against the truth; FID(b, a) agrees with it; FID(a, a) is 0 - all within the family's threshold."""
    f1, f2 = R.features(d, n1, n2)
    thr = dist_threshold(family, d)
    truth, sym, _ = dist_reference(d, n1, n2, "ab")
    want = truth if truth is not None else sym
    scale = max(1.0, abs(want))
    ab, fid = _distance(L, st, device, f1, f2)
    print(f"distance ({d},{n1},{n2}) {family}: device {ab:.15g} want {want:.15g} err {abs(ab - want) / scale:.3e} thr {thr:.3e} "
          f"sweeps {fid.last_info['sweeps']}")
    assert abs(ab - want) <= thr * scale, (ab, want, abs(ab - want) / scale, thr)
    ba, _ = _distance(L, st, device, f2, f1)
    print(f"  (b,a) differs by {abs(ab - ba) / scale:.3e}")
    assert abs(ab - ba) <= thr * scale, (ab, ba)
    aa, _ = _distance(L, st, device, f1, f1)
    print(f"  (a,a) = {aa:.3e}")
    assert abs(aa) <= thr, aa  # not clamped: it may be negative
    # the functional form on the same statistics
    mu1, s1 = M.frechet_stats(L, st, *fid.state(True)[:2], n1)
    mu2, s2 = M.frechet_stats(L, st, *fid.state(False)[:2], n2)
    assert float(MT.frechet_distance(mu1, s1, mu2, s2, lib=inject(L, device))) == ab


# ---- front end ----------------------------------------------------------------------------------------------------
class RecordingTower:
    """A stand-in for the CLIP tower: keeps its input, returns a fixed linear projection of a 7 x 7 pooling of it."""

    def __init__(self, device, out_dim=12):
        g = torch.Generator().manual_seed(5)
        self.weight = torch.randn(3 * 49, out_dim, generator=g).to(device)
        self.seen = None

    def encode_image(self, image):
        self.seen = image
        return torch.nn.functional.avg_pool2d(image, 32).reshape(image.shape[0], -1) @ self.weight


def check_clip_model(L, st, device):
    """ClipModel on uint8 [2,3,299,299]: the tower receives torch's pooled and normalised input (to fp32 rounding of a
    window mean: windows of at most 3 x 3 values in [0,1], 2^-21 absolute, divided by std >= 0.26) and its output is returned."""
    images = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 3, 299, 299), dtype=np.uint8)).to(device)
    tower = RecordingTower(device)
    out = MT.ClipModel(tower, lib=inject(L, device))(images)
    x = torch.nn.functional.adaptive_avg_pool2d(images.cpu().float() / 255, (224, 224))
    mean = torch.tensor(MT.CLIP_MEAN)[None, :, None, None]
    std = torch.tensor(MT.CLIP_STD)[None, :, None, None]
    want = (x - mean) / std
    assert tower.seen.shape == (2, 3, 224, 224) and tower.seen.dtype == torch.float32
    assert float((tower.seen.cpu() - want).abs().max()) <= 2.0 ** -21 / 0.26
    assert torch.equal(out, RecordingTower(device).encode_image(tower.seen))
    floats = MT.ClipModel(tower, lib=inject(L, device))(images.float() / 255)  # [0,1] floats are taken as they are
    assert float((floats - out).abs().max()) <= 1e-4 * float(out.abs().max())


FILES = (("b.png", (40, 31)), ("a.JPG", (64, 48)), ("c.jpeg", (299, 299)), ("d.PNG", (350, 300)), ("e.jpg", (17, 23)))


def write_images(directory, seed=0):
    """Five small RGB files (PNG and JPEG, extensions in both letter cases) plus two that are no images -> sorted names."""
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(50 + seed)
    for name, (w, h) in FILES:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255 // w + seed * 40) % 256, (yy * 255 // h), (xx + yy) % 256], -1) + rng.integers(-20, 20, (h, w, 3))
        fmt = "PNG" if name.lower().endswith("png") else "JPEG"
        PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(os.path.join(directory, name), format=fmt)
    with open(os.path.join(directory, "notes.txt"), "w") as f:
        f.write("not an image\n")
    os.makedirs(os.path.join(directory, "sub.png"), exist_ok=True)  # a directory is no file
    return sorted(name for name, _ in FILES)


def check_files(L, st, device, directory, decoder="pil"):
    names = write_images(directory)
    assert MT.list_image_files(directory) == names == ["a.JPG", "b.png", "c.jpeg", "d.PNG", "e.jpg"]
    got = MT.load_images_299(directory, names, decoder=decoder, device=device, lib=inject(L, device))
    assert got.shape == (5, 3, 299, 299) and got.dtype == torch.uint8 and got.device.type == device.type
    for k, name in enumerate(names):
        ref = np.asarray(PIL.Image.open(os.path.join(directory, name)).resize((299, 299), PIL.Image.LANCZOS))
        assert np.array_equal(got[k].cpu().numpy().transpose(1, 2, 0), ref), name
    assert MT.load_images_299(directory, [], device=device, lib=inject(L, device)).shape == (0, 3, 299, 299)


def check_cli(L, st, device, root):
    """The command line with a linear projection as the feature: the CSV holds the rounded distances of the fp64 route."""
    dirs = {name: os.path.join(root, name) for name in ("real", "method_a", "method_b")}
    for k, d in enumerate(dirs.values()):
        write_images(d, seed=k)
    g = torch.Generator().manual_seed(9)
    proj = torch.randn(3 * 16, 6, generator=g).to(device) / 255

    def feature(images):  # [N,3,299,299] uint8 -> [N,6]
        return torch.nn.functional.adaptive_avg_pool2d(images.float(), 4).reshape(images.shape[0], -1) @ proj

    out = os.path.join(root, "logs", "metric.csv")
    argv = ["--source_dataset", dirs["real"], "--methods_dataset", f"A,{dirs['method_a']}", f"B,{dirs['method_b']}", "--output", out,
            "--batch", "2"]
    fids = MT.main(argv, feature=feature, lib=inject(L, device), device=device)
    assert list(fids) == ["A", "B"]
    want = {}
    real = feature(MT.load_images_299(dirs["real"], MT.list_image_files(dirs["real"]), device=device, lib=inject(L, device)))
    for name, key in (("A", "method_a"), ("B", "method_b")):
        fake = feature(MT.load_images_299(dirs[key], MT.list_image_files(dirs[key]), device=device, lib=inject(L, device)))
        want[name] = R.fid_symmetric(*R.gaussian(real.cpu().numpy()), *R.gaussian(fake.cpu().numpy()))
        assert abs(fids[name] - want[name]) <= dist_threshold("deficient", 6) * max(1.0, abs(want[name])), (fids[name], want[name])
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [["", "FID_CLIP"]] + [[name, str(round(fids[name], 2))] for name in ("A", "B")]
    assert all(abs(float(r[1]) - want[r[0]]) <= 0.005 + 1e-9 for r in rows[1:])


# ---- error paths --------------------------------------------------------------------------------------------------
def check_errors(L, st, device):
    lib = inject(L, device)
    raises(NotImplementedError, lambda: MT.FrechetDistance(2048), "Inception")
    raises(NotImplementedError, lambda: MT.FrechetDistance(feature=64))
    f = _dev(stat_features(67, 24), device)
    fid = MT.FrechetDistance(lambda x: x, lib=lib)
    raises(RuntimeError, fid.compute, "More than one sample")
    fid.update_features(f, real=True)
    fid.update_features(f[:1], real=False)
    raises(RuntimeError, fid.compute, "More than one sample")  # one sample on the fake side
    raises(ValueError, lambda: fid.update_features(_dev(stat_features(5, 3), device), real=False), "dimension")
    raises(ValueError, lambda: fid.update_features(f[0], real=False))
    raises(ValueError, lambda: MT.frechet_distance(torch.zeros(3, device=device), torch.eye(3, device=device),
                                                   torch.zeros(4, device=device), torch.eye(4, device=device), lib=lib))
    dense = _dev(R.eig_matrix("spread", 24), device)
    raises(RuntimeError, lambda: M.sym_eigh_f64(L, st, dense, True, 1), "no convergence in 1 sweeps")
    # the C entry points: a null or misaligned pointer is an invalid argument, and nothing is launched
    d = 8
    buf = torch.zeros(4 * d * d + 64, dtype=torch.float64, device=device)
    feats = torch.ones((4, d), dtype=torch.float32, device=device)
    p, odd = buf.data_ptr(), buf.data_ptr() + 4
    sweeps, off = ctypes.c_int(0), ctypes.c_double(0.0)
    calls = []
    for bad in (None, odd):
        calls += [lambda b=bad: L.hf_frechet_accumulate_f64(b, p, feats.data_ptr(), 4, d, st),
                  lambda b=bad: L.hf_frechet_accumulate_f64(p, b, feats.data_ptr(), 4, d, st),
                  lambda b=bad: L.hf_frechet_stats_f64(b, p, p, p, 4, d, st),
                  lambda b=bad: L.hf_sym_eig_jacobi_f64(b, None, p, p, d, 30, ctypes.byref(sweeps), ctypes.byref(off), st),
                  lambda b=bad: L.hf_sym_eig_jacobi_f64(p, None, b, p, d, 30, ctypes.byref(sweeps), ctypes.byref(off), st),
                  lambda b=bad: L.hf_sym_eig_jacobi_f64(p, None, p, b, d, 30, ctypes.byref(sweeps), ctypes.byref(off), st),
                  lambda b=bad: L.hf_frechet_congruence_f64(p, p, p, b, p, d, st),
                  lambda b=bad: L.hf_frechet_finish_f64(b, p, p, p, p, p, d, st)]
    calls += [lambda: L.hf_frechet_accumulate_f64(p, p, None, 4, d, st),
              lambda: L.hf_frechet_accumulate_f64(p, p, feats.data_ptr() + 2, 4, d, st),
              lambda: L.hf_frechet_accumulate_f64(p, p, feats.data_ptr(), 0, d, st),
              lambda: L.hf_frechet_stats_f64(p, p, p, p, 1, d, st),
              lambda: L.hf_sym_eig_jacobi_f64(p, odd, p, p, d, 30, ctypes.byref(sweeps), ctypes.byref(off), st),
              lambda: L.hf_sym_eig_jacobi_f64(p, None, p, p, d, 0, ctypes.byref(sweeps), ctypes.byref(off), st),
              lambda: L.hf_sym_eig_jacobi_f64(p, None, p, p, 0, 30, ctypes.byref(sweeps), ctypes.byref(off), st)]
    for k, call in enumerate(calls):
        code = call()
        assert L.hf_strerror(code) == b"invalid argument", (k, code)
    if device.type == "cuda":
        torch.cuda.synchronize()
    assert not buf.any()
