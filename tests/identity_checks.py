"""TEST INFRASTRUCTURE - the checks of the identity-similarity path (csrc/identity.h, hairfastgan_amd.identity) against the
torch / numpy restatements (tests/identity_ref.py), shared by the hipsim tests (tests/test_sim_identity.py) and the GPU tests
(tests/test_gpu_identity.py): every function takes the library, the stream and the device to run on.

Rules.
  crop and pool  the bits of the fp32 restatement of the kernel's stated order (identity_ref.crop_avgpool_ordered), and
                 |out - truth| <= (n + 2) 2^-24 max|window| against the fp64 mean of a window of n pixels: n - 1 additions of
                 terms bounded by the maximum, divided by n, leave (n - 1) u max; the division adds u / 2 (+ spare).  With the
                 affine: |scale| times that, plus one rounding of the fused multiply-add, u (|scale mean| + |shift|).
  normalise      |out - truth| <= 2 u |truth| per element: the sum of squares is fp64, so the norm carries the one rounding of
                 the square root to fp32 (u / 2), the division another (u / 2), products of the two (spare).  A row's bits are
                 the same in a launch of 1 row and of 3.
  similarity     |out - numpy| <= 4 D 2^-53 sum_k |a_k b_k| (both sum D exact products in fp64, in different orders: at most
                 (D - 1) 2^-53 each, relative to the sum of magnitudes); the paired form and the matrix diagonal: equal bits.
  network        |embedding - truth| <= max(8 x the error of the same network evaluated in fp32 by torch on the CPU, floor) per
                 component of the unit row, the 8 x allowing for a different but equally valid summation order and for the
                 f16x3 operand split (22-bit products: the class of an fp32 reassociation).  floor = 3 u max|component|: the
                 error of the LAST stage alone on an embedding that is only known as fp32 numbers - each component rounded
                 (u / 2), hence the norm (u / 2 at most), the norm's own rounding (u / 2), the division (u / 2), + spare.  The
                 floor is about 3e-8 against 8 x 2e-7: the first term decides everywhere; it is there so that a case whose fp32
                 error happens to be tiny cannot demand more than the format gives.
                 Similarities: max(8 x the fp32 error of the similarity, 6 u): two unit rows with 3 u each.
                 fp32 errors of torch on the CPU (test_identity_ref.py measures them again; recorded with a third added, since
                 torch's summation order follows its thread count and vector width):
                   IR-SE50 at 112^2, four 256^2 images   component 2.1e-7 (largest component 0.19)   similarity 1.2e-7
                   two units at 28^2, two 40^2 images    component 9.0e-8                           similarity 7.4e-8
                   one unit at 14^2, the same images     component 5.6e-8                           similarity 4.9e-8
                 Device errors measured on the MI355X are recorded in DESIGN.md 4.28 with their ratios to these figures.
"""
import functools
import os

import numpy as np
import PIL.Image
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import _runtime
from hairfastgan_amd import identity as ID
from tests import identity_ref as R
from tests.metric_common import bits, inject, raises, read_scores

U32 = R.U32
EPS64 = 2.0 ** -53

#             name        n  c  h    w    (y0, x0, ch, cw)     oh   ow   affine
POOL_CASES = (("real", 1, 3, 256, 256, (35, 32, 188, 188), 112, 112, False),
              ("unequal", 1, 2, 11, 13, (2, 3, 7, 9), 4, 5, False),     # overlapping windows of 2 x 2, 2 x 3, 3 x 2 and 3 x 3
              ("identity", 1, 1, 9, 10, (1, 2, 6, 7), 6, 7, False),     # output size = crop size
              ("one_bin", 1, 2, 12, 13, (2, 1, 9, 11), 1, 1, False),    # a window of 99 pixels
              ("flush", 1, 1, 11, 13, (4, 5, 7, 8), 3, 3, False),       # the crop ends with the last row and column
              ("affine", 2, 3, 11, 13, (2, 3, 7, 9), 4, 5, True))
NORM_DIMS = (512, 5)
SMALL_UNITS = ((64, 64, 2), (64, 128, 2))   # planes 28, 14 and 7
SMALL_SIZE, SMALL_IMAGE, SMALL_CROP = 28, 40, (4, 5, 30, 31)
TINY_UNITS, TINY_SIZE = ((64, 64, 2),), 14  # planes 14 and 7: what the interpreter can afford for the host-side checks
CLI_CROP = (1, 2, 30, 29)                   # of the command line's 32 x 32 images
EMB_MEASURED = {"full": 2.8e-7, "small": 1.3e-7, "tiny": 7.5e-8}
SIM_MEASURED = {"full": 1.6e-7, "small": 1.0e-7, "tiny": 6.6e-8}
FULL_PAIRS = (1, 2, 3, 0)                   # image i is compared with image FULL_PAIRS[i]


def _rng(*key):
    return np.random.default_rng([23] + [int(v) for v in key])


# ---- crop and pool ------------------------------------------------------------------------------------------------
def check_crop_avgpool(L, st, device, name, n, c, h, w, crop, oh, ow, affine):
    rng = _rng(1, n, c, h, w, oh, ow)
    x = (rng.standard_normal((n, c, h, w)) + 0.5).astype(np.float32)
    scale = (0.5 + rng.random(c)).astype(np.float32) * np.where(np.arange(c) % 2, -1, 1).astype(np.float32) if affine else None
    shift = rng.standard_normal(c).astype(np.float32) if affine else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
    got = M.crop_avgpool(L, st, dev(x), *crop, oh, ow, dev(scale), dev(shift)).cpu().numpy()
    assert got.shape == (n, c, oh, ow) and got.dtype == np.float32
    want = R.crop_avgpool_ordered(x, *crop, oh, ow, scale, shift)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, float(np.abs(got - want).max()))
    truth, count, big = R.crop_avgpool(x, *crop, oh, ow, scale, shift)
    bound = (count[None, None] + 2) * U32 * big
    if affine:
        plain = R.crop_avgpool(x, *crop, oh, ow)[0]
        s64, t64 = scale.astype(np.float64)[None, :, None, None], shift.astype(np.float64)[None, :, None, None]
        bound = np.abs(s64) * bound + U32 * (np.abs(s64 * plain) + np.abs(t64))
    err = np.abs(got.astype(np.float64) - truth)
    print(f"crop_avgpool {name}: windows {int(count.min())}..{int(count.max())} pixels, err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (name, float((err / bound).max()))
    if name == "identity":
        y0, x0, ch, cw = crop
        assert np.array_equal(got, x[:, :, y0:y0 + ch, x0:x0 + cw])
    if name == "real":  # torch's own module on the cropped copy, in fp64
        y0, x0, ch, cw = crop
        ref = torch.nn.AdaptiveAvgPool2d((oh, ow))(torch.from_numpy(x).double()[:, :, y0:y0 + ch, x0:x0 + cw]).numpy()
        assert float(np.abs(truth - ref).max()) <= 1e-14


def check_crop_avgpool_refusals(L, st, device):
    """A window outside the image, a non-positive size, a null or misaligned pointer return HF_E_INVALID."""
    buf = torch.zeros(4096, device=device)
    p = buf.data_ptr()

    def call(out=p, x=p, h=11, w=13, y0=2, x0=3, ch=7, cw=9, oh=4, ow=5, n=1, c=2):
        return L.hf_crop_avgpool_f32(out, x, None, None, n, c, h, w, y0, x0, ch, cw, oh, ow, st)

    assert call() == 0 and call(y0=4, x0=4) == 0
    for kw in (dict(y0=5), dict(x0=5), dict(y0=-1), dict(x0=-1), dict(ch=0), dict(cw=-3), dict(oh=0), dict(ow=0), dict(n=0), dict(c=0),
               dict(h=0), dict(ch=12, y0=0), dict(out=None), dict(x=None), dict(x=p + 2)):
        assert call(**kw) == -1, kw


# ---- normalise ----------------------------------------------------------------------------------------------------
def check_normalize(L, st, device, d):
    x = torch.from_numpy(_rng(2, d).standard_normal((3, d)).astype(np.float32) * np.float32(3.0))
    out, norms = M.l2_normalize_rows(L, st, x.to(device), want_norms=True)
    truth = R.l2_normalize(x)
    err = (out.cpu().double() - truth).abs()
    assert bool((err <= 2 * U32 * truth.abs()).all()), float((err / truth.abs()).max() / U32)
    tn = x.double().norm(dim=1)
    assert bool(((norms.cpu().double() - tn).abs() <= U32 * tn).all())
    for r in range(3):  # a row's bits do not depend on the number of rows
        one = M.l2_normalize_rows(L, st, x[r:r + 1].to(device))
        assert np.array_equal(bits(one), bits(out[r:r + 1])), r
    assert np.array_equal(bits(M.l2_normalize_rows(L, st, x.to(device))), bits(out))
    buf = torch.zeros(64, device=device)
    p = buf.data_ptr()
    assert L.hf_l2_normalize_rows_f32(p, None, p, 2, 5, st) == 0
    for args in ((None, None, p, 2, 5), (p, None, None, 2, 5), (p, p + 2, p, 2, 5), (p, None, p, 0, 5), (p, None, p, 2, 0)):
        assert L.hf_l2_normalize_rows_f32(*args, st) == -1, args


# ---- similarity ---------------------------------------------------------------------------------------------------
def check_similarity(L, st, device):
    for d in NORM_DIMS:
        rng = _rng(3, d)
        a, b = rng.standard_normal((3, d)).astype(np.float32), rng.standard_normal((3, d)).astype(np.float32)
        ta, tb = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
        pair, full = M.row_similarity(L, st, ta, tb), M.row_similarity(L, st, ta, tb, paired=False)
        assert pair.shape == (3,) and full.shape == (3, 3) and pair.dtype == torch.float64
        assert np.array_equal(bits(pair), bits(full.diagonal()))
        assert np.array_equal(bits(M.row_similarity(L, st, ta[1:2], tb[1:2])), bits(pair[1:2]))   # N does not matter
        assert np.array_equal(bits(M.row_similarity(L, st, ta[2:], tb[:2], paired=False)), bits(full[2:, :2]))  # nor M
        a2, b5 = rng.standard_normal((2, d)).astype(np.float32), rng.standard_normal((5, d)).astype(np.float32)
        got = M.row_similarity(L, st, torch.from_numpy(a2).to(device), torch.from_numpy(b5).to(device), paired=False).cpu().numpy()
        mag = np.abs(a2.astype(np.float64)) @ np.abs(b5.astype(np.float64)).T
        err = np.abs(got - R.similarity(a2, b5, paired=False))
        assert got.shape == (2, 5) and (err <= 4 * d * EPS64 * mag).all(), float((err / mag).max() / EPS64)
    raises(ValueError, lambda: M.row_similarity(L, st, ta, tb[:2]))
    buf = torch.zeros(64, dtype=torch.float64, device=device)
    p = buf.data_ptr()
    assert L.hf_row_similarity_f64(p, p, p, 2, 2, 5, 1, st) == 0 and L.hf_row_similarity_f64(p, p, p, 2, 3, 5, 0, st) == 0
    for args in ((p, p, p, 2, 3, 5, 1), (None, p, p, 2, 2, 5, 1), (p + 4, p, p, 2, 2, 5, 1), (p, None, p, 2, 2, 5, 1), (p, p, p + 2, 2, 2, 5, 1),
                 (p, p, p, 0, 0, 5, 1), (p, p, p, 2, 0, 5, 0), (p, p, p, 2, 2, 0, 0)):
        assert L.hf_row_similarity_f64(*args, st) == -1, args


# ---- the network --------------------------------------------------------------------------------------------------
def _case(kind):
    """-> (units, input size, crop, state-dict seed, images)"""
    if kind == "full":
        return None, 112, R.CROP, 0, R.discriminating_images()
    images = R.discriminating_images(SMALL_IMAGE, 3, 1)[[0, 2]].contiguous()
    if kind == "tiny":
        return list(TINY_UNITS), TINY_SIZE, SMALL_CROP, 2, images
    return list(SMALL_UNITS), SMALL_SIZE, SMALL_CROP, 1, images


@functools.lru_cache(maxsize=None)
def state(kind):
    units, size, _, seed, _ = _case(kind)
    return R.discriminating_state(units, size, seed)


@functools.lru_cache(maxsize=None)
def truth(kind, dtype=torch.float64):
    """-> (unit embeddings of the case's images, the same with every residual branch removed) in `dtype` on the CPU."""
    units, size, crop, _, x = _case(kind)
    net = R.network(state(kind), units, size, dtype)
    return R.extract_feats(net, x, crop), R.extract_feats(net, x, crop, shortcut_only=True)


def fp32_errors(kind):
    """(largest component error, largest similarity error over all pairs) of torch's fp32 evaluation on the CPU."""
    f64, f32 = truth(kind)[0], truth(kind, torch.float32)[0].double()
    return float((f32 - f64).abs().max()), float((f32 @ f32.T - f64 @ f64.T).abs().max())


def thresholds(kind):
    """(per component, per similarity): the rule at the top of this file."""
    return max(8.0 * EMB_MEASURED[kind], 3 * U32 * float(truth(kind)[0].abs().max())), max(8.0 * SIM_MEASURED[kind], 6 * U32)


def make_idloss(L, device, kind, models={}):
    key = (kind, device.type)
    if key not in models:
        units, size, crop, _, _ = _case(kind)
        net = ID.Backbone(size, units=units)
        net.load_state_dict(state(kind))
        models[key] = ID.IDLoss(net.to(device), lib=inject(L, device), crop=crop)
    models[key].facenet.invalidate()  # the plan follows the precision mode of its first call
    return models[key]


def check_network(L, st, device, kind, every_row=True):
    """Embeddings and similarities of the case's images against the fp64 restatement; a row of the batch has the bits of a
    single-image call (every_row: all of them, else the first); two calls give equal bits."""
    x = _case(kind)[4].to(device)
    idl = make_idloss(L, device, kind)
    want = truth(kind)[0]
    thr_c, thr_s = thresholds(kind)
    got = idl.extract_feats(x)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.device.type == device.type
    err = float((got.cpu().double() - want).abs().max())
    print(f"identity {kind} {_runtime.conv_precision()}: component err {err:.3e} thr {thr_c:.3e} ({err / EMB_MEASURED[kind]:.2f} x fp32)")
    assert err <= thr_c, (kind, err, thr_c)
    assert float((got.cpu().double().norm(dim=1) - 1).abs().max()) <= 4 * U32
    full = M.row_similarity(L, st, got, got, paired=False).cpu()
    serr = float((full - want @ want.T).abs().max())
    print(f"identity {kind} {_runtime.conv_precision()}: similarity err {serr:.3e} thr {thr_s:.3e} ({serr / SIM_MEASURED[kind]:.2f} x fp32)")
    assert serr <= thr_s, (kind, serr, thr_s)
    assert float((full.diagonal() - 1).abs().max()) <= 2.0 ** -22
    for i in range(x.shape[0] if every_row else 1):
        assert np.array_equal(bits(idl.extract_feats(x[i:i + 1])), bits(got[i:i + 1])), i
    return got


def check_full_conditions():
    """The fp64 restatement itself discriminates: a near-identical pair, a pair of different images, and an embedding that
    the residual branches decide (a network that dropped them would be found)."""
    want, shortcut = truth("full")
    pairs = (want * want[list(FULL_PAIRS)]).sum(1)
    assert float(pairs.max()) >= 0.99 and float(pairs.min()) <= 0.75, pairs.tolist()
    assert float((want * shortcut).sum(1).abs().max()) <= 0.5


def check_similarity_full(L, st, device):
    """IDLoss.similarity on the four 256^2 images (image i against image FULL_PAIRS[i]) and on equal inputs."""
    x = _case("full")[4].to(device)
    idl = make_idloss(L, device, "full")
    want = truth("full")[0]
    thr_s = thresholds("full")[1]
    y = x[list(FULL_PAIRS)].contiguous()
    got = idl.similarity(x, y)
    ref = (want * want[list(FULL_PAIRS)]).sum(1)
    err = float((got.cpu() - ref).abs().max())
    print(f"identity similarity {_runtime.conv_precision()}: {got.tolist()} err {err:.3e} thr {thr_s:.3e} ({err / SIM_MEASURED['full']:.2f} x fp32)")
    assert got.shape == (4,) and got.dtype == torch.float64 and err <= thr_s, (err, thr_s)
    same = idl.similarity(x, x.clone())
    assert float((same.cpu() - 1).abs().max()) <= 2.0 ** -22
    assert np.array_equal(bits(idl.extract_feats(x)), bits(idl.extract_feats(x.clone())))
    mat = idl.similarity_matrix(x[:2], x)
    assert mat.shape == (2, 4) and float((mat.cpu() - want[:2] @ want.T).abs().max()) <= thr_s


def check_forward(L, st, device, kind):
    """Both forms of forward against the reference's loops in fp64."""
    units, size, crop, _, x = _case(kind)
    idl = make_idloss(L, device, kind)
    net = R.network(state(kind), units, size)
    thr_s = thresholds(kind)[1]
    order = list(range(1, x.shape[0])) + [0]
    y_hat, y, src = x, x[order].contiguous(), x.flip(0).contiguous()
    loss = idl(y_hat.to(device), y.to(device))
    want = float(R.id_loss(net, y_hat, y, crop=crop))
    assert loss.ndim == 0 and loss.dtype == torch.float32 and abs(float(loss) - want) <= thr_s + U32 * abs(want), (float(loss), want)
    loss3, improvement, logs = idl(y_hat.to(device), y.to(device), src.to(device))
    w_loss, w_imp, w_logs = R.id_loss(net, y_hat, y, src, crop=crop)
    assert torch.equal(loss3, loss) and abs(improvement - w_imp) <= 2 * thr_s
    assert len(logs) == x.shape[0] and all(set(d) == {"diff_target", "diff_input", "diff_views"} for d in logs)
    for d, w in zip(logs, w_logs):
        assert all(abs(d[k] - w[k]) <= thr_s for k in w), (d, w)


def check_refusals():
    """What needs no kernel: depths, modes and sizes that are not built, images too small for the crop."""
    raises(NotImplementedError, lambda: ID.Backbone(112, 100, "ir_se"))
    raises(NotImplementedError, lambda: ID.Backbone(112, 50, "ir"))
    raises(ValueError, lambda: ID.Backbone(128, 50, "ir_se"), "112 or 224")
    raises(ValueError, lambda: ID.Backbone(30, units=list(SMALL_UNITS)))
    idl = ID.IDLoss(ID.Backbone(SMALL_SIZE, units=list(SMALL_UNITS)), lib=object())
    raises(ValueError, lambda: idl.extract_feats(torch.zeros(1, 3, 222, 256)), "crop")
    raises(ValueError, lambda: idl.extract_feats(torch.zeros(1, 3, 256, 219)), "crop")
    raises(ValueError, lambda: idl.extract_feats(torch.zeros(1, 1, 256, 256)))
    raises(ValueError, lambda: idl.similarity(torch.zeros(1, 3, 256, 256), torch.zeros(2, 3, 256, 256)))


# ---- command line -------------------------------------------------------------------------------------------------
CLI_FILES = ("a.png", "b.png", "c.png")


def write_pairs(root):
    """Three pairs of 40 x 40 PNGs: smooth fields, the result a noisier and noisier copy of its ground truth."""
    imgs = R.discriminating_images(SMALL_IMAGE, 4, 2)[[0, 2, 3]]
    rng = np.random.default_rng(31)
    data, gt = os.path.join(root, "results"), os.path.join(root, "gt_images")
    os.makedirs(data), os.makedirs(gt)
    for k, name in enumerate(CLI_FILES):
        base = (imgs[k].permute(1, 2, 0).numpy() * 0.5 + 0.5) * 255
        other = base + rng.integers(-(6 + 40 * k), 7 + 40 * k, base.shape)
        for folder, img in ((gt, base), (data, other)):
            PIL.Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8), "RGB").save(os.path.join(folder, name))
    return data, gt


def check_cli(L, st, device, root, decoder="pil"):
    """scores_id.json has the file names as keys and the restatement's similarities as values, stat_id.txt the stated line; a
    missing ground-truth file raises."""
    data, gt = write_pairs(root)
    units, size = list(TINY_UNITS), TINY_SIZE
    net = ID.Backbone(size, units=units)
    net.load_state_dict(state("tiny"))
    model = ID.IDLoss(net.to(device), lib=inject(L, device), crop=CLI_CROP)
    scores = ID.main(["--data_path", data, "--gt_path", gt, "--size", "32", "--batch", "2", "--image_decoder", decoder], model=model,
                     lib=inject(L, device), device=device)
    ref_net = R.network(state("tiny"), units, size)

    def load(folder):
        arr = [np.asarray(PIL.Image.open(os.path.join(folder, n)).convert("RGB").resize((32, 32), PIL.Image.BILINEAR)) for n in CLI_FILES]
        return (torch.from_numpy(np.stack(arr)).permute(0, 3, 1, 2).double() / 255 - 0.5) / 0.5

    want = (R.extract_feats(ref_net, load(data), CLI_CROP) * R.extract_feats(ref_net, load(gt), CLI_CROP)).sum(1).tolist()
    saved, stat = read_scores(root, "id")
    assert list(saved) == list(CLI_FILES) == list(scores) and saved == scores
    thr_s = thresholds("tiny")[1]
    values = [saved[n] for n in CLI_FILES]
    print("cli similarities", values, want)
    assert all(abs(a - b) <= thr_s for a, b in zip(values, want)), (values, want)
    assert want[0] - want[2] > 0.01  # the noisier copy is less similar: the scores mean something
    assert stat == "Average similarity is {:.2f}+-{:.2f}".format(np.mean(values), np.std(values))
    os.remove(os.path.join(gt, CLI_FILES[1]))
    raises(FileNotFoundError, lambda: ID.main(["--data_path", data, "--gt_path", gt, "--size", "32"], model=model, lib=inject(L, device),
                                              device=device), CLI_FILES[1])
