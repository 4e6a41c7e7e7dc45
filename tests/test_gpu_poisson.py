"""GPU tests (-m gpu) of Poisson image blending (hairfastgan_amd.image_utils; csrc/poisson.h) against the CPU restatement
of utils/image_utils.py:58-94 (tests/poisson_ref.py).

The solver is compared bit for bit.  Masks come from an argmax (BiSeNet): an index is reproduced exactly wherever the
top-1 / top-2 logit margin exceeds the fp32 tolerance of the logits, so label flips are allowed only below the margin rule
of tests/test_gpu_parsing.py (5e-4 x the largest logit); the blend is then compared bit for bit given the GPU's mask."""
import numpy as np
import pytest
import torch

from oracle import cases as C
from oracle import ref_bisenet as BS
from tests import poisson_ref as R

pytestmark = pytest.mark.gpu

HAIR_BISENET = BS.BISENET_LABELS.index("hair")
L_EYE_BISENET = BS.BISENET_LABELS.index("l_eye")


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return torch.device("cuda:0")


def _params():
    """oracle.cases.bisenet_params() with the class-score rows of `hair` and `l_eye` exchanged: on [0,1] images the
    synthetic net never picks hair, with the exchange 5-10 % of the pixels are hair - masks with holes to solve around."""
    P = C.bisenet_params()
    for name in ("conv_out", "conv_out16", "conv_out32"):
        w = P[f"{name}.conv_out.weight"].clone()
        w[[HAIR_BISENET, L_EYE_BISENET]] = w[[L_EYE_BISENET, HAIR_BISENET]]
        P[f"{name}.conv_out.weight"] = w
    return P


def _net(dev, P):
    from hairfastgan_amd.face_parsing import BiSeNet

    net = BiSeNet(19).eval()
    net.load_state_dict(P)
    return net.to(dev)


def _image(h, w, seed):
    """[3,H,W] in [0,1]: a smooth pattern plus noise (regions in the parse, detail in the gradients)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    ph = torch.rand(3, generator=g) * 6
    base = torch.stack([torch.sin(3 * xx + yy + ph[0]), torch.cos(2 * yy - xx + ph[1]), torch.sin(4 * xx * yy + ph[2])])
    return (0.5 + 0.4 * base + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)


def test_solver_1024_bit_identical():
    from hairfastgan_amd import _runtime
    from hairfastgan_amd.image_utils import DEFAULT_TBLOCK, poisson_solve

    dev = _dev()
    rng = np.random.default_rng(0)
    H = W = 1024
    s, t = rng.integers(0, 256, (2, 1, 3, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    mask = np.where((yy - 400) ** 2 / 300 ** 2 + (xx - 600) ** 2 / 380 ** 2 <= 1, 255, 0).astype(np.uint8)
    mask[:, :40] = 255                                          # touches the left border
    b, x = R.setup(s[0], t[0], mask)
    done = 0
    for maxn in (0, 1, 115, 1000):
        x = R.jacobi(b, x, mask, maxn - done)
        done = maxn
        ref_out = R.finish(x, t[0], mask)
        for tblock in sorted({1, DEFAULT_TBLOCK}):
            out, xg = poisson_solve(_runtime.lib(), _runtime.stream(), torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev),
                                    torch.from_numpy(mask)[None, None].to(dev), maxn, tblock)
            xg = xg.cpu().numpy()[0]
            assert np.array_equal(xg, x), (maxn, tblock, float(np.abs(xg - x).max()))
            assert np.array_equal(out.cpu().numpy()[0], ref_out), (maxn, tblock)
        print(f"1024^2 solve, {maxn} sweeps: bit-identical for T = 1 and T = {DEFAULT_TBLOCK}")


def _check_blend(net, P, finals, faces, maxn, dilate_erosion=30):
    """poisson_blend on the GPU against the restatement: label flips only below the margin rule, the mask equal to the
    restatement's from the GPU's labels (and from the oracle's where no hair index flipped), the blend bit-identical."""
    from hairfastgan_amd.face_parsing import get_segmentation
    from hairfastgan_amd.image_utils import poisson_blend

    T = finals.shape[0]
    with torch.inference_mode():
        out, mask = poisson_blend(finals, faces, dilate_erosion, maxn, parsing=net)
        labels = get_segmentation(net, torch.cat([finals, faces]), resize=False).cpu()
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    images = torch.cat([finals, faces]).cpu()
    ref_labels = []
    for j in range(2 * T):
        logits = BS.bisenet_logits(P, images[j:j + 1])[0]
        ref = torch.tensor(BS.LABEL_REMAP)[logits.argmax(0)]
        top2 = logits.topk(2, dim=0).values
        margin, scale = top2[0] - top2[1], float(logits.abs().max())
        flips = labels[j, 0] != ref
        n = int(flips.sum())
        assert n == 0 or float(margin[flips].max()) <= 5e-4 * scale, (n, float(margin[flips].max()), scale)
        ref_labels.append(ref[None, None])
    hair_frac = [float((r == R.HAIR).float().mean()) for r in ref_labels]
    for i in range(T):
        assert np.array_equal(mask[i, 0], R.masks_from_labels(labels[i:i + 1], labels[T + i:T + i + 1], dilate_erosion))
        hair_flips = sum(int(((labels[j:j + 1] == R.HAIR) != (ref_labels[j] == R.HAIR)).sum()) for j in (i, T + i))
        if hair_flips == 0:
            assert np.array_equal(mask[i, 0], R.masks_from_labels(ref_labels[i], ref_labels[T + i], dilate_erosion))
        ro, _ = R.solve(R.quantize(faces[i]), R.quantize(finals[i]), mask[i, 0], maxn)
        assert np.array_equal(out[i], ro)
        print(f"{tuple(finals.shape[-2:])} pair {i}: {hair_flips} hair-index flips, {int((mask[i] == 255).sum())} mask pixels set, "
              f"blend bit-identical")
    assert max(hair_frac) > 0.01 and 0 < (mask == 255).mean() < 1, (hair_frac, (mask == 255).mean())
    return out, mask


@pytest.mark.parametrize("size", [512, 1024])
def test_poisson_blend_vs_restatement(size):
    dev = _dev()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P = _params()
    net = _net(dev, P)
    finals = _image(size, size, 1)[None].to(dev)
    faces = _image(size, size, 2)[None].to(dev)
    _check_blend(net, P, finals, faces, 115)


def test_batched_equals_single():
    from hairfastgan_amd.image_utils import poisson_blend

    dev = _dev()
    net = _net(dev, _params())
    finals = torch.stack([_image(512, 512, 10 + i) for i in range(3)]).to(dev)
    faces = torch.stack([_image(512, 512, 20 + i) for i in range(3)]).to(dev)
    with torch.inference_mode():
        out, mask = poisson_blend(finals, faces, parsing=net)
        for i in range(3):
            o1, m1 = poisson_blend(finals[i:i + 1], faces[i:i + 1], parsing=net)
            assert torch.equal(o1[0], out[i]) and torch.equal(m1[0], mask[i]), i
    assert not torch.equal(mask[0], mask[1])


def test_path_pil_and_tensor_inputs_agree(tmp_path):
    from PIL import Image

    from hairfastgan_amd.image_utils import poisson_image_blending

    dev = _dev()
    net = _net(dev, _params())
    final = _image(256, 256, 3).to(dev)
    face_u8 = R.quantize(_image(256, 256, 4)).transpose(1, 2, 0)          # [H,W,3]
    path = tmp_path / "face.png"
    Image.fromarray(face_u8, "RGB").save(path)
    results = [poisson_image_blending(final, f, parsing=net) for f in
               (str(path), path, Image.open(path), torch.from_numpy(face_u8.transpose(2, 0, 1).copy()).float().div(255))]
    for res, mask in results:
        assert res.mode == "RGB" and mask.mode == "RGB" and res.size == (256, 256) and mask.size == (256, 256)
        assert np.array_equal(np.asarray(res), np.asarray(results[0][0]))
        assert np.array_equal(np.asarray(mask), np.asarray(results[0][1]))


def test_hairfast_method_on_synthetic_swap():
    from oracle import ref_encoders as E
    from oracle import ref_postprocess as PP
    from oracle import ref_stylegan2 as O

    from hairfastgan_amd.hair_swap import HairFast, get_parser

    dev = _dev()
    args = get_parser().parse_args([])
    args.device = dev
    pp_shapes = PP.post_process_param_shapes()
    lat_shape = pp_shapes.pop("latent_avg")
    _, e4e_latent_avg = C.e4e_inputs(2)
    _, dlat = C.fs_inputs(2)
    hf = HairFast(args, generator_state={"g_ema": C.generator_params(O.generator_param_shapes(1024, 512, 8, 2)), "latent_avg": torch.zeros(512)},
                  e4e_state=C.params_from_shapes("e4e", E.e4e_param_shapes()), e4e_latent_avg=e4e_latent_avg,
                  fs_state=C.params_from_shapes("fs", E.fs_param_shapes()), fs_dlatent_avg=dlat,
                  pp_state=C.params_from_shapes("pp", pp_shapes),
                  pp_latent_avg=C.params_from_shapes("pp", {"latent_avg": lat_shape})["latent_avg"] * 0.1,
                  bisenet_state=C.pipeline_bisenet_params(), rotate_state=C.params_from_shapes("rotate", PP.rotate_param_shapes()),
                  blend_state=C.params_from_shapes("clipblend", PP.clip_blending_param_shapes()), clip_state=C.clip_params(),
                  shape_state=C.shape_adaptor_params(), sean_state=C.sean_params(), sean_mean_codes=C.sean_mean_codes())
    face, shape, color = (im.float().div(255).to(dev) for im in C.pipeline_images())
    final = hf.swap(face, shape, color)
    res, mask = hf.poisson_image_blending(final, face)
    H, W = final.shape[-2:]
    assert res.mode == "RGB" and mask.mode == "RGB" and res.size == (W, H) and mask.size == (W, H)
    res, mask = np.asarray(res), np.asarray(mask)
    om = R.omega(mask[:, :, 0])
    q_final = R.quantize(final).transpose(1, 2, 0)
    assert np.array_equal(res[~om], q_final[~om])
    assert all(np.array_equal(mask[:, :, c], mask[:, :, 0]) for c in (1, 2))
    [(res_b, mask_b)] = hf.poisson_image_blending_batch([final], [face])
    assert np.array_equal(np.asarray(res_b), res) and np.array_equal(np.asarray(mask_b), mask)
    print(f"HairFast.poisson_image_blending: {int(om.sum())} of {H * W} pixels solved")
