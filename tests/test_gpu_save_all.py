"""GPU tests (-m gpu) of `--save_all`: one `HairFast` with the synthetic state dicts and the formula noise of
tests/test_gpu_pipeline.py runs a swap and a `swap_batch` with args.save_all set; every file the reference's layout names
must exist - nothing else - and hold what the stages computed:

* a PNG of an image is, byte for byte, `((x + 1) / 2).clamp(0, 1).mul(255).byte()` (utils/save_utils.py:15) evaluated on the
  CPU on the recorded tensor it stands for (generator outputs, SEAN renderings);
* a PNG of a parse is the reference's colour (tests/golden/mask_colors.npz) of every label of the recorded parse / target;
* an npz array equals the recorded latent, with the reference's shape;
* the final image has the same bits with save_all on and off.

Measured on the MI355X: building the shared HairFast 12.2 s (what tests/test_gpu_pipeline.py, 11.9 s in the same run, pays
inside its test), the single swap test 3.4 s, the two-triple test 5.2 s."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

from oracle import cases as C
from oracle import ref_encoders as E
from oracle import ref_postprocess as PP
from oracle import ref_stylegan2 as O
from tests import export_checks as K

pytestmark = pytest.mark.gpu

NAMES = ("face", "shape", "color")
FILES_31 = sorted(
    [f"W+/{n}.{e}" for n in NAMES for e in ("png", "npz")] + [f"FS/{n}.{e}" for n in NAMES for e in ("png", "npz")]
    + ["Shape/shape_rotate_to_face.png", "Shape/color_rotate_to_face.png", "Shape/mask_face.png", "Shape/mask_shape.png",
       "Shape/mask_color.png", "Shape/mask_shape_rotate_to_face.png", "Shape/mask_color_rotate_to_face.png",
       "Shape/mask_face_shape_target.png", "Shape/mask_face_color_target.png"]
    + ["Align/face_shape_SEAN.png", "Align/shape_face_SEAN.png", "Align/face_shape_e4e.png", "Align/shape_face_e4e.png",
       "Align/face_shape_output.png", "Align/face_shape_F.npz", "Blending/blending.png", "Blending/blending.npz",
       "Final/final.png", "Final/final.npz"])
FACE_COLOR_FILES = ["Shape/color_rotate_to_face.png", "Shape/mask_color.png", "Shape/mask_color_rotate_to_face.png",
                    "Shape/mask_face_color_target.png"]


class Rig:
    """The HairFast under test with every source of randomness replaced by a formula and the stage results recorded."""

    def __init__(self):
        import hairfastgan_amd.hair_swap as HS
        from hairfastgan_amd.hair_swap import HairFast, get_parser

        self.HS = HS
        dev = self.dev = torch.device("cuda:0")
        args = get_parser().parse_args([])
        args.device = dev
        pp_shapes = PP.post_process_param_shapes()
        lat_shape = pp_shapes.pop("latent_avg")
        _, e4e_latent_avg = C.e4e_inputs(2)
        _, dlat = C.fs_inputs(2)
        hf = self.hf = HairFast(
            args, generator_state={"g_ema": C.generator_params(O.generator_param_shapes(1024, 512, 8, 2)), "latent_avg": torch.zeros(512)},
            e4e_state=C.params_from_shapes("e4e", E.e4e_param_shapes()), e4e_latent_avg=e4e_latent_avg,
            fs_state=C.params_from_shapes("fs", E.fs_param_shapes()), fs_dlatent_avg=dlat,
            pp_state=C.params_from_shapes("pp", pp_shapes),
            pp_latent_avg=C.params_from_shapes("pp", {"latent_avg": lat_shape})["latent_avg"] * 0.1,
            bisenet_state=C.pipeline_bisenet_params(), rotate_state=C.params_from_shapes("rotate", PP.rotate_param_shapes()),
            blend_state=C.params_from_shapes("clipblend", PP.clip_blending_param_shapes()), clip_state=C.clip_params(),
            shape_state=C.shape_adaptor_params(), sean_state=C.sean_params(), sean_mean_codes=C.sean_mean_codes())
        self.calls = []
        self.rec = {"parses": [], "targets": [], "sean": [], "embed": [], "align": []}
        gen_fwd = hf.net.generator.forward

        def recorded_forward(styles, **kw):
            out = gen_fwd(styles, randomize_noise=False, **kw)
            self.calls.append({"sig": (styles[0].shape[0], kw.get("start_layer", 0), kw.get("end_layer", 8)), "latent": styles[0],
                               "layer_in": kw.get("layer_in"), "out": out[0]})
            return out

        hf.net.generator.forward = recorded_forward
        hf.stages.sean_model.netG.noise_source = lambda d, sizes: [
            torch.cat([C.pipeline_sean_noise(dd * len(sizes) + i, r) for dd in range(d)]).to(dev) for i, r in enumerate(sizes)]
        rec = self.rec
        self.seg = seg = HS.get_segmentation
        HS.get_segmentation = lambda net, x, **kw: (rec["parses"].append(seg(net, x, **kw)) or rec["parses"][-1])
        adaptor = hf.stages.shape_adaptor
        hf.stages.shape_adaptor = lambda a, b: (rec["targets"].append(adaptor(a, b)) or rec["targets"][-1])
        sean = hf.stages.sean_inpaint_pairs
        hf.stages.sean_inpaint_pairs = lambda *a: (rec["sean"].append(sean(*a)) or rec["sean"][-1])
        emb = hf.embed.embedding_images
        hf.embed.embedding_images = lambda *a, **k: (rec["embed"].append(emb(*a, **k)) or rec["embed"][-1])
        alb = hf.align.align_images_batch
        hf.align.align_images_batch = lambda *a, **k: (rec["align"].append(alb(*a, **k)) or rec["align"][-1])
        # float images divided on the CPU, as the reference's equal_replacer / ImagesDataset do
        self.images = [im.float().div(255).to(dev) for im in C.pipeline_images()]

    def reset(self):
        self.calls.clear()
        for v in self.rec.values():
            v.clear()

    def close(self):
        self.HS.get_segmentation = self.seg


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    r = Rig()
    yield r
    r.close()


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root).replace(os.sep, "/") for dp, _, fs in os.walk(root) for f in fs)


def _png(path):
    with PIL.Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _image_bytes(x):
    """save_gen_image's bytes of one recorded image [3,H,W], on the CPU."""
    return ((x.detach().cpu() + 1) / 2).clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()


def _lookup():
    labels, rgb = K.golden_masks()
    table = np.zeros((256, 3), np.uint8)
    for k in set(labels.reshape(-1).tolist()):
        table[k] = rgb[labels == k][0]
    return table


def _check_images(root, expect):
    for rel, x in expect.items():
        got, ref = _png(root / rel), _image_bytes(x)
        assert got.shape == ref.shape and np.array_equal(got, ref), (rel, got.shape, int((got != ref).sum()))


def _check_masks(root, expect):
    table = _lookup()
    for rel, m in expect.items():
        m = m.detach().cpu().numpy().reshape(m.shape[-2:])
        assert 0 <= m.min() and m.max() <= 18
        assert np.array_equal(_png(root / rel), table[m]), rel


def _check_latents(root, expect):
    for rel, arrays in expect.items():
        with np.load(root / rel) as z:
            assert sorted(z.files) == sorted(arrays), (rel, z.files)
            for k, (x, shape) in arrays.items():
                assert z[k].shape == shape and z[k].dtype == np.float32, (rel, k, z[k].shape)
                assert np.array_equal(z[k], x.detach().cpu().numpy().reshape(shape)), (rel, k)


def _check_three_image_triple(root, embed, calls6, parses_rot, targets, sean, align, extra_w, extra_fs, w_rows, fs_rows, e4e_rows,
                              out_row):
    """Every file of a triple of three distinct images against the records: calls6 = its six generator calls,
    w_rows / fs_rows = its images' rows in the two extra calls, e4e_rows / out_row = its Align renderings' rows."""
    fs33, w03, rot, sean03, blend48, final58 = calls6
    images = {"Final/final.png": final58["out"][0], "Blending/blending.png": blend48["out"][0],
              "Shape/shape_rotate_to_face.png": rot["out"][0], "Shape/color_rotate_to_face.png": rot["out"][1],
              "Align/face_shape_SEAN.png": sean[0], "Align/shape_face_SEAN.png": sean[1],
              "Align/face_shape_e4e.png": extra_fs["out"][e4e_rows[0]], "Align/shape_face_e4e.png": extra_fs["out"][e4e_rows[1]],
              "Align/face_shape_output.png": extra_fs["out"][out_row]}
    for n, wr, fr in zip(NAMES, w_rows, fs_rows):
        images[f"W+/{n}.png"] = extra_w["out"][wr]
        images[f"FS/{n}.png"] = extra_fs["out"][fr]
        # the name -> image mapping: the rows rendered under a name are that image's own latents
        assert torch.equal(extra_w["latent"][wr], embed[n]["W"][0]), n
        assert torch.equal(extra_fs["latent"][fr], embed[n]["S"][0]) and torch.equal(extra_fs["layer_in"][fr], embed[n]["F"][0]), n
    for k in range(2):  # e4e of the two SEAN renderings: W and F of the 0->3 call on them
        assert torch.equal(extra_fs["latent"][e4e_rows[k]], sean03["latent"][k]) and torch.equal(extra_fs["layer_in"][e4e_rows[k]], sean03["out"][k])
    assert torch.equal(extra_fs["latent"][out_row], embed["face"]["S"][0])
    assert torch.equal(extra_fs["layer_in"][out_row], align["latent_F_align"][0])
    _check_images(root, images)
    _check_masks(root, {"Shape/mask_face.png": embed["face"]["mask"], "Shape/mask_shape.png": embed["shape"]["mask"],
                        "Shape/mask_color.png": embed["color"]["mask"], "Shape/mask_shape_rotate_to_face.png": parses_rot[0],
                        "Shape/mask_color_rotate_to_face.png": parses_rot[1], "Shape/mask_face_shape_target.png": targets[0],
                        "Shape/mask_face_color_target.png": targets[1]})
    latents = {"Align/face_shape_F.npz": {"latent_F_align": (align["latent_F_align"], (1, 512, 32, 32))},
               "Blending/blending.npz": {"S_blend": (blend48["latent"], (1, 18, 512))},
               "Final/final.npz": {"S_final": (final58["latent"], (1, 18, 512)), "F_final": (final58["layer_in"], (1, 512, 64, 64))}}
    for n in NAMES:
        latents[f"W+/{n}.npz"] = {"latent_W": (embed[n]["W"], (18, 512))}
        latents[f"FS/{n}.npz"] = {"latent_S": (embed[n]["S"], (18, 512)), "latent_F": (embed[n]["F"], (512, 32, 32))}
    _check_latents(root, latents)


SIX = [(3, 3, 3), (3, 0, 3), (2, 0, 8), (2, 0, 3), (1, 4, 8), (1, 5, 8)]


def test_swap_writes_the_reference_layout(rig, tmp_path):
    """One swap with save_all on, exp_name "t", then the same swap with it off."""
    hf, args = rig.hf, rig.hf.args
    args.save_all_dir = tmp_path
    rig.reset()
    args.save_all = True
    try:
        final_on = hf.swap(*rig.images, exp_name="t")
    finally:
        args.save_all = False
    calls, rec = list(rig.calls), {k: list(v) for k, v in rig.rec.items()}
    rig.reset()
    final_off = hf.swap(*rig.images, exp_name="t")
    assert [c["sig"] for c in rig.calls] == SIX  # nothing extra runs with save_all off
    assert torch.equal(final_on, final_off)
    assert _files(tmp_path) == ["t/" + f for f in FILES_31]
    assert [c["sig"] for c in calls] == SIX + [(3, 0, 8), (6, 4, 8)]
    assert len(rec["parses"]) == 2 and len(rec["targets"]) == 1 and len(rec["sean"]) == 1
    _check_three_image_triple(tmp_path / "t", rec["embed"][0], calls[:6], rec["parses"][1], rec["targets"][0], rec["sean"][0],
                              rec["align"][0][0], calls[6], calls[7], (0, 1, 2), (0, 1, 2), (3, 4), 5)
    assert torch.equal(final_on, ((calls[5]["out"][0] + 1) / 2).clip(0, 1))


def test_swap_batch_writes_every_triple(rig, tmp_path):
    """Two triples, the second with shape and color the same image, under exp_names "a" and "b"."""
    hf, args = rig.hf, rig.hf.args
    face, shape, color = rig.images
    args.save_all_dir = tmp_path
    rig.reset()
    args.save_all = True
    try:
        finals = hf.swap_batch([(face, shape, color), (shape, color, color)], exp_names=["a", "b"])
    finally:
        args.save_all = False
    calls, rec = rig.calls, rig.rec
    # triple 0 is one batched pass of its own, triple 1 (a repeated image) takes the reference's shortcuts one by one
    six_b = [(2, 3, 3), (2, 0, 3), (1, 0, 8), (2, 0, 3), (1, 4, 8), (1, 5, 8)]
    assert [c["sig"] for c in calls] == SIX + six_b + [(5, 0, 8), (11, 4, 8)]
    files_b = sorted(set(FILES_31) - set(FACE_COLOR_FILES))
    assert _files(tmp_path) == ["a/" + f for f in FILES_31] + ["b/" + f for f in files_b]
    extra_w, extra_fs = calls[12], calls[13]
    # rows of the 4->8 call: 5 embedded images, (e4e, e4e) of a and of b, then the outputs of a and of b
    _check_three_image_triple(tmp_path / "a", rec["embed"][0], calls[:6], rec["parses"][1], rec["targets"][0], rec["sean"][0],
                              rec["align"][0][0], extra_w, extra_fs, (0, 1, 2), (0, 1, 2), (5, 6), 9)
    assert torch.equal(finals[0], ((calls[5]["out"][0] + 1) / 2).clip(0, 1))
    # ---- triple 1: face = the shape image, shape = color = the color image ----
    root, embed, align = tmp_path / "b", rec["embed"][1], rec["align"][1][0]
    fs33, w03, rot, sean03, blend48, final58 = calls[6:12]
    assert torch.equal(embed["shape"]["W"], embed["color"]["W"]) and not torch.equal(embed["shape"]["W"], embed["face"]["W"])
    assert torch.equal(extra_w["latent"][3], embed["face"]["W"][0]) and torch.equal(extra_w["latent"][4], embed["shape"]["W"][0])
    assert torch.equal(extra_fs["latent"][7], sean03["latent"][0]) and torch.equal(extra_fs["layer_in"][10], align["latent_F_align"][0])
    _check_images(root, {"Final/final.png": final58["out"][0], "Blending/blending.png": blend48["out"][0],
                         "Shape/shape_rotate_to_face.png": rot["out"][0], "Align/face_shape_SEAN.png": rec["sean"][1][0],
                         "Align/shape_face_SEAN.png": rec["sean"][1][1], "Align/face_shape_e4e.png": extra_fs["out"][7],
                         "Align/shape_face_e4e.png": extra_fs["out"][8], "Align/face_shape_output.png": extra_fs["out"][10],
                         "W+/face.png": extra_w["out"][3], "W+/shape.png": extra_w["out"][4], "W+/color.png": extra_w["out"][4],
                         "FS/face.png": extra_fs["out"][3], "FS/shape.png": extra_fs["out"][4], "FS/color.png": extra_fs["out"][4]})
    _check_masks(root, {"Shape/mask_face.png": embed["face"]["mask"], "Shape/mask_shape.png": embed["shape"]["mask"],
                        "Shape/mask_shape_rotate_to_face.png": rec["parses"][3][0], "Shape/mask_face_shape_target.png": rec["targets"][1][0]})
    latents = {"Align/face_shape_F.npz": {"latent_F_align": (align["latent_F_align"], (1, 512, 32, 32))},
               "Blending/blending.npz": {"S_blend": (blend48["latent"], (1, 18, 512))},
               "Final/final.npz": {"S_final": (final58["latent"], (1, 18, 512)), "F_final": (final58["layer_in"], (1, 512, 64, 64))}}
    for n in NAMES:
        latents[f"W+/{n}.npz"] = {"latent_W": (embed[n]["W"], (18, 512))}
        latents[f"FS/{n}.npz"] = {"latent_S": (embed[n]["S"], (18, 512)), "latent_F": (embed[n]["F"], (512, 32, 32))}
    _check_latents(root, latents)
    assert torch.equal(finals[1], ((final58["out"][0] + 1) / 2).clip(0, 1))


def test_exp_names_of_the_wrong_length(rig):
    face, shape, color = rig.images
    with pytest.raises(ValueError, match="exp_names"):
        rig.hf.swap_batch([(face, shape, color), (shape, color, color)], exp_names=["a"])
