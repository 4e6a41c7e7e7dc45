"""GPU tests (-m gpu) of native FFHQ face alignment (hairfastgan_amd.face_align; csrc/align.h) through the C ABI against PIL
at test time, the CPU restatement (tests/align_ref.py) and the reference's own results (tests/golden/align.npz).

Resize, transform, the fused kernel and the unpadded alignments: byte-equal.  The pad stage: the tie rule of
tests/align_checks.py (eligible-byte counts recorded there in TIE_COUNTS)."""
import functools

import numpy as np
import PIL.Image
import pytest
import torch

from tests import align_checks as K
from tests import align_ref as R
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inputs(group, name):
    return R.case_inputs({"golden": R.GOLDEN_CASES, "small": R.SMALL_CASES}[group][name])


@pytest.mark.parametrize("in_w,in_h,out_w,out_h", K.RESIZE_CASES)
def test_resize_lanczos(in_w, in_h, out_w, out_h):
    K.check_resize(*gpu_ctx(), in_w, in_h, out_w, out_h)


@pytest.mark.parametrize("name", list(K.QUADS))
def test_quad_transform(name):
    K.check_transform(*gpu_ctx(), name)


def test_fused_equals_chained_pair_256_to_64():
    K.check_fused_small(*gpu_ctx())


def test_fused_equals_chained_pair_4096_to_1024(golden):
    """The fused kernel at its real sizes on the 600 x 500 case: the same bytes as transform + resize chained, and the
    reference's result."""
    from hairfastgan_amd import face_align as FA

    L, st, dev = gpu_ctx()
    arr, lm = _inputs("golden", "inside")
    stages = {}
    fused = FA.align_bytes(L, st, K.chw(arr, dev), lm, fused=True, stages=stages)
    pair = FA.transform_resize(L, st, stages["padded"], stages["plan"]["quad"], 4096, 1024, fused=False)
    assert torch.equal(fused, pair)
    big = FA.quad_transform(L, st, stages["padded"], stages["plan"]["quad"], 4096)
    assert torch.equal(FA.resize_lanczos(L, st, big, 1024, 1024), pair)
    G = golden("align.npz")
    (r0, r1), step = G["crop"], int(G["grid"])
    out = K.hwc(fused)
    assert np.array_equal(out[r0:r1, r0:r1], G["inside_crop"]) and np.array_equal(out[::step, ::step], G["inside_grid"])


@pytest.mark.parametrize("name", list(K.PAD_CASES))
def test_pad(name):
    K.check_pad(*gpu_ctx(), name)
    if name == "none":
        K.check_pad_invalid(*gpu_ctx())


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_align_face_golden(golden, name):
    """align_face at the reference's sizes against the reference's own result (a 128^2 crop and the every-8th-pixel grid)."""
    from hairfastgan_amd import face_align as FA

    L, st, dev = gpu_ctx()
    G = golden("align.npz")
    arr, lm = _inputs("golden", name)
    stages = {}
    out = K.hwc(FA.align_bytes(L, st, K.chw(arr, dev), lm, stages=stages))
    (r0, r1), step = G["crop"], int(G["grid"])
    expect_crop, expect_grid = G[f"{name}_crop"], G[f"{name}_grid"]
    if stages["plan"]["pad"] is not None:
        P = R.plan(lm, arr.shape[1], arr.shape[0])
        pre = R.pad_float(np.asarray(R.crop(PIL.Image.fromarray(arr, "RGB"), P)), P["pad"], P["blur"])
        k = K.assert_tie_rule(K.hwc(stages["padded"]), pre, "golden_" + name)
        # the golden result is the reference's from ITS padded image: its bytes at the eligible positions are in the file
        theirs = R.to_bytes(pre).reshape(-1)
        theirs[G[f"{name}_tie_index"]] = G[f"{name}_tie_bytes"]
        if not np.array_equal(theirs, K.hwc(stages["padded"]).reshape(-1)):
            full = np.asarray(R.finish(PIL.Image.fromarray(K.hwc(stages["padded"]), "RGB"), P))
            expect_crop, expect_grid = full[r0:r1, r0:r1], full[::step, ::step]
        print(f"{name}: {k} padded bytes differ from the restatement (ties)")
    assert np.array_equal(out[r0:r1, r0:r1], expect_crop) and np.array_equal(out[::step, ::step], expect_grid)
    [t] = FA.align_face([K.chw(arr, dev)], [lm])
    assert t.dtype == torch.float32 and t.shape == (3, 1024, 1024) and t.is_cuda
    assert torch.equal(t.cpu(), torch.from_numpy(out.transpose(2, 0, 1).copy()).float().div(255))  # ToTensor's bits


@pytest.mark.parametrize("name", list(R.SMALL_CASES))
def test_align_small_against_restatement(name):
    """The three geometries at output 64 / transform 256, every stage against the restatement; `inside` enters as a float
    tensor (the truncating byte conversion of ToPILImage)."""
    K.check_align_against_restatement(*gpu_ctx(), R.SMALL_CASES[name], 64, 256,
                                      count_key="small_corner" if name == "corner" else None, as_float=name == "inside")


def test_align_face_list_of_three_sizes():
    from hairfastgan_amd import face_align as FA

    L, st, dev = gpu_ctx()
    names = ["inside", "corner of a 140 x 110 image", "shrink"]
    pairs = [_inputs("small", "inside"), R.case_inputs((140, 110, 25, (24, 22, 20, 7.0))), _inputs("small", "shrink")]
    assert len({p[0].shape for p in pairs}) == 3
    images = [K.chw(pairs[0][0], dev), PIL.Image.fromarray(pairs[1][0], "RGB"), pairs[2][0]]  # tensor, PIL image, HWC array
    outs = FA.align_face(images, [p[1] for p in pairs], 64, 256, return_tensors=False)
    floats = FA.align_face(images, [p[1] for p in pairs], 64, 256)
    for n, (arr, lm), out, f in zip(names, pairs, outs, floats):
        assert out.dtype == torch.uint8 and out.shape == (3, 64, 64)
        assert torch.equal(out, FA.align_bytes(L, st, K.chw(arr, dev), lm, 64, 256)), n
        assert torch.equal(f.cpu(), out.cpu().float().div(255))
    b = torch.arange(256, dtype=torch.uint8, device=dev)
    assert torch.equal(FA.unit_float(b).cpu(), b.cpu().float().div(255))


def test_swap_align_true():
    """swap(..., align=True, landmarks=...) on the synthetic-parameter HairFast: the 4-tuple of the reference, the aligned
    images those of align_face, `final` bit-equal to the swap of the aligned images with align=False and the same seed."""
    from hairfastgan_amd import face_align as FA
    from tests.test_gpu_schedule import _hairfast

    _, _, dev = gpu_ctx()
    hf = _hairfast(dev)
    cases = [R.GOLDEN_CASES["inside"], R.GOLDEN_CASES["corner"], (640, 480, 17, (330, 200, 70, -11.0))]
    pairs = [R.case_inputs(c) for c in cases]
    images = [K.chw(arr, dev) for arr, _ in pairs]
    lms = [lm for _, lm in pairs]
    final, face, shape, color = hf.swap(*images, align=True, landmarks=lms, seed=7)
    aligned = FA.align_face(images, lms)
    for got, ref in zip((face, shape, color), aligned):
        assert got.shape == (3, 1024, 1024) and torch.equal(got, ref)
    assert final.shape == (3, 1024, 1024) and torch.isfinite(final).all()
    assert torch.equal(final, hf.swap(*aligned, seed=7))
    # the landmarks from a detector callable: it sees uint8 HWC arrays
    seen = []

    def detector(image):
        assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
        seen.append(image.shape)
        return next(lm for arr, lm in pairs if np.array_equal(arr, image))

    hf.landmark_detector = detector
    out = hf.swap_batch([tuple(images)], align=True, seed=7)
    assert len(seen) == 3 and len(out) == 1 and len(out[0]) == 4
    assert all(torch.equal(a, b) for a, b in zip(out[0], (final, face, shape, color)))
    hf.landmark_detector = None
    with pytest.raises(ValueError):
        hf.swap(*images, align=True, landmarks=[lms[0], lms[1][:10], lms[2]])
