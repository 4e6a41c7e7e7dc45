"""GPU tests (-m gpu) of pasting the aligned result back into the photograph (hairfastgan_amd.face_align.paste_back;
csrc/paste.h): the kernels through the C ABI against the PIL restatement (tests/paste_ref.py) byte for byte
(tests/paste_checks.py), then the public surface - face_align.paste_back, HairFast.paste_back, swap(paste_back=True)."""
import numpy as np
import PIL.Image
import pytest
import torch

from tests import align_ref as R
from tests import paste_checks as K
from tests import paste_ref as PR
from tests.metric_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(K.CASES))
def test_paste(name):
    K.check_paste(*gpu_ctx(), name)


def test_paste_user_mask_without_feather():
    K.check_paste(*gpu_ctx(), "down", feather=0.0, with_mask=True)


def test_multiply_all_byte_pairs():
    K.check_multiply(*gpu_ctx())


def test_invalid_arguments():
    K.check_paste_invalid(*gpu_ctx())


def test_paste_back_three_sizes():
    """face_align.paste_back on a list of three photographs of three sizes, each in another image form, the results in the
    three forms a result takes (float tensor, uint8 tensor, PIL image) - against the restatement; then one by one."""
    from hairfastgan_amd import face_align as FA

    _, _, dev = gpu_ctx()
    names = ["up", "rot30", "corner of a 140 x 110 photograph"]
    S = 64
    F = K.inputs("up")[1]
    cases = [(K.inputs("up")[0], K.inputs("up")[2]), (K.inputs("rot30")[0], K.inputs("rot30")[2]),
             (R.image(140, 110, 25), R.landmarks(24, 22, 20, 7.0))]
    assert len({p.shape for p, _ in cases}) == 3
    photos = [K.chw(cases[0][0], dev), PIL.Image.fromarray(cases[1][0], "RGB"), cases[2][0]]  # tensor, PIL image, HWC array
    kept = photos[0].clone()
    F_chw = K.chw(F, dev)
    results = [FA.unit_float(F_chw), F_chw, PIL.Image.fromarray(F, "RGB")]  # byte / 255 quantises back to the byte
    lms = [lm for _, lm in cases]
    outs = FA.paste_back(photos, results, lms, output_size=S, return_tensors=False)
    floats = FA.paste_back(photos, results, lms, output_size=S)
    assert torch.equal(photos[0], kept)
    for n, (arr, lm), out, f, photo, res in zip(names, cases, outs, floats, photos, results):
        ref = np.asarray(PR.paste(PIL.Image.fromarray(arr, "RGB"), PIL.Image.fromarray(F, "RGB"), lm)["out"])
        assert out.dtype == torch.uint8 and out.shape == (3, *arr.shape[:2]) and out.is_cuda, n
        assert np.array_equal(K.hwc(out), ref), n
        assert f.dtype == torch.float32 and torch.equal(f.cpu(), out.cpu().float().div(255)), n
        assert torch.equal(FA.paste_back(photo, res, lm, output_size=S, return_tensors=False), out), n  # one photograph: one tensor
    # a float crop-space mask and another feather through the public call
    mask = K.user_mask(S)
    out = FA.paste_back(photos[0], results[0], lms[0], mask=torch.from_numpy(mask), feather=0.25, output_size=S, return_tensors=False)
    ref = PR.paste(PIL.Image.fromarray(cases[0][0], "RGB"), PIL.Image.fromarray(F, "RGB"), lms[0], 0.25, mask)["out"]
    assert np.array_equal(K.hwc(out), np.asarray(ref))
    with pytest.raises(ValueError):
        FA.paste_back(photos[0], results[0], lms[0], output_size=2 * S)   # the result is not [3, 128, 128]
    with pytest.raises(ValueError):
        FA.paste_back(photos, results[:2], lms, output_size=S)


def test_swap_paste_back():
    """swap(..., align=True, paste_back=True) on the synthetic-parameter HairFast: the first four values bit-equal to the
    call without paste_back, the fifth face_align.paste_back of them, the photograph untouched; the same through
    swap_batch; HairFast.paste_back from arrays and from the detector callable."""
    from hairfastgan_amd import face_align as FA
    from tests.test_gpu_schedule import _hairfast

    _, _, dev = gpu_ctx()
    hf = _hairfast(dev)
    cases = [R.GOLDEN_CASES["inside"], R.GOLDEN_CASES["corner"], (640, 480, 17, (330, 200, 70, -11.0))]
    pairs = [R.case_inputs(c) for c in cases]
    images = [K.chw(arr, dev) for arr, _ in pairs]
    kept = images[0].clone()
    lms = [lm for _, lm in pairs]
    plain = hf.swap(*images, align=True, landmarks=lms, seed=7)
    out = hf.swap(*images, align=True, landmarks=lms, seed=7, paste_back=True)
    assert len(plain) == 4 and len(out) == 5
    assert all(torch.equal(a, b) for a, b in zip(out[:4], plain))
    assert torch.equal(images[0], kept)
    pasted = out[4]
    assert pasted.dtype == torch.float32 and pasted.shape == images[0].shape and pasted.is_cuda
    assert torch.equal(pasted, FA.paste_back(images[0], out[0], lms[0]))
    # against the restatement, from the bytes save_image would write for `final`
    final_u8 = (out[0].cpu() * 255 + 0.5).clamp(0, 255).to(torch.uint8).numpy().transpose(1, 2, 0)
    ref = PR.paste(PIL.Image.fromarray(pairs[0][0], "RGB"), PIL.Image.fromarray(final_u8, "RGB"), lms[0])
    assert ref["inverse"]["n"] < 1024  # the face is smaller than the crop: the result is reduced first
    assert torch.equal(pasted.cpu(), torch.from_numpy(np.asarray(ref["out"]).transpose(2, 0, 1).copy()).float().div(255))
    assert not torch.equal(pasted, images[0].float().div(255))

    batch = hf.swap_batch([tuple(images)], align=True, landmarks=[lms], seed=7, paste_back=True)
    assert len(batch) == 1 and len(batch[0]) == 5
    assert all(torch.equal(a, b) for a, b in zip(batch[0], out))

    assert torch.equal(hf.paste_back(out[0], images[0], landmarks=lms[0]), pasted)
    seen = []

    def detector(image):
        seen.append(image.shape)
        return next(lm for arr, lm in pairs if np.array_equal(arr, image))

    hf.landmark_detector = detector
    assert torch.equal(hf.paste_back(out[0], pairs[0][0]), pasted) and seen == [pairs[0][0].shape]  # an HWC array as the photograph
    hf.landmark_detector = None
    with pytest.raises(NotImplementedError):
        hf.paste_back(out[0], images[0])
    with pytest.raises(ValueError):
        hf.swap(*images, paste_back=True)
    with pytest.raises(ValueError):
        hf.swap_batch([tuple(images)], paste_back=True)
