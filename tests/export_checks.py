"""TEST INFRASTRUCTURE - the comparisons of the `--save_all` byte kernels (csrc/export.h) shared by the hipsim tests
(tests/test_sim_export.py) and the GPU tests (tests/test_gpu_export.py): every function takes the library, the stream and
the device to run on.

hf_image_to_bytes_f32: byte-EQUAL to the torch expression of the reference, evaluated on the CPU -
  floor:    ((x + 1) / 2).clamp(0, 1).mul(255).byte()               (utils/save_utils.py:15, ToPILImage)
  nearest:  x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)       (torchvision.utils.save_image)
with the range step of the other range in front ((x + 1) / 2 for (-1, 1), nothing for (0, 1)).  The inputs are not noise:
for every byte k the float32 nearest each rule's boundary - 2k/255 - 1 and k/255 (floor), (k - 0.5)/255 and its (-1, 1)
form (2k - 1)/255 - 1 (nearest) - with its two `nextafter` neighbours, plus -1, 1, +-1.5, -0.0 and +-inf: 3080 values,
fed through each shape in consecutive chunks (the last one filled by wrapping around).  One NaN per case is checked
against the stated 0, not against torch.

hf_labels_to_rgb_i64: tests/golden/mask_colors.npz holds the reference's `mask_to_rgb(pred, 0)` of every label 0..20 and 255
(tools/make_export_golden.py); 254, -1 and 2^40 must be black."""
import functools
import os

import numpy as np
import torch

from hairfastgan_amd import _marshal as M
from hairfastgan_amd import image_utils as IU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_colors.npz")

# [B,3,H,W]: scalar tail on every row and odd row starts / the vector path only / vector body over more than one wave /
# one pixel per image
SHAPES = [(2, 3, 5, 7), (1, 3, 4, 8), (1, 3, 3, 260), (3, 3, 1, 1)]
RANGES = [(-1, 1), (0, 1)]


@functools.lru_cache(maxsize=None)
def boundary_values():
    k = np.arange(256, dtype=np.float64)
    centres = np.concatenate([2 * k / 255 - 1, k / 255, (k - 0.5) / 255, (2 * k - 1) / 255 - 1]).astype(np.float32)
    vals = np.concatenate([centres, np.nextafter(centres, np.float32(-np.inf)), np.nextafter(centres, np.float32(np.inf)),
                           np.array([-1, 1, 1.5, -1.5, -0.0, np.inf, -np.inf, 0.5], np.float32)])
    assert vals.dtype == np.float32 and vals.size == 3080
    return torch.from_numpy(vals)


def expected_bytes(x, value_range, rounding, layout):
    """The reference's torch expression on the CPU tensor x [B,3,H,W]."""
    t = (x + 1) / 2 if value_range == (-1, 1) else x
    if rounding == "floor":
        out = t.clamp(0, 1).mul(255).byte()
    else:
        out = t.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
    return out.permute(0, 2, 3, 1).contiguous() if layout == "hwc" else out


def chunks(shape):
    vals = boundary_values()
    n = int(np.prod(shape))
    for c0 in range(0, vals.numel(), n):
        idx = (torch.arange(n) + c0) % vals.numel()
        yield vals[idx].reshape(shape)


def check_to_bytes(L, st, device, shape, value_range, rounding, layout):
    lo, hi = value_range
    for x in chunks(shape):
        got = M.image_to_bytes(L, st, x.to(device), lo, hi, IU.ROUNDINGS[rounding], IU.LAYOUTS[layout]).cpu()
        ref = expected_bytes(x, value_range, rounding, layout)
        assert got.shape == ref.shape and got.dtype == torch.uint8
        assert torch.equal(got, ref), (shape, value_range, rounding, layout, int((got != ref).sum()))
    # one NaN (in the middle of a group of four where the vector path runs): the stated 0, every other byte unchanged
    x = next(chunks(shape)).clone()
    flat = x.view(-1)
    pos = min(1, flat.numel() - 1)
    flat[pos] = float("nan")
    got = M.image_to_bytes(L, st, x.to(device), lo, hi, IU.ROUNDINGS[rounding], IU.LAYOUTS[layout]).cpu()
    clean = x.clone()
    clean.view(-1)[pos] = -8.0  # any value that gives 0 under both rules
    ref = expected_bytes(clean, value_range, rounding, layout)
    assert torch.equal(got, ref), (shape, value_range, rounding, layout, "NaN")


def check_to_bytes_unaligned(L, st, device):
    """A row width the vector path takes, on a base 4 bytes past a 16-byte boundary: the scalar path, same bytes."""
    shape = (1, 3, 4, 8)
    x = next(chunks(shape))
    buf = torch.zeros(x.numel() + 4, dtype=torch.float32, device=device)
    view = buf[1:1 + x.numel()].view(shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    for rounding in IU.ROUNDINGS:
        for layout in IU.LAYOUTS:
            got = M.image_to_bytes(L, st, view, -1, 1, IU.ROUNDINGS[rounding], IU.LAYOUTS[layout]).cpu()
            assert torch.equal(got, expected_bytes(x, (-1, 1), rounding, layout)), (rounding, layout)


def check_general_range(L, st, device):
    """A range that is neither of the two: t = (x - lo) / (hi - lo), each step one float32 rounding."""
    x = next(chunks((1, 3, 3, 260)))
    lo, hi = -0.25, 2.5
    t = (x - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    got = M.image_to_bytes(L, st, x.to(device), lo, hi, 0, 1).cpu()
    assert torch.equal(got, t.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def golden_masks():
    with np.load(GOLDEN) as g:
        return g["labels"].copy(), g["rgb"].copy()


def check_labels_to_rgb(L, st, device):
    labels, rgb = golden_masks()                     # [2,5,7] with every value of 0..20 and 255, [2,5,7,3]
    assert set(labels.reshape(-1).tolist()) == set(range(21)) | {255}
    labels, rgb = labels.copy().reshape(-1), rgb.copy().reshape(-1, 3)
    for pos, value in zip((66, 67, 68), (254, -1, 2 ** 40)):  # positions whose golden value (0, 1, 2) also occurs earlier
        labels[pos] = value
        rgb[pos] = 0
    assert set(labels.tolist()) == set(range(21)) | {254, 255, -1, 2 ** 40}
    t = torch.from_numpy(labels.reshape(2, 1, 5, 7)).to(device)
    got = M.labels_to_rgb(L, st, t[:, 0], IU.label_palette(device)).cpu().numpy()
    assert got.shape == (2, 5, 7, 3) and got.dtype == np.uint8
    assert np.array_equal(got, rgb.reshape(2, 5, 7, 3)), np.argwhere((got != rgb.reshape(2, 5, 7, 3)).any(-1))
    assert (got.reshape(-1, 3)[labels == 255] == 255).all() and (got.reshape(-1, 3)[labels == 20] == 0).all()
    return t


def check_palette_is_the_goldens():
    labels, rgb = golden_masks()
    for k, colour in IU.LABEL_COLORS.items():
        assert (rgb[labels == k] == np.array(colour, np.uint8)).all(), k
    assert sorted(IU.LABEL_COLORS) == list(range(19)) and IU.label_palette("cpu").numel() == 57


def check_invalid(L, st, device):
    x = torch.zeros(1, 3, 4, 8, device=device)
    out = torch.zeros(1, 4, 8, 3, dtype=torch.uint8, device=device)
    lab = torch.zeros(4, 8, dtype=torch.int64, device=device)
    pal = IU.label_palette(device)
    calls = {
        "null out": lambda: L.hf_image_to_bytes_f32(None, x.data_ptr(), 1, 4, 8, -1.0, 1.0, 0, 1, st),
        "null in": lambda: L.hf_image_to_bytes_f32(out.data_ptr(), None, 1, 4, 8, -1.0, 1.0, 0, 1, st),
        "hi == lo": lambda: L.hf_image_to_bytes_f32(out.data_ptr(), x.data_ptr(), 1, 4, 8, 1.0, 1.0, 0, 1, st),
        "hi < lo": lambda: L.hf_image_to_bytes_f32(out.data_ptr(), x.data_ptr(), 1, 4, 8, 1.0, -1.0, 0, 1, st),
        "no rows": lambda: L.hf_image_to_bytes_f32(out.data_ptr(), x.data_ptr(), 1, 0, 8, -1.0, 1.0, 0, 1, st),
        "null palette": lambda: L.hf_labels_to_rgb_i64(out.data_ptr(), lab.data_ptr(), 32, None, 19, 255, st),
        "null labels": lambda: L.hf_labels_to_rgb_i64(out.data_ptr(), None, 32, pal.data_ptr(), 19, 255, st),
        "no pixels": lambda: L.hf_labels_to_rgb_i64(out.data_ptr(), lab.data_ptr(), 0, pal.data_ptr(), 19, 255, st),
    }
    for what, call in calls.items():
        try:
            M.check(L, call(), what)
        except RuntimeError as e:
            assert "invalid argument" in str(e), (what, e)
        else:
            raise AssertionError(f"{what}: must be refused")
    assert not out.cpu().any()  # nothing was launched
    # the Python side: dtype, rank and channel count, before anything reaches the library
    for exc, call in [(TypeError, lambda: M.image_to_bytes(L, st, x.double(), -1, 1, 0, 1)),
                      (ValueError, lambda: M.image_to_bytes(L, st, x[:, :2], -1, 1, 0, 1)),
                      (ValueError, lambda: M.image_to_bytes(L, st, x[0], -1, 1, 0, 1)),
                      (ValueError, lambda: M.image_to_bytes(L, st, x, 1, 1, 0, 1)),
                      (TypeError, lambda: M.labels_to_rgb(L, st, lab.int(), pal)),
                      (ValueError, lambda: M.labels_to_rgb(L, st, lab, pal[:, :2])),
                      (TypeError, lambda: IU.to_bytes(x.half())),
                      (TypeError, lambda: IU.to_bytes(x.cpu().numpy())),
                      (ValueError, lambda: IU.to_bytes(x[:, :1])),
                      (ValueError, lambda: IU.to_bytes(x, rounding="round")),
                      (ValueError, lambda: IU.to_bytes(x, layout="nhwc")),
                      (ValueError, lambda: IU.to_bytes(x, value_range=(1, 0))),
                      (TypeError, lambda: IU.labels_to_rgb(lab.float())),
                      (ValueError, lambda: IU.labels_to_rgb(lab[None, None].expand(1, 2, 4, 8))),
                      (ValueError, lambda: IU.save_image(x.expand(2, 3, 4, 8), "unused.png")),
                      (TypeError, lambda: IU.save_image(out, "unused.png"))]:
        try:
            call()
        except exc:
            pass
        else:
            raise AssertionError(f"expected {exc.__name__}")
