"""`poisson_image_blending` of the reference's utils/image_utils.py:58-94 on the MI355X kernels.

The reference parses the swap result and the source face with BiSeNet, frees the union of their hair regions, grows
it by `dilate_erosion` rounds of 4-neighbour dilation, writes final / face / mask as PNGs (torchvision `save_image`)
and runs `fpie -s face -t final -m mask -n maxn -b taichi-gpu -g max`: Poisson image editing that pastes the face's
non-hair region back into the result with mixed ("max") gradients.  Here every step runs on the HIP library:

1. masks: ONE BiSeNet parse of the 2T images (hairfastgan_amd.face_parsing), hair = CelebAMask label 13,
   keep = (1 - hair_final) * (1 - hair_face); the reference's bicubic resize to 1024^2 is the identity at that size;
2. free mask: mask = 1 - dilate(1 - keep), `dilate_erosion` rounds of the cross (hf_dilate_erode_f32);
3. PNG round trip: save_image's bytes of final, face and mask (hf_quantize_u8_f32);
4. fpie's solve: setup of the right-hand side, `maxn` synchronous Jacobi sweeps blocked T deep in LDS, the u8 result
   (hf_poisson_setup_u8 / hf_poisson_jacobi_f32 / hf_poisson_finish_u8).

Quirk kept from the reference: the images go into BiSeNet UN-normalised, as [0,1] RGB (the swap path normalises its
parser input with the ImageNet statistics; utils/image_utils.py:66-67 does not).

What is pinned: BiSeNet (oracle/ref_bisenet.py), the dilation (the reference's F.conv2d loop) and the save_image
quantisation are pinned to the reference through the oracle.  Step 4 is a restatement of fpie's equation solver,
whose source is not available: three details are unverified - the mask threshold (byte >= 128), the sweep-count
convention (`-n maxn` = maxn sweeps from X_0 = target) and truncation (not rounding) of the solution to bytes.
fpie's GPU backends may order the updates differently; they solve the same discrete system, and the synchronous form
here is the deterministic definition the tests pin (tests/poisson_ref.py).

Deviations from the reference, by design:
* final and face must have the same H x W; the mask follows that size (the reference hard-codes 1024^2);
* an empty solve region (fpie fails on it) returns save_image's bytes of `final` unchanged;
* nothing is written to disk and no external tool runs; `poisson_blend` is a batched form the reference lacks.

Also here: the image side of `--save_all` (utils/save_utils.py:12-30) - `to_bytes` (ToPILImage's / save_image's bytes of
float images, hf_image_to_bytes_f32), `labels_to_rgb` (`mask_to_rgb(pred, 0)`, hf_labels_to_rgb_i64) and `save_image`
(main.py:44's torchvision call for one image).  The bytes are made on the device: a quarter of the float image crosses to
the host.  `encode_png` / `save_images` / `save_image(encoder="device")` make the PNG file itself on the device
(hf_png_encode_u8): only the compressed bytes cross and no zlib runs on the host.  `encode_jpeg` and `format="jpeg"` do the
same for JPEG (hf_jpeg_encode_u8): the file Pillow's libjpeg would write, without the pixels crossing to the host.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _marshal as M
from ._runtime import lib, require_gpu, stream
from .face_parsing import get_segmentation

HAIR = 13                # CelebAMask label order (face_parsing.LABEL_REMAP)
DEFAULT_TBLOCK = 8       # sweeps per launch of the Jacobi chain: measured, profiles/poisson_bench.json
_PARSING = None          # the default BiSeNet, built once (the reference's singleton, my_parsing_util.py:77-79)
UNKNOWN_LABEL = 255      # drawn white by labels_to_rgb
# The colour of each of the 19 CelebAMask-HQ labels in a `--save_all` mask PNG (label -> R, G, B; the values
# `mask_to_rgb(pred, draw_type=0)` of models/CtrlHair/util/mask_color_util.py draws, pinned by tests/golden/mask_colors.npz).
LABEL_COLORS = {
    0: (0, 128, 64), 1: (204, 0, 0), 2: (76, 153, 0), 3: (204, 204, 0), 4: (51, 51, 255), 5: (204, 0, 204), 6: (0, 255, 255),
    7: (51, 255, 255), 8: (102, 51, 0), 9: (255, 0, 0), 10: (102, 204, 0), 11: (255, 255, 0), 12: (0, 0, 153),
    HAIR: (0, 0, 204), 14: (255, 51, 153), 15: (0, 204, 204), 16: (0, 51, 0), 17: (255, 153, 51), 18: (0, 204, 0),
}
_PALETTES = {}           # device -> the table as a 57-byte uint8 buffer [19,3]


def default_parsing(device="cuda"):
    """BiSeNet from pretrained_models/BiSeNet/face_parsing_79999_iter.pth (cwd / HAIRFAST_PRETRAINED_ROOT), built once;
    FileNotFoundError if the checkpoint is missing."""
    global _PARSING
    if _PARSING is None:
        from .hair_swap import build_parsing

        _PARSING = build_parsing(SimpleNamespace(device=device))
    return _PARSING


def poisson_solve(L, st, src, tgt, mask, maxn, tblock=None):
    """fpie's solve on u8 tensors: src (face) / tgt (final) [N,C,H,W], mask [N,1,H,W] -> (u8 result [N,C,H,W], fp32 X).
    `maxn` sweeps: launches of `tblock` sweeps, the remainder in one launch of the shallowest instance that holds it;
    the result is the same bits for every tblock."""
    T = DEFAULT_TBLOCK if tblock is None else tblock
    if T not in M.POISSON_TBLOCKS:
        raise ValueError(f"tblock must be one of {M.POISSON_TBLOCKS}; got {T}")
    if maxn < 0:
        raise ValueError(f"maxn must be >= 0; got {maxn}")
    b, x = M.poisson_setup(L, st, src, tgt, mask)
    full, rest = divmod(int(maxn), T)
    launches = [(T, T)] * full + ([(rest, min(t for t in M.POISSON_TBLOCKS if t >= rest))] if rest else [])
    y = torch.empty_like(x) if launches else None
    for sweeps, depth in launches:
        M.poisson_jacobi_into(L, st, y, x, b, mask, sweeps, depth)
        x, y = y, x
    return M.poisson_finish(L, st, x, tgt, mask), x


def blend_masks(parsing, finals, faces, dilate_erosion=30):
    """Steps 1-3 for T pairs: finals / faces fp32 [T,3,H,W] in [0,1] on the GPU -> u8 free mask [T,1,H,W] (0 / 255:
    255 where the face is pasted back).  One BiSeNet call on the 2T images."""
    T = finals.shape[0]
    L, st = lib(), stream()
    labels = get_segmentation(parsing, torch.cat([finals, faces]), resize=False)  # un-normalised input: the reference's quirk
    hair = labels == HAIR
    free = (hair[:T] | hair[T:]).float()                                           # 1 - keep
    dilated, _ = M.dilate_erode(L, st, free, dilate_erosion)
    return M.quantize_u8(L, st, 1.0 - dilated)


@torch.inference_mode()
def poisson_blend(finals, faces, dilate_erosion=30, maxn=115, parsing=None, tblock=None):
    """Batched GPU form of `poisson_image_blending`: finals (swap results) and faces fp32 [T,3,H,W] in [0,1] ->
    (u8 result [T,3,H,W], u8 mask [T,1,H,W]).  One BiSeNet call on 2T images and one solver chain; each image's
    bytes equal those of a T = 1 call (batch-invariant plans, the library default; hairfastgan_amd._runtime)."""
    if finals.ndim != 4 or finals.shape[1] != 3 or finals.shape != faces.shape:
        raise ValueError(f"finals and faces must both be [T,3,H,W]; got {tuple(finals.shape)} and {tuple(faces.shape)}")
    if not 0 <= dilate_erosion <= 64:
        raise ValueError(f"dilate_erosion must be in [0, 64]; got {dilate_erosion}")
    require_gpu(finals, faces)
    parsing = parsing if parsing is not None else default_parsing(finals.device)
    finals, faces = finals.float().contiguous(), faces.float().contiguous()
    mask = blend_masks(parsing, finals, faces, dilate_erosion)
    L, st = lib(), stream()
    out, _ = poisson_solve(L, st, M.quantize_u8(L, st, faces), M.quantize_u8(L, st, finals), mask, maxn, tblock)
    return out, mask


def _as_image(img, device):
    """Tensor [3,H,W] (float in [0,1] as is; uint8 / 255 on the CPU); a path or PIL image through ToTensor."""
    from .hair_swap import HairFast

    if isinstance(img, torch.Tensor) and img.dtype is not torch.uint8:
        t = img
    else:
        if isinstance(img, str) or hasattr(img, "__fspath__"):
            from PIL import Image

            with Image.open(img) as im:  # transforms.ToTensor()(Image.open(path))
                im.load()
                img = im.copy()
        t = HairFast._as_tensor(img)
        if t.dtype is torch.uint8:
            t = t.cpu().to(torch.float32).div(255)
    if t.ndim != 3 or t.shape[0] != 3:
        raise ValueError(f"expected a 3-channel image [3,H,W]; got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32)


def _to_pil(u8_hw3):
    from PIL import Image

    return Image.fromarray(np.ascontiguousarray(u8_hw3.cpu().numpy()), "RGB")


def poisson_image_blending(final_image, face_image, dilate_erosion=30, maxn=115, *, parsing=None, tblock=None):
    """utils/image_utils.py:58-94: final_image [3,H,W] float in [0,1] (what `swap` returns), face_image a path, a PIL
    image or a tensor of the same H x W -> (PIL result, PIL mask), both RGB; the mask is 255 where the face was pasted
    back.  `parsing`: a BiSeNet (default: built once from its checkpoint, FileNotFoundError if missing)."""
    return poisson_image_blending_many([final_image], [face_image], dilate_erosion, maxn, parsing=parsing, tblock=tblock)[0]


def poisson_image_blending_many(final_images, face_images, dilate_erosion=30, maxn=115, *, parsing=None, tblock=None):
    """`poisson_image_blending` for lists of pairs of one size (e.g. `HairFast.swap_batch` results and their faces) as ONE
    `poisson_blend` call -> list of (PIL result, PIL mask)."""
    if len(final_images) != len(face_images) or not final_images:
        raise ValueError("one face image per final image, at least one pair")
    first = final_images[0]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device("cuda")
    finals = [_as_image(x, dev) for x in final_images]
    faces = [_as_image(x, dev) for x in face_images]
    if len({tuple(x.shape) for x in finals + faces}) != 1:
        raise ValueError(f"final and face images must all have one size; got {sorted({tuple(x.shape) for x in finals + faces})}")
    out, mask = poisson_blend(torch.stack(finals), torch.stack(faces), dilate_erosion, maxn, parsing=parsing, tblock=tblock)
    return [(_to_pil(out[i].permute(1, 2, 0)), _to_pil(mask[i, 0, :, :, None].expand(-1, -1, 3))) for i in range(len(finals))]


# ---------------------------------------------------------------------------------------------
# bytes of images and label maps (--save_all; csrc/export.h)
# ---------------------------------------------------------------------------------------------
ROUNDINGS = {"floor": 0, "nearest": 1}
LAYOUTS = {"hwc": 1, "chw": 0}


def _images_4d(images, what):
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor; got {type(images)}")
    if images.dtype != torch.float32:
        raise TypeError(f"{what}: expected a float32 tensor; got {images.dtype}")
    if images.ndim not in (3, 4):
        raise ValueError(f"{what}: expected [3,H,W] or [B,3,H,W]; got {tuple(images.shape)}")
    if images.shape[-3] != 3:
        raise ValueError(f"{what}: expected 3 channels; got {tuple(images.shape)}")
    return images if images.ndim == 4 else images.unsqueeze(0)


def to_bytes(images, value_range=(-1, 1), rounding="floor", layout="hwc"):
    """Float images fp32 [B,3,H,W] (or [3,H,W]) on the GPU -> uint8 [B,H,W,3] (`layout="hwc"`, what PIL takes) or [B,3,H,W]
    ("chw"), byte-equal to the torch expressions of the reference:
      rounding="floor",   value_range=(-1, 1): `save_gen_image` - ToPILImage of ((x + 1) / 2).clamp(0, 1): trunc(t * 255)
      rounding="nearest", value_range=(0, 1):  `torchvision.utils.save_image` - x.mul(255).add(0.5).clamp(0, 255), truncated
    value_range=(lo, hi) maps t = (x - lo) / (hi - lo) first.  NaN gives 0."""
    batched = isinstance(images, torch.Tensor) and images.ndim == 4
    x = _images_4d(images, "to_bytes")
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be one of {tuple(ROUNDINGS)}; got {rounding!r}")
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {tuple(LAYOUTS)}; got {layout!r}")
    lo, hi = value_range
    if not float(hi) > float(lo):
        raise ValueError(f"value_range needs lo < hi; got {value_range}")
    require_gpu(x)
    out = M.image_to_bytes(lib(), stream(), x, lo, hi, ROUNDINGS[rounding], LAYOUTS[layout])
    return out if batched else out[0]


def label_palette(device):
    """LABEL_COLORS as the uint8 [19,3] device buffer hf_labels_to_rgb_i64 reads (57 bytes, made once per device)."""
    device = torch.device(device)
    if device not in _PALETTES:
        _PALETTES[device] = torch.tensor([LABEL_COLORS[k] for k in range(len(LABEL_COLORS))], dtype=torch.uint8).to(device)
    return _PALETTES[device]


def labels_to_rgb(labels):
    """`mask_to_rgb(pred, 0)` (models/CtrlHair/util/mask_color_util.py:15-64) on the GPU: int64 label maps [B,1,H,W] (or
    [B,H,W] / [H,W]) -> uint8 [B,H,W,3] ([H,W,3]).  Labels 0..18 take LABEL_COLORS, 255 is white, anything else black."""
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels_to_rgb: expected a torch.Tensor; got {type(labels)}")
    if labels.dtype != torch.int64:
        raise TypeError(f"labels_to_rgb: expected int64 labels; got {labels.dtype}")
    if labels.ndim == 4:
        if labels.shape[1] != 1:
            raise ValueError(f"labels_to_rgb: expected one channel [B,1,H,W]; got {tuple(labels.shape)}")
        labels = labels[:, 0]
    elif labels.ndim not in (2, 3):
        raise ValueError(f"labels_to_rgb: expected [B,1,H,W], [B,H,W] or [H,W]; got {tuple(labels.shape)}")
    require_gpu(labels)
    return M.labels_to_rgb(lib(), stream(), labels, label_palette(labels.device), UNKNOWN_LABEL)


def save_image(image, path, value_range=(0, 1), rounding="nearest", encoder="pil", format=None, quality=75,
               subsampling="4:2:0", **pil_kwargs):
    """`torchvision.utils.save_image(image, path)` for ONE image (main.py:44) without torchvision: fp32 [3,H,W] (or
    [1,3,H,W]) in [0,1] on the GPU -> `to_bytes(value_range, rounding)`, then `encoder`: "pil" - the bytes go to the host and
    PIL makes the file, `pil_kwargs` go to `Image.save`; "device" - `encode_png` / `encode_jpeg` makes the file on the GPU and
    only its bytes cross (no `pil_kwargs`).  `format`: None - PNG from the device encoder whatever the suffix, PIL chooses by
    the suffix; "jpeg" - baseline JPEG of `quality` and `subsampling` with one restart interval per MCU row, the same file
    from both encoders (`save_images` has the details)."""
    if encoder not in ENCODERS:
        raise ValueError(f"encoder must be one of {ENCODERS}; got {encoder!r}")
    if encoder == "device" and pil_kwargs:
        raise TypeError(f"save_image(encoder='device') takes no PIL arguments; got {sorted(pil_kwargs)}")
    _check_format(format, quality, subsampling)
    x = _images_4d(image, "save_image")
    if x.shape[0] != 1:
        raise ValueError(f"save_image writes one image; got a batch of {x.shape[0]}")
    if encoder == "device":
        save_images(x, [path], value_range, rounding, "device", format, quality, subsampling)
    else:
        _to_pil(to_bytes(x, value_range, rounding, "hwc")[0]).save(path, **_pil_format(format, quality, subsampling), **pil_kwargs)


# ---------------------------------------------------------------------------------------------
# PNG files made on the device (csrc/png.h)
# ---------------------------------------------------------------------------------------------
ENCODERS = ("pil", "device")
PNG_FILTERS = M.PNG_FILTERS


FORMATS = (None, "jpeg")
JPEG_SUBSAMPLINGS = M.JPEG_SUBSAMPLINGS


def _check_format(format, quality, subsampling):
    if format not in FORMATS:
        raise ValueError(f"format must be one of {FORMATS}; got {format!r}")
    if format is None and (quality != 75 or subsampling != "4:2:0"):
        raise TypeError("quality and subsampling belong to format='jpeg'")
    if format == "jpeg":
        _check_jpeg(quality, subsampling)


def _check_jpeg(quality, subsampling):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"quality must be an integer in 1..100; got {quality!r}")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {tuple(JPEG_SUBSAMPLINGS)}; got {subsampling!r}")


def _pil_format(format, quality, subsampling):
    """`Image.save` arguments with which PIL writes the file the device encoder writes."""
    if format is None:
        return {}
    return {"format": "JPEG", "quality": quality, "subsampling": subsampling, "restart_marker_rows": 1}


def fetch_files(files, sizes, rows=None):
    """The files of `M.png_encode` / `M.jpeg_encode` on the host: {row: bytes} for `rows` (default: all).  One
    synchronisation (the copy of `sizes`), then one copy of exactly the encoded bytes."""
    n = sizes.cpu().tolist()
    rows = list(range(len(n))) if rows is None else sorted(set(rows))
    parts = [files[r, :n[r]] for r in rows]
    host = (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy().tobytes()
    out, pos = {}, 0
    for r in rows:
        out[r] = host[pos:pos + n[r]]
        pos += n[r]
    return out


def _u8_images(images, what):
    """The input forms of encode_png / encode_jpeg -> (uint8 [B,H,W,1|3], whether it was a single image)."""
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor; got {type(images)}")
    if images.dtype != torch.uint8:
        raise TypeError(f"{what}: expected uint8 images; got {images.dtype}")
    if images.ndim == 2:
        return images[None, :, :, None], True
    if images.ndim == 3 and images.shape[-1] == 3:  # [H,W,3]; a batch of three-pixel-wide grey images goes in as [B,H,3,1]
        return images[None], True
    if images.ndim == 3:
        return images[..., None], False
    if images.ndim == 4 and images.shape[-1] in (1, 3):
        return images, False
    raise ValueError(f"{what}: expected [B,H,W,3], [B,H,W,1], [B,H,W], [H,W,3] or [H,W]; got {tuple(images.shape)}")


def encode_png(images, filter="adaptive"):
    """uint8 images on the GPU - [B,H,W,3], [B,H,W,1], [B,H,W], [H,W,3] or [H,W] - -> list of B complete PNG files as
    `bytes` (a single image: `bytes`), RGB or greyscale, encoded on the device (hf_png_encode_u8: row filters, one
    dynamic-Huffman block with distance-1 matches per group of rows, checksums).  `filter`: "none",
    "sub", "up" on every row, or "adaptive" (per row the type with the smallest sum of absolute residuals).  A file decodes
    to exactly the input bytes; it is not the file PIL would write.  One encode call, one synchronisation, one copy."""
    x, single = _u8_images(images, "encode_png")
    if filter not in PNG_FILTERS:
        raise ValueError(f"filter must be one of {tuple(PNG_FILTERS)}; got {filter!r}")
    require_gpu(x)
    files = fetch_files(*M.png_encode(lib(), stream(), x, PNG_FILTERS[filter]))
    return files[0] if single else [files[k] for k in range(x.shape[0])]


def encode_jpeg(images, quality=75, subsampling="4:2:0"):
    """uint8 images on the GPU - [B,H,W,3], [B,H,W,1], [B,H,W], [H,W,3] or [H,W], the forms `encode_png` takes; the
    uint8 photograph of `paste_back(..., return_tensors=False)` is planar [3,H,W] and goes in as its `.permute(1, 2, 0)` view,
    the float one through `to_bytes(x, (0, 1), "nearest")` or `save_image(format="jpeg")` - -> list of B complete JPEG files as `bytes` (a single
    image: `bytes`), encoded on the device (hf_jpeg_encode_u8).  Baseline JFIF, YCbCr or greyscale,
    `quality` 1..100 with libjpeg's tables, `subsampling` "4:4:4", "4:2:2" or "4:2:0" (no effect on grey images), the standard
    Huffman tables, one restart interval per MCU row: byte for byte the file of
    `PIL.Image.save(format="JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)`.  One encode call, one
    synchronisation, one copy of exactly the encoded bytes."""
    x, single = _u8_images(images, "encode_jpeg")
    _check_jpeg(quality, subsampling)
    require_gpu(x)
    files = fetch_files(*M.jpeg_encode(lib(), stream(), x, quality, JPEG_SUBSAMPLINGS[subsampling]))
    return files[0] if single else [files[k] for k in range(x.shape[0])]


def save_images(images, paths, value_range=(0, 1), rounding="nearest", encoder="device", format=None, quality=75,
                subsampling="4:2:0"):
    """A batch of float images fp32 [B,3,H,W] on the GPU to `paths` (one per image): ONE `to_bytes` call and, with
    encoder="device", ONE `encode_png` / `encode_jpeg` call; "pil" encodes each image on the host.  `format=None`: PNG files
    from the device encoder whatever the suffix, PIL chooses by the suffix.  `format="jpeg"`: JPEG of `quality` (1..100) and
    `subsampling` ("4:4:4", "4:2:2", "4:2:0"); PIL is then called with restart_marker_rows=1, so both encoders write the same
    file.  `quality` or `subsampling` other than the defaults without format="jpeg" is a TypeError."""
    if encoder not in ENCODERS:
        raise ValueError(f"encoder must be one of {ENCODERS}; got {encoder!r}")
    _check_format(format, quality, subsampling)
    x = _images_4d(images, "save_images")
    paths = list(paths)
    if len(paths) != x.shape[0]:
        raise ValueError(f"save_images: {x.shape[0]} images, {len(paths)} paths")
    u8 = to_bytes(x, value_range, rounding, "hwc")
    if encoder == "device":
        for path, data in zip(paths, encode_png(u8) if format is None else encode_jpeg(u8, quality, subsampling)):
            with open(path, "wb") as fh:
                fh.write(data)
    else:
        host = u8.cpu()
        for k, path in enumerate(paths):
            _to_pil(host[k]).save(path, **_pil_format(format, quality, subsampling))
