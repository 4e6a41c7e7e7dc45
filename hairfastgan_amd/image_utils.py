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
`decode_jpeg` / `read_images(decoder="device")` are the way back (hf_jpeg_decode_u8): the host reads a baseline JPEG file's
header segments, the entropy-coded bytes go to the device as they are and the pixels Pillow would return are made there.
`decode_png` does the same for PNG files (hf_png_decode_u8): the host walks the chunks, the IDAT payloads go to the device as
they are, and inflate, the Adler-32, the row filters and the pixel conversion run there; `read_images(decoder="device")`
sends each file to the decoder of its kind.
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


def _fetch_encoded(x, single, encoded):
    files = fetch_files(*encoded)  # encoded: (files, sizes) of the batch x
    return files[0] if single else [files[k] for k in range(x.shape[0])]


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
    return _fetch_encoded(x, single, M.png_encode(lib(), stream(), x, PNG_FILTERS[filter]))


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
    return _fetch_encoded(x, single, M.jpeg_encode(lib(), stream(), x, quality, JPEG_SUBSAMPLINGS[subsampling]))


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


# ---------------------------------------------------------------------------------------------
# JPEG files decoded on the device (csrc/jpeg_decode.h)
# ---------------------------------------------------------------------------------------------
DECODERS = ("pil", "device")
JPEG_MODES = ("RGB", "unchanged")
_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic coding",
              0xCA: "arithmetic coding, progressive", 0xCB: "arithmetic coding, lossless", 0xCD: "arithmetic coding",
              0xCE: "arithmetic coding", 0xCF: "arithmetic coding"}
_ZIGZAG = np.array(sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8)))


def parse_jpeg_header(data):
    """The marker segments of a JPEG file from SOI to the end of SOS (pure Python, no GPU; the scan is not looked at) ->
    SimpleNamespace: height, width, components (1 or 3), hs, vs (luma sampling factors), restart_interval (0: none),
    scan_start (offset of the first entropy-coded byte) and tables - the uint8 [2048] record hf_jpeg_decode_u8 reads: the
    quantisation table of every component and its DC and AC Huffman tables.  ValueError, naming the property, for what the
    device decoder does not take: anything but baseline sequential Huffman coding (SOF0) with 8-bit samples and 8-bit
    quantisation tables; other than 1 or 3 components; an Adobe transform other than YCbCr; sampling other than 4:4:4,
    4:2:2 and 4:2:0; more than one scan - and for a header that is corrupt."""
    data = bytes(data) if not isinstance(data, bytes) else data
    if len(data) < 4 or data[:2] != b"\xFF\xD8":
        raise ValueError("not a JPEG file: no SOI marker")
    pos, qt, huff, ri, sof, adobe, jfif = 2, {}, {}, 0, None, None, False
    while True:
        while pos + 1 < len(data) and data[pos] == 0xFF and data[pos + 1] == 0xFF:  # fill bytes
            pos += 1
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError("corrupt JPEG header: no marker where one must stand")
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        if n < 2 or len(body) != n - 2:
            raise ValueError("corrupt JPEG header: a truncated segment")
        pos += 2 + n
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("unsupported JPEG: 16-bit quantisation tables")
                if len(body) < 65:
                    raise ValueError("corrupt JPEG header: a short DQT segment")
                qt[body[0] & 15] = np.frombuffer(body[1:65], np.uint8)
                body = body[65:]
        elif marker == 0xC4:
            while body:
                n_sym = sum(body[1:17]) if len(body) >= 17 else 257
                if n_sym > 256 or len(body) < 17 + n_sym or (body[0] & 15) > 3 or (body[0] >> 4) > 1:
                    raise ValueError("corrupt JPEG header: a bad DHT segment")
                code = 0
                for length in range(1, 17):
                    code += body[length]
                    if code > (1 << length):
                        raise ValueError("corrupt JPEG header: an over-subscribed Huffman table")
                    code <<= 1
                huff[body[0]] = body[1:17 + n_sym]
                body = body[17 + n_sym:]
        elif marker == 0xDD:
            if len(body) != 2:
                raise ValueError("corrupt JPEG header: a bad DRI segment")
            ri = int.from_bytes(body, "big")
        elif marker == 0xC0:
            if sof is not None:
                raise ValueError("corrupt JPEG header: two frame headers")
            sof = body
        elif marker in _SOF_NAMES:
            raise ValueError(f"unsupported JPEG: {_SOF_NAMES[marker]} (SOF{marker - 0xC0}); baseline sequential Huffman only")
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif marker == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif marker == 0xD9:
            raise ValueError("corrupt JPEG: EOI before any scan")
        elif marker == 0xDA:
            break
    if sof is None or len(sof) < 6 or len(sof) != 6 + 3 * sof[5]:
        raise ValueError("corrupt JPEG header: no SOF0 frame header before the scan")
    if sof[0] != 8:
        raise ValueError(f"unsupported JPEG: {sof[0]}-bit samples")
    h, w, nc = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if h == 0 or w == 0:
        raise ValueError("unsupported JPEG: a zero dimension (height given by a DNL marker)")
    if nc not in (1, 3):
        raise ValueError(f"unsupported JPEG: {nc} components" + (" (CMYK / YCCK)" if nc == 4 else ""))
    ids = [sof[6 + 3 * k] for k in range(nc)]
    samp = [(sof[7 + 3 * k] >> 4, sof[7 + 3 * k] & 15) for k in range(nc)]
    if nc == 3 and (adobe == 0 or (adobe is None and not jfif and ids == [82, 71, 66])):
        raise ValueError("unsupported JPEG: an RGB file (Adobe transform 0); YCbCr only")
    if nc == 3 and adobe not in (None, 1):
        raise ValueError(f"unsupported JPEG: Adobe colour transform {adobe}")
    if nc == 1:
        samp = [(1, 1)]  # a single component is not interleaved: its sampling factors mean nothing
    elif samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
        raise ValueError("unsupported JPEG: sampling factors " + ", ".join(f"{a}x{b}" for a, b in samp) + "; 4:4:4, 4:2:2 and 4:2:0 only")
    if len(body) < 1 or len(body) != 4 + 2 * body[0] or body[0] != nc:
        raise ValueError("unsupported JPEG: more than one scan (a scan that does not hold every component)")
    if (body[-3], body[-2], body[-1]) != (0, 63, 0):
        raise ValueError("unsupported JPEG: a scan of part of the spectrum (progressive parameters)")
    tables = np.zeros(M.JPEG_TABLE_BYTES, np.uint8)
    q16 = tables[:384].view(np.uint16).reshape(3, 64)
    for k in range(nc):
        if body[1 + 2 * k] != ids[k]:
            raise ValueError("unsupported JPEG: the scan's components are not in frame order")
        tq, td, ta = sof[8 + 3 * k], body[2 + 2 * k] >> 4, 0x10 | (body[2 + 2 * k] & 15)
        if tq not in qt or td not in huff or ta not in huff:
            raise ValueError("corrupt JPEG header: a table the scan needs is not defined")
        q16[k, _ZIGZAG] = qt[tq]
        for slot, t in ((k, huff[td]), (3 + k, huff[ta])):
            tables[384 + 272 * slot:384 + 272 * slot + len(t)] = np.frombuffer(t, np.uint8)
    return SimpleNamespace(height=h, width=w, components=nc, hs=samp[0][0], vs=samp[0][1], restart_interval=ri, scan_start=pos,
                           tables=tables)


def _jpeg_bytes(f):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    if isinstance(f, str) or hasattr(f, "__fspath__"):
        with open(f, "rb") as fh:
            return fh.read()
    raise TypeError(f"decode_jpeg: expected bytes or a path; got {type(f)}")


def decode_jpeg(files, mode="RGB", dtype=torch.uint8, device="cuda", sub_bytes=0):
    """Baseline JPEG files - `bytes`, a path, or a list of either - decoded on the device (hf_jpeg_decode_u8; DESIGN.md
    section 4.23) -> a device tensor (a list of them for a list): uint8 [H,W,3], the pixels of
    `PIL.Image.open(f).convert("RGB")` byte for byte ("unchanged": [H,W,1] for a grey file); with dtype=torch.float32
    [3,H,W] ([1,H,W]) = byte / 255 in the CPU's bits.  The host reads the header segments only; files of one geometry
    share one set of launches, all files one copy to the device and one synchronisation.  ValueError for a file the
    decoder does not take (`parse_jpeg_header`) or whose scan is corrupt; there is no fallback to PIL."""
    if mode not in JPEG_MODES:
        raise ValueError(f"mode must be one of {JPEG_MODES}; got {mode!r}")
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"dtype must be torch.uint8 or torch.float32; got {dtype}")
    single = not isinstance(files, (list, tuple))
    datas = [_jpeg_bytes(f) for f in ([files] if single else files)]
    if not datas:
        return []
    device = torch.device(device)
    if device.type != "cuda":
        require_gpu(torch.empty(0, device=device))
    heads = [parse_jpeg_header(d) for d in datas]
    groups = {}
    for k, hd in enumerate(heads):
        groups.setdefault((hd.height, hd.width, hd.components, hd.hs, hd.vs, hd.restart_interval), []).append(k)
    # one host buffer: per group the offsets and the tables, then every scan; one copy
    order = [k for ks in groups.values() for k in ks]
    head_bytes = sum(8 * (len(ks) + 1) + 8 + M.JPEG_TABLE_BYTES * len(ks) for ks in groups.values())
    head_bytes = (head_bytes + 15) // 16 * 16
    total = head_bytes + sum(len(datas[k]) - heads[k].scan_start for k in order)
    host = np.zeros(total + 16, np.uint8)
    pos, spos, layout = 0, head_bytes, []
    for key, ks in groups.items():
        off = host[pos:pos + 8 * (len(ks) + 1)].view(np.int64)
        tab_at = pos + 8 * (len(ks) + 1)
        start = spos
        for j, k in enumerate(ks):
            scan = memoryview(datas[k])[heads[k].scan_start:]
            off[j] = spos - start
            host[spos:spos + len(scan)] = np.frombuffer(scan, np.uint8)
            host[tab_at + j * M.JPEG_TABLE_BYTES:tab_at + (j + 1) * M.JPEG_TABLE_BYTES] = heads[k].tables
            spos += len(scan)
        off[len(ks)] = spos - start
        layout.append((key, ks, pos, tab_at, start, spos, max(len(datas[k]) - heads[k].scan_start for k in ks)))
        pos = tab_at + M.JPEG_TABLE_BYTES * len(ks)
        pos = (pos + 7) // 8 * 8
    blob = torch.from_numpy(host).to(device)
    L, st = lib(), stream()
    results, statuses = [None] * len(datas), []
    for (h, w, nc, hs, vs, ri), ks, off_at, tab_at, start, end, longest in layout:
        oc = 1 if (nc == 1 and mode == "unchanged") else 3
        u8, f32, status = M.jpeg_decode(L, st, blob[start:max(end, start + 1)], blob[off_at:off_at + 8 * (len(ks) + 1)].view(torch.int64), longest,
                                        blob[tab_at:tab_at + M.JPEG_TABLE_BYTES * len(ks)].view(len(ks), M.JPEG_TABLE_BYTES), h, w, nc, hs, vs, ri,
                                        oc, dtype is torch.uint8, dtype is torch.float32, sub_bytes)
        statuses.append(status[:, 0])
        for j, k in enumerate(ks):
            results[k] = u8[j] if dtype is torch.uint8 else f32[j]
    codes = torch.cat(statuses).cpu().tolist()  # the one synchronisation
    for k, code in zip(order, codes):
        if code:
            raise ValueError(f"corrupt JPEG scan (file {k}): {M.JPEG_DECODE_ERRORS.get(code, code)}")
    return results[0] if single else results


# ---------------------------------------------------------------------------------------------
# PNG files decoded on the device (csrc/png_decode.h)
# ---------------------------------------------------------------------------------------------
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_MODES = ("RGB", "unchanged")


def parse_png_header(data):
    """The chunks of a PNG file (pure Python, no GPU; no byte of the IDAT payloads is looked at) -> SimpleNamespace: height,
    width, color_type, channels (samples per pixel in the file), palette (uint8 [256,3], a short PLTE padded with zeros),
    idat (the (offset, length) pairs of the IDAT payloads in file order) and idat_bytes (their sum).  The CRC-32 of IHDR and
    PLTE is checked; tRNS, gAMA, iCCP and every other ancillary chunk are ignored.  ValueError("unsupported PNG: ...") for
    what the device decoder does not take: a bit depth other than 8, Adam7 interlace, an unknown colour type, compression
    or filter method, a zero dimension, no IHDR, no IDAT, colour type 3 without PLTE."""
    import zlib

    data = bytes(data) if not isinstance(data, bytes) else data
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("unsupported PNG: not a PNG file (no signature)")
    pos, ihdr, palette, idat = 8, None, None, []
    while pos + 8 <= len(data):
        n, ctype = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            if ctype == b"IDAT" or not idat:
                raise ValueError("unsupported PNG: a truncated chunk")
            break
        if ctype in (b"IHDR", b"PLTE") and zlib.crc32(data[pos + 4:pos + 8 + n]) != int.from_bytes(data[pos + 8 + n:pos + 12 + n], "big"):
            raise ValueError(f"unsupported PNG: the CRC of {ctype.decode()} does not match")
        if pos == 8 and (ctype != b"IHDR" or n != 13):
            raise ValueError("unsupported PNG: no IHDR chunk at the start")
        if ctype == b"IHDR":
            ihdr = data[pos + 8:pos + 21]
        elif ctype == b"PLTE":
            if n % 3 or n > 768:
                raise ValueError("unsupported PNG: a bad PLTE chunk")
            palette = np.zeros((256, 3), np.uint8)
            palette[:n // 3] = np.frombuffer(data[pos + 8:pos + 8 + n], np.uint8).reshape(-1, 3)
        elif ctype == b"IDAT":
            idat.append((pos + 8, n))
        elif ctype == b"IEND":
            break
        pos += 12 + n
    if ihdr is None:
        raise ValueError("unsupported PNG: no IHDR chunk at the start")
    w, h = int.from_bytes(ihdr[0:4], "big"), int.from_bytes(ihdr[4:8], "big")
    depth, color_type, compression, filter_method, interlace = ihdr[8:13]
    if w == 0 or h == 0:
        raise ValueError("unsupported PNG: a zero dimension")
    if color_type not in M.PNG_COLOR_CHANNELS:
        raise ValueError(f"unsupported PNG: colour type {color_type}")
    if depth != 8:
        raise ValueError(f"unsupported PNG: bit depth {depth}; 8 only")
    if compression != 0 or filter_method != 0:
        raise ValueError(f"unsupported PNG: compression method {compression}, filter method {filter_method}")
    if interlace != 0:
        raise ValueError("unsupported PNG: Adam7 interlace")
    if not idat:
        raise ValueError("unsupported PNG: no IDAT chunk")
    if color_type == 3 and palette is None:
        raise ValueError("unsupported PNG: colour type 3 without a PLTE chunk")
    if palette is None:
        palette = np.zeros((256, 3), np.uint8)
    return SimpleNamespace(height=h, width=w, color_type=color_type, channels=M.PNG_COLOR_CHANNELS[color_type], palette=palette,
                           idat=idat, idat_bytes=sum(n for _, n in idat))


def _file_bytes(f, what):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    if isinstance(f, str) or hasattr(f, "__fspath__"):
        with open(f, "rb") as fh:
            return fh.read()
    raise TypeError(f"{what}: expected bytes or a path; got {type(f)}")


def decode_png(files, mode="RGB", dtype=torch.uint8, device="cuda", token_cap=0):
    """PNG files - `bytes`, a path, or a list of either - decoded on the device (hf_png_decode_u8) ->
    a device tensor (a list of them for a list): uint8 [H,W,3], the pixels of `PIL.Image.open(f).convert("RGB")` byte for
    byte ("unchanged": the file's samples [H,W,1|2|3|4], a palette file expanded to 3); with dtype=torch.float32 [C,H,W] =
    byte / 255 in the CPU's bits.  Bit depth 8, no interlace, colour types 0, 2, 3, 4 and 6.  The host walks the chunks and
    concatenates the IDAT payloads; it inflates nothing.  Files of one geometry (height, width, colour type) share one set
    of launches, all files one copy to the device and one synchronisation.  ValueError for a file the decoder does not take
    (`parse_png_header`) or whose stream is corrupt; there is no fallback to PIL."""
    if mode not in PNG_MODES:
        raise ValueError(f"mode must be one of {PNG_MODES}; got {mode!r}")
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"dtype must be torch.uint8 or torch.float32; got {dtype}")
    single = not isinstance(files, (list, tuple))
    datas = [_file_bytes(f, "decode_png") for f in ([files] if single else files)]
    if not datas:
        return []
    device = torch.device(device)
    if device.type != "cuda":
        require_gpu(torch.empty(0, device=device))
    heads = [parse_png_header(d) for d in datas]
    groups = {}
    for k, hd in enumerate(heads):
        groups.setdefault((hd.height, hd.width, hd.color_type), []).append(k)
    # one host buffer: per group the offsets and (colour type 3) the palettes, then every stream; one copy
    order = [k for ks in groups.values() for k in ks]
    head_bytes = sum(8 * (len(ks) + 1) + 8 + (768 * len(ks) if key[2] == 3 else 0) for key, ks in groups.items())
    head_bytes = (head_bytes + 15) // 16 * 16
    host = np.zeros(head_bytes + sum(heads[k].idat_bytes for k in order) + 16, np.uint8)
    pos, spos, layout = 0, head_bytes, []
    for key, ks in groups.items():
        off = host[pos:pos + 8 * (len(ks) + 1)].view(np.int64)
        pal_at = pos + 8 * (len(ks) + 1)
        start = spos
        for j, k in enumerate(ks):
            off[j] = spos - start
            view = memoryview(datas[k])
            for at, n in heads[k].idat:
                host[spos:spos + n] = np.frombuffer(view[at:at + n], np.uint8)
                spos += n
            if key[2] == 3:
                host[pal_at + 768 * j:pal_at + 768 * (j + 1)] = heads[k].palette.reshape(-1)
        off[len(ks)] = spos - start
        layout.append((key, ks, pos, pal_at, start, spos, max(heads[k].idat_bytes for k in ks)))
        pos = pal_at + (768 * len(ks) if key[2] == 3 else 0)
        pos = (pos + 7) // 8 * 8
    blob = torch.from_numpy(host).to(device)
    L, st = lib(), stream()
    results, statuses = [None] * len(datas), []
    for (h, w, ct), ks, off_at, pal_at, start, end, longest in layout:
        oc = 3 if (mode == "RGB" or ct == 3) else M.PNG_COLOR_CHANNELS[ct]
        u8, f32, status = M.png_decode(L, st, blob[start:max(end, start + 1)], blob[off_at:off_at + 8 * (len(ks) + 1)].view(torch.int64), longest,
                                       blob[pal_at:pal_at + 768 * len(ks)].view(len(ks), 256, 3) if ct == 3 else None, h, w, ct, oc,
                                       dtype is torch.uint8, dtype is torch.float32, token_cap)
        statuses.append(status[:, 0])
        for j, k in enumerate(ks):
            results[k] = u8[j] if dtype is torch.uint8 else f32[j]
    codes = torch.cat(statuses).cpu().tolist()  # the one synchronisation
    for k, code in zip(order, codes):
        if code:
            raise ValueError(f"corrupt PNG (file {k}): {M.PNG_DECODE_ERRORS.get(code, code)}")
    return results[0] if single else results


def read_images(paths, decoder="pil"):
    """Image files -> list of uint8 [3,H,W] tensors, what `torchvision.io.read_image(path, mode=RGB)` gives: decoder="pil" on
    the host (CPU tensors); "device" - PNG files (by their signature) with `decode_png`, JPEG files (FF D8) with `decode_jpeg`,
    one call per kind, anything else a ValueError - device tensors, views of [H,W,3], in the order of `paths`."""
    if decoder not in DECODERS:
        raise ValueError(f"decoder must be one of {DECODERS}; got {decoder!r}")
    paths = list(paths)
    if decoder == "device":
        datas = [_file_bytes(p, "read_images") for p in paths]
        kinds = ["png" if d[:8] == PNG_SIGNATURE else "jpeg" if d[:2] == b"\xFF\xD8" else None for d in datas]
        if None in kinds:
            raise ValueError(f"read_images(decoder='device'): neither a PNG nor a JPEG file: {paths[kinds.index(None)]}")
        out = [None] * len(paths)
        for kind, decode in (("png", decode_png), ("jpeg", decode_jpeg)):
            ks = [k for k, x in enumerate(kinds) if x == kind]
            for k, t in zip(ks, decode([datas[k] for k in ks]) if ks else []):
                out[k] = t.permute(2, 0, 1)
        return out
    from .hair_swap import _read_image_rgb

    return [_read_image_rgb(p) for p in paths]
