"""FFHQ face alignment from 68 landmarks: the image half of the reference's utils/shape_predictor.py:104-185 on the
MI355X kernels of csrc/align.h (the reference runs it with PIL and scipy on the CPU, 0.3-0.5 s per image).

The other half - dlib's face detector and 68-point predictor (shape_predictor.py:32-77) - is a third-party model and
stays an injection point: `align_face` takes the landmarks, `HairFast(..., landmark_detector=...)` a callable.

Per image:

1. `alignment_plan`: the oriented crop quad from the eye and mouth landmarks, the shrink factor, crop box and pad
   widths - host float64 numpy, expression for expression as in the reference;
2. shrink (qsize >= 2 * output_size): PIL's 8-bit Lanczos resize (hf_resize_lanczos_u8);
3. crop: a slice;
4. pad (the quad leaves the image): reflect pad, Gaussian-blurred and median-faded border (hf_align_pad_blur_f32, a sort
   for the per-channel median, hf_align_pad_finish_u8);
5. `Image.transform(transform_size^2, QUAD, BILINEAR)` + `resize(output_size^2, LANCZOS)`: ONE launch with the
   intermediate in LDS when transform_size = 4 * output_size (hf_quad_lanczos4_u8; the reference's 4096 -> 1024), else
   hf_quad_bilinear_u8 + hf_resize_lanczos_u8;
6. ToTensor: byte / 255 (hf_u8_to_unit_f32).

Images are planar uint8 [3,H,W] on the device throughout.  Steps 2, 5 and 6 reproduce Pillow's bytes exactly (integer
arithmetic; double with one truncation); step 4 is float32 with double accumulation like numpy 1.x + scipy and can differ
from them by one level only where the value before `rint` sits on a rounding tie.

The way back - `paste_back`: the result computed from an aligned crop put into the photograph where the crop came from
(no counterpart in the reference).  `paste_plan` inverts the plan to an affine map crop ->
photograph; the result is reduced to the face's size in the photograph (hf_resize_lanczos_u8) and ONE launch warps it and
its feather mask onto the region of interest and composites them (hf_paste_quad_u8; csrc/paste.h) - Pillow's bytes again.
"""
import functools

import numpy as np
import torch

from . import _marshal as M
from ._runtime import lib, stream

PRECISION_BITS = 32 - 8 - 2  # Pillow's Resample.c: 8-bit pixels, 22-bit fixed-point weights in an int32 accumulator
LANCZOS_SUPPORT = 3.0
# transform + resize as one launch where the library has the ratio (None: yes; False: always the chained pair).
# Measured: profiles/align_bench.json, DESIGN.md section 4.16.
USE_FUSED = None


# ---------------------------------------------------------------------------------------------
# host tables (double; Pillow's precompute_coeffs / normalize_coeffs_8bpc, Image.__transformer, scipy's _gaussian_kernel1d)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def lanczos_coeffs(in_size, out_size):
    """Tables of one Lanczos pass in_size -> out_size: (bounds int32 [out,2] = (first tap, tap count), kk int32
    [out,ksize] fixed-point weights).  All rows at once; a row's weights are summed in tap order (cumsum), as Pillow does."""
    return _filter_coeffs(in_size, out_size, LANCZOS_SUPPORT,
                          lambda t: np.where((t >= -3.0) & (t < 3.0), _sinc(t) * _sinc(t / 3.0), 0.0))


@functools.lru_cache(maxsize=32)
def bilinear_coeffs(in_size, out_size):
    """The same tables for Pillow's BILINEAR (triangle) filter, support 1: hf_resize_lanczos_u8 takes host tables and does
    not know its filter, so `Image.resize(size, BILINEAR)` is the same kernel with these."""
    return _filter_coeffs(in_size, out_size, 1.0, lambda t: np.where(np.abs(t) < 1.0, 1.0 - np.abs(t), 0.0))


def _filter_coeffs(in_size, out_size, filter_support, weight):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for a filter of the given support; weight(t) -> filter values."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = filter_support * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size) + 0.5) * scale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)              # C's (int): truncation
    count = np.minimum((center + support + 0.5).astype(np.int64), in_size) - first
    tap = np.arange(ksize)[None, :]
    t = ((tap + first[:, None]) - center[:, None] + 0.5) * (1.0 / fs)
    w = np.where(tap < count[:, None], weight(t), 0.0)
    total = np.cumsum(w, axis=1)[:, -1:]                                          # + 0.0 for the dead taps changes nothing
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    q = np.where(w < 0, w * (1 << PRECISION_BITS) - 0.5, w * (1 << PRECISION_BITS) + 0.5).astype(np.int64)
    return np.stack([first, count], 1).astype(np.int32), q.astype(np.int32)


def _sinc(x):
    x = np.asarray(x, np.float64) * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def quad_coefficients(quad, out_w, out_h):
    """Pillow's Image.__transformer for QUAD: quad [4,2] (NW, SW, SE, NE, already + 0.5) -> a0..a7."""
    (x0, y0), sw, se, ne = [(float(p[0]), float(p[1])) for p in np.asarray(quad, np.float64).reshape(4, 2)]
    As = 1.0 / out_w
    At = 1.0 / out_h
    return (x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
            y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At)


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage._gaussian_kernel1d(sigma, 0, radius) with radius = int(truncate * sigma + 0.5) -> (weights, radius)."""
    radius = int(truncate * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum(), radius


def fade_ramps(width, height, pad):
    """The two float32 ramps of the fade mask (shape_predictor.py:173, numpy 1.x's float32 form):
    mask[y, x] = max(mask_x[x], mask_y[y])."""
    pad = [int(v) for v in pad]
    x = np.arange(width)
    y = np.arange(height)
    mask_x = 1.0 - np.minimum(np.float32(x) / np.float32(pad[0]), np.float32(width - 1 - x) / np.float32(pad[2]))
    mask_y = 1.0 - np.minimum(np.float32(y) / np.float32(pad[1]), np.float32(height - 1 - y) / np.float32(pad[3]))
    return mask_x.astype(np.float32), mask_y.astype(np.float32)


# ---------------------------------------------------------------------------------------------
# the plan (shape_predictor.py:105-179)
# ---------------------------------------------------------------------------------------------
def check_landmarks(lm):
    lm = np.asarray(lm)
    if lm.shape != (68, 2) or lm.dtype.kind not in "iuf":
        raise ValueError(f"landmarks must be a numeric [68, 2] array (dlib's 68-point model); got shape {lm.shape}, dtype {lm.dtype}")
    return lm


def _bounding_box(quad):
    """Integer box (x0, y0, x1, y1) around the quad's corners: floor of the minima, ceil of the maxima."""
    xs, ys = quad[:, 0], quad[:, 1]
    return int(np.floor(min(xs))), int(np.floor(min(ys))), int(np.ceil(max(xs))), int(np.ceil(max(ys)))


def face_quad(lm):
    """The oriented square around a face (FFHQ's rule, shape_predictor.py:116-132): its horizontal half-axis `u` is the
    eye-to-eye vector combined with the eye-to-mouth vector turned by a quarter turn, scaled to the larger of 2 x the eye
    distance and 1.8 x the eye-mouth distance; its centre sits a tenth of the way from the eyes to the mouth.
    -> (float64 [4,2] corners NW, SW, SE, NE; side length)."""
    lm = check_landmarks(lm)
    left_eye = np.mean(lm[36:42], axis=0)
    right_eye = np.mean(lm[42:48], axis=0)
    eyes = (left_eye + right_eye) * 0.5
    across = right_eye - left_eye
    mouth = (lm[48] + lm[54]) * 0.5                  # the outer mouth corners
    down = mouth - eyes
    u = across - np.flipud(down) * [-1, 1]
    u /= np.hypot(*u)
    u *= max(np.hypot(*across) * 2.0, np.hypot(*down) * 1.8)
    v = np.flipud(u) * [-1, 1]
    centre = eyes + down * 0.1
    quad = np.stack([centre - u - v, centre - u + v, centre + u + v, centre + u - v])
    side = np.hypot(*u) * 2
    if not np.isfinite(quad).all() or not side > 0:
        raise ValueError("degenerate landmarks: the eyes and the mouth coincide")
    return quad, side


def alignment_plan(lm, width, height, output_size=1024, transform_size=4096, enable_padding=True):
    """The geometry of one alignment for a width x height image (shape_predictor.py:105-179, the same float64 operations
    in the same order): dict with
      shrink, rsize (None: no shrink)   the integer factor and the (w, h) after PIL's Lanczos shrink
      border, crop (None: no crop)      the crop box (x0, y0, x1, y1) in the shrunk image
      pad (None: no padding), blur      the pad widths (left, top, right, bottom) and the Gaussian sigma
      qsize                             the quad's side after the shrink
      quad_input / quad_shrunk / quad_cropped / quad   float64 [4,2] (NW, SW, SE, NE) after each step
      size_cropped / size               (w, h) of the image after the crop / entering the transform."""
    quad, side = face_quad(lm)
    w, h = int(width), int(height)
    plan = {"quad_input": quad.copy(), "qsize_input": float(side), "size_input": (w, h),
            "output_size": int(output_size), "transform_size": int(transform_size)}

    # a face several times larger than the output is first reduced by an integer factor
    factor = int(np.floor(side / output_size * 0.5))
    plan["shrink"], plan["rsize"] = factor, None
    if factor > 1:
        w, h = int(np.rint(float(w) / factor)), int(np.rint(float(h) / factor))
        plan["rsize"] = (w, h)
        quad /= factor
        side /= factor
    plan["quad_shrunk"], plan["qsize"] = quad.copy(), float(side)

    # keep the quad's box plus a margin of a tenth of its side, cut at the image
    margin = max(int(np.rint(side * 0.1)), 3)
    bx0, by0, bx1, by1 = _bounding_box(quad)
    box = (max(bx0 - margin, 0), max(by0 - margin, 0), min(bx1 + margin, w), min(by1 + margin, h))
    plan["border"], plan["crop"] = margin, None
    if box[2] - box[0] < w or box[3] - box[1] < h:
        if box[2] <= box[0] or box[3] <= box[1]:
            raise ValueError(f"the face quad lies outside the {w} x {h} image (crop box {box})")
        plan["crop"] = box
        w, h = box[2] - box[0], box[3] - box[1]
        quad -= box[0:2]
    plan["quad_cropped"], plan["size_cropped"] = quad.copy(), (w, h)

    # where quad + margin still leaves the image, every side is extended by at least 0.3 of the quad's side
    bx0, by0, bx1, by1 = _bounding_box(quad)
    short = (max(-bx0 + margin, 0), max(-by0 + margin, 0), max(bx1 - w + margin, 0), max(by1 - h + margin, 0))
    plan["pad"], plan["blur"] = None, float(side * 0.02)
    if enable_padding and max(short) > margin - 4:
        least = int(np.rint(side * 0.3))
        widths = tuple(max(int(s_), least) for s_ in short)
        plan["pad"] = widths
        w, h = w + widths[0] + widths[2], h + widths[1] + widths[3]
        quad += widths[:2]
    plan["quad"], plan["size"] = quad.copy(), (w, h)
    return plan


# ---------------------------------------------------------------------------------------------
# device stages
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def _device_coeffs(in_size, out_size, device, coeffs=lanczos_coeffs):
    bounds, kk = coeffs(in_size, out_size)
    return torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device)


def resize_lanczos(L, st, img, out_w, out_h, coeffs=lanczos_coeffs):
    """PIL Image.resize((out_w, out_h), LANCZOS) of planar uint8 [C,H,W]."""
    h, w = img.shape[-2:]
    if (out_h, out_w) == (h, w):
        return img.clone()
    tx = _device_coeffs(w, out_w, img.device, coeffs) if out_w != w else None
    ty = _device_coeffs(h, out_h, img.device, coeffs) if out_h != h else None
    return M.resize_lanczos_u8(L, st, img, out_h, out_w, tx, ty)


def resize_bilinear(L, st, img, out_w, out_h):
    """PIL Image.resize((out_w, out_h), BILINEAR) of planar uint8 [C,H,W]."""
    return resize_lanczos(L, st, img, out_w, out_h, bilinear_coeffs)


def quad_transform(L, st, img, quad, size):
    """PIL Image.transform((size, size), QUAD, quad + 0.5, BILINEAR) of planar uint8 [C,H,W]; quad as in the plan."""
    return M.quad_bilinear_u8(L, st, img, quad_coefficients(np.asarray(quad, np.float64) + 0.5, size, size), size, size)


def fused_available(L, transform_size, output_size):
    return transform_size == L.hf_quad_lanczos4_ratio() * output_size


def transform_resize(L, st, img, quad, transform_size, output_size, fused=None):
    """Steps 5: -> uint8 [C, output_size, output_size] (output_size >= transform_size: the transform alone, as the
    reference).  fused: None = the one-launch form where the library has the ratio; False = the chained pair; True = the
    one-launch form or ValueError."""
    fused = USE_FUSED if fused is None else fused
    can = output_size < transform_size and fused_available(L, transform_size, output_size)
    if fused and not can:
        raise ValueError(f"the fused transform is instantiated for transform_size = {L.hf_quad_lanczos4_ratio()} * output_size; "
                         f"got {transform_size} / {output_size}")
    if can and fused is not False:
        coef = quad_coefficients(np.asarray(quad, np.float64) + 0.5, transform_size, transform_size)
        return M.quad_lanczos4_u8(L, st, img, coef, output_size, _device_coeffs(transform_size, output_size, img.device))
    big = quad_transform(L, st, img, quad, transform_size)
    return resize_lanczos(L, st, big, output_size, output_size) if output_size < transform_size else big


def pad_blur_fade(L, st, img, pad, blur, return_float=False):
    """shape_predictor.py:168-178 on planar uint8 [C,h,w]: -> uint8 [C,H,W] (and the float32 image before rint)."""
    pad = tuple(int(v) for v in pad)
    h, w = img.shape[-2:]
    H, W = h + pad[1] + pad[3], w + pad[0] + pad[2]
    weights, radius = gaussian_weights(blur)
    mask_x, mask_y = fade_ramps(W, H, pad)
    dev = img.device
    mask_x, mask_y = torch.from_numpy(mask_x).to(dev), torch.from_numpy(mask_y).to(dev)
    blurred = M.align_pad_blur(L, st, img, torch.from_numpy(weights).to(dev), radius, mask_x, mask_y, pad)
    # np.median over a plane: the middle value, or the float32 mean of the two middle values
    flat = blurred.flatten(1).sort(dim=1).values
    n = flat.shape[1]
    median = flat[:, n // 2] if n % 2 else (flat[:, n // 2 - 1] + flat[:, n // 2]) / 2
    return M.align_pad_finish(L, st, blurred, median.contiguous(), mask_x, mask_y, return_float)


def to_bytes(img, device=None):
    """One image in the forms `swap` takes (after HairFast._as_tensor) -> planar uint8 [3,H,W] on the device, as the
    reference's ToPILImage: a float tensor is mul(255) and truncated, a uint8 tensor is taken as is."""
    if not isinstance(img, torch.Tensor):
        from .hair_swap import HairFast

        img = HairFast._as_tensor(img)
    if img.ndim != 3 or img.shape[0] != 3:
        raise ValueError(f"face alignment takes 3-channel images [3,H,W]; got {tuple(img.shape)}")
    if device is not None:
        img = img.to(device)
    if img.dtype is not torch.uint8:
        if not img.is_floating_point():
            raise ValueError(f"image tensors are uint8 or float in [0,1]; got {img.dtype}")
        img = img.mul(255).to(torch.uint8)
    return img.contiguous()


def align_bytes(L, st, img, lm, output_size=1024, transform_size=4096, enable_padding=True, fused=None, stages=None):
    """One planar uint8 [3,H,W] image -> uint8 [3, output_size, output_size] on library L and stream st.  stages: a dict
    that receives the plan and the image after each step (tests)."""
    plan = alignment_plan(lm, img.shape[2], img.shape[1], output_size, transform_size, enable_padding)
    if plan["rsize"] is not None:
        img = resize_lanczos(L, st, img, *plan["rsize"])
    shrunk = img
    if plan["crop"] is not None:
        x0, y0, x1, y1 = plan["crop"]
        img = img[:, y0:y1, x0:x1].contiguous()
    cropped = img
    pre = None
    if plan["pad"] is not None:
        img, pre = pad_blur_fade(L, st, img, plan["pad"], plan["blur"], return_float=stages is not None)
    out = transform_resize(L, st, img, plan["quad"], transform_size, output_size, fused)
    if stages is not None:
        stages.update(plan=plan, shrunk=shrunk, cropped=cropped, padded=img, pre=pre, out=out)
    return out


def unit_float(img_u8):
    """ToTensor: uint8 -> float32 byte / 255 with the bits of the CPU's division."""
    return M.u8_to_unit(lib(), stream(), img_u8)


@torch.inference_mode()
def align_face(images, landmarks, output_size=1024, transform_size=4096, enable_padding=True, return_tensors=True, *,
               fused=None, device="cuda"):
    """The reference's `align_face(images)` (shape_predictor.py:80-194) with the landmarks supplied: images - one or a
    list of the forms `swap` takes; landmarks - one [68,2] array per image -> list of [3, output_size, output_size]
    float tensors in [0,1] on the device (uint8 with return_tensors=False, the reference's PIL images).  The defaults are
    the reference's constants."""
    if not isinstance(images, (list, tuple)):
        images = [images]
    landmarks = list(landmarks) if not (isinstance(landmarks, np.ndarray) and landmarks.ndim == 2) else [landmarks]
    if len(landmarks) != len(images):
        raise ValueError(f"one [68,2] landmark array per image: {len(images)} images, {len(landmarks)} landmark arrays")
    landmarks = [check_landmarks(lm) for lm in landmarks]
    out = []
    for img, lm in zip(images, landmarks):
        dev = img.device if isinstance(img, torch.Tensor) and img.is_cuda else torch.device(device)
        img = to_bytes(img, dev)
        aligned = align_bytes(lib(), stream(), img, lm, output_size, transform_size, enable_padding, fused)
        out.append(unit_float(aligned) if return_tensors else aligned)
    return out


# ---------------------------------------------------------------------------------------------
# paste back: the aligned result onto the photograph it was cropped from (csrc/paste.h)
# ---------------------------------------------------------------------------------------------
def paste_plan(plan):
    """The inverse geometry of an `alignment_plan`: the affine map p = A c + b from crop coordinates c in [0, S]^2
    (S = output_size) to photograph coordinates, both continuous (pixel i covers [i, i + 1)), in float64: dict with
      A [2,2], b [2], det      the map (columns of A: the crop's x and y axes in the photograph) and det A
      n                        the side of the result before the warp: the crop's side in photograph pixels, rounded, at most S
      roi                      (x0, y0, x1, y1): the box of the mapped crop cut at the photograph, or None if they do not meet
      quad [4,2]               the ROI's corners (NW, SW, SE, NE) in the n x n result: the `data` of Image.transform(QUAD)."""
    S = plan["output_size"]
    Q = plan["quad"]
    o = Q[0] + 0.5                                     # the transform samples at quad + 0.5 (quad_transform)
    ex = (Q[3] - Q[0]) / S
    ey = (Q[1] - Q[0]) / S
    off = np.zeros(2)
    if plan["pad"] is not None:
        off = off - np.asarray(plan["pad"][:2], np.float64)
    if plan["crop"] is not None:
        off = off + np.asarray(plan["crop"][:2], np.float64)
    sc = np.ones(2)
    if plan["rsize"] is not None:                      # the Lanczos shrink scales each axis by its own ratio
        sc = np.asarray(plan["size_input"], np.float64) / np.asarray(plan["rsize"], np.float64)
    A = np.stack([ex * sc, ey * sc], axis=1)
    b = (o + off) * sc
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    if not np.isfinite(det) or det == 0.0:
        raise ValueError("degenerate alignment plan: the crop has no area in the photograph")
    side = np.sqrt(abs(det)) * S
    n = int(min(max(np.rint(side), 1), S))
    corners = np.array([[0.0, 0.0], [0.0, S], [S, S], [S, 0.0]])
    px = A[0, 0] * corners[:, 0] + A[0, 1] * corners[:, 1] + b[0]
    py = A[1, 0] * corners[:, 0] + A[1, 1] * corners[:, 1] + b[1]
    w, h = plan["size_input"]
    x0, y0 = max(int(np.floor(px.min())), 0), max(int(np.floor(py.min())), 0)
    x1, y1 = min(int(np.ceil(px.max())), w), min(int(np.ceil(py.max())), h)
    out = {"A": A, "b": b, "det": float(det), "side": float(side), "n": n, "roi": None, "quad": None}
    if x1 > x0 and y1 > y0:
        out["roi"] = (x0, y0, x1, y1)
        box = np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], np.float64)
        dx, dy = box[:, 0] - b[0], box[:, 1] - b[1]
        k = n / S
        out["quad"] = np.stack([(A[1, 1] * dx - A[0, 1] * dy) / det * k, (A[0, 0] * dy - A[1, 0] * dx) / det * k], axis=1)
    return out


def feather_mask(n, feather):
    """The n x n byte mask that fades the pasted square out towards its edges: a smoothstep over the outer `feather` of the
    side on each axis (0 at the edge, 255 from `feather` inwards), the two axes multiplied; feather = 0: all 255."""
    n, feather = int(n), float(feather)
    if n < 1 or not 0.0 <= feather < np.inf:
        raise ValueError(f"feather_mask: n >= 1 and a finite feather >= 0; got n = {n}, feather = {feather}")
    x = np.arange(n) + 0.5
    d = np.minimum(x, n - x) / n
    r = np.clip(d / feather, 0.0, 1.0) if feather > 0 else np.ones(n)
    r = r * r * (3.0 - 2.0 * r)
    return np.floor(255.0 * np.outer(r, r) + 0.5).astype(np.uint8)


@functools.lru_cache(maxsize=4)
def _device_feather(n, feather, device):
    return torch.from_numpy(feather_mask(n, feather)).to(device)


def mask_bytes(mask, size, device):
    """A crop-space mask [size, size] (tensor or array; uint8, or float in [0,1]: floor(v * 255 + 0.5), clipped) -> uint8
    on the device."""
    mask = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
    if tuple(mask.shape) != (size, size):
        raise ValueError(f"the paste mask is given in crop space, [{size}, {size}]; got {tuple(mask.shape)}")
    mask = mask.to(device)
    if mask.dtype is not torch.uint8:
        if not mask.is_floating_point():
            raise ValueError(f"the paste mask is uint8 or float in [0,1]; got {mask.dtype}")
        mask = mask.double().mul(255).add(0.5).floor().clamp(0, 255).to(torch.uint8)
    return mask.contiguous()


def paste_bytes(L, st, photo, result, lm, mask=None, feather=0.1, output_size=1024, stages=None):
    """One planar uint8 photograph [3,H,W] and the aligned uint8 result [3,S,S] (S = output_size) of the alignment of that
    photograph from landmarks lm -> a new uint8 [3,H,W]: the photograph with the result warped back to where the crop came
    from, through the feather mask times `mask` (uint8 [S,S] or None).  stages: a dict that receives the plan, the inverse
    plan, the resized result and the mask plane (tests)."""
    S = int(output_size)
    if photo.ndim != 3 or tuple(result.shape) != (photo.shape[0], S, S):
        raise ValueError(f"paste: a photograph [3,H,W] and its aligned result [3,{S},{S}]; got {tuple(photo.shape)}, {tuple(result.shape)}")
    plan = alignment_plan(lm, photo.shape[2], photo.shape[1], S)
    inv = paste_plan(plan)
    n = inv["n"]
    out = photo.clone()
    small = resize_lanczos(L, st, result, n, n) if n < S else result
    plane = _device_feather(n, float(feather), photo.device)
    if mask is not None:
        if mask.dtype is not torch.uint8 or tuple(mask.shape) != (S, S):
            raise ValueError(f"paste: the mask is uint8 [{S}, {S}] here (mask_bytes); got {mask.dtype} {tuple(mask.shape)}")
        user = resize_lanczos(L, st, mask[None], n, n)[0] if n < S else mask
        plane = M.multiply_u8(L, st, user, plane)
    if inv["roi"] is not None:
        x0, y0, x1, y1 = inv["roi"]
        M.paste_quad_u8(L, st, out, small, plane, quad_coefficients(inv["quad"], x1 - x0, y1 - y0), inv["roi"])
    if stages is not None:
        stages.update(plan=plan, inverse=inv, result=small, mask=plane, out=out)
    return out


def result_bytes(result, device):
    """The result of a swap in the forms `paste_back` takes -> planar uint8 [3,S,S] on the device: a float tensor [3,S,S] in
    [0,1] with the bytes image_utils.save_image writes (x * 255 + 0.5, clamped, truncated); a uint8 tensor [3,S,S], HWC
    array or PIL image (what poisson_image_blending returns) as is."""
    if isinstance(result, torch.Tensor) and result.is_floating_point():
        from .image_utils import to_bytes as quantise

        if result.ndim != 3:
            raise ValueError(f"paste: one result [3,S,S] per photograph; got {tuple(result.shape)}")
        return quantise(result.to(device).float().contiguous(), (0, 1), "nearest", "chw")
    if not isinstance(result, torch.Tensor):
        arr = np.asarray(result)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f"paste: an image that is not a tensor is uint8 [S,S,3]; got {arr.dtype} {arr.shape}")
        result = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
    if result.dtype is not torch.uint8 or result.ndim != 3 or result.shape[0] != 3:
        raise ValueError(f"paste: a result tensor is float in [0,1] or uint8, [3,S,S]; got {result.dtype} {tuple(result.shape)}")
    return result.to(device).contiguous()


@torch.inference_mode()
def paste_back(photo, result, landmarks, *, mask=None, feather=0.1, output_size=1024, return_tensors=True, device="cuda"):
    """The inverse of `align_face` for the result of a swap: `photo` (the image forms `swap` takes) with `result` - the
    [3, output_size, output_size] image computed from its aligned crop: what `swap` or `poisson_image_blending` returns -
    put back where the crop was taken, from the same [68,2] `landmarks`.  The photograph is not modified.

    mask: optional crop-space [output_size, output_size] weights (uint8, or float in [0,1]) that multiply the feather -
    e.g. a hair mask; feather: the share of the crop's side over which the square fades out at its edges.
    photo / result / landmarks (and mask) may be lists of equal length: one launch per photograph, a list is returned.
    -> float [3,H,W] in [0,1] on the device (uint8 with return_tensors=False).  To write it as a JPEG without the pixels
    crossing to the host: `image_utils.encode_jpeg(pasted_u8.permute(1, 2, 0))` for the uint8 form, or
    `image_utils.save_image(pasted, path, encoder="device", format="jpeg")` for the float one."""
    many = isinstance(photo, (list, tuple))
    photos = list(photo) if many else [photo]
    results = list(result) if many else [result]
    landmarks = list(landmarks) if many else [landmarks]
    masks = (list(mask) if many else [mask]) if mask is not None else [None] * len(photos)
    if not len(photos) == len(results) == len(landmarks) == len(masks):
        raise ValueError(f"paste_back: one result, one [68,2] landmark array (and one mask) per photograph; got {len(photos)} "
                         f"photographs, {len(results)} results, {len(landmarks)} landmark arrays, {len(masks)} masks")
    S = int(output_size)
    out = []
    for img, res, lm, mk in zip(photos, results, landmarks, masks):
        dev = img.device if isinstance(img, torch.Tensor) and img.is_cuda else torch.device(device)
        img = to_bytes(img, dev)
        res = result_bytes(res, dev)
        mk = mask_bytes(mk, S, dev) if mk is not None else None
        pasted = paste_bytes(lib(), stream(), img, res, check_landmarks(lm), mk, feather, S)
        out.append(unit_float(pasted) if return_tensors else pasted)
    return out if many else out[0]


def landmarks_for(images_u8, source):
    """`source`: a sequence of [68,2] arrays, or a callable image (uint8 HWC numpy array) -> [68,2]."""
    if callable(source):
        return [check_landmarks(source(np.ascontiguousarray(im.permute(1, 2, 0).cpu().numpy()))) for im in images_u8]
    source = list(source)
    if len(source) != len(images_u8):
        raise ValueError(f"landmarks: one [68,2] array per image ({len(images_u8)}); got {len(source)}")
    return [check_landmarks(lm) for lm in source]
