"""TEST INFRASTRUCTURE - CPU restatement with PIL of `face_align.paste_back`: the aligned result of a swap put back into
the photograph it was cropped from.  The reference has no counterpart; this chain of Pillow operations IS the contract
(DESIGN.md section 4.19), and the device path (csrc/paste.h) is compared with it byte for byte.

    inverse map -> size -> mask plane -> ROI + quad -> Image.transform x 2 -> Image.composite

The geometry is written out coordinate by coordinate in Python floats (the product's `paste_plan` is the vector form of
the same IEEE operations in the same order).  Inputs come from tests/align_ref.py (`landmarks`, `image`, `plan`, `align`).
Pillow 12.2.0: ImageChops.multiply is floor(x y / 255), Image.composite is t = a m + b (255 - m) + 128, ((t >> 8) + t) >> 8
(both checked exhaustively in tests/test_paste_ref.py).
"""
import math

import numpy as np
import PIL.Image
import PIL.ImageChops

from tests import align_ref as R


def inverse(P):
    """The affine map crop -> photograph of the plan P (align_ref.plan), continuous coordinates, pixel i = [i, i + 1):
    p = A c + b for c in [0, S]^2 -> dict(A = ((a00, a01), (a10, a11)), b = (bx, by), det, n, roi, data)."""
    S = P["output_size"]
    Q = P["quad"]
    (nwx, nwy), (swx, swy), _, (nex, ney) = [(float(c[0]), float(c[1])) for c in Q]
    ox, oy = nwx + 0.5, nwy + 0.5                      # Image.transform was given quad + 0.5
    exx, exy = (nex - nwx) / S, (ney - nwy) / S        # one crop pixel to the right, in the transformed image
    eyx, eyy = (swx - nwx) / S, (swy - nwy) / S        # one crop pixel down
    offx = offy = 0.0
    if P["pad"] is not None:
        offx, offy = offx - P["pad"][0], offy - P["pad"][1]
    if P["crop"] is not None:
        offx, offy = offx + P["crop"][0], offy + P["crop"][1]
    scx = scy = 1.0
    if P["rsize"] is not None:
        scx, scy = P["size_input"][0] / P["rsize"][0], P["size_input"][1] / P["rsize"][1]
    a00, a01, a10, a11 = exx * scx, eyx * scx, exy * scy, eyy * scy
    bx, by = (ox + offx) * scx, (oy + offy) * scy
    det = a00 * a11 - a01 * a10
    side = math.sqrt(abs(det)) * S
    n = int(min(max(np.rint(side), 1), S))

    def to_photo(cx, cy):
        return a00 * cx + a01 * cy + bx, a10 * cx + a11 * cy + by

    pts = [to_photo(0.0, 0.0), to_photo(0.0, float(S)), to_photo(float(S), float(S)), to_photo(float(S), 0.0)]
    w, h = P["size_input"]
    x0, y0 = max(math.floor(min(p[0] for p in pts)), 0), max(math.floor(min(p[1] for p in pts)), 0)
    x1, y1 = min(math.ceil(max(p[0] for p in pts)), w), min(math.ceil(max(p[1] for p in pts)), h)
    out = {"A": ((a00, a01), (a10, a11)), "b": (bx, by), "det": det, "n": n, "roi": None, "data": None}
    if x1 > x0 and y1 > y0:
        k = n / S

        def to_result(X, Y):
            dx, dy = X - bx, Y - by
            return (a11 * dx - a01 * dy) / det * k, (a00 * dy - a10 * dx) / det * k

        out["roi"] = (x0, y0, x1, y1)
        out["data"] = [v for X, Y in ((x0, y0), (x0, y1), (x1, y1), (x1, y0)) for v in to_result(float(X), float(Y))]  # NW, SW, SE, NE
    return out


def feather_plane(n, feather):
    """uint8 [n,n]: a smoothstep from 0 at the square's edge to 255 at `feather` of the side inwards, per axis, multiplied."""
    r = []
    for i in range(n):
        x = i + 0.5
        d = min(x, n - x) / n
        t = min(max(d / feather, 0.0), 1.0) if feather > 0 else 1.0
        r.append(t * t * (3.0 - 2.0 * t))
    r = np.array(r, np.float64)
    return np.floor(255.0 * (r[:, None] * r[None, :]) + 0.5).astype(np.uint8)


def quantise_mask(mask):
    mask = np.asarray(mask)
    if mask.dtype == np.uint8:
        return mask
    return np.clip(np.floor(mask.astype(np.float64) * 255 + 0.5), 0, 255).astype(np.uint8)


def paste(photo, result, lm, feather=0.1, mask=None):
    """photo: PIL RGB; result: PIL RGB S x S, the aligned image of `photo` from landmarks lm after whatever was done to it;
    mask: crop-space [S,S] array (uint8 or float in [0,1]) or None -> dict(plan, inverse, result (resized), mask (the plane),
    warped, warped_mask, out (PIL RGB, the photograph's size))."""
    S = result.size[0]
    P = R.plan(lm, photo.size[0], photo.size[1], S)
    inv = inverse(P)
    n = inv["n"]
    small = result.resize((n, n), PIL.Image.LANCZOS) if n < S else result
    plane = PIL.Image.fromarray(feather_plane(n, feather), "L")
    if mask is not None:
        user = PIL.Image.fromarray(quantise_mask(mask), "L")
        if n < S:
            user = user.resize((n, n), PIL.Image.LANCZOS)
        plane = PIL.ImageChops.multiply(user, plane)
    out = photo.copy()
    stages = {"plan": P, "inverse": inv, "result": small, "mask": plane, "warped": None, "warped_mask": None}
    if inv["roi"] is not None:
        x0, y0, x1, y1 = inv["roi"]
        size = (x1 - x0, y1 - y0)
        warped = small.transform(size, PIL.Image.QUAD, inv["data"], PIL.Image.BILINEAR)
        warped_mask = plane.transform(size, PIL.Image.QUAD, inv["data"], PIL.Image.BILINEAR)
        out.paste(PIL.Image.composite(warped, photo.crop(inv["roi"]), warped_mask), (x0, y0))
        stages.update(warped=warped, warped_mask=warped_mask)
    stages["out"] = out
    return stages


def blob_image(width, height, centres, sigma):
    """uint8 HWC image: black with a white Gaussian blob (peak 255, the same in every channel) at each centre (continuous
    coordinates)."""
    ys, xs = np.arange(height)[:, None] + 0.5, np.arange(width)[None, :] + 0.5
    img = np.zeros((height, width))
    for cx, cy in centres:
        img += 255.0 * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2.0 * sigma * sigma))
    return np.repeat(np.clip(np.rint(img), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def centroid(plane, cx, cy, radius):
    """Intensity centroid (continuous coordinates) of a 2-D array inside the box of half-width `radius` around (cx, cy)."""
    h, w = plane.shape
    x0, x1 = max(int(math.floor(cx - radius)), 0), min(int(math.ceil(cx + radius)), w)
    y0, y1 = max(int(math.floor(cy - radius)), 0), min(int(math.ceil(cy + radius)), h)
    win = plane[y0:y1, x0:x1].astype(np.float64)
    ys, xs = np.arange(y0, y1)[:, None] + 0.5, np.arange(x0, x1)[None, :] + 0.5
    total = win.sum()
    return float((win * xs).sum() / total), float((win * ys).sum() / total)
