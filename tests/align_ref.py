"""TEST INFRASTRUCTURE - CPU restatement of the reference's FFHQ face alignment from landmarks
(utils/shape_predictor.py:104-185) with PIL and scipy, split into stages so that a mismatch can be located:

    plan -> shrink -> crop -> pad -> transform -> resize

`output_size` / `transform_size` are parameters (the reference hard-codes 1024 / 4096) so that tests can run small.  The
pad stage is the float32 form of the reference's pinned numpy 1.x environment: the pad widths are Python ints here, so
the fade mask and both products are float32 under numpy 1.x and numpy 2 alike (with the reference's `np.maximum(pad,
...)` the widths are np.int64 scalars, which numpy 2 promotes to float64).  It also returns the float32 image before
`rint`: the tie rule of the tests (a byte may differ by one level only where that value lies within 1e-3 of a
half-integer) is evaluated on it.  tests/test_align_ref.py pins this file to the reference through tests/golden/align.npz.
"""
import math

import numpy as np
import PIL.Image
import scipy.ndimage

TIE_EPS = 1e-3


def _hyp(a, b):
    return float(np.hypot(a, b))  # (math.hypot rounds differently from the C library's hypot that numpy calls)


def plan(lm, width, height, output_size=1024, transform_size=4096, enable_padding=True):
    """The geometry of :105-179 for an image of width x height, written out coordinate by coordinate in Python floats
    (the product's `alignment_plan` is the vector form: two writings of the same IEEE operations in the same order, which
    tests/test_align_ref.py compares): a dict of the integers of every step and the quad (float64 [4,2]: NW, SW, SE, NE)
    after each."""
    lm = np.asarray(lm)
    lex, ley = float(np.mean(lm[36:42, 0])), float(np.mean(lm[36:42, 1]))
    rex, rey = float(np.mean(lm[42:48, 0])), float(np.mean(lm[42:48, 1]))
    ex, ey = (lex + rex) * 0.5, (ley + rey) * 0.5                    # between the eyes
    ax, ay = rex - lex, rey - ley                                    # eye to eye
    mx, my = float(lm[48, 0] + lm[54, 0]) * 0.5, float(lm[48, 1] + lm[54, 1]) * 0.5
    dx, dy = mx - ex, my - ey                                        # eyes to mouth
    ux, uy = ax - dy * -1, ay - dx * 1
    norm = _hyp(ux, uy)
    ux, uy = ux / norm, uy / norm
    reach = max(_hyp(ax, ay) * 2.0, _hyp(dx, dy) * 1.8)
    ux, uy = ux * reach, uy * reach
    vx, vy = uy * -1, ux * 1
    cx, cy = ex + dx * 0.1, ey + dy * 0.1
    corners = [[cx - ux - vx, cy - uy - vy], [cx - ux + vx, cy - uy + vy], [cx + ux + vx, cy + uy + vy], [cx + ux - vx, cy + uy - vy]]
    side = _hyp(ux, uy) * 2
    w, h = int(width), int(height)
    P = {"quad_input": np.array(corners, np.float64), "qsize_input": side, "size_input": (w, h),
         "output_size": int(output_size), "transform_size": int(transform_size)}

    def box():
        xs, ys = [c[0] for c in corners], [c[1] for c in corners]
        return math.floor(min(xs)), math.floor(min(ys)), math.ceil(max(xs)), math.ceil(max(ys))

    factor = int(math.floor(side / output_size * 0.5))
    P["shrink"], P["rsize"] = factor, None
    if factor > 1:
        w, h = int(np.rint(float(w) / factor)), int(np.rint(float(h) / factor))
        P["rsize"] = (w, h)
        corners = [[c[0] / factor, c[1] / factor] for c in corners]
        side = side / factor
    P["quad_shrunk"], P["qsize"] = np.array(corners, np.float64), side

    margin = max(int(np.rint(side * 0.1)), 3)
    x0, y0, x1, y1 = box()
    cut = (max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, w), min(y1 + margin, h))
    P["border"], P["crop"] = margin, None
    if cut[2] - cut[0] < w or cut[3] - cut[1] < h:
        P["crop"] = cut
        w, h = cut[2] - cut[0], cut[3] - cut[1]
        corners = [[c[0] - cut[0], c[1] - cut[1]] for c in corners]
    P["quad_cropped"], P["size_cropped"] = np.array(corners, np.float64), (w, h)

    x0, y0, x1, y1 = box()
    short = (max(margin - x0, 0), max(margin - y0, 0), max(x1 - w + margin, 0), max(y1 - h + margin, 0))
    P["pad"], P["blur"] = None, side * 0.02
    if enable_padding and max(short) > margin - 4:
        least = int(np.rint(side * 0.3))
        widths = tuple(max(v, least) for v in short)
        P["pad"] = widths
        w, h = w + widths[0] + widths[2], h + widths[1] + widths[3]
        corners = [[c[0] + widths[0], c[1] + widths[1]] for c in corners]
    P["quad"], P["size"] = np.array(corners, np.float64), (w, h)
    return P


def shrink(img, P):
    return img.resize(P["rsize"], PIL.Image.LANCZOS) if P["rsize"] is not None else img


def crop(img, P):
    return img.crop(P["crop"]) if P["crop"] is not None else img


def pad_float(arr_u8, pad, blur):
    """:170-177 on an HWC byte array -> the float32 image before `rint`.  float32 arithmetic throughout: the widths are
    Python ints, so no operand is promoted to float64."""
    left, top, right, bottom = (int(v) for v in pad)
    canvas = np.pad(arr_u8.astype(np.float32), ((top, bottom), (left, right), (0, 0)), mode="reflect")
    height, width = canvas.shape[:2]
    col = np.arange(width, dtype=np.float32)
    row = np.arange(height, dtype=np.float32)
    near_x = 1.0 - np.minimum(col / left, ((width - 1) - col) / right)        # 1 at the left / right edge, <= 0 inside
    near_y = 1.0 - np.minimum(row / top, ((height - 1) - row) / bottom)
    edge = np.maximum(near_x[None, :, None], near_y[:, None, None])
    assert edge.dtype == np.float32
    soft = scipy.ndimage.gaussian_filter(canvas, [blur, blur, 0])
    canvas += (soft - canvas) * np.clip(edge * 3.0 + 1.0, 0.0, 1.0)            # blurred towards the edge
    canvas += (np.median(canvas, axis=(0, 1)) - canvas) * np.clip(edge, 0.0, 1.0)  # and faded to the median colour
    assert canvas.dtype == np.float32
    return canvas


def to_bytes(pre):
    return np.uint8(np.clip(np.rint(pre), 0, 255))


def pad(img, P):
    """-> (PIL image, float32 HWC image before rint or None when the plan does not pad)."""
    if P["pad"] is None:
        return img, None
    pre = pad_float(np.asarray(img), P["pad"], P["blur"])
    return PIL.Image.fromarray(to_bytes(pre), 'RGB'), pre


def tie_eligible(pre):
    """Bytes that may differ by one level: the float32 value before rint within TIE_EPS of a half-integer."""
    f = pre.astype(np.float64)
    return np.abs(f - np.floor(f) - 0.5) < TIE_EPS


def transform(img, quad, transform_size):
    return img.transform((transform_size, transform_size), PIL.Image.QUAD, (np.asarray(quad) + 0.5).flatten(), PIL.Image.BILINEAR)


def resize(img, output_size):
    return img.resize((output_size, output_size), PIL.Image.LANCZOS) if output_size < img.size[0] else img


def finish(padded, P):
    """transform + resize of an already padded PIL image (the stages after `pad`)."""
    return resize(transform(padded, P["quad"], P["transform_size"]), P["output_size"])


def align(img, lm, output_size=1024, transform_size=4096, enable_padding=True):
    """All stages on a PIL RGB image -> dict(plan, shrunk, cropped, padded, pre, transformed, out); `out` is what the
    reference's align_face(return_tensors=False) returns for this image and these landmarks."""
    P = plan(lm, img.size[0], img.size[1], output_size, transform_size, enable_padding)
    S = {"plan": P}
    S["shrunk"] = shrink(img, P)
    S["cropped"] = crop(S["shrunk"], P)
    S["padded"], S["pre"] = pad(S["cropped"], P)
    S["transformed"] = transform(S["padded"], P["quad"], transform_size)
    S["out"] = resize(S["transformed"], output_size)
    return S


# ---- the seeded inputs of tests/golden/align.npz (tools/make_align_golden.py) and of the small-size tests ----
def landmarks(cx, cy, eye_dist, angle_deg=0.0):
    """68 integer landmarks of a schematic face: only the eyes (36-47) and the mouth corners (48, 54) enter the plan."""
    lm = np.zeros((68, 2), np.float64)
    t = np.linspace(0, 2 * np.pi, 6, endpoint=False)
    ring = np.stack([np.cos(t), np.sin(t) * 0.5], 1) * eye_dist * 0.15
    lm[36:42] = ring + [-eye_dist / 2, 0]
    lm[42:48] = ring + [eye_dist / 2, 0]
    t = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    lm[48:60] = np.stack([-np.cos(t) * eye_dist * 0.4, np.sin(t) * eye_dist * 0.1], 1) + [0, eye_dist * 1.1]
    a = np.deg2rad(angle_deg)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return np.rint(lm @ rot.T + [cx, cy]).astype(np.int64)


def image(width, height, seed, face=None):
    """Seeded uint8 HWC test image: a smooth separable pattern per channel plus integer noise; with face = (cx, cy, radius)
    only inside that disc, on a flat backdrop elsewhere (a portrait in front of a wall: where the backdrop fills the fade
    zone of the pad stage and is the median, the padded float image holds exact integers there - far fewer bytes whose
    value before rint sits next to a half-integer than in an image that is textured everywhere)."""
    rng = np.random.default_rng(seed)
    ph = rng.random(6) * 6
    ys, xs = np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32)
    img = rng.integers(0, 41, (height, width, 3), dtype=np.uint8)
    for c in range(3):  # 107 +- 90 plus noise in [0, 40]: inside [17, 237]
        base = np.outer(np.sin(ys / (53 + 9 * c) + ph[c]) * np.float32(90.0), np.cos(xs / (37 + 11 * c) + ph[3 + c]))
        base += np.float32(107.0)
        np.rint(base, out=base)
        img[:, :, c] += base.astype(np.uint8)
    if face is not None:
        cx, cy, radius = face
        outside = (ys[:, None] - cy) ** 2 + (xs[None, :] - cx) ** 2 > radius * radius
        np.copyto(img, np.array([96, 141, 180], np.uint8), where=outside[:, :, None])
    return img


def case_inputs(case):
    """(uint8 HWC image, [68,2] landmarks) of an entry of GOLDEN_CASES / SMALL_CASES."""
    width, height, seed, lm_args = case
    cx, cy, eye_dist, _ = lm_args
    return image(width, height, seed, (cx, cy + 0.3 * eye_dist, 1.6 * eye_dist)), landmarks(*lm_args)


# name -> (width, height, image seed, landmark arguments): a face well inside the image, the same face near a corner
# (the pad path), an image large enough that shrink >= 2 (qsize >= 4096)
GOLDEN_CASES = {
    "inside": (600, 500, 11, (300, 230, 80, 7.0)),
    "corner": (600, 500, 11, (95, 90, 80, 7.0)),
    "shrink": (4500, 4500, 13, (2250, 2137, 1030, -4.0)),
}
# the same three geometries at a size where transform 256 / output 64 leaves them in the same regime
SMALL_CASES = {
    "inside": (150, 125, 21, (75, 57, 20, 7.0)),
    "corner": (150, 125, 21, (24, 22, 20, 7.0)),
    "shrink": (1300, 1300, 23, (650, 620, 262, -4.0)),
}
