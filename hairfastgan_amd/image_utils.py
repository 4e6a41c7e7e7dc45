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
