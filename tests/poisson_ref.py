"""Test helper: CPU restatement of the reference's poisson_image_blending (utils/image_utils.py:58-94).

* `quantize` - torchvision save_image's bytes: mul(255), add_(0.5), clamp_(0, 255), to(uint8), fp32, two roundings;
* `dilate_erosion_mask` - DilateErosion.mask (utils/image_utils.py:42-55), the reference's F.conv2d loop;
* `masks_from_labels` / `poisson_image_blending_ref` - steps 1-3 with oracle.ref_bisenet.get_segmentation;
* `setup` / `jacobi` / `finish` / `solve` - numpy fp32 restatement of `fpie -g max` (step 4).

Step 4 is NOT pinned: fpie's source is not available.  Unverified: the mask threshold (byte >= 128), the sweep-count
convention (`-n maxn` = maxn synchronous sweeps from X_0 = target) and truncation of the solution to bytes.  BiSeNet,
the dilation and the quantisation are the reference's code paths (the oracle pins BiSeNet)."""
import numpy as np
import torch
import torch.nn.functional as F

HAIR = 13
_NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0))  # left, right, up, down


def quantize(x):
    """save_image's bytes of a float array / tensor (any shape)."""
    x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    v = x * np.float32(255)
    v = v + np.float32(0.5)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)


def omega(mask):
    """mask u8 [H,W] -> bool [H,W]: byte >= 128, outermost rows and columns excluded."""
    om = np.asarray(mask) >= 128
    om[0, :] = om[-1, :] = om[:, 0] = om[:, -1] = False
    return om


def setup(s, t, mask):
    """s (source = face), t (target = final) u8 [C,H,W], mask u8 [H,W] -> (B, X_0) fp32 [C,H,W], 0 off Omega."""
    s, t = np.asarray(s).astype(np.int64), np.asarray(t).astype(np.int64)
    om = omega(mask)
    H, W = om.shape
    acc = np.zeros(t.shape, np.int64)
    if H >= 3 and W >= 3:
        sp, tp = s[:, 1:-1, 1:-1], t[:, 1:-1, 1:-1]
        inner = np.zeros(sp.shape, np.int64)
        for dy, dx in _NEIGHBOURS:
            sq = s[:, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
            tq = t[:, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
            gs, gt = sp - sq, tp - tq
            inner += np.where(np.abs(gs) < np.abs(gt), gt, gs)                      # tie: the source gradient
            inner += np.where(om[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx], 0, tq)     # boundary of Omega: the target
        acc[:, 1:-1, 1:-1] = inner
    b = np.where(om, acc, 0).astype(np.float32)
    x0 = np.where(om, t, 0).astype(np.float32)
    return b, x0


def jacobi(b, x, mask, sweeps):
    """`sweeps` synchronous sweeps X <- ((((B + up) + down) + left) + right) / 4 on Omega (fp32), X = 0 off Omega."""
    om = omega(mask)[1:-1, 1:-1]
    x = np.array(x, np.float32)
    for _ in range(sweeps):
        nx = np.zeros_like(x)
        v = (((b[:, 1:-1, 1:-1] + x[:, :-2, 1:-1]) + x[:, 2:, 1:-1]) + x[:, 1:-1, :-2]) + x[:, 1:-1, 2:]
        nx[:, 1:-1, 1:-1] = np.where(om, v / np.float32(4), np.float32(0))
        x = nx
    return x


def finish(x, t, mask):
    om = omega(mask)
    return np.where(om, np.clip(x, np.float32(0), np.float32(255)).astype(np.uint8), np.asarray(t)).astype(np.uint8)


def solve(s, t, mask, maxn):
    """`fpie -s s -t t -m mask -n maxn -g max` -> (u8 result [C,H,W], fp32 X after maxn sweeps)."""
    b, x = setup(s, t, mask)
    x = jacobi(b, x, mask, maxn)
    return finish(x, t, mask), x


def dilate_erosion_mask(mask, dilate_erosion):
    """utils/image_utils.py:42-55 (DilateErosion.mask) on the CPU."""
    weight = torch.Tensor([[False, True, False], [True, True, True], [False, True, False]]).float()[None, None, ...]
    masks = mask.clone().repeat(*([2] + [1] * (len(mask.shape) - 1))).float()
    sum_w = weight.sum().item()
    n = len(mask)
    for _ in range(dilate_erosion):
        masks = F.conv2d(masks, weight, bias=None, stride=1, padding="same", dilation=1, groups=1)
        masks[:n] = (masks[:n] > 0).float()
        masks[n:] = (masks[n:] == sum_w).float()
    return masks[:n], masks[n:]


def masks_from_labels(final_labels, face_labels, dilate_erosion=30):
    """utils/image_utils.py:69-76 + save_image of the mask: CelebAMask labels [1,1,H,W] of final and face -> the mask
    PNG's byte plane u8 [H,W] (the PNG repeats it in three channels).  The bicubic resize runs at the image size (the
    reference's 1024^2 is the identity there; other sizes are this project's extension)."""
    hair_target = torch.where(final_labels == HAIR, torch.ones_like(final_labels), torch.zeros_like(final_labels))
    hair_face = torch.where(face_labels == HAIR, torch.ones_like(face_labels), torch.zeros_like(face_labels))
    keep = F.interpolate(((1 - hair_target) * (1 - hair_face)).float(), size=tuple(final_labels.shape[-2:]), mode="bicubic")
    dilation, _ = dilate_erosion_mask(1 - keep, dilate_erosion)
    mask_save = 1 - dilation[0]          # [1,H,W]
    return quantize(mask_save)[0]


def poisson_image_blending_ref(P, final_image, face_image, dilate_erosion=30, maxn=115):
    """The whole reference function on the CPU with the oracle's BiSeNet (parameters P): final / face [3,H,W] float in
    [0,1] -> (u8 result [3,H,W], u8 mask plane [H,W])."""
    from oracle import ref_bisenet as BS

    final_labels = BS.get_segmentation(P, final_image[None].float(), resize=False)   # un-normalised: the reference's quirk
    face_labels = BS.get_segmentation(P, face_image[None].float(), resize=False)
    mask = masks_from_labels(final_labels, face_labels, dilate_erosion)
    out, _ = solve(quantize(face_image), quantize(final_image), mask, maxn)
    return out, mask
