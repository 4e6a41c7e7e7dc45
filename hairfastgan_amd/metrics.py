"""FID-CLIP on the device: the metric the reference's authors judge results with (scripts/fid_metric.py:25-50,
utils/train.py:90-161), which there is torchmetrics' FrechetInceptionDistance around `ClipModel` plus a host LAPACK.

    python -m hairfastgan_amd.metrics --source_dataset DIR --methods_dataset name,DIR [name,DIR ...] --output logs/metric.csv

Pieces, all on the library's kernels:
  files -> uint8 [N,3,299,299]      `read_images` + Pillow-exact Lanczos resize (hf_resize_lanczos_u8): `load_images_299`
  images -> features [N,512]        `ClipModel`: byte / 255, adaptive average pooling to 224^2, CLIP normalisation, the
                                    native ViT-B/32 image tower (clip_vit.py)
  features -> sum, cov_sum (fp64)   `FrechetDistance.update`: hf_frechet_accumulate_f64, streaming and reproducible
  statistics -> distance            `FrechetDistance.compute`: hf_frechet_stats_f64, two Jacobi eigensolves
                                    (hf_sym_eig_jacobi_f64) around hf_frechet_congruence_f64, hf_frechet_finish_f64
The host lists files and copies one double per method back.  The Inception-v3 half of fid_metric.py (the plain `FID` column)
is `FrechetDistance(hairfastgan_amd.inception.InceptionV3(2048, weights=...))`, the command line's --fid; its weights are an
explicit argument (`checkpoints.inception_fid()` finds the published file), never an implicit download.

The command lines that score a folder of results against a folder of ground truth (`lpips`, `identity`) share their file
handling here: `load_pairs`, `add_pair_arguments`, `unit_range`, `score_pairs`.

Every entry point takes `lib=None`: the loaded HIP library on torch's current stream.  Tests hand in the CPU interpreter
build of the same kernel sources and CPU tensors.
"""
import argparse
import csv
import json
import os
from pathlib import Path

import torch

from . import _marshal as M

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _backend(lib, *tensors):
    """-> (library, stream): the product's on torch's current stream (GPU tensors only), or the one handed in."""
    if lib is not None:
        return lib, None
    from . import _runtime

    _runtime.require_gpu(*tensors)
    return _runtime.lib(), _runtime.stream()


class ClipModel:
    """models/Encoders.py:140-160: uint8 images are divided by 255, every image is average-pooled to 224^2
    (AdaptiveAvgPool2d), normalised with CLIP's mean / std and embedded by `tower.encode_image`.

    tower: a `clip_vit.ClipImageTower` (default: ViT-B/32 with the weights `checkpoints.clip_tower()` finds) or anything
    with `encode_image([B,3,224,224]) -> [B,d]`."""

    def __init__(self, tower=None, lib=None):
        if tower is None:
            from .checkpoints import clip_tower
            from .clip_vit import ClipImageTower

            tower = ClipImageTower().eval()
            tower.load_clip_state_dict(clip_tower())
            tower = tower.to("cuda")
        self.tower = tower
        self._lib = lib

    @torch.inference_mode()
    def __call__(self, images):
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f"expected images [B,3,H,W]; got {tuple(images.shape)}")
        L, st = _backend(self._lib, images)
        x = M.u8_to_unit(L, st, images) if images.dtype == torch.uint8 else images.float()
        pooled = torch.empty((x.shape[0], 3, 224, 224), dtype=torch.float32, device=x.device)
        M.adaptive_avgpool_into(L, st, pooled, x, 0)
        mean = torch.tensor(CLIP_MEAN, dtype=torch.float32, device=x.device)[None, :, None, None]
        std = torch.tensor(CLIP_STD, dtype=torch.float32, device=x.device)[None, :, None, None]
        return self.tower.encode_image((pooled - mean) / std)  # T.Normalize: sub, then div


class FrechetDistance:
    """The call surface of torchmetrics' FrechetInceptionDistance as scripts/fid_metric.py uses it, on the device.

    feature: a callable images -> features [N,d] (fp32 or fp16), e.g. `ClipModel()` or `inception.InceptionV3(2048, weights)`.
        An int (torchmetrics' Inception-v3 layer widths 64 / 192 / 768 / 2048) raises NotImplementedError: torchmetrics then
        downloads weights, here they are an explicit argument of the module.
    reset_real_features: False keeps the statistics of the real side over `reset()`.
    normalize: accepted for signature compatibility and WITHOUT effect: in torchmetrics it only rescales [0,1] float
        images to bytes in front of the built-in Inception network and is not applied with a feature module - stated
        from memory of torchmetrics' source and NOT checked against an installed copy (torchmetrics is no dependency of
        this package); `ClipModel` takes bytes and [0,1] floats alike.

    State per side: sum [d] and cov_sum [d,d] in fp64 and the sample count n (int64), all on the device of the first
    features.  Updates are order-dependent only in the last bits and reproducible: k updates with consecutive slices give
    the bits of one update with the whole."""

    def __init__(self, feature, reset_real_features=True, normalize=False, max_sweeps=30, lib=None):
        if isinstance(feature, int):
            raise NotImplementedError(
                f"feature={feature}: an integer would need the Inception-v3 weights downloaded implicitly; pass the module with its "
                f"weights, FrechetDistance(InceptionV3({feature}, weights=checkpoints.inception_fid())) from hairfastgan_amd.inception, "
                "or another feature module such as hairfastgan_amd.metrics.ClipModel()")
        if not callable(feature):
            raise TypeError("feature must be a callable images -> [N,d]")
        self.feature = feature
        self.reset_real_features = bool(reset_real_features)
        self.normalize = bool(normalize)
        self.max_sweeps = int(max_sweeps)
        self._lib = lib
        self._state = {True: None, False: None}  # real -> [sum, cov_sum, n tensor, n]
        self.last_info = None

    def to(self, *args, **kwargs):
        return self

    def eval(self):
        return self

    def state(self, real):
        """(sum, cov_sum, n) of one side - device tensors - or None before its first update."""
        s = self._state[bool(real)]
        return None if s is None else tuple(s[:3])

    @torch.inference_mode()
    def update(self, imgs, real):
        self.update_features(self.feature(imgs), real)

    @torch.inference_mode()
    def update_features(self, feats, real):
        if feats.ndim != 2:
            raise ValueError(f"features must be [N,d]; got {tuple(feats.shape)}")
        real = bool(real)
        L, st = _backend(self._lib, feats)
        d = feats.shape[1]
        for side in (True, False):
            s = self._state[side]
            if s is not None and s[0].numel() != d:
                raise ValueError(f"features of dimension {d}, but the {'real' if side else 'fake'} side holds dimension {s[0].numel()}")
        if self._state[real] is None:
            self._state[real] = [torch.zeros(d, dtype=torch.float64, device=feats.device),
                                 torch.zeros((d, d), dtype=torch.float64, device=feats.device),
                                 torch.zeros((), dtype=torch.int64, device=feats.device), 0]
        s = self._state[real]
        M.frechet_accumulate_into(L, st, s[0], s[1], feats)
        s[2] += feats.shape[0]
        s[3] += feats.shape[0]

    @torch.inference_mode()
    def compute(self):
        """-> the distance, a 0-d float64 tensor on the device (not clamped at 0, like the reference)."""
        real, fake = self._state[True], self._state[False]
        if real is None or fake is None or real[3] < 2 or fake[3] < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        if real[0].numel() != fake[0].numel():
            raise ValueError("the two sides differ in feature dimension")
        L, st = _backend(self._lib, real[0], fake[0])
        mu1, s1 = M.frechet_stats(L, st, real[0], real[1], real[3])
        mu2, s2 = M.frechet_stats(L, st, fake[0], fake[1], fake[3])
        self.last_info = {}
        return M.frechet_distance_from_stats(L, st, mu1, s1, mu2, s2, self.max_sweeps, self.last_info)

    def reset(self):
        self._state[False] = None
        if self.reset_real_features:
            self._state[True] = None


def _f64_arg(t):
    return t.to(torch.float64).contiguous()


@torch.inference_mode()
def frechet_distance(mu1, sigma1, mu2, sigma2, max_sweeps=30, lib=None):
    """|mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 (sigma1 sigma2)^(1/2)) of device tensors -> 0-d float64 device tensor."""
    L, st = _backend(lib, mu1, sigma1, mu2, sigma2)
    return M.frechet_distance_from_stats(L, st, _f64_arg(mu1), _f64_arg(sigma1), _f64_arg(mu2), _f64_arg(sigma2), max_sweeps)


@torch.inference_mode()
def sym_eigh(a, max_sweeps=30, lib=None):
    """Eigenvalues (ascending) and eigenvectors (columns) of a symmetric device matrix in fp64, like torch.linalg.eigh,
    by the library's Jacobi solver.  RuntimeError when `max_sweeps` sweeps do not converge."""
    L, st = _backend(lib, a)
    w, v = M.sym_eigh_f64(L, st, _f64_arg(a), True, max_sweeps)
    w, order = torch.sort(w)
    return w, v[:, order].contiguous()


def list_image_files(directory):
    """utils/image_utils.py:97-108: the .jpg / .jpeg / .png files (any letter case) of a directory, sorted."""
    return [e for e in sorted(os.listdir(directory))
            if os.path.isfile(os.path.join(directory, e)) and Path(e).suffix.lower() in IMAGE_EXTENSIONS]


@torch.inference_mode()
def load_images_299(directory, files, decoder="pil", device=None, lib=None):
    """utils/train.py:90-122 for RGB files: uint8 [N,3,299,299], every image byte-equal to
    `Image.open(p).resize((299, 299), Image.LANCZOS)`.  decoder: `read_images`' ("pil" decodes on the host, "device" on the
    GPU); the resize runs on the device either way."""
    from . import face_align as FA
    from .image_utils import read_images

    device = torch.device(device if device is not None else "cuda")
    images = [t.to(device) for t in read_images([os.path.join(directory, f) for f in files], decoder=decoder)]
    if not images:
        return torch.empty((0, 3, 299, 299), dtype=torch.uint8, device=device)
    L, st = _backend(lib, *images)
    return torch.stack([FA.resize_lanczos(L, st, img.contiguous(), 299, 299) for img in images])


def load_pairs(data_path, gt_path, names, size, decoder="pil", device=None, lib=None):
    """-> (results, ground truth) uint8 [N,3,size,size]: the files `names` of both folders, each byte-equal to
    `Image.open(p).convert("RGB").resize((size, size), BILINEAR)`."""
    from . import face_align as FA
    from .image_utils import read_images

    device = torch.device(device if device is not None else "cuda")
    out = []
    for folder in (data_path, gt_path):
        images = [t.to(device).contiguous() for t in read_images([os.path.join(folder, f) for f in names], decoder=decoder)]
        L, st = _backend(lib, *images)
        out.append(torch.stack([FA.resize_bilinear(L, st, img, size, size) for img in images]))
    return out


def add_pair_arguments(parser, batch):
    """The arguments every paired-folder command line takes (`lpips`, `identity`); `batch`: the default of --batch."""
    parser.add_argument("--data_path", type=str, default="results")
    parser.add_argument("--gt_path", type=str, default="gt_images")
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--image_decoder", choices=("pil", "device"), default="pil", help="where the files are decoded")
    parser.add_argument("--batch", type=int, default=batch)


def score_pairs(args, score, tag, sentence, device=None, lib=None):
    """The scoring loop of calc_losses_on_images.py: every image file of args.data_path against the file of the same name in
    args.gt_path (FileNotFoundError when one has none), args.batch pairs at a time.  score(results, ground truth), both uint8
    [N,3,size,size], -> [N] float64; it is first called after the folders are checked.  Prints `sentence`.format(mean,
    population std) and writes it to inference_metrics/stat_<tag>.txt and the scores to scores_<tag>.json next to
    args.data_path.  -> {file name: score}."""
    names = list_image_files(args.data_path)
    missing = [f for f in names if not os.path.isfile(os.path.join(args.gt_path, f))]
    if missing:
        raise FileNotFoundError(f"no ground truth for {missing[0]} in '{args.gt_path}'")
    scores = {}
    for k in range(0, len(names), max(args.batch, 1)):
        part = names[k:k + max(args.batch, 1)]
        res, gt = load_pairs(args.data_path, args.gt_path, part, args.size, args.image_decoder, device, lib)
        scores.update(zip(part, score(res, gt).tolist()))  # one copy per batch
    values = torch.tensor(list(scores.values()), dtype=torch.float64)
    mean = float(values.mean()) if len(scores) else float("nan")
    std = float(values.std(unbiased=False)) if len(scores) else float("nan")
    result_str = sentence.format(mean, std)
    print(result_str)
    out_path = os.path.join(os.path.dirname(args.data_path), "inference_metrics")
    os.makedirs(out_path, exist_ok=True)
    with open(os.path.join(out_path, f"stat_{tag}.txt"), "w") as f:
        f.write(result_str)
    with open(os.path.join(out_path, f"scores_{tag}.json"), "w") as f:
        json.dump(scores, f)
    return scores


def unit_range(images_u8):
    """ToTensor + Normalize(0.5, 0.5) of uint8 images: fp32 in [-1, 1]."""
    return (images_u8.float() / 255 - 0.5) / 0.5


@torch.inference_mode()
def compute_fid_datasets(datasets, target, feature, batch=128, lib=None):
    """scripts/fid_metric.py:25-50: datasets = {name: images uint8 [N,3,H,W]}; the statistics of datasets[target] are
    taken once, every other entry is measured against them -> {name: distance (float)}."""
    fid = FrechetDistance(feature, reset_real_features=False, normalize=False, lib=lib)
    for k in range(0, datasets[target].shape[0], batch):
        fid.update(datasets[target][k:k + batch], real=True)
    result = {}
    for key, images in datasets.items():
        if key == target:
            continue
        fid.reset()
        for k in range(0, images.shape[0], batch):
            fid.update(images[k:k + batch], real=False)
        result[key] = fid.compute()
    return {key: value.item() for key, value in result.items()}  # the one copy per method


def _name_path(pair):
    name, path = pair.split(",", 1)
    return name, Path(path)


def main(argv=None, feature=None, lib=None, device=None, inception=None):
    """The command line of scripts/fid_metric.py: the FID_CLIP column and, with --fid, the plain FID column in front of it (the
    reference's order).  `feature`: the FID_CLIP feature module (default `ClipModel()`); `inception`: the FID one (default
    `InceptionV3(2048)` with the weights of --inception_weights or of `checkpoints.inception_fid`).
    -> {method: FID_CLIP}, with --fid {"FID": {method: value}, "FID_CLIP": {method: value}}."""
    parser = argparse.ArgumentParser(prog="python -m hairfastgan_amd.metrics", description="Compute FID-CLIP (and FID)")
    parser.add_argument("--source_dataset", type=Path, required=True, help="Dataset with real faces")
    parser.add_argument("--methods_dataset", type=_name_path, nargs="+", required=True, help="name,DIR of each method's results")
    parser.add_argument("--output", type=Path, default=Path("logs/metric.csv"), help="the CSV file to write")
    parser.add_argument("--image_decoder", choices=("pil", "device"), default="pil", help="where the files are decoded")
    parser.add_argument("--batch", type=int, default=128)
    parser.add_argument("--fid", action="store_true", help="also the Inception-v3 FID column")
    parser.add_argument("--inception_weights", type=str, default=None,
                        help="pt_inception-2015-12-05-6726825d.pth (default: HAIRFAST_INCEPTION_WEIGHTS or torch's hub cache)")
    args = parser.parse_args(argv)

    def load(path):
        return load_images_299(path, list_image_files(path), args.image_decoder, device, lib)

    source = args.source_dataset.name
    datasets = {source: load(args.source_dataset)}
    for method, path in args.methods_dataset:
        datasets[method] = load(path)
    columns = {}
    if args.fid:
        if inception is None:
            from .checkpoints import inception_fid
            from .inception import InceptionV3

            inception = InceptionV3(2048, weights=inception_fid(path=args.inception_weights), lib=lib)
            inception = inception.to(device if device is not None else "cuda")
        columns["FID"] = compute_fid_datasets(datasets, source, inception, args.batch, lib)
    columns["FID_CLIP"] = compute_fid_datasets(datasets, source, feature if feature is not None else ClipModel(lib=lib), args.batch, lib)
    names = list(columns["FID_CLIP"])
    rows = [(name, *(str(round(col[name], 2)) for col in columns.values())) for name in names]  # DataFrame.round(2).to_csv's digits
    print(f"{'':<24}" + "".join(f"{c:>10}" for c in columns))
    for name, *values in rows:
        print(f"{name:<24}" + "".join(f"{v:>10}" for v in values))
    os.makedirs(args.output.parent, exist_ok=True)
    with open(args.output, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(["", *columns])
        out.writerows(rows)
    return columns if args.fid else columns["FID_CLIP"]


if __name__ == "__main__":
    main()
