"""bench.py's --dump-outputs files and what a plain run (no --full) puts in its line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_or_first_item_plus_seeded_sample(tmp_path):
    import bench

    small = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "a"), "x", small)
    assert sorted(os.listdir(tmp_path / "a")) == ["x.npy"]
    got = np.load(tmp_path / "a" / "x.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())

    # the default run's images (8 x 3 x 1024^2 fp32 = 100 MB) do not fit the 64 MB budget: first image + sample
    big = torch.randn(8, 3, 1024, 1024, generator=torch.Generator().manual_seed(0))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), "image", big)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["image_0.npy", "image_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 64 << 20
    first = np.load(tmp_path / "b" / "image_0.npy")
    assert first.dtype == np.float32 and np.array_equal(first, big[0].numpy())
    sample = np.load(tmp_path / "b" / "image_sample.npy")
    assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_SAMPLE,)
    idx = np.sort(np.random.default_rng(0).choice(big.numel(), size=bench.DUMP_SAMPLE, replace=False))
    assert np.all(np.diff(idx) > 0) and idx[0] < big[0].numel() and idx[-1] >= 7 * big[0].numel()  # spread over the batch
    assert np.array_equal(sample, big.reshape(-1).numpy()[idx])
    assert np.array_equal(sample, np.load(tmp_path / "c" / "image_sample.npy"))  # the sample is fixed, not drawn per run

    u8 = torch.full((2, 3, 8, 8), 200, dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path / "d"), "images_u8", u8)
    got = np.load(tmp_path / "d" / "images_u8.npy")
    assert got.dtype == np.float32 and np.all(got == 200.0)


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_last_step(tmp_path):
    """A plain run prints the headline line without the --full objects, and --dump-outputs holds the images of the
    LAST timed step: the same seed, latents and number of forwards in this process reproduce them."""
    import bench
    from hairfastgan_amd import _runtime

    steps, warmup = 3, 1
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--priming", "0", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "stylegan2_generator_fwd_1024_images_per_sec" and line["unit"] == "images/s"
    # the child runs in the modes the environment configures; earlier tests may have switched this process's modes since
    mode = os.environ.get("HAIRFAST_CONV_PRECISION", "f16x3")
    invariant = os.environ.get("HAIRFAST_DETERMINISTIC", "1") not in ("", "0")
    assert line["higher_is_better"] is True and line["dtype"] == bench.DTYPES["f16x3" if mode == "auto" else mode]
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["ms_per_step"] > 0 and abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    for key in ("roofline", "exact_f32", "f16_mode", "swap_schedule", "swap_pipeline", "cpu_baseline", "summary"):
        assert key not in line, key

    dev = torch.device("cuda:0")
    g, _ = bench.build_generator(dev)
    torch.manual_seed(3407)
    latent = torch.randn(8, 18, 512, device=dev)
    with torch.inference_mode(), _runtime.conv_precision_scope(mode), _runtime.batch_invariant_scope(invariant):
        for _ in range(warmup + steps):
            img, _ = g([latent], input_is_latent=True)
        img = img.cpu()
    first = np.load(out_dir / "image_0.npy")
    sample = np.load(out_dir / "image_sample.npy")
    idx = np.sort(np.random.default_rng(0).choice(img.numel(), size=bench.DUMP_SAMPLE, replace=False))
    scale = max(1.0, float(img.abs().max()))
    assert np.abs(first - img[0].numpy()).max() <= 1e-4 * scale
    assert np.abs(sample - img.reshape(-1).numpy()[idx]).max() <= 1e-4 * scale
