"""rcot_noise_u8 (csrc/noise.hip) on a 1356 x 2040 image for the three models, and the folder loader alone for the degradation chain
``chain_blur_g1.6+noise_g10+jpeg_q40`` next to ``jpeg_q10`` — uncached against the device-resident training set, by the method of
scripts/bench_loader.py, both tasks in the same call on the same box.

    python scripts/bench_chain.py > profiles/degradation_chain.txt

Bytes of a noise pass: the image read once and written once, 6 B per pixel.  Roofline time = bytes / 6.3 TB/s (the achievable rate of
DESIGN.md section 6, the yardstick of profiles/jpeg_roundtrip.txt and profiles/resize_passes.txt).  A 1356 x 2040 image (8.3 MB) stays
in the Infinity Cache once warm: the figures are cache-resident rates, as they are inside the loader.  ``gray`` makes one deviate per
pixel where ``g`` and ``pg`` make three: the ratio of their times says how much of the time is the deviates.

Device time: HIP events around single calls (median, minimum and maximum of 30 after 5 warm-ups, the cases alternating inside every
round) and the library's own per-dispatch time stamps over 30 calls: kernel time alone.

Loader: 64 images of 321 x 481 (smooth content plus mild noise, as scripts/bench_loader.py writes them), B = 8, P = 128, --threads 4
and 16; windows as there.  The chain has a noise stage, so the cache keeps the decoded images only and the chain runs for every sample
on both routes; what the cached route saves is the decode and the upload.

There is no fallback: without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys
import tempfile
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_loader as BL  # noqa: E402
from bench_resize import event_us, kernel_rows  # noqa: E402

H, W = 1356, 2040
ROUNDS, WARMUP = 30, 5
HBM = 6.3e12
CHAIN = "chain_blur_g1.6+noise_g10+jpeg_q40"
STEP_RATE = 113.0                                            # patches/s of the fastest training step (bf16x3, one MI355X: README)
CASES = (("g", 25.0, 0.0, False), ("gray", 25.0, 0.0, False), ("pg", 0.5, 2.0, False), ("g", 25.0, 0.0, True))


def kernel_table(be):
    g = np.random.Generator(np.random.PCG64(1))
    ph = g.uniform(0, 6.28, 2)
    base = 128 + 60 * np.sin(np.linspace(0, 6, H) + ph[0])[:, None, None] * np.cos(np.linspace(0, 5, W) + ph[1])[None, :, None]
    img = torch.from_numpy(np.clip(base + g.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)).to(be.device)
    nb = 6 * H * W
    roof = nb / HBM * 1e6
    print(f"rcot_noise_u8 on {H} x {W}, {torch.cuda.get_device_name(0)}; {nb / 1e6:.1f} MB read + written, roofline = bytes / "
          f"{HBM / 1e12:.1f} TB/s = {roof:.2f} us")
    cases = {}
    for model, p0, p1, inplace in CASES:
        src = img.clone()
        out = src if inplace else torch.empty_like(src)
        cases[(model, inplace)] = (lambda src=src, out=out, model=model, p0=p0, p1=p1: be.noise_u8(src, model, p0, p1, 7, out=out))
    samples = {k: [] for k in cases}
    for r in range(WARMUP + ROUNDS):
        for k, fn in cases.items():
            us = event_us(fn)
            if r >= WARMUP:
                samples[k].append(us)
    print("[model | HIP events per call, us: median min max | kernel time alone from the library's per-dispatch time stamps, us per launch | "
          "kernel time / roofline]")
    for k, v in samples.items():
        rows = kernel_rows(be, cases[k], ROUNDS)
        assert len(rows) == 1 and rows[0][1] == ROUNDS, rows                # one launch per call
        print(f"  {k[0]:<4} {'in place' if k[1] else 'out of place':<12} | {statistics.median(v):7.1f} {min(v):7.1f} {max(v):7.1f} | {rows[0][2]:7.2f} | "
              f"x{rows[0][2] / roof:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--sr_batches", type=int, default=100)
    ap.add_argument("--warm_batches", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cache_gb", type=float, default=16.0)
    ap.add_argument("--images", type=int, default=64)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: scripts/bench_chain.py measures the HIP path only")
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    kernel_table(be)
    with tempfile.TemporaryDirectory() as root:
        BL.make_folders(root, 1, 0, opt.images, 0)
        folder = f"{root}/Denoise/"
        tasks = {"chain": Namespace(de_type=[CHAIN], chain_dir=folder, patch_size=BL.P),
                 "jpeg_q10": Namespace(de_type=["jpeg_q10"], jpeg_dir=folder, patch_size=BL.P)}
        print(f"\n{opt.images} images of 321 x 481 (smooth content plus mild noise); chain = --de_type {CHAIN}, 4:2:0, replicate")
        rows = BL.loader_table(tasks, be, opt)
    slowest = min(k * BL.B / dt for _, task, _, route, k, dt, _ in rows if (task, route) == ("chain", "uncached"))
    print(f"\nthe condition: the chain's uncached loader, slowest window {slowest:.1f} patches/s, "
          f"{'delivers more than' if slowest > STEP_RATE else 'does NOT deliver'} the {STEP_RATE:.0f} patches/s of the fastest training step "
          f"(bf16x3): x{slowest / STEP_RATE:.2f}")


if __name__ == "__main__":
    main()
