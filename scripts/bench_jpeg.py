"""rcot_jpeg_roundtrip (csrc/jpeg.hip) on 321 x 481, 1024 x 1024 and 1356 x 2040 images at 4:2:0 and 4:4:4, quality 10, against the
host's round trip of the same images — PIL encode + decode on one core, then the upload — in the same call; and the folder loader
alone for ``jpeg_q10``, uncached against the device-resident training set, by the method of scripts/bench_loader.py.

    python scripts/bench_jpeg.py > profiles/jpeg_roundtrip.txt

Bytes of a round trip: 4:4:4 reads the image once and writes it once, 6 B per pixel.  4:2:0 adds the decoded planes, written by the
first launch and read by the second: 1.5 B per pixel of the image rounded up to tiles of 16 x 64, twice.  Roofline time = bytes /
6.3 TB/s (the achievable rate of DESIGN.md section 6).  Images of these sizes stay in the Infinity Cache once warm: the figures are
cache-resident rates, as they are inside the loader, where the upload has just written the image.

Device time: HIP events around single calls (median, minimum and maximum of 30 after 5 warm-ups, the cases alternating inside every
round) and the library's own per-dispatch time stamps over 30 calls: kernel time alone, per symbol.  Host time: a host clock around
``Image.save`` to memory + ``Image.open`` + ``np.array`` + the upload, ended by a device synchronise; median of 10 after 2.

Loader: 64 images of 321 x 481 (smooth content plus mild noise, as scripts/bench_loader.py writes them), B = 8, P = 128,
--threads 4 and 16; windows as there.

There is no fallback: without a GPU the script fails.
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_loader as BL  # noqa: E402
from bench_resize import event_us, kernel_rows  # noqa: E402

SIZES = ((321, 481), (1024, 1024), (1356, 2040))
QUALITY = 10
ROUNDS, WARMUP = 30, 5
HBM = 6.3e12


def moved_bytes(h, w, sub):
    tiles = -(-w // 64) * -(-h // 16)
    return 6 * h * w + (2 * tiles * 1536 if sub == 2 else 0)


def host_roundtrip_ms(img, sub, device):
    from PIL import Image
    v = []
    for r in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=QUALITY, subsampling=sub)
        out = np.array(Image.open(io.BytesIO(buf.getvalue())))
        d = torch.from_numpy(out).to(device)
        torch.cuda.synchronize()
        if r >= 2:
            v.append((time.perf_counter() - t0) * 1e3)
    return d, v


def kernel_table(be):
    g = np.random.Generator(np.random.PCG64(1))
    print(f"rcot_jpeg_roundtrip at quality {QUALITY}, {torch.cuda.get_device_name(0)}; roofline = bytes / {HBM / 1e12:.1f} TB/s")
    cases = {}
    for h, w in SIZES:
        ph = g.uniform(0, 6.28, 2)
        base = 128 + 60 * np.sin(np.linspace(0, 6, h) + ph[0])[:, None, None] * np.cos(np.linspace(0, 5, w) + ph[1])[None, :, None]
        img = np.clip(base + g.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)
        d = torch.from_numpy(img).to(be.device)
        for sub in (2, 0):
            out = torch.empty_like(d)
            cases[(h, w, sub)] = (img, (lambda d=d, sub=sub, out=out: be.jpeg_roundtrip(d, QUALITY, sub, out=out)), out)
    samples = {k: [] for k in cases}
    for r in range(WARMUP + ROUNDS):
        for k, (_, fn, _) in cases.items():
            us = event_us(fn)
            if r >= WARMUP:
                samples[k].append(us)
    print("[HIP events per call, us: median min max | MB | roofline us | median / roofline]   then the host's round trip of the same image "
          "[PIL encode + decode on one core + upload, ms: median min max | device result equals the host's]")
    for k, v in samples.items():
        h, w, sub = k
        img, fn, out = cases[k]
        nb = moved_bytes(h, w, sub)
        roof = nb / HBM * 1e6
        fn()
        host, hv = host_roundtrip_ms(img, sub, be.device)
        same = bool(torch.equal(host, out))
        print(f"  {h} x {w} {'4:2:0' if sub == 2 else '4:4:4'} {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f} | {nb / 1e6:6.1f} | "
              f"{roof:5.1f} | x{statistics.median(v) / roof:.1f}   host {statistics.median(hv):7.2f} {min(hv):7.2f} {max(hv):7.2f} ms | "
              f"{'equal' if same else 'DIFFERENT'}")
    print("kernel time from the library's per-dispatch time stamps [symbol | launches | us per launch]")
    for k, (_, fn, _) in cases.items():
        h, w, sub = k
        rows = kernel_rows(be, fn, ROUNDS)
        total = sum(us * n for _, n, us in rows) / ROUNDS
        roof = moved_bytes(h, w, sub) / HBM * 1e6
        print(f"    {h} x {w} {'4:2:0' if sub == 2 else '4:4:4'}: {total:.1f} us per call, x{total / roof:.1f} of the roofline's {roof:.1f} us")
        for sym, n, us in rows:
            print(f"        {sym} | {n} | {us:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--sr_batches", type=int, default=100)
    ap.add_argument("--warm_batches", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cache_gb", type=float, default=16.0)
    ap.add_argument("--images", type=int, default=64)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: scripts/bench_jpeg.py measures the HIP path only")
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    kernel_table(be)
    with tempfile.TemporaryDirectory() as root:
        BL.make_folders(root, 1, 0, opt.images, 0)
        args = Namespace(de_type=[f"jpeg_q{QUALITY}"], jpeg_dir=f"{root}/Denoise/", patch_size=BL.P)
        print(f"\n{opt.images} images of 321 x 481 (smooth content plus mild noise), --de_type jpeg_q{QUALITY}, 4:2:0")
        BL.loader_table({f"jpeg_q{QUALITY}": args}, be, opt)


if __name__ == "__main__":
    main()
