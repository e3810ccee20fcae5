"""rcot_blur_u8 (csrc/blur.hip) on one 1356 x 2040 image for the PSFs g1.6k7, g5k31, m31a30 and the 63 x 63 box (replicated border), and the
BD call (g1.6k7, every third pixel), against ``scipy.ndimage.correlate`` of the same image on one host core and against the time the
image's bytes take at 6.3 TB/s.

    python scripts/bench_blur.py > profiles/blur_psf.txt

Bytes of a blur: the image read once and the result written once, 6 B per pixel (3 + 1 / 3 for the BD call).  Roofline time = bytes /
6.3 TB/s (the achievable rate of DESIGN.md section 6).  A K x K correlation is arithmetic, not traffic: K^2 integer multiply-adds per
byte, so the second yardstick is the multiply-add rate, listed per case (non-zero taps only: zero taps are skipped).

Device time: HIP events around single calls (median, minimum and maximum of 20 after 3 warm-ups, the cases alternating inside every
round) and the library's own per-dispatch time stamps over 20 calls: kernel time alone, per symbol.  Host time: a host clock around
``scipy.ndimage.correlate`` (float64, mode nearest) of the three channels, one run per case; the device result is compared with it
(it may differ by one grey level at .5 ties: tests/test_blur_cpu.py).

There is no fallback: without a GPU the script fails.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_resize import event_us, kernel_rows  # noqa: E402

H, W = 1356, 2040
ROUNDS, WARMUP = 20, 3
HBM = 6.3e12


def main():
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: scripts/bench_blur.py measures the HIP path only")
    from rcot_amd import blur as B
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    g = np.random.Generator(np.random.PCG64(1))
    base = 128 + 60 * np.sin(np.linspace(0, 6, H))[:, None, None] * np.cos(np.linspace(0, 5, W))[None, :, None]
    img = np.clip(base + g.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    d = torch.from_numpy(img).to(be.device)
    psfs = {"g1.6k7": B.psf_of("g1.6k7"), "g5k31": B.psf_of("g5k31"), "m31a30": B.psf_of("m31a30"), "box63": np.full((63, 63), 1.0 / 3969)}
    cases = {}
    for name, h in psfs.items():
        q = B.quantise_psf(h)
        out = torch.empty_like(d)
        cases[name] = (h, q, (lambda p=B.device_psf(q, be.device), out=out: be.blur_u8(d, p, 0, out=out)), out, 1)
    Hc, Wc = H - H % 3, W - W % 3
    d3 = d[:Hc, :Wc].contiguous()
    out3 = torch.empty(Hc // 3, Wc // 3, 3, dtype=torch.uint8, device=be.device)
    q7 = B.psf_q_of("g1.6k7")
    cases["bd: g1.6k7 /3"] = (psfs["g1.6k7"], q7, (lambda p=B.device_psf(q7, be.device): be.blur_u8(d3, p, 0, 3, 1, out=out3)), out3, 3)
    print(f"rcot_blur_u8 on one {H} x {W} image, replicated border, {torch.cuda.get_device_name(0)}; roofline = bytes / {HBM / 1e12:.1f} TB/s")
    samples = {k: [] for k in cases}
    for r in range(WARMUP + ROUNDS):
        for k, c in cases.items():
            us = event_us(c[2])
            if r >= WARMUP:
                samples[k].append(us)
    print("[HIP events per call, us: median min max | non-zero taps | G multiply-adds/s | roofline us | median / roofline]   then "
          "scipy.ndimage.correlate on one host core [ms | max |device - host| | % of bytes that differ]")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for k, v in samples.items():
        h, q, fn, out, step = cases[k]
        hh, ww = (Hc, Wc) if step == 3 else (H, W)
        nb = 3 * hh * ww + 3 * (hh // step) * (ww // step)
        roof = nb / HBM * 1e6
        nz = int(np.count_nonzero(q))
        med = statistics.median(v)
        rate = nz * 3 * (hh // step) * (ww // step) / (med * 1e-6) / 1e9
        line = f"  {k:14s} {med:9.1f} {min(v):9.1f} {max(v):9.1f} | {nz:5d} | {rate:8.0f} | {roof:5.2f} | x{med / roof:.1f}"
        if ndimage is not None:
            src = img[:hh, :ww]
            t0 = time.perf_counter()
            host = np.stack([ndimage.correlate(src[..., c].astype(np.float64), h, mode="nearest") for c in range(3)], axis=-1)
            ms = (time.perf_counter() - t0) * 1e3
            host = np.floor(host + 0.5).astype(np.int64)
            if step == 3:
                host = host[1::3, 1::3]
            fn()
            diff = np.abs(out.cpu().numpy().astype(np.int64) - host)
            line += f"   host {ms:9.1f} ms | {int(diff.max())} | {100.0 * np.count_nonzero(diff) / diff.size:.4f}"
        else:
            line += "   host: scipy is not installed"
        print(line, flush=True)
    print("kernel time from the library's per-dispatch time stamps [symbol | launches | us per launch]")
    for k, c in cases.items():
        for sym, n, us in kernel_rows(be, c[2], ROUNDS):
            print(f"    {k:14s} {sym} | {n} | {us:.2f}")


if __name__ == "__main__":
    main()
