"""rcot_resize_axis (csrc/resize.hip) on one 1356 x 2040 x 3 image (DIV2K's usual size): the four passes of the super-resolution
degradation (rows then columns down by s, rows then columns up by s) and the whole 8-bit chain ``sr_degrade_u8`` for s = 2, 3, 4,
each against the time its bytes take at the achievable HBM rate.

    python scripts/bench_resize.py > profiles/resize_passes.txt

Bytes of a pass: 4 planes (n_in + n_out) other-axis-length — the source read once, the result written once; the tap tables
(out_len x K x 8 bytes) stay in cache.  The chain adds two ingests (3 B in, 12 B out per pixel) and two quantisations (12 B in, 3 B
out).  Roofline time = bytes / 6.3 TB/s (the achievable rate of DESIGN.md section 6).

Device time: HIP events around single calls, the median, minimum and maximum of 30 after 5 warm-ups, the passes alternating inside
every round; and the library's own per-dispatch time stamps (rcot_profile_begin / _end) over 30 calls: kernel time alone, per symbol.
The image is 33 MB, so every pass runs from the Infinity Cache once warm: the figures are cache-resident rates, as they are inside the
loader, where the upload has just written the image.
"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcot_amd import resize as RZ  # noqa: E402
from rcot_amd.ops import HipBackend  # noqa: E402

H, W, PLANES = 1356, 2040, 3
ROUNDS, WARMUP = 30, 5
HBM = 6.3e12


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernel_rows(be, fn, calls):
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    rows = []
    for ln in buf.value.decode(errors="replace").splitlines():
        parts = ln.rsplit("|", 2)
        if len(parts) == 3 and not parts[0].startswith("#"):
            rows.append((parts[0], int(parts[1]), float(parts[2]) * 1e3 / int(parts[1])))
    return rows


def main():
    be = HipBackend()
    g = np.random.Generator(np.random.PCG64(1))
    u8 = torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).cuda()
    print(f"rcot_resize_axis on one {H} x {W} x {PLANES} image, {torch.cuda.get_device_name(0)}; roofline = bytes / {HBM / 1e12:.1f} TB/s")
    for s in (2, 3, 4):
        Hc, Wc = H - H % s, W - W % s
        img = u8[:Hc, :Wc].contiguous()
        x = be.image_ingest(img, Hc, Wc, "none").view(3, Hc, Wc)
        h, w = Hc // s, Wc // s
        passes, cur = [], x
        for name, axis, n_in, n_out in (("rows down", 0, Hc, h), ("cols down", 1, Wc, w), ("rows up", 0, h, Hc), ("cols up", 1, w, Wc)):
            idx, taps = RZ.device_taps(n_in, n_out, be.device)
            other = cur.shape[2] if axis == 0 else cur.shape[1]
            out = be.resize_axis(cur, axis, idx, taps)
            passes.append((name, cur, axis, idx, taps, out, 4 * PLANES * (n_in + n_out) * other, idx.shape[1]))
            cur = out
        calls = {p[0]: (lambda p=p: be.resize_axis(p[1], p[2], p[3], p[4], out=p[5])) for p in passes}
        calls["sr_degrade_u8"] = lambda: RZ.sr_degrade_u8(img, s, be)
        nbytes = {p[0]: p[6] for p in passes}
        nbytes["sr_degrade_u8"] = sum(nbytes.values()) + 15 * (Hc * Wc + h * w) * 2
        samples = {k: [] for k in calls}
        for r in range(WARMUP + ROUNDS):
            for k, fn in calls.items():
                us = event_us(fn)
                if r >= WARMUP:
                    samples[k].append(us)
        print(f"x{s}: {Hc} x {Wc} <-> {h} x {w}   [HIP events per call, us: median min max | MB | roofline us | median / roofline]")
        for k, v in samples.items():
            roof = nbytes[k] / HBM * 1e6
            K = next((p[7] for p in passes if p[0] == k), None)
            tag = f"{k} (K = {K})" if K else f"{k} (8 launches)"
            print(f"  {tag:<26} {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f} | {nbytes[k] / 1e6:7.1f} | {roof:6.1f} | x{statistics.median(v) / roof:.1f}")
        print("  kernel time from the library's per-dispatch time stamps [symbol | launches | us per launch]")
        for k, fn in calls.items():
            rows = kernel_rows(be, fn, ROUNDS)
            print(f"    {k}: {sum(us * n for _, n, us in rows) / ROUNDS:.1f} us per call")
            for sym, n, us in rows:
                print(f"        {sym} | {n} | {us:.2f}")


if __name__ == "__main__":
    main()
