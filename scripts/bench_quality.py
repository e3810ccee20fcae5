"""rcot_image_quality (csrc/quality.hip) on one 720 x 1280 pair for the four (window, space) protocols, next to rcot_image_egress with
statistics on the same image in the same call, and next to the host's numpy restatement.

    python scripts/bench_quality.py > profiles/quality_metrics.txt

Device time, two ways.  (1) HIP events around single calls: the median of 20 after 3 warm-ups, egress and the four protocols
alternating inside every round.  A call is two launches of a few microseconds each, so this figure holds the gap between them too.
(2) The library's own per-dispatch time stamps (rcot_profile_begin / _end) over 20 calls: kernel time alone, per symbol.  The script
exits non-zero, after printing everything, when a protocol's kernel time (2) is not below the egress kernel's.
Host time: quality.ssim_windowed on the same pair, best of 3.  Accuracy: the worst |device - host| SSIM over the shapes and inputs of
tests/test_quality_gpu.py and for the timed pair.
"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rcot_amd import quality as Q  # noqa: E402
from rcot_amd.ops import HipBackend  # noqa: E402

H, W = 720, 1280
PROTOCOLS = [(wn, sp) for wn in ("uniform7", "gauss11") for sp in ("rgb", "y")]
ROUNDS, WARMUP = 20, 3


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernel_rows(be, fn, calls):
    """[(symbol, launches, us per launch)] from the library's per-dispatch time stamps"""
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
    from test_quality_cpu import image_pairs
    from test_quality_gpu import SIZES
    be = HipBackend()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    g = np.random.Generator(np.random.PCG64(1))
    tar = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    out = np.clip(tar.astype(np.int64) + g.integers(-20, 21, size=tar.shape), 0, 255).astype(np.uint8)
    td, od = dev(tar), dev(out)
    restored = (od.permute(2, 0, 1).float() / 255).contiguous()
    print(f"rcot_image_quality on one {H} x {W} pair (random target, target + integer noise in +-20), {torch.cuda.get_device_name(0)}")

    calls = {"egress": lambda: be.image_egress(restored, H, W, target=td, want_out=True, want_stats=True)}
    for wn, sp in PROTOCOLS:
        calls[f"{wn} {sp}"] = (lambda wn=wn, sp=sp: be.image_quality(td, od, wn, sp))
    samples = {k: [] for k in calls}
    for r in range(WARMUP + ROUNDS):
        for k, fn in calls.items():
            us = event_us(fn)
            if r >= WARMUP:
                samples[k].append(us)
    print(f"(1) HIP events around one call (two launches), median of {ROUNDS} after {WARMUP} warm-ups, alternating in every round [us: median min max]")
    for k, v in samples.items():
        name = "rcot_image_egress, 8-bit output + statistics" if k == "egress" else f"rcot_image_quality {k}"
        print(f"  {name:<46} {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f}")

    print(f"(2) kernel time from the library's per-dispatch time stamps, {ROUNDS} calls each [symbol | launches | us per launch]")
    ktime = {}
    for k, fn in calls.items():
        rows = kernel_rows(be, fn, ROUNDS)
        ktime[k] = sum(us for _, _, us in rows)
        print(f"  {k}: {ktime[k]:.1f} us per call")
        for sym, n, us in rows:
            print(f"      {sym} | {n} | {us:.2f}")
    slow = [k for k in calls if k != "egress" and not ktime[k] < ktime["egress"]]
    for k in calls:
        if k != "egress":
            print(f"  {k}: x{ktime[k] / ktime['egress']:.2f} of rcot_image_egress's kernel time" + ("   <-- NOT below it" if k in slow else ""))

    print("(3) the host: quality.ssim_windowed (numpy fp64) on the same pair, best of 3 [s], and device against host")
    worst_pair = 0.0
    for wn, sp in PROTOCOLS:
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            want = Q.ssim_windowed(tar, out, wn, sp)
            best = min(best, time.perf_counter() - t0)
        st = be.image_quality(td, od, wn, sp).cpu().numpy()
        m = Q.quality_metrics(st)
        e, n = Q.sqerr_sums(tar, out, sp)
        assert st[0] == e and st[1] == n
        worst_pair = max(worst_pair, abs(m["ssim"] - want))
        print(f"  {wn:<8} {sp:<3} host {best:.3f} s   SSIM device {m['ssim']:.15f} host {want:.15f} |diff| {abs(m['ssim'] - want):.2e}   PSNR {m['psnr']:.6f} dB")

    print("(4) worst |device - host| SSIM over the shapes and inputs of tests/test_quality_gpu.py (bar there: 1e-10)")
    worst = {p: (0.0, None) for p in PROTOCOLS}
    for h, w in SIZES:
        for kind, a, b in image_pairs(h * 1000 + w, h, w, extreme=True):
            ad, bd = dev(a), dev(b)
            for wn, sp in PROTOCOLS:
                total, count = Q.ssim_sums(a, b, wn, sp)
                if not count:
                    continue
                st = be.image_quality(ad, bd, wn, sp).cpu().numpy()
                d = abs(st[2] / st[3] - total / count)
                if d >= worst[(wn, sp)][0]:
                    worst[(wn, sp)] = (d, f"{h} x {w} {kind}")
    for (wn, sp), (d, where) in worst.items():
        print(f"  {wn:<8} {sp:<3} {d:.3e}   ({where})")
    print(f"  over all: {max(d for d, _ in worst.values()):.3e}; the timed pair: {worst_pair:.3e}")
    if slow:
        raise SystemExit(f"rcot_image_quality is NOT below rcot_image_egress with statistics for: {', '.join(slow)}")


if __name__ == "__main__":
    main()
