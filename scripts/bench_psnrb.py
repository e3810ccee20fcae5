"""rcot_image_blockiness (csrc/quality.hip) on 1356 x 2040 pairs (a DIV2K-sized image) in rgb and in y, next to
rcot_image_quality(uniform7) on the same pairs and space in the same run, and next to the time its bytes take at the chip's measured
HBM rate.

    python scripts/bench_psnrb.py [--out profiles/psnrb.txt]

rcot_image_quality is the yardstick: it reads the same bytes and does strictly more arithmetic, so the new kernel must not be slower.
The script exits non-zero, after writing everything, when it is.

Device time, two ways.  (1) HIP events around single calls, the median of 20 after 3 warm-ups, the four calls alternating inside every
round: a call is two launches, so this figure holds the gap between them too.  (2) The library's own per-dispatch time stamps
(rcot_profile_begin / _end): kernel time alone, per symbol; 10 sessions of 4 calls per entry, the entries alternating, the median
session.  Every call takes the next of 20 pairs (332 MB in all, more than the 256 MiB Infinity Cache), so that the bytes come from HBM
as they do for a folder of images, not from a cache that the previous call warmed.
Bytes: the two images, 2 x 3 h w (the one-pixel halo of a tile is 5 % more requests, served by the caches).  HBM_RATE is the measured
float4-copy rate of the chip, 6.3 TB/s.  The integers of every timed pair are checked against the host once.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcot_amd import quality as Q  # noqa: E402
from rcot_amd.ops import HipBackend  # noqa: E402

H, W = 1356, 2040
PAIRS = 20
ROUNDS, WARMUP = 20, 3
SESSIONS, CALLS = 10, 4
HBM_RATE = 6.3e12


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernel_rows(be, fn, calls):
    """{symbol: us per launch} from the library's per-dispatch time stamps"""
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    rows = {}
    for ln in buf.value.decode(errors="replace").splitlines():
        parts = ln.rsplit("|", 2)
        if len(parts) == 3 and not parts[0].startswith("#"):
            rows[parts[0]] = float(parts[2]) * 1e3 / int(parts[1])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psnrb.txt"))
    out_path = ap.parse_args().out
    be = HipBackend()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(1)
    pairs = []
    for _ in range(PAIRS):                                                     # a random target and target + integer noise in +-20
        t = torch.randint(0, 256, (H, W, 3), device="cuda", generator=g, dtype=torch.int16)
        o = (t + torch.randint(-20, 21, (H, W, 3), device="cuda", generator=g, dtype=torch.int16)).clamp_(0, 255)
        pairs.append((t.to(torch.uint8), o.to(torch.uint8)))
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % PAIRS
        return pairs[turn[0]]

    say(f"rcot_image_blockiness and rcot_image_quality(uniform7) on {H} x {W} pairs, {torch.cuda.get_device_name(0)}")
    say(f"every call takes the next of {PAIRS} pairs ({PAIRS * 2 * 3 * H * W / 1e6:.0f} MB in all): the bytes come from HBM")
    tar, out = pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy()
    for sp in Q.SPACES:                                                        # the timed code computes the host's integers
        got = be.image_blockiness(pairs[0][1], pairs[0][0], sp, 2, 2).cpu().numpy()
        assert np.array_equal(got, Q.blockiness_stats(out, tar, sp, 2, 2)), sp
        say(f"  {sp:<3} PSNR-B {Q.psnrb_from_sums(got, H, W, 2, 2):.6f} dB (grid origin (2, 2)), PSNR {Q.psnr_u8(tar, out, sp):.6f} dB: device integers == host")

    calls = {}
    for sp in Q.SPACES:
        calls[f"blockiness {sp}"] = (lambda sp=sp: be.image_blockiness(*nxt()[::-1], sp))
        calls[f"quality uniform7 {sp}"] = (lambda sp=sp: be.image_quality(*nxt(), "uniform7", sp))
    samples = {k: [] for k in calls}
    for r in range(WARMUP + ROUNDS):
        for k, fn in calls.items():
            us = event_us(fn)
            if r >= WARMUP:
                samples[k].append(us)
    say(f"(1) HIP events around one call (two launches), median of {ROUNDS} after {WARMUP} warm-ups, alternating in every round [us: median min max]")
    for k, v in samples.items():
        say(f"  rcot_image_{k:<24} {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f}")

    say(f"(2) kernel time from the library's per-dispatch time stamps: {SESSIONS} sessions of {CALLS} calls per entry, the entries alternating; "
        f"the median session [us per call], then its symbols [us per launch]")
    sessions = {k: [] for k in calls}
    for _ in range(SESSIONS):
        for k, fn in calls.items():
            sessions[k].append(kernel_rows(be, fn, CALLS))
    ktime = {}
    for k, v in sessions.items():
        v.sort(key=lambda rows: sum(rows.values()))
        med = v[len(v) // 2]
        ktime[k] = sum(med.values())
        say(f"  {k}: {ktime[k]:.2f} us per call (sessions: min {sum(v[0].values()):.2f}, max {sum(v[-1].values()):.2f})")
        for sym, us in med.items():
            say(f"      {sym} | {us:.2f}")
    say("(3) the comparison")
    floor_us = 2 * 3 * H * W / HBM_RATE * 1e6
    slow = []
    for sp in Q.SPACES:
        b, q = ktime[f"blockiness {sp}"], ktime[f"quality uniform7 {sp}"]
        if not b <= q:
            slow.append(sp)
        say(f"  {sp:<3} rcot_image_blockiness {b:.2f} us = x{b / q:.2f} of rcot_image_quality(uniform7)'s {q:.2f} us"
            + ("   <-- SLOWER than the yardstick" if sp in slow else "") +
            f";  its {2 * 3 * H * W / 1e6:.1f} MB take {floor_us:.2f} us at {HBM_RATE / 1e12:.1f} TB/s: x{b / floor_us:.1f} of that")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    if slow:
        raise SystemExit(f"rcot_image_blockiness is SLOWER than rcot_image_quality(uniform7) in: {', '.join(slow)}")


if __name__ == "__main__":
    main()
