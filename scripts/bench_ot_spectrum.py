"""Time rcot_ot_spectrum alone over patch sizes: the radix-2 line transform at powers of two (the yardstick), the mixed-radix
Stockham transform at the sizes between them and Bluestein at 544 = 32 * 17: three instantiations of the same pass kernels.

    python scripts/bench_ot_spectrum.py [--calls 200] [--batch 16] > profiles/ot_spectrum_sizes.txt

B = 16, every de_id = 3 (all 48 planes take the spectral branch).  Per size: warm-up calls, then device events around `--calls`
back-to-back calls on one stream, ending in a synchronise; prints us per call and ns per pixel (B * 3 * P * P pixels per call),
the kernel family of the rows and of the columns pass, and the ratio to the nearest power of two below / above in the same run.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcot_amd import lib  # noqa: E402
from rcot_amd.ops import HipBackend  # noqa: E402

SIZES = [64, 96, 128, 160, 192, 224, 256, 320, 352, 384, 512, 544]


def family(n):
    rad = (ctypes.c_int * 10)()
    ns = lib.load().rcot_fft_plan(n, ctypes.cast(rad, ctypes.c_void_p), 10)
    if ns == 0:
        return f"bluestein M={rad[0]}"
    r = list(rad[:ns])
    return "radix-2" if set(r) == {2} else "mixed " + "x".join(str(v) for v in r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    assert args.calls >= 200, "at least 200 calls per size"
    be = HipBackend()
    B = args.batch
    de = torch.full((B,), 3, dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(1)
    rows = {}
    print(f"# rcot_ot_spectrum alone, B = {B}, de_id = 3, {args.calls} calls per size after {args.warmup} warm-up calls; {torch.cuda.get_device_name(0)}")
    print(f"# {'P':>4} {'us/call':>10} {'ns/pixel':>9}  line FFT")
    for P in SIZES:
        deg = (0.3 * torch.randn(B, 3, P, P, generator=g)).cuda()
        out = (0.3 * torch.randn(B, 3, P, P, generator=g)).cuda()
        gF, spec = be.empty(B, 3, P, P), be.empty(B)
        for _ in range(args.warmup):
            be.ot_spectrum(deg, out, de, gF, spec)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            be.ot_spectrum(deg, out, de, gF, spec)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.calls
        rows[P] = us * 1e3 / (B * 3 * P * P)
        print(f"  {P:>4} {us:>10.1f} {rows[P]:>9.3f}  {family(P)}")
    print("# ratio of ns/pixel to the neighbouring powers of two (same run)")
    for P in SIZES:
        if P & (P - 1):
            lo = 1 << (P.bit_length() - 1)
            hi = lo * 2
            print(f"  {P:>4}: x{rows[P] / rows[lo]:.2f} of {lo}" + (f", x{rows[P] / rows[hi]:.2f} of {hi}" if hi in rows else ""))


if __name__ == "__main__":
    main()
