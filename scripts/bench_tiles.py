"""Tiled and x8 self-ensemble inference (rcot_amd/tiles.py, csrc/views.hip) on one 1024 x 1024 x 3 image, tile 256, overlap 32.

    python scripts/bench_tiles.py [--parent TREE] [--rounds 2] > profiles/tiled_inference.txt

(1) The two kernels alone: rcot_view_gather and rcot_view_blend for modes {0}, for the four shape-keeping maps, for the four transposing
    maps (2, 3, 6, 7: through the LDS tile) and for all 8.  Kernel time from the library's per-dispatch time stamps (rcot_profile_begin /
    _end) over 20 calls after 3 warm-ups; bytes from the shapes (gather: every view read once from the image and written once; blend:
    every view read once, the image written once, the taps not counted); GB/s = bytes / kernel time, next to the 6.3 TB/s a float4 copy
    reaches on this device.
(2) End to end, both networks with seeded weights, milliseconds per image (host clock around the calls, ending in a synchronise; one
    warm-up, then the mean of REPS): ``tester.restore(net, x, 256, 32, mult)`` as it stands, ``restore_views`` at tile_batch 1 and 0 (the
    25 tiles in one call), and with the 8-view ensemble (200 views) at tile_batch 1 and 25.  Every (tree, network) runs in a process of
    its own; with ``--parent TREE`` (a built checkout of the parent commit) the parent's ``restore`` runs in alternation with this
    tree's, round by round, on the same device.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 1024
TILE, OVERLAP = 256, 32
COPY_TBS = 6.3


def kernel_us(be, fn, calls=20, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    us = 0.0
    for ln in buf.value.decode(errors="replace").splitlines():
        parts = ln.rsplit("|", 2)
        if len(parts) == 3 and not parts[0].startswith("#"):
            us += float(parts[2]) * 1e3 / calls
    return us


def kernels():
    import torch
    from rcot_amd import tiles as TL
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    p = TL.plan(H, W, TILE, OVERLAP, 8, 1)
    x = torch.rand(3, H, W, device="cuda")
    wy, wx = (torch.from_numpy(TL.window_taps(T, OVERLAP, "linear")).cuda() for T in (p.Th, p.Tw))
    print(f"(1) kernels: {H} x {W} x 3 fp32, tile {TILE}, overlap {OVERLAP}: {len(p.ys)} x {len(p.xs)} windows of {p.Th} x {p.Tw}; "
          f"{torch.cuda.get_device_name(0)}; a float4 copy reaches {COPY_TBS} TB/s")
    print("    modes                  views   kernel          us      MB    GB/s   of copy")
    for label, modes in (("{0}", (0,)), ("{0,1,4,5} plain", (0, 1, 4, 5)), ("{2,3,6,7} transposing", (2, 3, 6, 7)), ("all 8", TL.ENSEMBLE_MODES[8])):
        n = len(modes) * len(p.ys) * len(p.xs)
        vbytes = n * 3 * p.Th * p.Tw * 4
        views = be.view_gather(x, p.ys, p.xs, modes, p.Th, p.Tw)
        out = be.empty(3, H, W)
        rows = (("gather", 2 * vbytes, lambda: be.view_gather(x, p.ys, p.xs, modes, p.Th, p.Tw, out=views)),
                ("blend", vbytes + 3 * H * W * 4, lambda: be.view_blend(views, H, W, p.ys, p.xs, modes, p.Th, p.Tw, out=out)),
                ("blend linear", vbytes + 3 * H * W * 4, lambda: be.view_blend(views, H, W, p.ys, p.xs, modes, p.Th, p.Tw, wy, wx, out=out)))
        for kname, nbytes, fn in rows:
            us = kernel_us(be, fn)
            gbs = nbytes / us / 1e3
            print(f"    {label:<22} {n:5d}   {kname:<13} {us:7.1f} {nbytes / 1e6:7.1f} {gbs:7.0f}   {gbs / (COPY_TBS * 1e3):6.1%}")


def worker(tree, which, reps):
    """one (tree, network): ms per image of every configuration the tree has -> one JSON line"""
    sys.path.insert(0, tree)
    import torch
    from rcot_amd import tester as TS
    from rcot_amd.ops import default_backend
    be = default_backend()
    if which == "restormer":
        from rcot_amd.net_restormer import T_net
        net, mult = T_net(decoder=True, seed=1), 8
    else:
        from rcot_amd.mprnet_hip import MPRNetHip
        net, mult = MPRNetHip(backend=be, seed=1), 4
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    configs = {"restore --tile 256 (as it stands)": lambda: TS.restore(net, x, TILE, OVERLAP, mult)}
    try:
        from rcot_amd import tiles as TL
    except ImportError:
        TL = None
    if TL is not None:
        p1, p8 = TL.plan(H, W, TILE, OVERLAP, mult, 1), TL.plan(H, W, TILE, OVERLAP, mult, 8)
        configs["views linear, tile_batch 1"] = lambda: TL.restore_views(net, x, p1, "linear", 1)
        configs["views linear, tile_batch 0 (25)"] = lambda: TL.restore_views(net, x, p1, "linear", 0)
        configs["ensemble 8 linear, tile_batch 1"] = lambda: TL.restore_views(net, x, p8, "linear", 1)
        configs["ensemble 8 linear, tile_batch 25"] = lambda: TL.restore_views(net, x, p8, "linear", 25)
    res, ref = {}, None
    for name, fn in configs.items():
        y = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t0) / reps * 1e3, 2)
        if ref is None:
            ref = y
        elif "ensemble" not in name:
            res[name + " | max abs diff to restore"] = float((y - ref).abs().max())
        del y
    print(json.dumps({"tree": tree, "net": which, "ms": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, to alternate with")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    opt = ap.parse_args()
    if opt.worker:
        return worker(opt.worker[0], opt.worker[1], opt.reps)
    sys.path.insert(0, ROOT)
    kernels()
    print(f"(2) end to end, ms per {H} x {W} image (mean of {opt.reps} after one warm-up), one process per line, in the order run")
    trees = ([os.path.abspath(opt.parent)] if opt.parent else []) + [ROOT]
    for which in ("mprnet", "restormer"):
        for r in range(opt.rounds):
            for tree in trees:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, which, "--reps", str(opt.reps)],
                                     capture_output=True, text=True, timeout=900)
                if out.returncode:
                    sys.stdout.write(out.stdout[-2000:] + out.stderr[-4000:])
                    raise SystemExit(f"worker {tree} {which} ended with {out.returncode}: nothing further is started")
                line = json.loads(out.stdout.strip().splitlines()[-1])
                tag = "parent" if tree != ROOT else "this tree"
                print(f"  round {r + 1} {which:<9} {tag}")
                for k, v in line["ms"].items():
                    print(f"      {k:<62} {v}")
                sys.stdout.flush()


if __name__ == "__main__":
    main()
