"""One validation of 68 synthetic 321 x 481 / 481 x 321 PNG pairs (the sizes of BSD68 / Rain100L), five ways, in one process on one GPU:

    (a) trainer.evaluate(..., pad="reflect"): every PNG decoded and uploaded again, one image per network call
    (b) the resident suite (rcot_amd/valsuite.py) at --val_batch 1
    (c) --val_batch 4      (d) --val_batch 8      (e) --val_batch 0 (a whole group of 34 images per call)

    python scripts/bench_valsuite.py [--out profiles/valsuite.txt] [--rounds 4]

(1) Wall time per validation (perf_counter around the call, the device synchronised before and after): ROUNDS blocks, each running
    (a) .. (e) once in that order after one untimed warm-up block, so that a drift of the clocks meets every configuration alike; per
    configuration the median, the minimum and the maximum over the blocks.  The verdict compares (c) .. (e) with (b): a batch size
    counts as faster only when its median lies below (b)'s by more than (b)'s own block-to-block spread (max - min).
(2) Network time per image at B = 1, 4, 8 and 34 on 328 x 488 planes: HIP events around the network call alone, median of 5.
(3) Kernel time of rcot_image_ingest_batch / rcot_image_egress_batch on a group of 34 against 34 single launches, from the library's
    per-dispatch time stamps (rcot_profile_begin / _end), the median of 5 sessions, the entries alternating.
Every configuration's mean psnr_float is printed: (b) .. (e) process the same 68 images as (a).
"""
import argparse
import ctypes
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcot_amd import params as P  # noqa: E402
from rcot_amd import trainer as TR  # noqa: E402
from rcot_amd import valsuite as V  # noqa: E402
from rcot_amd.net_restormer import T_net  # noqa: E402
from rcot_amd.ops import HipBackend  # noqa: E402

PAIRS = 68
BATCHES = (1, 4, 8, 0)


def write_folders(root):
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(1))
    os.makedirs(f"{root}/tar")
    os.makedirs(f"{root}/deg")
    for i in range(PAIRS):
        h, w = (321, 481) if i % 2 == 0 else (481, 321)
        t = np.clip(128 + 70 * np.sin(np.linspace(0, 5 + i % 7, h))[:, None, None] * np.cos(np.linspace(0, 4, w))[None, :, None]
                    + g.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(t).save(f"{root}/tar/{i:03d}.png")
        Image.fromarray(np.clip(t + g.normal(0, 25, t.shape), 0, 255).astype(np.uint8)).save(f"{root}/deg/{i:03d}.png")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_us(be, fn):
    """(total us, {symbol: (launches, us per launch)}) of one call of ``fn`` from the library's per-dispatch time stamps"""
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    fn()
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    rows = {}
    for ln in buf.value.decode(errors="replace").splitlines():
        parts = ln.rsplit("|", 2)
        if len(parts) == 3 and not parts[0].startswith("#"):
            rows[parts[0].strip()] = (int(parts[1]), float(parts[2]) * 1e3 / int(parts[1]))
    return sum(n * us for n, us in rows.values()), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valsuite.txt"))
    ap.add_argument("--rounds", type=int, default=4)
    opt = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix="valsuite_bench_")
    try:
        write_folders(root)
        be = HipBackend()
        net = T_net(decoder=True, backend=be)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()})
        tar_list, deg_list = sorted(os.listdir(f"{root}/tar")), sorted(os.listdir(f"{root}/deg"))
        tar_list, deg_list = [f"{root}/tar/{n}" for n in tar_list], [f"{root}/deg/{n}" for n in deg_list]
        specs = V.parse_val_sets([["bsd", "paired", f"{root}/tar/", f"{root}/deg/"]])
        say(f"one validation of {PAIRS} pairs, 321 x 481 and 481 x 321 alternating, reflect-padded to 328 x 488 / 488 x 328; T_net with seeded "
            f"parameters, fp32; {torch.cuda.get_device_name(0)}")
        suites = {}
        for b in BATCHES:
            dt, suites[b] = wall(lambda b=b: V.ValSuite(be, specs, net.size_multiple, "reflect", b, 8.0, verbose=False))
            say(f"set-up of the resident suite, --val_batch {b}: {dt * 1e3:.0f} ms (decode + upload of {2 * PAIRS} PNGs, once per run); "
                f"{suites[b].cache.bytes / 2 ** 20:.1f} MiB resident")
        configs = {"(a) evaluate(pad=reflect)": lambda: TR.evaluate(net, deg_list, tar_list, pad="reflect")}
        for tag, b in zip("bcde", BATCHES):
            configs[f"({tag}) suite --val_batch {b}"] = (lambda b=b: suites[b].run(net)["mean"]["psnr_float"])

        say(f"(1) wall time per validation [ms]: {opt.rounds} blocks of (a) .. (e) after one warm-up block; median, min, max; mean psnr_float")
        samples, figure = {k: [] for k in configs}, {}
        for r in range(opt.rounds + 1):
            for k, fn in configs.items():
                dt, figure[k] = wall(fn)
                if r:
                    samples[k].append(dt * 1e3)
        for k, v in samples.items():
            say(f"  {k:<28} {statistics.median(v):9.1f} {min(v):9.1f} {max(v):9.1f}   per image {statistics.median(v) / PAIRS:6.2f}   psnr_float {figure[k]:.4f}"
                f"   blocks: {' '.join(f'{x:.1f}' for x in v)}")
        keys = list(configs)
        base = samples[keys[1]]
        spread = max(base) - min(base)
        say(f"  block-to-block spread of (b): {spread:.1f} ms")
        for k in keys[2:]:
            gain = statistics.median(base) - statistics.median(samples[k])
            say(f"  {k}: {gain:+.1f} ms against (b) -> " + ("FASTER than (b) by more than its spread" if gain > spread else
                                                              "not faster than (b) by more than its spread"))
        say(f"  (b) against (a): {statistics.median(samples[keys[0]]) - statistics.median(base):+.1f} ms per validation "
            f"(the decode and the upload that residency removes)")

        say("(2) network time per image on 328 x 488 planes [ms]: HIP events around the network call alone, median of 5")
        images, groups = suites[0].sets["bsd"]
        members = groups[(328, 488)]
        for B in (1, 4, 8, len(members)):
            xb = be.image_ingest_batch([images[i].deg for i in members[:B]], 328, 488, "reflect")
            net(xb)
            v = [event_ms(lambda: net(xb)) for _ in range(5)]
            say(f"  B = {B:>2}: {statistics.median(v) / B:7.2f} per image ({statistics.median(v):8.1f} per call; min {min(v):.1f}, max {max(v):.1f})")
            del xb

        say(f"(3) kernel time on the group of {len(members)} 321 x 481 images [us], per-dispatch time stamps, median of 5 sessions, alternating")
        ims = [images[i] for i in members]
        sizes, tars, degs = [(im.h, im.w) for im in ims], [im.tar for im in ims], [im.deg for im in ims]
        xb = be.image_ingest_batch(degs, 328, 488, "reflect")
        out = net(xb[:2].contiguous())
        rest = out.repeat(len(ims) // 2, 1, 1, 1).contiguous()                 # something restored-like in every slot
        entries = {
            "ingest, one batched launch": lambda: be.image_ingest_batch(degs, 328, 488, "reflect", out=xb),
            f"ingest, {len(ims)} single launches": lambda: [be.image_ingest(d, 328, 488, "reflect", out=xb[i]) for i, d in enumerate(degs)],
            "egress + statistics, two batched launches": lambda: be.image_egress_batch(rest, sizes, tars, want_out=True, want_stats=True),
            f"egress + statistics, {2 * len(ims)} single launches": lambda: [be.image_egress(rest[i], h, w, target=tars[i], want_out=True, want_stats=True)
                                                                            for i, (h, w) in enumerate(sizes)],
        }
        sess = {k: [] for k in entries}
        for fn in entries.values():
            fn()
        for _ in range(5):
            for k, fn in entries.items():
                sess[k].append(kernel_us(be, fn))
        for k, v in sess.items():
            v.sort(key=lambda t: t[0])
            tot, rows = v[len(v) // 2]
            say(f"  {k}: {tot:.1f} us (sessions: min {v[0][0]:.1f}, max {v[-1][0]:.1f})")
            for sym, (n, us) in rows.items():
                say(f"      {sym} | {n} x {us:.2f}")
        b1, _, st1 = be.image_egress(rest[3], *sizes[3], target=tars[3], want_out=True, want_stats=True)
        bo, bst = be.image_egress_batch(rest, sizes, tars, want_out=True, want_stats=True)
        assert torch.equal(bo[3], b1) and torch.equal(bst[3].view(torch.int64), st1.view(torch.int64))
        say("  (slot 3 of the batched egress == the single launch, 8-bit image and the four doubles bit for bit)")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
