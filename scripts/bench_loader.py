"""The training-data loader ALONE (rcot_amd/data.py::FolderLoader) on real folders, uncached against the device-resident
training set (rcot_amd/imagecache.py), and rcot_patch_prep_batch against B rcot_patch_prep launches.

    python scripts/bench_loader.py > profiles/loader_cache.txt

Folders are written into a temporary directory from a seed: smooth content plus mild noise, as tests/synth_folders.py::dataset_tree
makes it (PNGs of pure noise neither compress nor decode like photographs; these compress better than photographs do, so the decode
times below are a LOWER bound of a real set's).
    derain   200 pairs of 321 x 481               (x360 in the sample list, as Rain100L)
    denoise   64 images of 321 x 481               (denoise_15 / _25 / _50, x5 each)
    sr_x4     16 images of 1356 x 2040             (x5; the whole HR image is degraded on the device)

Per folder, B = 8, P = 128, --threads 4 and 16, three routes:
    uncached      cache=None: every sample decodes its file(s), uploads them and launches rcot_patch_prep (sr: after sr_degrade_u8)
    cached cold   a fresh cache, the FIRST epoch (at most --batches batches of it): every file is met for the first time
    cached warm   the batches that follow on the same cache
A window is a run of consecutive batches (epochs follow each other) timed with a host clock that stops after a device synchronise;
nothing consumes the batches.  Windows have --batches batches, with two exceptions: the uncached and cold sr_x4 windows have
--sr_batches (the route is too slow for more on a shared GPU), and the warm cached windows have --warm_batches (a few hundred of
them last a few hundredths of a second, which measures the clock).  A cold window ends with the first epoch where that is shorter.
The routes alternate in one process and the whole table is made twice.
The two consumption rates are the README's: 105.8 patches/s (Restormer fp32 step) and 221 patches/s (MPRNet step).

There is no fallback: without a GPU the script fails.
"""
import argparse
import contextlib
import ctypes
import io
import itertools
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

B, P = 8, 128
RATES = (105.8, 221.0)


def write_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def make_folders(root, seed, n_pairs, n_den, n_hr):
    g = np.random.Generator(np.random.PCG64(seed))

    def smooth(h, w):
        ph = g.uniform(0, 6.28, 2)
        base = 128 + 60 * np.sin(np.linspace(0, 6, h) + ph[0])[:, None, None] * np.cos(np.linspace(0, 5, w) + ph[1])[None, :, None]
        return np.clip(base + g.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    for d_ in ("noisy", "rainy"):
        os.makedirs(f"{root}/lists/{d_}")
    for i in range(n_pairs):
        t = smooth(321, 481)
        write_png(f"{root}/Derain/gt/norain-{i}.png", t)
        write_png(f"{root}/Derain/rainy/rain-{i}.png", np.clip(t + g.normal(0, 8, t.shape), 0, 255).astype(np.uint8))
    open(f"{root}/lists/rainy/rainTrain.txt", "w").write("".join(f"rainy/rain-{i}.png\n" for i in range(n_pairs)))
    for i in range(n_den):
        write_png(f"{root}/Denoise/d{i}.png", smooth(321, 481))
    open(f"{root}/lists/noisy/denoise.txt", "w").write("".join(f"d{i}.png\n" for i in range(n_den)))
    for i in range(n_hr):
        write_png(f"{root}/HR/hr{i}.png", smooth(1356, 2040))
    common = dict(data_file_dir=f"{root}/lists/", denoise_dir=f"{root}/Denoise/", derain_dir=f"{root}/Derain/", sr_dir=f"{root}/HR/",
                  patch_size=P)
    return {"derain": Namespace(de_type=["derain"], **common),
            "denoise": Namespace(de_type=["denoise_15", "denoise_25", "denoise_50"], **common),
            "sr_x4": Namespace(de_type=["sr_x4"], **common)}


def stream(loader):
    """consecutive epochs of a loader as one stream of batches"""
    while True:
        yield from loader


def window(batches, n):
    """n batches of an iterator -> (batches taken, seconds), the clock stopped after a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k = 0
    for _ in itertools.islice(batches, n):
        k += 1
    torch.cuda.synchronize()
    return k, time.perf_counter() - t0


def loader_table(tasks, be, opt):
    from rcot_amd.data import FolderLoader
    from rcot_amd.imagecache import DeviceImageCache

    def make(args, threads, cache=None):
        with contextlib.redirect_stdout(io.StringIO()):                     # (the loader's "...total sample ids" line)
            return FolderLoader(args, B, seed=3, backend=be, threads=threads, cache=cache)
    rows = []
    for rep in range(opt.repeats):
        for task, args in tasks.items():
            slow = opt.sr_batches if task.startswith("sr") else opt.batches
            for threads in (4, 16):
                plain = stream(make(args, threads))
                window(plain, opt.warmup)
                k, dt = window(plain, slow)
                rows.append((rep, task, threads, "uncached", k, dt, ""))
                plain.close()
                cache = DeviceImageCache(be, int(opt.cache_gb * 2 ** 30))
                loader = make(args, threads, cache)
                cached = stream(loader)
                k, dt = window(cached, min(slow, len(loader)))
                rows.append((rep, task, threads, "cached cold", k, dt, f"{cache.misses} misses, {cache.bytes / 2 ** 20:.0f} MiB"))
                k, dt = window(cached, opt.warm_batches)
                rows.append((rep, task, threads, "cached warm", k, dt, cache.report().split(", ", 1)[1]))
                cached.close()
                del cache, loader
    print(f"\nloader alone, B = {B}, P = {P}: patches/s  [repeat | task | threads | route | batches | seconds | patches/s | "
          f"x {RATES[0]} | x {RATES[1]} | cache]")
    for rep, task, threads, route, k, dt, note in rows:
        pps = k * B / dt
        print(f"  {rep} | {task:<7} | {threads:>2} | {route:<11} | {k:>4} | {dt:7.3f} | {pps:9.1f} | {pps / RATES[0]:6.2f} | "
              f"{pps / RATES[1]:6.2f} | {note}")
    print("\nsummary (both repeats, min .. max patches/s)")
    for task in tasks:
        for threads in (4, 16):
            cells = []
            for route in ("uncached", "cached cold", "cached warm"):
                v = [k * B / dt for rep, t, th, r, k, dt, _ in rows if (t, th, r) == (task, threads, route)]
                cells.append(f"{route} {min(v):.1f} .. {max(v):.1f}")
            print(f"  {task:<7} threads {threads:>2}: " + " | ".join(cells))
    print("\nDoes the loader alone deliver what the training step consumes?  (slowest window of the repeats; the loader has the host "
          "thread and the GPU to itself here, inside training it shares both with the step)")
    for task in tasks:
        for threads in (4, 16):
            slowest = lambda route: min(k * B / dt for rep, t, th, r, k, dt, _ in rows if (t, th, r) == (task, threads, route))
            u, w = slowest("uncached"), slowest("cached warm")
            verdict = " and ".join(f"{'keeps up with' if u > rate else 'does NOT keep up with'} the {name} step ({u / rate:.2f} x {rate})"
                                   for name, rate in zip(("Restormer fp32", "MPRNet"), RATES))
            print(f"  {task:<7} threads {threads:>2}: uncached {u:.1f} patches/s {verdict}; cached warm {w:.1f} patches/s is "
                  f"{'faster' if w > u else 'NOT faster'} than uncached ({w / u:.1f} x)")
    return rows


def kernel_us(be, fn, calls):
    """kernel time alone from the library's per-dispatch time stamps -> us per call of fn"""
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    total = 0.0
    for ln in buf.value.decode(errors="replace").splitlines():
        parts = ln.rsplit("|", 2)
        if len(parts) == 3 and not parts[0].startswith("#"):
            total += float(parts[2]) * 1e3
    return total / calls


def span_us(fn, calls):
    """device events around ``calls`` calls -> us per call: what the stream is busy (or waiting for the host) per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def kernel_table(be):
    g = np.random.Generator(np.random.PCG64(2))
    imgs = [torch.from_numpy(g.integers(0, 256, size=(320, 480, 3), dtype=np.uint8)).to(be.device) for _ in range(2 * B)]
    deg, clean = be.empty(B, 3, P, P), be.empty(B, 3, P, P)
    print(f"\nrcot_patch_prep_batch (one launch, the table upload included) against {B} rcot_patch_prep launches, B = {B}, P = {P}, on "
          f"{2 * B} resident 320 x 480 images  [us per batch: median min max of 20 rounds of 50 calls]")
    for kind in ("paired", "noise"):
        for mode in (0, 5, 2):
            rows = [(imgs[2 * b], imgs[2 * b + 1] if kind == "paired" else None, 17 * b, 31 * b, mode, 0.0 if kind == "paired" else 25.0,
                     100 + b) for b in range(B)]

            def one():
                be.patch_prep_batch(rows, P, deg, clean)

            def eight():
                for b, (c, d, y0, x0, m, s, seed) in enumerate(rows):
                    be.patch_prep(c, d, y0, x0, P, m, s, seed, deg[b], clean[b])
            one(); eight()
            spans = {"batch": [], "8 launches": []}
            for _ in range(20):
                spans["batch"].append(span_us(one, 50))
                spans["8 launches"].append(span_us(eight, 50))
            kern = {"batch": kernel_us(be, one, 50), "8 launches": kernel_us(be, eight, 50)}
            for name, v in spans.items():
                print(f"  {kind:<6} mode {mode} | {name:<10} | device-event span {statistics.median(v):7.1f} {min(v):7.1f} {max(v):7.1f} | "
                      f"kernel time alone {kern[name]:6.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--sr_batches", type=int, default=100, help="batches of the uncached and cold sr_x4 windows")
    ap.add_argument("--warm_batches", type=int, default=3000, help="batches of the warm cached windows (300 would last 30 ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cache_gb", type=float, default=16.0)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--den", type=int, default=64)
    ap.add_argument("--hr", type=int, default=16)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: scripts/bench_loader.py measures the HIP path only")
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    print(f"{torch.cuda.get_device_name(0)}; content: smooth plus mild noise (decodes faster than photographs; pure noise would not "
          f"decode like photographs either)")
    kernel_table(be)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        tasks = make_folders(root, 1, opt.pairs, opt.den, opt.hr)
        print(f"\nfolders written in {time.perf_counter() - t0:.1f} s: {opt.pairs} rain pairs and {opt.den} denoise images of 321 x 481, "
              f"{opt.hr} HR images of 1356 x 2040")
        loader_table(tasks, be, opt)


if __name__ == "__main__":
    main()
