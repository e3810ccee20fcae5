"""The call trace of ``FolderLoader`` with every task family in one ``--de_type`` list, on a backend that launches nothing
(tests/golden/loader_trace.json, scripts/make_loader_trace_fixture.py, tests/test_datacache_cpu.py).

``tree(root)`` writes three lossless PNGs of 48 x 64, 50 x 70 and 66 x 81 (PCG64 seeds), their paired twins and the list files.
``record(root)`` drives the loader at P = 32 and batch 4 for two epochs — uncached, cached with a generous budget and cached with a
budget that leaves some images transient; world 1, and world 2 with both ranks — and returns the log as JSON-ready lists:

  per call of one of the five whole-image entry points (replaced on their modules by a cheap deterministic function of the input and
  the arguments): the name, every scalar argument, the shape and CRC32 of the image passed in;
  per ``patch_prep`` / row of ``patch_prep_batch``: the scalars, the shapes and CRC32s of both images;
  per batch the names and labels; per epoch the cache's keys in insertion order, ``hits``, ``misses``, ``bytes`` and the four counters.

``digest(log)`` is what the fixture holds: per run its route, world and rank, per batch the first 16 hex digits of a SHA-256 that
runs over every entry of the log up to and including that batch (the sample ids, the calls, the rows, names and labels, the cache's key
lists), and per epoch of a cached run the cache's seven numbers.  The first batch whose digits differ is where two traces part.

No codec and no kernel enters: the log is a function of the loader's host code alone."""
import hashlib
import json
import os
import zlib
from argparse import Namespace

import numpy as np
import torch

P, BATCH, EPOCHS, SEED = 32, 4, 2, 13
SIZES = {"a": (48, 64), "b": (50, 70), "c": (66, 81)}
DE_TYPE = ["denoise_25", "single", "sr_x2", "sr_x3", "sr_bd_x3", "jpeg_q10", "blur_g1.6", "blur_m15", "chain_sr_x3+blur_g1.6",
           "chain_blur_m15+noise_g5-20+jpeg_q20-40"]
BUDGETS = {"generous": 1 << 30, "small": 100_000}                           # of 33 images, 9216 .. 15360 bytes each


def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(path)


def tree(root: str) -> Namespace:
    for i, (n, (h, w)) in enumerate(SIZES.items()):
        _png(f"{root}/clean/{n}.png", h, w, 90 + i)
        _png(f"{root}/single/target/{n}.png", h, w, 90 + i)
        _png(f"{root}/single/degraded/{n}.png", h, w, 190 + i)
    os.makedirs(f"{root}/lists/noisy")
    open(f"{root}/lists/noisy/denoise.txt", "w").write("".join(f"{n}.png\n" for n in SIZES))
    clean = f"{root}/clean/"
    return Namespace(de_type=list(DE_TYPE), data_file_dir=f"{root}/lists/", denoise_dir=clean, single_dir=f"{root}/single", sr_dir=clean,
                     jpeg_dir=clean, blur_dir=clean, chain_dir=clean, blur_border="mirror", jpeg_subsampling="444", patch_size=P)


def _plain(v, root):
    """a value of the log as JSON holds it: tuples as lists, paths relative to the tree"""
    if isinstance(v, (tuple, list)):
        return [_plain(x, root) for x in v]
    if isinstance(v, str):
        return v.replace(root, "")
    if isinstance(v, (np.ndarray, np.generic)):
        return _plain(v.tolist(), root)
    return v


def _img(t):
    return None if t is None else [list(t.shape), zlib.crc32(t.contiguous().numpy().tobytes())]


class Recorder:
    """a backend that launches nothing and keeps what it was called with"""
    device = torch.device("cpu")
    _plan = None

    def __init__(self, log, root):
        self.log, self.root = log, root

    def _row(self, clean_img, deg_img, y0, x0, mode, sigma, seed):
        return [_img(clean_img), _img(deg_img), y0, x0, mode, sigma, seed]

    def patch_prep(self, clean_img, deg_img, y0, x0, P, mode, sigma, seed, deg_out, clean_out):
        self.log.append(["patch_prep", P, self._row(clean_img, deg_img, y0, x0, mode, sigma, seed)])
        deg_out.zero_()
        clean_out.zero_()

    def patch_prep_batch(self, rows, P, deg_out, clean_out):
        self.log.append(["patch_prep_batch", P, [self._row(*r) for r in rows]])
        deg_out.zero_()
        clean_out.zero_()


def _entry_points(log, root):
    """(module, name, double) of the five entry points: each double logs its call and returns the input XOR a byte of its arguments"""
    from rcot_amd import blur, chain, jpeg, resize

    def double(name):
        def fn(img, *args):
            *scalars, be = args
            assert isinstance(be, Recorder)
            plain = _plain(scalars, root)
            log.append([name, plain, _img(img)])
            return img ^ (zlib.crc32(repr((name, plain)).encode()) & 0xFF)
        return fn
    return [(m, n, double(n)) for m, n in ((resize, "sr_degrade_u8"), (jpeg, "jpeg_degrade_u8"), (blur, "blur_degrade_u8"),
                                           (blur, "bd_degrade_u8"), (chain, "chain_degrade_u8"))]


def record(root: str) -> list:
    """the whole log (module docstring); ``root``: an empty folder the tree is written to"""
    from rcot_amd import data as D
    from rcot_amd.imagecache import DeviceImageCache
    root = str(root)
    args = tree(root)
    log = []
    doubles = _entry_points(log, root)
    real = [getattr(m, n) for m, n, _ in doubles]
    for m, n, fn in doubles:
        setattr(m, n, fn)
    try:
        for world, rank in ((1, 0), (2, 0), (2, 1)):
            for route in ("uncached", *BUDGETS):
                be = Recorder(log, root)
                cache = None if route == "uncached" else DeviceImageCache(be, BUDGETS[route])
                loader = D.FolderLoader(args, BATCH // world, seed=SEED, rank=rank, world=world, backend=be, threads=2, cache=cache)
                if len(log) == 0:
                    log.append(["ids", _plain([list(s.items()) for s in loader.ids], root)])
                log.append(["run", route, world, rank, len(loader.ids)])
                for epoch in range(EPOCHS):
                    for [names, labels], deg, clean in loader:
                        log.append(["batch", names, labels.tolist(), list(deg.shape), list(clean.shape)])
                    if cache is not None:
                        log.append(["cache", _plain(cache.keys(), root), cache.hits, cache.misses, cache.bytes, cache.sr_degradations,
                                    cache.jpeg_degradations, cache.blur_degradations, cache.chain_degradations])
    finally:
        for (m, n, _), fn in zip(doubles, real):
            setattr(m, n, fn)
    return log


def digest(log: list) -> list:
    """the log as the fixture holds it (module docstring): [{"run": [route, world, rank, samples], "batches": [...], "cache": [...]}, ...]"""
    h, runs = hashlib.sha256(), []
    for e in log:
        h.update(json.dumps(e, separators=(",", ":")).encode())
        if e[0] == "run":
            runs.append({"run": e[1:], "batches": [], "cache": []})
        elif e[0] == "batch":
            runs[-1]["batches"].append(h.copy().hexdigest()[:16])
        elif e[0] == "cache":
            runs[-1]["cache"].append(e[2:])
    return runs
