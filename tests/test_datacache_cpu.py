"""CPU tier: the device-resident training set (rcot_amd/imagecache.py) behind ``FolderLoader(..., cache=...)`` on the miniature tree
of tests/test_data_cpu.py — the cached loader's batches equal the uncached loader's bit for bit over two epochs and across ranks,
every file is decoded once, the budget rule, the host check of ``patch_prep_batch``'s rows, and the loader's call trace over every
task family against the trace recorded before the whole-image tasks moved into one table (tests/loader_trace.py).  Kernel layer: a subclass of the
numpy test double whose ``patch_prep_batch`` loops over its ``patch_prep``."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from host_double import TorchDouble
from rcot_amd import data as D
from rcot_amd.imagecache import DeviceImageCache
from rcot_amd.ops import check_patch_rows

P = 32


class BatchDouble(TorchDouble):
    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.batch_calls = 0

    def patch_prep_batch(self, rows, P, deg_out, clean_out):
        check_patch_rows(rows, P, deg_out, clean_out)
        self.batch_calls += 1
        for b, (clean_img, deg_img, y0, x0, mode, sigma, seed) in enumerate(rows):
            self.patch_prep(clean_img, deg_img, y0, x0, P, mode, sigma, seed, deg_out[b], clean_out[b])


def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(a).save(path)
    return a


@pytest.fixture()
def tree(tmp_path):
    """the miniature tree of tests/test_data_cpu.py: 3 listed denoise images (and one that is not), 2 rain pairs, 1 haze pair"""
    r = str(tmp_path)
    den = [f"img{i}.png" for i in range(3)]
    for i, n in enumerate(den):
        _png(f"{r}/Denoise/{n}", 70 + i, 90 + 2 * i, 10 + i)
    _png(f"{r}/Denoise/not_listed.png", 64, 64, 99)
    os.makedirs(f"{r}/lists/noisy"); os.makedirs(f"{r}/lists/rainy"); os.makedirs(f"{r}/lists/hazy")
    open(f"{r}/lists/noisy/denoise.txt", "w").write("\n".join(den) + "\n")
    open(f"{r}/lists/rainy/rainTrain.txt", "w").write("rainy/rain-1.png\nrainy/rain-2.png\n")
    for i in (1, 2):
        _png(f"{r}/Derain/rainy/rain-{i}.png", 80, 96, 20 + i)
        _png(f"{r}/Derain/gt/norain-{i}.png", 80, 96, 30 + i)
    open(f"{r}/lists/hazy/hazy_outside.txt", "w").write("synthetic/part1/0025_0.8_0.04.png\n")
    _png(f"{r}/Dehaze/synthetic/part1/0025_0.8_0.04.png", 72, 72, 41)
    _png(f"{r}/Dehaze/original/0025.png", 72, 72, 42)
    return Namespace(de_type=["denoise_15", "denoise_50", "derain", "dehaze"], data_file_dir=f"{r}/lists/", denoise_dir=f"{r}/Denoise/",
                     derain_dir=f"{r}/Derain/", dehaze_dir=f"{r}/Dehaze/", patch_size=P)


def _small(args):
    """the same tree with the denoise and haze tasks only (31 samples instead of 751): the per-test work stays small"""
    return Namespace(**{**vars(args), "de_type": ["denoise_15", "denoise_50", "dehaze"]})


def _epochs(loader, n_epochs):
    return [batch for _ in range(n_epochs) for batch in loader]


def _assert_same(got, want):
    assert len(got) == len(want) and len(got) > 0
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
        assert not torch.isnan(d1).any() and not torch.isnan(c1).any()


@pytest.mark.parametrize("world,rank,batch", [(1, 0, 4), (2, 0, 2), (2, 1, 2)])
def test_cached_batches_equal_uncached_over_two_epochs(tree, world, rank, batch):
    """all four tasks (751 samples), two consecutive epochs, every batch"""
    be = BatchDouble()
    cache = DeviceImageCache(be, 1 << 30)
    cached = D.FolderLoader(tree, batch, seed=7, rank=rank, world=world, backend=be, cache=cache)
    plain = D.FolderLoader(tree, batch, seed=7, rank=rank, world=world, backend=be)
    got, want = _epochs(cached, 2), _epochs(plain, 2)
    _assert_same(got, want)
    assert be.batch_calls == len(got)                                       # ONE launch per batch
    assert {int(v) for b in want for v in b[0][1]} >= {3} and cache.hits > 0
    assert not torch.equal(got[0][1], got[len(got) // 2][1])                           # the second epoch is another epoch


def test_every_file_is_decoded_once(tree, monkeypatch):
    args = _small(tree)
    calls = []
    real = D._read_rgb
    monkeypatch.setattr(D, "_read_rgb", lambda path: (calls.append(path), real(path))[1])
    be = BatchDouble()
    cache = DeviceImageCache(be, 1 << 30)
    cached = D.FolderLoader(args, 4, seed=3, backend=be, threads=3, cache=cache)
    got = _epochs(cached, 2)
    used = {f for s in cached.ids for f in (s["file"], s["gt"]) if f is not None}
    assert len(used) == 5                                                   # 3 denoise images, the hazy image and its original
    assert sorted(calls) == sorted(used)                                    # exactly once per distinct file, over two epochs
    resolutions = 2 * sum(1 if s["gt"] is None else 2 for s in cached.ids)
    assert cache.hits + cache.misses == resolutions and cache.misses == len(used) == cache.images
    assert cache.bytes == sum(t.numel() for t in (cache.lookup(k) for k in cache.keys()))
    assert cache.sr_degradations == 0
    del calls[:]
    plain = D.FolderLoader(args, 4, seed=3, backend=be, threads=3)
    want = _epochs(plain, 2)
    assert len(calls) == resolutions                                        # uncached: once or twice per SAMPLE
    _assert_same(got, want)
    assert len(got) == 2 * len(plain) == 16


def test_budget_keeps_the_first_images_touched_and_nothing_else(tree):
    args = _small(tree)
    be = BatchDouble()
    probe = DeviceImageCache(be, 1 << 30)
    _epochs(D.FolderLoader(args, 4, seed=3, backend=be, cache=probe), 1)
    first = probe.keys()[:2]
    sizes = [probe.lookup(k).numel() for k in first]
    budget = sizes[0] + sizes[1]                                            # holds the first two images touched and not a byte more

    class Watched(DeviceImageCache):
        def offer(self, key, img):
            out = super().offer(key, img)
            assert self.bytes <= self.budget
            return out

    cache = Watched(be, budget)
    got = _epochs(D.FolderLoader(args, 4, seed=3, backend=be, cache=cache), 2)
    assert cache.keys() == first and cache.bytes == sizes[0] + sizes[1] == budget
    want = _epochs(D.FolderLoader(args, 4, seed=3, backend=be), 2)
    _assert_same(got, want)
    assert cache.misses > 5                                                 # what is not resident is a miss every time it is met
    none = DeviceImageCache(be, 0)
    got0 = _epochs(D.FolderLoader(args, 4, seed=3, backend=be, cache=none), 1)
    assert none.images == 0 and none.bytes == 0 and none.hits == 0 and none.misses > 0
    _assert_same(got0, want[:8])


def test_row_check_refuses_before_any_launch():
    be = BatchDouble()
    H, W = 40, 48
    img = torch.zeros(H, W, 3, dtype=torch.uint8)
    out = lambda n=1: (torch.full((n, 3, P, P), float("nan")), torch.full((n, 3, P, P), float("nan")))
    ok = (img, None, H - P, W - P, 7, 15.0, 1)
    d, c = out(2)
    be.patch_prep_batch([ok, (img, img.clone(), 0, 0, 0, 0.0, 2)], P, d, c)     # the last window and the last mode are fine
    assert not torch.isnan(d).any() and not torch.isnan(c).any()
    bad = {
        "window": (img, None, H - P + 1, 0, 1, 15.0, 1),                        # y0 + P == H + 1
        "window x": (img, None, 0, W - P + 1, 1, 15.0, 1),
        "negative": (img, None, -1, 0, 1, 15.0, 1),
        "mode": (img, None, 0, 0, 8, 15.0, 1),
        "pair": (img, torch.zeros(H, W + 1, 3, dtype=torch.uint8), 0, 0, 1, 0.0, 1),
        "dtype": (img.float(), None, 0, 0, 1, 15.0, 1),
        "deg dtype": (img, img.to(torch.int32), 0, 0, 1, 0.0, 1),
        "strides": (torch.zeros(H, 2 * W, 3, dtype=torch.uint8)[:, ::2], None, 0, 0, 1, 15.0, 1),
    }
    for name, row in bad.items():
        d, c = out(2)
        with pytest.raises(ValueError, match="row 1"):
            check_patch_rows([ok, row], P, d, c)
        with pytest.raises(ValueError):
            be.patch_prep_batch([ok, row], P, d, c)
        assert torch.isnan(d).all() and torch.isnan(c).all() and be.batch_calls == 1, name   # nothing was written, row 0 included
    d, c = out(1)
    with pytest.raises(ValueError):
        check_patch_rows([ok, ok], P, d, c)                                     # outputs of another batch size
    with pytest.raises(ValueError):
        check_patch_rows([], P, d, c)
    with pytest.raises(ValueError):
        check_patch_rows([ok], 0, d, c)


def test_call_trace_of_every_family_is_the_recorded_one(tmp_path):
    """tests/golden/loader_trace.json (scripts/make_loader_trace_fixture.py; recorded from the commit the file names, the parent of the
    change that put the whole-image tasks into one table): every draw, entry-point call, patch_prep row, batch, cache insertion and
    counter of all task families at once — uncached, cached at two budgets, world 1 and both ranks of world 2, two epochs — held
    batch by batch through a SHA-256 that runs over every entry of the log (tests/loader_trace.py::digest)"""
    import json
    import loader_trace as LT
    from conftest import GOLD
    want = json.load(open(os.path.join(GOLD, "loader_trace.json")))
    log = json.loads(json.dumps(LT.record(tmp_path)))                       # tuples as the lists JSON makes of them
    got = LT.digest(log)
    assert [r["run"] for r in got] == [r["run"] for r in want["runs"]] and len(got) == 9
    for g, w in zip(got, want["runs"]):
        first = next((k for k, (x, y) in enumerate(zip(g["batches"], w["batches"])) if x != y), None)
        assert first is None and len(g["batches"]) == len(w["batches"]), (g["run"], "first batch that differs", first)
        assert g["cache"] == w["cache"], g["run"]
    assert len(log) == want["entries"] == 2803
    kinds = {e[0] for e in log}
    assert kinds == {"ids", "run", "batch", "cache", "patch_prep", "patch_prep_batch", "sr_degrade_u8", "jpeg_degrade_u8", "blur_degrade_u8",
                     "bd_degrade_u8", "chain_degrade_u8"}


def test_trainer_flags():
    from rcot_amd import trainer as TR
    o = TR.parser.parse_args([])
    assert o.data_cache == "off" and o.data_cache_gb == 16.0
    o = TR.parser.parse_args(["--data_cache", "device", "--data_cache_gb", "0.5"])
    assert o.data_cache == "device" and o.data_cache_gb == 0.5
    with pytest.raises(SystemExit):
        TR.parser.parse_args(["--data_cache", "host"])
    c = DeviceImageCache(BatchDouble(), 2 ** 30)
    assert c.report() == "data cache: 0 images, 0.0 MiB of 1 GiB, 0 hits, 0 misses, 0 sr degradations"
