"""GPU tier of the device-resident training set: rcot_patch_prep_batch against rcot_patch_prep, bit for bit, on guard-banded,
pre-poisoned buffers (tests/guarded.py); its refusal; ``FolderLoader(..., cache=DeviceImageCache(...))`` against the uncached loader
on the device, with the count of whole-image degradations; the trainer CLI with ``--data_cache device``."""
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from guarded import GuardSet
from synth_folders import dataset_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


@pytest.fixture
def gs():
    s = GuardSet("cuda")
    yield s
    s.check()


SIZES = ((37, 45), (33, 64), (32, 32))


def _images(gs, sizes=SIZES):
    """per size a (clean, paired degraded) couple of guarded device images"""
    g = np.random.Generator(np.random.PCG64(11))
    mk = lambda h, w, name: gs.tensor(torch.from_numpy(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)), name)
    return [(mk(h, w, f"clean {h}x{w}"), mk(h, w, f"deg {h}x{w}")) for h, w in sizes]


def _both(hip, gs, rows, P):
    """one rcot_patch_prep_batch launch against len(rows) rcot_patch_prep launches into a second guarded pair"""
    B = len(rows)
    d, c = gs.empty((B, 3, P, P), name="batch deg_out"), gs.empty((B, 3, P, P), name="batch clean_out")
    hip.patch_prep_batch(rows, P, d, c)
    gs.check()
    d1, c1 = gs.empty((B, 3, P, P), name="single deg_out"), gs.empty((B, 3, P, P), name="single clean_out")
    for b, (clean, deg, y0, x0, mode, sigma, seed) in enumerate(rows):
        hip.patch_prep(clean, deg, y0, x0, P, mode, sigma, seed, d1[b], c1[b])
        gs.check()
    assert not torch.isnan(d1).any() and not torch.isnan(c1).any()                 # every element of the reference was written
    assert torch.equal(d, d1) and torch.equal(c, c1)
    return d, c


def test_batch_rows_of_mixed_images_modes_and_kinds(hip, gs):
    """P = 32, B = 5, two launches: three images of 37 x 45, 33 x 64 and 32 x 32 (its window is the whole image), modes 0..7, paired
    rows and noise rows (sigma 15 and 50, seeds that differ, one above 2^63) in the same launch, windows on the last row and column"""
    (a, ad), (b, bd), (w, wd) = _images(gs)
    first = [(a, None, 5, 13, 0, 15.0, 101), (b, bd, 1, 32, 1, 0.0, 1), (w, None, 0, 0, 2, 50.0, (1 << 64) - 3),
             (a, ad, 5, 0, 3, 0.0, 1), (b, None, 0, 7, 4, 50.0, 103)]
    second = [(w, wd, 0, 0, 5, 0.0, 1), (a, None, 0, 13, 6, 50.0, 104), (b, bd, 1, 0, 7, 0.0, 1), (w, None, 0, 0, 7, 15.0, 105),
              (a, ad, 5, 13, 2, 0.0, 1)]
    for rows in (first, second):
        d, c = _both(hip, gs, rows, 32)
        for r, (clean, deg, *_rest) in enumerate(rows):
            assert not torch.equal(d[r], c[r])                                       # a degraded patch is not its clean one
    # the same noise row twice in one launch gives the same bits; another seed does not
    d, _ = _both(hip, gs, [(a, None, 2, 3, 1, 15.0, 7), (a, None, 2, 3, 1, 15.0, 7), (a, None, 2, 3, 1, 15.0, 8)], 32)
    assert torch.equal(d[0], d[1]) and not torch.equal(d[0], d[2])


@pytest.mark.parametrize("P", [5, 33])
@pytest.mark.parametrize("B", [1, 3])
def test_partial_and_ragged_blocks(hip, gs, P, B):
    """P = 5: 25 pixels, one partial workgroup; P = 33: 1089 pixels, four full workgroups and one of 65 threads' worth"""
    (a, ad), (b, bd), _ = _images(gs)
    rows = [(a, None, 37 - P, 45 - P, 6, 25.0, 9), (b, bd, 33 - P, 64 - P, 3, 0.0, 1), (a, ad, 0, 0, 7, 0.0, 1)][:B]
    _both(hip, gs, rows, P)


def test_many_samples_in_one_launch(hip, gs):
    """B = 64 at P = 32: 256 workgroups, the sample index far beyond one wavefront's worth of blocks"""
    imgs = _images(gs)
    rng = np.random.Generator(np.random.PCG64(5))
    rows = []
    for r in range(64):
        clean, deg = imgs[r % 3]
        H, W = clean.shape[:2]
        paired = bool(rng.integers(0, 2))
        rows.append((clean, deg if paired else None, int(rng.integers(0, H - 32 + 1)), int(rng.integers(0, W - 32 + 1)), r % 8,
                     0.0 if paired else (15.0, 25.0, 50.0)[r % 3], 1000 + r))
    _both(hip, gs, rows, 32)


def test_out_of_range_row_is_refused_before_the_launch(hip, gs):
    (a, ad), (b, bd), _ = _images(gs)
    d, c = gs.empty((2, 3, 32, 32), name="deg_out"), gs.empty((2, 3, 32, 32), name="clean_out")
    before = d.view(torch.int32).clone(), c.view(torch.int32).clone()
    ok = (a, ad, 0, 0, 1, 0.0, 1)
    for bad in ((b, None, 2, 0, 1, 15.0, 1),              # y0 + P == H + 1
                (b, None, 0, 33, 1, 15.0, 1),             # x0 + P == W + 1
                (b, None, 0, 0, 8, 15.0, 1),              # no such map
                (b, ad, 0, 0, 1, 0.0, 1)):                # a pair of two shapes
        with pytest.raises(ValueError):
            hip.patch_prep_batch([ok, bad], 32, d, c)
        gs.check()
        assert torch.equal(d.view(torch.int32), before[0]) and torch.equal(c.view(torch.int32), before[1])   # row 0 included
    from rcot_amd import lib
    assert hip.L.rcot_patch_prep_batch(None, 1, 32, d.data_ptr(), c.data_ptr(), hip._st()) == -1
    assert hip.L.rcot_patch_prep_batch(d.data_ptr(), 0, 32, d.data_ptr(), c.data_ptr(), hip._st()) == -1
    assert hip.L.rcot_patch_prep_batch(d.data_ptr(), 1, 0, d.data_ptr(), c.data_ptr(), hip._st()) == -1
    assert lib.ABI_VERSION >= 31
    gs.check()
    assert torch.equal(d.view(torch.int32), before[0]) and torch.equal(c.view(torch.int32), before[1])


def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(path)


def test_cached_loader_equals_uncached_on_the_device(hip, tmp_path, monkeypatch):
    """3 denoise images, 2 rain pairs and 2 HR images of 96 x 120 for sr_x2; P = 32, batch 4, two epochs (745 samples each)"""
    from rcot_amd import data as D
    from rcot_amd import resize as RZ
    from rcot_amd.imagecache import DeviceImageCache
    r = str(tmp_path)
    for i in range(3):
        _png(f"{r}/Denoise/img{i}.png", 70 + i, 90 + 2 * i, 10 + i)
    for d_ in ("noisy", "rainy"):
        os.makedirs(f"{r}/lists/{d_}")
    open(f"{r}/lists/noisy/denoise.txt", "w").write("\n".join(f"img{i}.png" for i in range(3)) + "\n")
    open(f"{r}/lists/rainy/rainTrain.txt", "w").write("rainy/rain-1.png\nrainy/rain-2.png\n")
    for i in (1, 2):
        _png(f"{r}/Derain/rainy/rain-{i}.png", 80, 96, 20 + i)
        _png(f"{r}/Derain/gt/norain-{i}.png", 80, 96, 30 + i)
        _png(f"{r}/HR/hr{i}.png", 96, 120, 40 + i)
    args = Namespace(de_type=["denoise_25", "derain", "sr_x2"], data_file_dir=f"{r}/lists/", denoise_dir=f"{r}/Denoise/",
                     derain_dir=f"{r}/Derain/", sr_dir=f"{r}/HR/", patch_size=32)
    count = [0]
    real = RZ.sr_degrade_u8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(RZ, "sr_degrade_u8", counted)
    cache = DeviceImageCache(hip, 1 << 30)
    cached = D.FolderLoader(args, 4, seed=5, backend=hip, threads=4, cache=cache)
    got = [b for _ in range(2) for b in cached]
    assert count[0] == 2 == cache.sr_degradations                               # once per HR file
    assert cache.images == 3 + 4 + 2 + 2 == cache.misses and cache.hits > 1400
    count[0] = 0
    plain = D.FolderLoader(args, 4, seed=5, backend=hip, threads=4)
    want = [b for _ in range(2) for b in plain]
    assert count[0] == 2 * 10                                                   # once per SR sample: 2 files x5, two epochs
    assert len(got) == len(want) == 2 * len(plain) == 2 * 187
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
    assert not torch.equal(got[0][1], got[187][1])


def test_every_task_family_at_once_cached_equals_uncached(hip, tmp_path):
    """the --de_type list of tests/loader_trace.py — denoise, a paired task, sr_x2, sr_x3, sr_bd_x3, jpeg_q10, blur_g1.6, blur_m15, a
    cacheable chain with an SR stage and a drawn chain — on its three images of 48 x 64, 50 x 70 and 66 x 81 (the crops to 16 and to
    3 both act: 50 x 70 -> 48 x 64 -> 48 x 63); P = 32, batch 4, two epochs of 150 samples"""
    import loader_trace as LT
    from rcot_amd import chain as C
    from rcot_amd import data as D
    from rcot_amd.imagecache import DeviceImageCache
    args = LT.tree(str(tmp_path))
    cache = DeviceImageCache(hip, 1 << 30)
    cached = D.FolderLoader(args, 4, seed=LT.SEED, backend=hip, threads=4, cache=cache)
    plain = D.FolderLoader(args, 4, seed=LT.SEED, backend=hip, threads=4)
    got, want = [b for _ in range(2) for b in cached], [b for _ in range(2) for b in plain]
    assert len(got) == len(want) == 2 * 38
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
    assert not torch.equal(got[0][1], got[38][1]) and not torch.equal(got[0][2], got[38][2])      # the second epoch is another epoch
    files = len(LT.SIZES)
    assert cache.sr_degradations == files * 2                                 # sr_x2, sr_x3
    assert cache.jpeg_degradations == files * 1                               # jpeg_q10
    assert cache.blur_degradations == files * 2                               # blur_g1.6, sr_bd_x3 (blur_m15 draws its angle)
    assert cache.chain_degradations == files * 1                              # chain_sr_x3+blur_g1.6 (the other chain draws)
    clean = [f"{tmp_path}/clean/{n}.png" for n in LT.SIZES]
    twins = {k for k in cache.keys() if k[1] != "crop16"}
    kept = C.canonical(C.parse_de_type("chain_sr_x3+blur_g1.6"))
    assert twins == {key for f in clean for key in ((f, "sr", 2), (f, "sr", 3), (f, "bd", 3), (f, "jpeg", 10, 0), (f, "blur", "g1.6", "mirror"),
                                                    (f, "chain", kept, "mirror", 0))}      # no twin of blur_m15 or of the drawn chain
    assert cache.images == len(twins) + 3 * files + 2 * files == cache.misses  # + crop16, mod 2, mod 3; + the paired task's two folders


def test_trainer_cli_with_the_device_cache(tmp_path):
    """--data_cache device on synth_folders.dataset_tree: 3 files, 15 samples, two epochs of 5 iterations at P = 32"""
    root = str(tmp_path)
    dataset_tree(root)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--batchSize", "3", "--patch_size", "32", "--de_type", "denoise_25", "--nEpochs", "2",
           "--denoise_dir", f"{root}/Denoise/", "--data_file_dir", f"{root}/lists/", "--degset", f"{root}/val/input/",
           "--tarset", f"{root}/val/target/", "--pairnum", "10000000", "--seed", "4", "--type", "Cached", "--sigma", "1",
           "--data_cache", "device", "--data_cache_gb", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "...total sample ids: 15" in r.stdout and "Epoch 2(0/5)" in r.stdout
    lines = re.findall(r"^data cache: (\d+) images, ([0-9.]+) MiB of 1 GiB, (\d+) hits, (\d+) misses, (\d+) sr degradations$", r.stdout, flags=re.M)
    assert len(lines) == 2, r.stdout[-3000:]
    (n1, mib1, h1, m1, s1), (n2, mib2, h2, m2, s2) = [tuple(float(v) for v in ln) for ln in lines]
    assert n1 == n2 == m1 == m2 == 3 and s1 == s2 == 0                          # every distinct file missed once, in epoch 1
    assert h1 == 15 - 3 and h2 - h1 == 15                                       # epoch 2 is served from the device alone
    assert abs(mib1 - 3 * 96 * 112 * 3 / 2 ** 20) < 0.06 and mib2 == mib1
