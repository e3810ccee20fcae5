"""GPU tier of the degradation chains (rcot_amd/chain.py): a chain against the hand composition of its stages, byte for byte; the order
of the stages; the folder loader with and without the device cache; a --de_type list that mixes a chain with jpeg_q10; the folder tool
against the tester's --savedeg; the trainer CLI."""
import os
import random
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from rcot_amd import blur as B
from rcot_amd import chain as C
from rcot_amd import jpeg as J
from rcot_amd import params as P
from rcot_amd import resize as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _u8(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def img(hip):
    return torch.from_numpy(_u8(21, 48, 80)).cuda()


def _chain(hip, img, name, seed=9, values=None, border="replicate", sub=2):
    spec = C.parse_de_type(name)
    before = img.clone()
    out = C.chain_degrade_u8(img, spec, C.Draws(seed, values if values is not None else (None,) * len(spec)), border, sub, hip)
    assert torch.equal(img, before) and out.data_ptr() != img.data_ptr() and out.shape == img.shape and out.dtype == torch.uint8
    return out


# ------------------------------------------------------------------ composition: differential against the stages' own entry points
def test_a_chain_is_the_hand_composition_of_its_stages(hip, img):
    g16 = B.psf_q_of("g1.6")
    want = J.jpeg_degrade_u8(B.blur_degrade_u8(img, g16, "replicate", hip), 30, 2, hip)
    assert torch.equal(_chain(hip, img, "chain_blur_g1.6+jpeg_q30"), want)
    want = B.blur_degrade_u8(R.sr_degrade_u8(img, 2, hip), B.psf_q_of("g2k15"), "replicate", hip)
    assert torch.equal(_chain(hip, img, "chain_sr_x2+blur_g2k15"), want)
    # the noise stage is stage 1 of the chain: its seed is stage_seed(seed, 1)
    noisy = hip.noise_u8(B.blur_degrade_u8(img, g16, "replicate", hip), "g", 10.0, 0.0, C.stage_seed(9, 1))
    want = J.jpeg_degrade_u8(noisy, 40, 2, hip)
    got = _chain(hip, img, "chain_blur_g1.6+noise_g10+jpeg_q40")
    assert torch.equal(got, want)
    assert not torch.equal(got, _chain(hip, img, "chain_blur_g1.6+noise_g10+jpeg_q40", seed=10))
    assert not torch.equal(got, J.jpeg_degrade_u8(hip.noise_u8(B.blur_degrade_u8(img, g16, "replicate", hip), "g", 10.0, 0.0, 9), 40, 2, hip))
    # the flags reach the stages that read them; the drawn values replace the ranges
    want = J.jpeg_degrade_u8(B.blur_degrade_u8(img, g16, "wrap", hip), 30, 0, hip)
    assert torch.equal(_chain(hip, img, "chain_blur_g1.6+jpeg_q30", border="wrap", sub=0), want)
    want = hip.noise_u8(J.jpeg_degrade_u8(B.blur_degrade_u8(img, B.psf_q_of("m15", 37), "mirror", hip), 23, 2, hip), "gray", 7.25, 0.0,
                        C.stage_seed(9, 2))
    assert torch.equal(_chain(hip, img, "chain_blur_m15+jpeg_q20-40+noise_gray5-20", values=(37, 23, 7.25), border="mirror"), want)
    want = hip.noise_u8(R.sr_degrade_u8(img, 4, hip), "pg", 0.5, 2.0, C.stage_seed(9, 1))
    assert torch.equal(_chain(hip, img, "chain_sr_x4+noise_pg0.5x2"), want)


def test_two_noise_stages_are_independent_and_the_order_matters(hip, img):
    a = _chain(hip, img, "chain_noise_g10+jpeg_q20")
    b = _chain(hip, img, "chain_jpeg_q20+noise_g10")
    assert not torch.equal(a, b)
    assert torch.equal(a, J.jpeg_degrade_u8(hip.noise_u8(img, "g", 10.0, 0.0, C.stage_seed(9, 0)), 20, 2, hip))
    assert torch.equal(b, hip.noise_u8(J.jpeg_degrade_u8(img, 20, 2, hip), "g", 10.0, 0.0, C.stage_seed(9, 1)))
    flat = torch.full((64, 64, 3), 128, dtype=torch.uint8, device="cuda")
    one = _chain(hip, flat, "chain_noise_g10").cpu().numpy().astype(np.float64) - 128
    two = _chain(hip, flat, "chain_noise_g10+noise_g10").cpu().numpy().astype(np.float64) - 128
    second = two - one                                              # what the second stage added to the first stage's output
    c = float(((one - one.mean()) * (second - second.mean())).sum() / np.sqrt(((one - one.mean()) ** 2).sum() * ((second - second.mean()) ** 2).sum()))
    assert abs(c) <= 5 / np.sqrt(one.size), c                       # 5 standard errors of a correlation of N independent pairs


# ------------------------------------------------------------------ the loader
DETERMINISTIC, NOISY, RANGED = "chain_blur_g1.6+jpeg_q30", "chain_blur_g1.6+noise_g10+jpeg_q40", "chain_blur_m15+noise_g5-20+jpeg_q20-40"


@pytest.fixture
def folder(tmp_path):
    """four 64 x 96 PNGs -> (args, clean images by name)"""
    from PIL import Image
    os.makedirs(tmp_path / "clean")
    imgs = {n: _u8(40 + i, 64, 96) for i, n in enumerate("abcd")}
    for n, a in imgs.items():
        Image.fromarray(a).save(tmp_path / "clean" / f"{n}.png")
    return Namespace(de_type=[], chain_dir=str(tmp_path / "clean") + "/", jpeg_dir=str(tmp_path / "clean") + "/", patch_size=32), imgs


def _count_chains(monkeypatch):
    count = [0]
    real = C.chain_degrade_u8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(C, "chain_degrade_u8", counted)
    return count


@pytest.mark.parametrize("name", [DETERMINISTIC, NOISY, RANGED], ids=["deterministic", "noise", "ranged"])
def test_cached_loader_equals_uncached(hip, folder, monkeypatch, name):
    from rcot_amd import data as D
    from rcot_amd.imagecache import DeviceImageCache
    args, _ = folder
    args.de_type = [name]
    count = _count_chains(monkeypatch)
    cache = DeviceImageCache(hip, 1 << 30)
    cached = D.FolderLoader(args, 3, seed=5, backend=hip, threads=2, cache=cache)
    got = [b for _ in range(2) for b in cached]
    n_cached = count[0]
    plain = D.FolderLoader(args, 3, seed=5, backend=hip, threads=2)
    want = [b for _ in range(2) for b in plain]
    assert len(plain) == 7 and len(got) == len(want) == 14 and count[0] - n_cached == 40       # 20 samples an epoch
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2) and l1.tolist() == [7] * len(n1), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
        assert not torch.equal(d1, c1), k
    files = sorted(os.path.join(args.chain_dir, f"{n}.png") for n in "abcd")
    assert all((f, "crop16") in cache for f in files)
    twins = sorted(k for k in cache.keys() if k[1] == "chain")
    if name == DETERMINISTIC:                                                                  # one twin per image, made once
        assert n_cached == 4 == cache.chain_degradations and twins == sorted((f, "chain", name, "replicate", 2) for f in files)
        assert cache.report().endswith("0 sr degradations, 4 chain degradations")
    else:                                                                                      # only the decoded images are kept
        assert n_cached == 40 and cache.chain_degradations == 0 and twins == [] and cache.images == 4
    # another epoch is another epoch, and the same seed repeats the run
    assert not torch.equal(got[0][1], got[7][1])
    rerun = D.FolderLoader(args, 3, seed=5, backend=hip, threads=2)
    again = [b for _ in range(2) for b in rerun]
    assert len(again) == 14
    assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(again, want))


def test_noise_is_drawn_anew_for_every_sample(hip, folder):
    """the same image under the noise chain in two samples: with the crop and the augmentation undone by taking the SAME draws for both,
    only the noise seed differs — and the degraded patches differ, while the clean ones are equal"""
    from rcot_amd import data as D
    args, imgs = folder
    args.de_type = [NOISY]
    loader = D.FolderLoader(args, 3, seed=5, backend=hip)
    sid = loader.ids[0]

    class Fixed(random.Random):
        """the crop origin and the mode of every sample are those of the first; the noise seed is the stream's own"""
        def randint(self, a, b):
            return a + (b - a) // 2
    out = []
    for k in (1, 2):
        d, c = torch.empty(3, 32, 32, device="cuda"), torch.empty(3, 32, 32, device="cuda")
        loader._sample(Fixed(k), sid, d, c)
        out.append((d, c))
    assert torch.equal(out[0][1], out[1][1]) and not torch.equal(out[0][0], out[1][0])
    d, c = torch.empty(3, 32, 32, device="cuda"), torch.empty(3, 32, 32, device="cuda")
    loader._sample(Fixed(1), sid, d, c)
    assert torch.equal(d, out[0][0]) and torch.equal(c, out[0][1])                             # the same stream, the same patch


def test_a_chain_in_the_list_leaves_the_other_tasks_draws_alone(hip, folder):
    """--de_type chain + jpeg_q10: every jpeg_q10 sample is cut with the three common draws of its global position — the patch a list
    without chains gives a jpeg_q10 sample with those draws (made here through the loader's own kernel)"""
    from rcot_amd import data as D
    args, imgs = folder
    args.de_type = [RANGED, "jpeg_q10"]
    seed, Bn = 5, 3
    mixed = D.FolderLoader(args, Bn, seed=seed, backend=hip)
    assert len(mixed.ids) == 40 and len(mixed) == 14
    order = list(range(40))
    random.Random(seed * 1_000_003 + 1).shuffle(order)
    twin = {}
    seen = {"jpeg": 0, "chain": 0}
    for it, ([names, de_id], deg, clean) in enumerate(mixed):
        for j, n in enumerate(names):
            pos = it * Bn + j
            sid = mixed.ids[order[pos]]
            assert os.path.basename(sid["file"]) == n + ".png"
            rng = random.Random((seed * 1_000_003 + 1) * 2_147_483_659 + pos)
            y0, x0, mode, nseed = rng.randint(0, 64 - 32), rng.randint(0, 96 - 32), rng.randint(1, 7), rng.getrandbits(63)
            a = torch.from_numpy(imgs[n]).cuda()
            d, c = torch.empty(3, 32, 32, device="cuda"), torch.empty(3, 32, 32, device="cuda")
            if "jpeg" in sid:
                if n not in twin:
                    twin[n] = J.jpeg_degrade_u8(a, 10, 2, hip)
                hip.patch_prep(a, twin[n], y0, x0, 32, mode, 0.0, nseed, d, c)
                seen["jpeg"] += 1
            else:                                                    # and the chain's own draws follow, in stage order
                draws = C.Draws(nseed, (rng.randint(0, 179), rng.uniform(5.0, 20.0), rng.randint(20, 40)))
                hip.patch_prep(a, C.chain_degrade_u8(a, sid["chain"][0], draws, "replicate", 2, hip), y0, x0, 32, mode, 0.0, nseed, d, c)
                seen["chain"] += 1
            assert torch.equal(deg[j], d) and torch.equal(clean[j], c), (it, j, n)
    assert seen == {"jpeg": 20, "chain": 20}
    # the jpeg-only list at the same seed: its sample at a position has the draws of that position too (same sizes: the same crop)
    args.de_type = ["jpeg_q10"]
    only = D.FolderLoader(args, Bn, seed=seed, backend=hip)
    order = list(range(20))
    random.Random(seed * 1_000_003 + 1).shuffle(order)
    ([names, _], deg, clean) = next(iter(only))
    assert names == [os.path.basename(only.ids[k]["file"])[:-4] for k in order[:Bn]]
    for j, n in enumerate(names):
        rng = random.Random((seed * 1_000_003 + 1) * 2_147_483_659 + j)
        y0, x0, mode, nseed = rng.randint(0, 32), rng.randint(0, 64), rng.randint(1, 7), rng.getrandbits(63)
        a = torch.from_numpy(imgs[n]).cuda()
        d, c = torch.empty(3, 32, 32, device="cuda"), torch.empty(3, 32, 32, device="cuda")
        hip.patch_prep(a, twin.get(n, J.jpeg_degrade_u8(a, 10, 2, hip)), y0, x0, 32, mode, 0.0, nseed, d, c)
        assert torch.equal(deg[j], d) and torch.equal(clean[j], c), (j, n)


# ------------------------------------------------------------------ the folder tool, the tester, the trainer
def _checkpoint(path):
    from rcot_amd.compat import shim
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()}
    torch.save({"epoch": 1, "Tnet": shim().T_net.from_state_dict(prm, decoder=True)}, path)
    return path


def test_folder_tool_and_tester_write_the_same_bytes(hip, folder, tmp_path):
    from PIL import Image
    from rcot_amd import tester as TS
    args, imgs = folder
    spec = C.parse_de_type(RANGED)
    assert C.main(["--in", args.chain_dir, "--out", str(tmp_path / "tool"), "--chain", RANGED, "--seed", "3"], backend=hip) == 4
    assert C.main(["--in", args.chain_dir, "--out", str(tmp_path / "tool4"), "--chain", RANGED[len("chain_"):], "--seed", "4"], backend=hip) == 4
    for i, n in enumerate("abcd"):                                                            # the per-file rule, by hand
        want = C.chain_degrade_u8(torch.from_numpy(imgs[n]).cuda(), spec, C.file_draws(spec, 3, i), "replicate", 2, hip)
        assert np.array_equal(np.array(Image.open(tmp_path / "tool" / f"{n}.png")), want.cpu().numpy()), n
        assert open(tmp_path / "tool" / f"{n}.png", "rb").read() != open(tmp_path / "tool4" / f"{n}.png", "rb").read(), n
    ck = _checkpoint(str(tmp_path / "net.pth"))
    out = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres",
                       str(tmp_path / tag / "RES") + "/"]
    # --degset names a folder that does not exist and is not read
    base = ["--model", ck, "--tarset", args.chain_dir, "--degset", str(tmp_path / "nowhere") + "/"]
    r = TS.main(base + out("t") + ["--chain", RANGED, "--seed", "3", "--savedeg", str(tmp_path / "t" / "DEG")])
    assert r["images"] == 4 and np.isfinite(r["psnr"])
    for n in "abcd":
        assert open(tmp_path / "t" / "DEG" / f"{n}.png", "rb").read() == open(tmp_path / "tool" / f"{n}.png", "rb").read(), n
        assert np.array_equal(np.array(Image.open(tmp_path / "t" / "TAR" / f"{n}.png")), imgs[n]), n
    with pytest.raises(SystemExit, match="--chain makes the network's input from the target"):
        TS.main(base + out("x") + ["--chain", RANGED, "--jpeg_q", "10"])
    assert not os.path.exists(tmp_path / "x")


def test_trainer_cli_chain(hip, tmp_path):
    """--de_type chain_blur_g1.6+noise_g5-20+jpeg_q20-40 on one 64 x 96 image: 5 samples, two iterations of one epoch at P = 32, a
    two-image validation folder made by the folder tool; finite losses, a validation line and a checkpoint"""
    from PIL import Image
    os.makedirs(tmp_path / "clean")
    os.makedirs(tmp_path / "val")
    Image.fromarray(_u8(60, 64, 96)).save(tmp_path / "clean" / "a.png")
    for i in range(2):
        Image.fromarray(_u8(61 + i, 32, 48)).save(tmp_path / "val" / f"v{i}.png")
    name = "chain_blur_g1.6+noise_g5-20+jpeg_q20-40"
    assert C.main(["--in", str(tmp_path / "val"), "--out", str(tmp_path / "valdeg"), "--chain", name, "--seed", "4"], backend=hip) == 2
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--de_type", name, "--chain_dir", str(tmp_path / "clean"), "--patch_size", "32",
           "--batchSize", "3", "--nEpochs", "1", "--pairnum", "10000000", "--seed", "4", "--type", "Chain", "--sigma", "1", "--degset",
           str(tmp_path / "valdeg") + "/", "--tarset", str(tmp_path / "val") + "/"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "...total sample ids: 5" in r.stdout and "Epoch 1(0/2)" in r.stdout
    losses = [float(v) for v in re.findall(r"Loss_\w+: ([-+0-9.eEnaif]+)", r.stdout)]
    assert len(losses) >= 2 and np.isfinite(losses).all(), r.stdout[-2000:]
    assert os.path.isfile(tmp_path / "checkpoint" / "model_Chain__1_1.0.pth"), (os.listdir(tmp_path), r.stdout[-2000:])
    val = open(tmp_path / "checksample" / "Chain" / "validation_results.txt").read()
    assert re.search(r"Epoch 1, psnr [0-9.]+,", val), val
