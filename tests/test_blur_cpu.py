"""CPU tier of the deblurring tasks: the numpy restatement of the PSF blur (tests/blur_double.py, written from the rule in csrc/blur.hip)
against an independent float64 filter (scipy.ndimage.correlate) and against plain shifted / padded indexing; the PSF builders, the
quantisation and the spec grammar; the sample lists, the ``blur_<spec>`` / ``sr_bd_x3`` names, every up-front refusal and the cache keys;
the folder loader, the folder CLI and the BD chain on a CPU double of the backend."""
import os
import random
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import blur_double as BD
import resize_double as RD
from conftest import ROOT
from rcot_amd import blur as B
from test_jpeg_cpu import contents

BORDERS = ("replicate", "mirror", "wrap")
SCIPY_MODE = {"replicate": "nearest", "mirror": "mirror", "wrap": "wrap"}


def box(K):
    return np.full((K, K), 1.0 / (K * K))


def delta(K, i, j):
    h = np.zeros((K, K))
    h[i, j] = 1.0
    return h


#: name -> float64 PSF: the cases of the comparison with the float filter
PSFS = {"g1.6k7": lambda: B.psf_of("g1.6k7"), "g4k25": lambda: B.psf_of("g4k25"), "g5k31": lambda: B.psf_of("g5k31"),
        "aniso15": lambda: B.psf_gaussian_aniso(15, 4.0, 1.5, 30), "m15a30": lambda: B.psf_of("m15a30"), "m31a77": lambda: B.psf_of("m31a77"),
        "box31": lambda: box(31)}


def float_filter(img, h, border):
    """the independent filter: scipy's float64 correlation per channel, then floor(x + 0.5)"""
    ndi = pytest.importorskip("scipy.ndimage")
    out = np.stack([ndi.correlate(img[..., c].astype(np.float64), h, mode=SCIPY_MODE[border]) for c in range(3)], axis=-1)
    return np.floor(out + 0.5).astype(np.int64)


@pytest.mark.parametrize("name", list(PSFS))
def test_restatement_against_float_filter(name):
    """The restatement quantises its weights to 2^-22, so it may differ from the float64 filter by one grey level where the float result
    sits within about K^2 2^-23 255 of a .5 tie: max |difference| <= 1 and at most 1 % of the bytes differ, per (PSF, image, border)"""
    pytest.importorskip("scipy")
    h = PSFS[name]()
    q = B.quantise_psf(h)
    imgs = contents(97, 123, 11)
    for kind in ("noise", "smooth", "sat"):
        for border in BORDERS:
            got = BD.blur_np(imgs[kind], q, border).astype(np.int64)
            want = float_filter(imgs[kind], h, border)
            diff = np.abs(got - want)
            print(f"{name} {kind} {border}: max |diff| {int(diff.max())}, {100.0 * np.count_nonzero(diff) / diff.size:.4f} % differ")
            assert int(diff.max()) <= 1, (name, kind, border)
            assert np.count_nonzero(diff) <= 0.01 * diff.size, (name, kind, border, np.count_nonzero(diff))


def test_restatement_is_exact_where_no_tie_can_move():
    pytest.importorskip("scipy")
    imgs = contents(41, 57, 12)
    dyadic = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.float64) / 16
    for h in (delta(1, 0, 0), delta(5, 2, 2), dyadic):
        q = B.quantise_psf(h)
        for kind in ("noise", "sat", "smooth"):
            for border in BORDERS:
                assert np.array_equal(BD.blur_np(imgs[kind], q, border), float_filter(imgs[kind], h, border)), (h.shape, kind, border)


def test_delta_and_constant_images_come_back():
    """no filter needed: the centred delta returns the image, any PSF returns a constant image"""
    imgs = contents(41, 57, 12)
    for border in BORDERS:
        for K in (1, 5):
            assert np.array_equal(BD.blur_np(imgs["noise"], B.quantise_psf(delta(K, K // 2, K // 2)), border), imgs["noise"]), (K, border)
    for name in PSFS:                                                           # any PSF on a constant image
        q = B.quantise_psf(PSFS[name]())
        for border in BORDERS:
            assert np.array_equal(BD.blur_np(imgs["const"], q, border), imgs["const"]), (name, border)


def test_orientation_is_a_correlation():
    """the single weight at [0][0] reads the pixel r up and r to the left, the one at [K - 1][K - 1] the pixel r down and to the right:
    under ``wrap`` the shifted image itself.  A flipped kernel swaps the two."""
    img = contents(23, 31, 13)["noise"]
    for K in (3, 7, 31):
        r = (K - 1) // 2
        first, last = B.quantise_psf(delta(K, 0, 0)), B.quantise_psf(delta(K, K - 1, K - 1))
        assert np.array_equal(BD.blur_np(img, first, "wrap"), np.roll(img, (r, r), axis=(0, 1))), K
        assert np.array_equal(BD.blur_np(img, last, "wrap"), np.roll(img, (-r, -r), axis=(0, 1))), K
        row = B.quantise_psf(delta(K, r, 0))                                    # row r, column 0: r to the left, same row
        assert np.array_equal(BD.blur_np(img, row, "wrap"), np.roll(img, r, axis=1)), K


def padded_reference(img, q, border):
    """the rule through np.pad's index arrays (edge / reflect / wrap) and a sliding window: no code shared with ``border_index``"""
    K = q.shape[0]
    r = (K - 1) // 2
    mode = {"replicate": "edge", "mirror": "reflect", "wrap": "wrap"}[border]
    iy = np.pad(np.arange(img.shape[0]), r, mode=mode)
    ix = np.pad(np.arange(img.shape[1]), r, mode=mode)
    big = img[np.ix_(iy, ix)].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(big, (K, K), axis=(0, 1))      # [H, W, 3, K, K]
    acc = np.einsum("hwcij,ij->hwc", win, q.astype(np.int64))
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (3, 40), (40, 3), (7, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_smaller_than_the_radius(shape):
    img = contents(*shape, 14)["noise"]
    for h in (B.psf_of("g5k31"), B.psf_of("m31a77"), box(31), delta(31, 0, 30)):
        q = B.quantise_psf(h)
        for border in BORDERS:
            assert np.array_equal(BD.blur_np(img, q, border), padded_reference(img, q, border)), (shape, border)


def test_border_maps():
    p = np.arange(-9, 10)
    assert BD.border_index(p, 4, "replicate").tolist() == [0] * 9 + [0, 1, 2, 3] + [3] * 6
    assert BD.border_index(p, 4, "mirror").tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3]
    assert BD.border_index(p, 4, "wrap").tolist() == [3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    for border in BORDERS:
        assert BD.border_index(p, 1, border).tolist() == [0] * 19
    assert BD.border_index(p, 2, "mirror").tolist() == [abs(v) % 2 for v in p]


def test_step_and_phase_sample_the_plain_blur():
    for shape in ((9, 12), (96, 123), (66, 130)):
        img = contents(*shape, 15)["noise"]
        for h, border in ((B.psf_of("g1.6k7"), "replicate"), (B.psf_of("m15a30"), "mirror"), (B.psf_of("g2k15"), "wrap")):
            q = B.quantise_psf(h)
            full = BD.blur_np(img, q, border)
            for step, phase in ((3, 1), (2, 0), (2, 1)):
                if shape[0] % step or shape[1] % step:
                    continue
                got = BD.blur_np(img, q, border, step, phase)
                assert got.shape == (shape[0] // step, shape[1] // step, 3)
                assert np.array_equal(got, full[phase::step, phase::step]), (shape, step, phase)
    with pytest.raises(AssertionError):
        BD.blur_np(contents(9, 12, 1)["noise"], B.quantise_psf(box(3)), "wrap", 2, 0)      # 9 is no multiple of 2


def test_quantise_psf():
    for name in PSFS:
        h = PSFS[name]()
        q = B.quantise_psf(h)
        assert q.dtype == np.int32 and q.shape == h.shape and int(q.sum(dtype=np.int64)) == 1 << 22 and int(q.min()) >= 0, name
        assert np.abs(q / float(1 << 22) - h).max() <= 2.0 ** -22, name
        assert np.array_equal(q, B.quantise_psf(h.copy())), name
    # ties: every tap of the box has the same fractional part; the remainder goes to the lowest row-major indices
    for K in (3, 31, 63):
        q = B.quantise_psf(box(K)).ravel()
        base, rest = divmod(1 << 22, K * K)
        assert q.tolist() == [base + 1] * rest + [base] * (K * K - rest), K
    assert B.quantise_psf(delta(1, 0, 0)).tolist() == [[1 << 22]]
    bad = [-box(3), box(3) * 2, box(3) * 0.5, box(4), np.full((3, 5), 1 / 15.0), np.array([[0.5, 0.6, -0.1]]), box(3).ravel()]
    neg = box(3)
    neg[0, 0], neg[0, 1] = -0.1, neg[0, 1] + 0.1 + neg[0, 0]                   # sums to 1, one entry negative
    nan = box(3)
    nan[1, 1] = np.nan
    for h in bad + [neg, nan]:
        with pytest.raises(ValueError):
            B.quantise_psf(h)
    for q in (np.ones((3, 3), np.int32), np.full((1, 1), 1 << 22, np.int64), -B.quantise_psf(box(3)), B.quantise_psf(box(3))[:, :1],
              np.zeros((65, 65), np.int32)):
        with pytest.raises(ValueError):
            B.check_psf_q(q)


def test_psf_builders():
    """motion at 0 and 90 degrees: all mass on the middle row resp. column (cos and sin are exact at multiples of 90), one the transpose
    of the other.  Under the splatting rule the L - 2 inner taps are flat up to the ripple of a tent sampled at the spacing (L - 1) / 8 L
    (below 1 %: the tent's spectrum at 8 or more cycles), and each end tap, fed from one side only, holds between 0.5 and 0.6 of one."""
    for L in (3, 15, 31, 63):
        c = (L - 1) // 2
        h, v = B.psf_motion(L, 0), B.psf_motion(L, 90)
        assert h.shape == (L, L) and abs(h.sum() - 1) < 1e-12 and np.count_nonzero(np.delete(h, c, axis=0)) == 0
        assert np.count_nonzero(np.delete(v, c, axis=1)) == 0 and np.allclose(v.T, h, rtol=0, atol=1e-12)
        assert np.allclose(h[c], h[c, ::-1], rtol=0, atol=1e-12)
        inner = h[c, 1:-1]
        assert inner.max() <= 1.01 * inner.min() and 0.5 * inner.min() <= h[c, 0] <= 0.6 * inner.max()
    d = B.psf_motion(15, 45)                                # along the anti-diagonal (up and to the right), 7 cos 45 = 4.95 each way
    assert d[2, 12] > 0 and d[12, 2] > 0 and d[2, 2] == 0 and d[12, 12] == 0 and d[0, 14] == 0 and np.allclose(d, d[::-1, ::-1], atol=1e-12)
    g = B.psf_gaussian(7, 1.6)
    assert abs(g.sum() - 1) < 1e-12 and np.array_equal(g, g.T) and np.array_equal(g, g[::-1]) and g[3, 3] == g.max()
    assert abs(g[3, 4] / g[3, 3] - np.exp(-1 / (2 * 1.6 ** 2))) < 1e-12
    assert np.count_nonzero(B.psf_gaussian(63, 0.5) == 0) > 0                  # values below eps * max are zeroed
    a = B.psf_gaussian_aniso(15, 4.0, 1.0, 0)
    assert abs(a.sum() - 1) < 1e-12 and a[7, 12] > a[12, 7]                    # the long axis lies along x at 0 degrees
    assert np.allclose(B.psf_gaussian_aniso(15, 2.0, 2.0, 37), B.psf_gaussian(15, 2.0), atol=1e-12)
    assert np.allclose(B.psf_gaussian_aniso(15, 4.0, 1.0, 90), a.T, atol=1e-12)
    for fn in (lambda: B.psf_gaussian(6, 1.0), lambda: B.psf_gaussian(7, 0), lambda: B.psf_motion(14, 0),
               lambda: B.psf_gaussian_aniso(7, 1.0, -1.0, 0)):
        with pytest.raises(ValueError):
            fn()


def test_parse_psf():
    assert B.parse_psf("g1.6") == ("g", 1.6, 11) and B.parse_psf("g2k15") == ("g", 2.0, 15) and B.parse_psf("g10") == ("g", 10.0, 61)
    assert B.parse_psf("g1.6k7") == ("g", 1.6, 7) and B.parse_psf("g0.5k1") == ("g", 0.5, 1)
    assert B.parse_psf("a4x1r30") == ("a", 4.0, 1.0, 30, 25) and B.parse_psf("a3x1.5r120k15") == ("a", 3.0, 1.5, 120, 15)
    assert B.parse_psf("m15") == ("m", 15, None) and B.parse_psf("m15a30") == ("m", 15, 30) and B.parse_psf("m63a179") == ("m", 63, 179)
    assert B.parse_psf("m3a0") == ("m", 3, 0) and B.needs_angle("m15") and not B.needs_angle("m15a0") and not B.needs_angle("g2")
    for bad in ("g0", "g0.0", "g-1", "g10.5", "g", "g1.6k8", "g1.6k65", "g1.6k0", "g1.6 ", " g1.6", "G1.6", "g1.6k", "g1e0", "m14", "m1", "m65",
                "m15a180", "m15a-1", "m15a30.5", "m15a", "m", "a4x1", "a4x0r30", "a4x1r180", "a0x1r30", "a4x1r30k14", "a11x1r0", "box31", ""):
        with pytest.raises(ValueError) as e:
            B.parse_psf(bad)
        assert "g<sigma>[k<K>]" in str(e.value) and len(str(e.value).splitlines()) == 1, bad
    assert B.parse_de_type("blur_g1.6") == "g1.6" and B.parse_de_type("blur_m15a30") == "m15a30"
    assert B.parse_de_type("deblur") is None and B.parse_de_type("sr_bd_x3") is None and B.parse_de_type("jpeg_q10") is None
    for bad in ("blur", "blur_", "blurg1.6", "blur_g0", "blur_m14"):
        with pytest.raises(ValueError):
            B.parse_de_type(bad)
    assert B.psf_q_of("m15", 30).tolist() == B.psf_q_of("m15a30").tolist()
    with pytest.raises(ValueError):
        B.psf_q_of("m15")


# ------------------------------------------------------------------ the loader and the CLI on the double
def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(a).save(path)
    return a


def blur_folder(root):
    """two sharp images, 48 x 64 and 50 x 70 (cropped to 48 x 64 by the loader, to 48 x 63 as HR images of scale 3), and two listed
    denoise images -> (args, sharp images).  --blur_dir, --sr_dir and --jpeg_dir name the one folder"""
    imgs = {"a": _png(f"{root}/sharp/a.png", 48, 64, 51), "b": _png(f"{root}/sharp/b.png", 50, 70, 52)}
    for i in range(2):
        _png(f"{root}/Denoise/d{i}.png", 40 + i, 52, 60 + i)
    os.makedirs(f"{root}/lists/noisy")
    open(f"{root}/lists/noisy/denoise.txt", "w").write("d0.png\nd1.png\n")
    args = Namespace(de_type=["blur_g1.6"], blur_dir=f"{root}/sharp/", sr_dir=f"{root}/sharp/", jpeg_dir=f"{root}/sharp/",
                     data_file_dir=f"{root}/lists/", denoise_dir=f"{root}/Denoise/", patch_size=32)
    return args, imgs


def test_sample_ids_and_up_front_refusals(tmp_path):
    from rcot_amd import data as D
    from rcot_amd import tester as TS
    args, _ = blur_folder(str(tmp_path))
    ids = D.build_sample_ids(args)
    assert len(ids) == 10 and all(s["de"] == 5 and s["gt"] is None and s["blur"] == ("g1.6", "replicate") and "sr" not in s for s in ids)
    assert sorted({os.path.basename(s["file"]) for s in ids}) == ["a.png", "b.png"]
    assert D.FolderLoader._file_keys(ids[-1]) == [((ids[-1]["file"], "crop16"), ids[-1]["file"], 0)]
    assert D.FolderLoader._decode(ids[-1])[0].shape == (48, 64, 3)
    mix = Namespace(**{**vars(args), "de_type": ["blur_m15", "sr_bd_x3", "sr_x3", "blur_g2k15"], "blur_border": "wrap"})
    ids = D.build_sample_ids(mix)
    assert len(ids) == 40 and sorted({s.get("blur") for s in ids}, key=str) == [("g2k15", "wrap"), ("m15", "wrap"), None]
    bd = [s for s in ids if s.get("bd")]
    sr = [s for s in ids if s.get("sr") and not s.get("bd")]
    assert len(bd) == len(sr) == 10 and all(s["de"] == 7 and s["sr"] == 3 for s in bd + sr)
    assert D.FolderLoader._file_keys(bd[0]) == D.FolderLoader._file_keys([s for s in sr if s["file"] == bd[0]["file"]][0])   # one HR entry
    assert D.FolderLoader._decode(bd[-1])[0].shape == (48, 63, 3)                # crop16 of 50 x 70, then the multiple of 3
    for bad, word in ((dict(blur_dir=None), "--blur_dir"), (dict(de_type=["blur_g0"]), "g<sigma>"), (dict(de_type=["blur_m14"]), "odd in 3"),
                      (dict(de_type=["blurry"]), "blur_<spec>"), (dict(blur_border="zero"), "--blur_border"),
                      (dict(de_type=["sr_bd_x3"], sr_dir=None), "--sr_dir")):
        with pytest.raises(SystemExit, match=word):
            D.build_sample_ids(Namespace(**{**vars(args), **bad}))
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    one_line = lambda r, word: r.returncode != 0 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run("rcot_amd.trainer", "--de_type", "blur_g1.6", "--patch_size", "32")
    assert one_line(r, "--blur_dir"), r.stderr
    r = run("rcot_amd.trainer", "--de_type", "denoise_25", "blur_m14a30", "--blur_dir", args.blur_dir, "--patch_size", "32")
    assert one_line(r, "odd in 3"), r.stderr
    r = run("rcot_amd.trainer", "--de_type", "sr_bd_x3", "--sr_dir", args.sr_dir, "--synthetic", "--patch_size", "32")
    assert one_line(r, "--synthetic"), r.stderr
    # the tester: refused before the checkpoint or a GPU is touched
    for flags, word in ((["--blur", "g1.6", "--sr_scale", "2"], "--sr_scale"), (["--blur", "g1.6", "--noise_sigma", "25"], "--noise_sigma"),
                        (["--blur", "g1.6", "--jpeg_q", "10"], "--jpeg_q"), (["--blur", "g0"], "g<sigma>"), (["--blur", "m15"], "fixed angle"),
                        (["--sr_degradation", "bd"], "--sr_scale 3"), (["--sr_degradation", "bd", "--sr_scale", "2"], "--sr_scale 3"),
                        (["--sr_degradation", "bd", "--sr_scale", "3", "--sr_from", "lr"], "--sr_from target")):
        with pytest.raises(SystemExit, match=word) as e:
            TS.main(["--model", "/nonexistent/model.pth"] + flags)
        assert len(str(e.value).splitlines()) == 1
    for flags in (["--blur_border", "zero"], ["--sr_degradation", "gauss"]):
        with pytest.raises(SystemExit):
            TS.parser.parse_args(flags)
    o = TS.parser.parse_args([])
    assert o.blur is None and o.blur_border == "replicate" and o.sr_degradation == "bicubic"
    if not torch.cuda.is_available():
        r = run("rcot_amd.blur", "--in", args.blur_dir, "--out", str(tmp_path / "q"), "--psf", "g1.6")
        assert r.returncode != 0 and "No GPU found" in r.stderr and not (tmp_path / "q").exists(), r.stderr
    r = run("rcot_amd.blur", "--in", args.blur_dir, "--out", str(tmp_path / "q"), "--psf", "m15")
    assert one_line(r, "fixed angle") and not (tmp_path / "q").exists(), r.stderr


def bd_chain_np(hr):
    """the BD degradation restated: blur g1.6k7 (replicate), the centre of each 3 x 3 cell, the restated bicubic enlargement"""
    lr = BD.blur_np(hr, B.psf_q_of("g1.6k7"), "replicate")[1::3, 1::3]
    return RD.upscale_u8_np(np.ascontiguousarray(lr), hr.shape[0], hr.shape[1])


def loader_batches_match_restated_chain(tmp_path, backend, task):
    """FolderLoader with one blur task on the two images of ``blur_folder``: ``degraded`` is bit-equal to the crop and dihedral map of the
    restated whole-image degradation, / 255; ``clean`` to the crop of the sharp image.  The loader's draws are redone here, the angle of
    ``blur_m15`` included (shared with tests/test_blur_gpu.py)"""
    from rcot_amd import data as D
    from rcot_amd.resize import modcrop
    args, imgs = blur_folder(str(tmp_path))
    args.de_type = [task]
    args.blur_border = "mirror"
    loader = D.FolderLoader(args, 4, seed=5, backend=backend)
    assert len(loader) == 3                                                    # 10 samples / 4
    dbl = BD.BlurDouble()
    chain, seen, angles = {}, 0, set()
    for it, ([names, de_id], deg, clean) in enumerate(loader):
        assert de_id.tolist() == [7 if task == "sr_bd_x3" else 5] * len(names) and deg.shape == clean.shape == (len(names), 3, 32, 32)
        for j, n in enumerate(names):
            # the loader's own draws (rcot_amd/data.py): crop origin, augmentation mode, noise seed, then the angle, in this order
            rng = random.Random((5 * 1_000_003 + 1) * 2_147_483_659 + it * 4 + j)
            img = np.ascontiguousarray(D.crop_to_multiple(imgs[n], 16))
            if task == "sr_bd_x3":
                img = np.ascontiguousarray(modcrop(img, 3))
            H, W = img.shape[:2]
            assert (H, W) == ((48, 63) if task == "sr_bd_x3" else (48, 64))
            y0, x0, mode = rng.randint(0, H - 32), rng.randint(0, W - 32), rng.randint(1, 7)
            rng.getrandbits(63)
            if task == "sr_bd_x3":
                key, make = n, lambda: bd_chain_np(img)
            elif task == "blur_m15":
                angle = rng.randint(0, 179)
                angles.add(angle)
                key, make = (n, angle), lambda: BD.blur_np(img, B.psf_q_of("m15", angle), "mirror")
            else:
                key, make = n, lambda: BD.blur_np(img, B.psf_q_of(task[5:]), "mirror")
            if key not in chain:
                chain[key] = make()
            d, c = torch.empty(3, 32, 32), torch.empty(3, 32, 32)
            dbl.patch_prep(torch.from_numpy(img), torch.from_numpy(chain[key]), y0, x0, 32, mode, 0.0, 1, d, c)
            assert torch.equal(deg[j].cpu(), d) and torch.equal(clean[j].cpu(), c), (it, j, n)
            assert not torch.equal(d, c)
            seen += 1
    assert seen == 10 and (task != "blur_m15" or len(angles) > 5)


@pytest.mark.parametrize("task", ["blur_g1.6", "blur_m15", "blur_m15a30", "sr_bd_x3"])
def test_folder_loader_on_cpu_double(tmp_path, task):
    loader_batches_match_restated_chain(tmp_path, BD.BlurDouble(), task)


CACHE_LISTS = [["blur_g1.6"], ["blur_m15"], ["sr_bd_x3", "sr_x3"], ["blur_g2k15", "jpeg_q10", "denoise_25"]]


def cached_equals_uncached(tmp_path, backend, de_type, count):
    """two epochs of the cached loader against the uncached one, bit for bit.  The twins of fixed PSFs and of BD are made in the first
    epoch, once per file, under (path, "blur", spec, border) and (path, "bd", 3); a ``blur_m<L>`` twin is made per sample and not kept,
    its sharp image is.  ``count()``: whole-image blurs so far (shared with the GPU tier)"""
    from rcot_amd import data as D
    from rcot_amd.imagecache import DeviceImageCache
    args, _ = blur_folder(str(tmp_path))
    args.de_type = de_type
    fixed = [t[5:] for t in de_type if t.startswith("blur_") and not B.needs_angle(t[5:])]
    drawn = [t for t in de_type if t.startswith("blur_") and B.needs_angle(t[5:])]
    bd = int("sr_bd_x3" in de_type)
    kept = 2 * (len(fixed) + bd)
    cache = DeviceImageCache(backend, 1 << 30)
    cached = D.FolderLoader(args, 4, seed=5, backend=backend, threads=2, cache=cache)
    n0 = count()
    first = list(cached)
    assert count() - n0 == kept + 10 * len(drawn) and cache.blur_degradations == kept
    second = list(cached)
    assert count() - n0 == kept + 20 * len(drawn) and cache.blur_degradations == kept       # the second epoch keeps none anew
    files = sorted(os.path.join(args.blur_dir, n) for n in ("a.png", "b.png"))
    assert sorted(k for k in cache.keys() if k[1] == "blur") == sorted((f, "blur", s, "replicate") for f in files for s in fixed)
    assert sorted(k for k in cache.keys() if k[1] == "bd") == [(f, "bd", 3) for f in files] * bd
    assert sorted(k for k in cache.keys() if len(k) == 4 and k[2] == "mod") == [(f, "crop16", "mod", 3) for f in files] * bd   # one HR entry
    if fixed or drawn or "jpeg_q10" in de_type:
        assert all((f, "crop16") in cache for f in files)                         # the sharp image stays, also of blur_m15
    assert cache.sr_degradations == (2 if "sr_x3" in de_type else 0)
    tail = f"{cache.sr_degradations} sr degradations" + (", 2 jpeg degradations" if "jpeg_q10" in de_type else "")
    assert cache.report().endswith(tail + (f", {kept} blur degradations" if kept else ""))
    n0 = count()
    plain = D.FolderLoader(args, 4, seed=5, backend=backend, threads=2)
    want = [b for _ in range(2) for b in plain]
    assert count() - n0 == 2 * 10 * (len(fixed) + len(drawn) + bd)                # once per blur sample, two epochs
    got = first + second
    assert len(got) == len(want) == 2 * len(plain) and len(plain) == -(-10 * len(de_type) // 4)
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
    assert not torch.equal(first[0][1], second[0][1])                            # the second epoch is another epoch


@pytest.mark.parametrize("de_type", CACHE_LISTS, ids=lambda d: "+".join(d))
def test_cached_loader_equals_uncached_on_cpu_double(tmp_path, de_type):
    be = BD.BlurDouble()
    cached_equals_uncached(tmp_path, be, de_type, lambda: be.blurs)


def test_cache_report_is_unchanged_without_blur_samples():
    from rcot_amd.imagecache import DeviceImageCache
    c = DeviceImageCache(BD.BlurDouble(), 1 << 20)
    assert c.blur_degradations == 0 and c.report().endswith("0 misses, 0 sr degradations")
    c.jpeg_degradations = 3
    assert c.report().endswith("0 sr degradations, 3 jpeg degradations")
    c.blur_degradations = 2
    assert c.report().endswith("0 sr degradations, 3 jpeg degradations, 2 blur degradations")


def test_bd_chain_and_device_psf_on_cpu_double():
    be = BD.BlurDouble()
    hr = contents(48, 63, 16)["smooth"]
    t = torch.from_numpy(hr)
    lr = B.bd_downscale_u8(t, be).numpy()
    assert lr.shape == (16, 21, 3) and np.array_equal(lr, BD.blur_np(hr, B.psf_q_of("g1.6k7"), "replicate")[1::3, 1::3])
    assert np.array_equal(B.bd_degrade_u8(t, be).numpy(), bd_chain_np(hr)) and be.blurs == 2
    for bad in (hr[:47], hr[:, :62], hr[:0]):
        with pytest.raises(ValueError, match="multiple of 3"):
            B.bd_degrade_u8(torch.from_numpy(np.ascontiguousarray(bad)), be)
    q = B.psf_q_of("g1.6k7")
    assert B.device_psf(q, be.device) is B.device_psf(q.copy(), be.device)       # one copy per (device, PSF bytes)
    assert B.device_psf(q, be.device) is not B.device_psf(B.psf_q_of("g1.6"), be.device)
    with pytest.raises(ValueError):
        B.blur_degrade_u8(t, q, "zero", be)
    with pytest.raises(ValueError):
        B.blur_degrade_u8(t, q + 1, "wrap", be)                                  # the sum is checked before the upload
    assert be.blurs == 2
    assert np.array_equal(B.blur_degrade_u8(t, q, "wrap", be).numpy(), BD.blur_np(hr, q, "wrap"))


def test_folder_cli_on_cpu_double(tmp_path):
    """python -m rcot_amd.blur's ``main`` on a three-image folder, in both modes (the 2 x 40 image is smaller than a BD cell: skipped)"""
    from PIL import Image
    src = tmp_path / "in"
    imgs = {"a.png": _png(str(src / "a.png"), 24, 40, 1), "b.jpg.png": _png(str(src / "b.jpg.png"), 17, 10, 2), "c.png": _png(str(src / "c.png"), 2, 40, 3)}
    os.makedirs(src / "sub")                                                     # a folder inside is passed over
    be = BD.BlurDouble()
    assert B.main(["--in", str(src), "--out", str(tmp_path / "blur"), "--psf", "m15a30", "--border", "wrap"], backend=be) == 3
    assert sorted(os.listdir(tmp_path / "blur")) == sorted(imgs)
    for n, a in imgs.items():
        assert np.array_equal(np.array(Image.open(tmp_path / "blur" / n)), BD.blur_np(a, B.psf_q_of("m15a30"), "wrap")), n
    assert B.main(["--in", str(src), "--out", str(tmp_path / "bd"), "--mode", "bd", "--psf", "ignored"], backend=be) == 2
    assert sorted(os.listdir(tmp_path / "bd")) == ["a.png", "b.jpg.png"]
    for n, (h, w) in (("a.png", (24, 39)), ("b.jpg.png", (15, 9))):
        got = np.array(Image.open(tmp_path / "bd" / n))
        assert got.shape == (h, w, 3) and np.array_equal(got, bd_chain_np(np.ascontiguousarray(imgs[n][:h, :w]))), n
    for argv, word in ((["--psf", "g0"], "g<sigma>"), (["--psf", "m15"], "fixed angle"), ([], "--psf")):
        with pytest.raises(SystemExit, match=word):
            B.main(["--in", str(src), "--out", str(tmp_path / "bad")] + argv, backend=be)
    assert not (tmp_path / "bad").exists()
