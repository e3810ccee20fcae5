"""CPU tier of the compression-artifact task: the numpy restatement of the JPEG round trip (tests/jpeg_double.py, written from the rule in
csrc/jpeg.hip) against Pillow on libjpeg-turbo, byte for byte; the quantisation tables; the sample lists, the ``jpeg_q<Q>`` names, every
up-front refusal and the cache keys; the folder loader and the folder CLI on a CPU double of the backend."""
import os
import random
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import jpeg_double as JD
from conftest import ROOT
from rcot_amd import jpeg as J

SHAPES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 17), (9, 16), (15, 33), (2, 40), (40, 56), (97, 123), (321, 481)]
QUALITIES = (1, 10, 40, 50, 75, 100)


def contents(h, w, seed):
    """name -> uint8 [h, w, 3]: uniform noise, random 0 / 255 (reaches the clamp of the inverse DCT), smooth + noise, constant"""
    g = np.random.Generator(np.random.PCG64(seed))
    smooth = 128 + 60 * np.sin(np.linspace(0, 6, h))[:, None, None] * np.cos(np.linspace(0, 5, w))[None, :, None] + g.normal(0, 4, (h, w, 3))
    return {"noise": g.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "sat": (g.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8),
            "smooth": np.clip(smooth, 0, 255).astype(np.uint8), "const": np.full((h, w, 3), 77, dtype=np.uint8)}


def _need_turbo():
    from PIL import features
    if not features.check("libjpeg_turbo"):
        pytest.skip("Pillow is not built on libjpeg-turbo: the byte-for-byte oracle of the JPEG round trip is that codec")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow_byte_for_byte(shape):
    _need_turbo()
    h, w = shape
    n = 0
    for name, img in contents(h, w, 100 * h + w).items():
        for q in QUALITIES:
            for sub in (0, 2):
                if sub == 2 and w <= 4:                                          # 1 x 1: 4:4:4 only
                    continue
                got, want = JD.roundtrip_np(img, q, sub), JD.pil_roundtrip(img, q, sub)
                assert got.dtype == np.uint8 and got.shape == img.shape
                assert np.array_equal(got, want), (name, q, sub, int((got != want).sum()))
                n += 1
    assert n == (24 if w <= 4 else 48)


def test_even_heights_pad_the_downsampled_plane():
    """4:2:0 at H = 8, 24, 40: replicating the last DOWNSAMPLED chroma row is not replicating full-resolution rows; Pillow agrees with
    the former"""
    _need_turbo()
    for h in (8, 24, 40):
        img = contents(h, 24, h)["noise"]
        assert np.array_equal(JD.roundtrip_np(img, 75, 2), JD.pil_roundtrip(img, 75, 2)), h


@pytest.mark.parametrize("q", [1, 10, 49, 50, 90, 100])
def test_quant_tables_equal_pillows(q):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=q)
    qt = Image.open(io.BytesIO(buf.getvalue())).quantization
    luma, chroma = J.quant_tables(q)
    assert list(qt[0]) == luma and list(qt[1]) == chroma
    assert len(luma) == len(chroma) == 64 and min(luma + chroma) >= 1 and max(luma + chroma) <= 255


def test_quality_and_name_parsing():
    assert J.parse_de_type("jpeg_q10") == 10 and J.parse_de_type("jpeg_q1") == 1 and J.parse_de_type("jpeg_q100") == 100
    assert J.parse_de_type("denoise_25") is None and J.parse_de_type("sr_x4") is None and J.parse_de_type("single") is None
    for bad in ("jpeg_q0", "jpeg_q101", "jpeg_q", "jpeg_10", "jpeg", "jpeg_q1x", "jpeg_q-5", "jpeg_q10 ", "jpegq10"):
        with pytest.raises(ValueError):
            J.parse_de_type(bad)
    for bad in (0, 101, -1, 10.5):
        with pytest.raises(ValueError):
            J.quant_tables(bad)
    be = JD.JpegDouble()
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        J.jpeg_degrade_u8(img, 10, 1, be)                                        # 4:2:2 is not offered
    with pytest.raises(ValueError, match="wider than 4"):
        J.jpeg_degrade_u8(img[:, :4].contiguous(), 10, 2, be)
    assert be.roundtrips == 0
    assert tuple(J.jpeg_degrade_u8(img[:, :4].contiguous(), 10, 0, be).shape) == (8, 4, 3)


def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(a).save(path)
    return a


def jpeg_folder(root):
    """two clean images, 48 x 64 and 50 x 70 (cropped to 48 x 64 by the loader), and two listed denoise images -> (args, clean images)"""
    imgs = {"a": _png(f"{root}/clean/a.png", 48, 64, 31), "b": _png(f"{root}/clean/b.png", 50, 70, 32)}
    for i in range(2):
        _png(f"{root}/Denoise/d{i}.png", 40 + i, 52, 40 + i)
    os.makedirs(f"{root}/lists/noisy")
    open(f"{root}/lists/noisy/denoise.txt", "w").write("d0.png\nd1.png\n")
    args = Namespace(de_type=["jpeg_q10"], jpeg_dir=f"{root}/clean/", data_file_dir=f"{root}/lists/", denoise_dir=f"{root}/Denoise/",
                     patch_size=32)
    return args, imgs


def test_sample_ids_and_up_front_refusals(tmp_path):
    from rcot_amd import data as D
    from rcot_amd import tester as TS
    args, _ = jpeg_folder(str(tmp_path))
    ids = D.build_sample_ids(args)
    assert len(ids) == 10 and all(s["de"] == 7 and s["gt"] is None and s["jpeg"] == (10, 2) and "sr" not in s for s in ids)   # `single`, x5
    assert sorted({os.path.basename(s["file"]) for s in ids}) == ["a.png", "b.png"]
    mix = Namespace(**{**vars(args), "de_type": ["jpeg_q10", "jpeg_q40", "denoise_25"], "jpeg_subsampling": "444"})
    ids = D.build_sample_ids(mix)
    assert len(ids) == 30 and sorted({s.get("jpeg") for s in ids}, key=str) == [(10, 0), (40, 0), None]
    assert D.FolderLoader._decode(ids[-1])[0].shape == (48, 64, 3)               # crop16 of 50 x 70, nothing else
    assert D.FolderLoader._file_keys(ids[-1]) == [((ids[-1]["file"], "crop16"), ids[-1]["file"], 0)]
    for bad, word in ((dict(jpeg_dir=None), "--jpeg_dir"), (dict(de_type=["jpeg_q0"]), "1 .. 100"), (dict(de_type=["jpeg_10"]), "jpeg_q<Q>"),
                      (dict(jpeg_subsampling="422"), "--jpeg_subsampling")):
        with pytest.raises(SystemExit, match=word):
            D.build_sample_ids(Namespace(**{**vars(args), **bad}))
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    one_line = lambda r, word: r.returncode != 0 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run("rcot_amd.trainer", "--de_type", "jpeg_q10", "--patch_size", "32")
    assert one_line(r, "--jpeg_dir"), r.stderr
    r = run("rcot_amd.trainer", "--de_type", "jpeg_q10", "--jpeg_dir", args.jpeg_dir, "--synthetic", "--patch_size", "32")
    assert one_line(r, "--synthetic"), r.stderr
    r = run("rcot_amd.trainer", "--de_type", "denoise_25", "jpeg_q101", "--jpeg_dir", args.jpeg_dir, "--patch_size", "32")
    assert one_line(r, "1 .. 100"), r.stderr
    r = run("rcot_amd.trainer", "--de_type", "jpeg_quality10", "--jpeg_dir", args.jpeg_dir, "--patch_size", "32")
    assert one_line(r, "jpeg_q<Q>"), r.stderr
    # the tester: refused before the checkpoint or a GPU is touched
    for flags, word in ((["--jpeg_q", "10", "--sr_scale", "2"], "--sr_scale"), (["--jpeg_q", "10", "--noise_sigma", "25"], "--noise_sigma"),
                        (["--jpeg_q", "101"], "1 .. 100"), (["--jpeg_q", "-1"], "1 .. 100")):
        with pytest.raises(SystemExit, match=word):
            TS.main(["--model", "/nonexistent/model.pth"] + flags)
    with pytest.raises(SystemExit):
        TS.parser.parse_args(["--jpeg_subsampling", "422"])
    o = TS.parser.parse_args([])
    assert o.jpeg_q == 0 and o.jpeg_subsampling == "420"
    if not torch.cuda.is_available():
        r = run("rcot_amd.jpeg", "--in", args.jpeg_dir, "--out", str(tmp_path / "q"), "--quality", "10")
        assert r.returncode != 0 and "No GPU found" in r.stderr and not (tmp_path / "q").exists(), r.stderr
    r = run("rcot_amd.jpeg", "--in", args.jpeg_dir, "--out", str(tmp_path / "q"), "--quality", "0")
    assert one_line(r, "1 .. 100") and not (tmp_path / "q").exists(), r.stderr


def loader_batches_match_restated_chain(tmp_path, backend, subsampling="420"):
    """FolderLoader with jpeg_q10 on the two images of ``jpeg_folder``: ``degraded`` is bit-equal to the crop and dihedral map of the
    PIL round trip of the whole (crop16) image, / 255; ``clean`` to the crop of the clean image (shared with tests/test_jpeg_gpu.py)"""
    from rcot_amd import data as D
    args, imgs = jpeg_folder(str(tmp_path))
    args.jpeg_subsampling = subsampling
    loader = D.FolderLoader(args, 4, seed=5, backend=backend)
    assert len(loader) == 3                                                    # 10 samples / 4
    dbl = JD.JpegDouble()
    chain, seen = {}, 0
    for it, ([names, de_id], deg, clean) in enumerate(loader):
        assert de_id.tolist() == [7] * len(names) and deg.shape == clean.shape == (len(names), 3, 32, 32)
        for j, n in enumerate(names):
            # the loader's own draws (rcot_amd/data.py): crop origin, augmentation mode, noise seed, in this order
            rng = random.Random((5 * 1_000_003 + 1) * 2_147_483_659 + it * 4 + j)
            img = np.ascontiguousarray(D.crop_to_multiple(imgs[n], 16))
            assert img.shape == (48, 64, 3)
            y0, x0, mode = rng.randint(0, 48 - 32), rng.randint(0, 64 - 32), rng.randint(1, 7)
            if n not in chain:
                chain[n] = JD.pil_roundtrip(img, 10, J.SUBSAMPLING[subsampling])
            d, c = torch.empty(3, 32, 32), torch.empty(3, 32, 32)
            dbl.patch_prep(torch.from_numpy(img), torch.from_numpy(chain[n]), y0, x0, 32, mode, 0.0, 1, d, c)
            assert torch.equal(deg[j].cpu(), d) and torch.equal(clean[j].cpu(), c), (it, j, n)
            assert not torch.equal(d, c)
            seen += 1
    assert seen == 10


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_folder_loader_on_cpu_double(tmp_path, subsampling):
    _need_turbo()
    loader_batches_match_restated_chain(tmp_path, JD.JpegDouble(), subsampling)


def cached_equals_uncached(tmp_path, backend, de_type, count):
    """two epochs of the cached loader against the uncached one, bit for bit; the degraded twins are made in the first epoch, once per
    (file, quality), under the keys (path, "jpeg", Q, S).  ``count()``: whole-image round trips so far (shared with the GPU tier)"""
    from rcot_amd import data as D
    from rcot_amd.imagecache import DeviceImageCache
    args, _ = jpeg_folder(str(tmp_path))
    args.de_type = de_type
    qs = [J.parse_de_type(t) for t in de_type if J.parse_de_type(t)]
    cache = DeviceImageCache(backend, 1 << 30)
    cached = D.FolderLoader(args, 4, seed=5, backend=backend, threads=2, cache=cache)
    n0 = count()
    first = list(cached)
    assert count() - n0 == 2 * len(qs) == cache.jpeg_degradations and cache.sr_degradations == 0
    second = list(cached)
    assert count() - n0 == 2 * len(qs) == cache.jpeg_degradations               # the second epoch makes none
    files = sorted(os.path.join(args.jpeg_dir, n) for n in ("a.png", "b.png"))
    assert sorted(k for k in cache.keys() if k[1] == "jpeg") == sorted((f, "jpeg", q, 2) for f in files for q in qs)
    assert all((f, "crop16") in cache for f in files)
    assert cache.report().endswith(f"0 sr degradations, {2 * len(qs)} jpeg degradations")
    n0 = count()
    plain = D.FolderLoader(args, 4, seed=5, backend=backend, threads=2)
    want = [b for _ in range(2) for b in plain]
    assert count() - n0 == 2 * 10 * len(qs)                                      # once per jpeg sample, two epochs
    got = first + second
    assert len(got) == len(want) == 2 * len(plain) and len(plain) == -(-(10 * len(qs) + (10 if "denoise_25" in de_type else 0)) // 4)
    for k, (([n1, l1], d1, c1), ([n2, l2], d2, c2)) in enumerate(zip(got, want)):
        assert n1 == n2 and torch.equal(l1, l2), k
        assert torch.equal(d1, d2) and torch.equal(c1, c2), k
    assert not torch.equal(first[0][1], second[0][1])                            # the second epoch is another epoch


@pytest.mark.parametrize("de_type", [["jpeg_q10"], ["jpeg_q10", "jpeg_q40", "denoise_25"]], ids=lambda d: "+".join(d))
def test_cached_loader_equals_uncached_on_cpu_double(tmp_path, de_type):
    be = JD.JpegDouble()
    cached_equals_uncached(tmp_path, be, de_type, lambda: be.roundtrips)


def test_cache_report_is_unchanged_without_jpeg_samples():
    from rcot_amd.imagecache import DeviceImageCache
    c = DeviceImageCache(JD.JpegDouble(), 1 << 20)
    assert c.jpeg_degradations == 0 and c.report().endswith("0 misses, 0 sr degradations")


def test_folder_cli_on_cpu_double(tmp_path):
    """python -m rcot_amd.jpeg's ``main`` on a three-image folder (one of them 4 pixels wide: skipped at 4:2:0, written at 4:4:4)"""
    from PIL import Image
    src = tmp_path / "in"
    imgs = {"a": _png(str(src / "a.png"), 24, 40, 1), "b": _png(str(src / "b.jpg.png"), 17, 9, 2), "c": _png(str(src / "c.png"), 9, 4, 3)}
    os.makedirs(src / "sub")                                                     # a folder inside is passed over
    be = JD.JpegDouble()
    assert J.main(["--in", str(src), "--out", str(tmp_path / "o420"), "--quality", "20"], backend=be) == 2
    assert sorted(os.listdir(tmp_path / "o420")) == ["a.png", "b.jpg.png"]
    assert J.main(["--in", str(src), "--out", str(tmp_path / "o444"), "--quality", "40", "--subsampling", "444"], backend=be) == 3
    for out, q, sub, names in (("o420", 20, 2, ("a", "b")), ("o444", 40, 0, ("a", "b", "c"))):
        for n in names:
            fn = {"a": "a.png", "b": "b.jpg.png", "c": "c.png"}[n]
            assert np.array_equal(np.array(Image.open(tmp_path / out / fn)), JD.roundtrip_np(imgs[n], q, sub)), (out, n)
    with pytest.raises(SystemExit, match="1 .. 100"):
        J.main(["--in", str(src), "--out", str(tmp_path / "bad"), "--quality", "101"], backend=be)
