"""GPU tier of the deblurring tasks: rcot_blur_u8 against the numpy restatement (tests/blur_double.py; tests/test_blur_cpu.py holds it
against an independent filter), byte for byte, on guard-banded, pre-poisoned buffers (tests/guarded.py; the PSF is guarded too); step and
phase; its refusals; determinism and alignment; the folder loader with and without the device cache; the trainer CLI and the tester CLI
with the blur flags.

The shapes are chosen for the tile of blur_tile_kernel, 32 rows x 256 BYTES of the image's rows (85 1/3 pixels: a tile need not start on
a pixel): 33 x 86 is one row and two bytes past one tile, 32 x 256 exactly 1 x 3 tiles, 64 x 520 is 2 x 7 tiles with a last tile column
of 24 bytes, and 352 x 2064 (in the place of the issue's 128 x 2064, which is only 100 of these tiles) is 11 x 25 = 275 tiles, more
workgroups than the 256 CUs; it runs g1.6k7 and m31a77 only.  Every other shape runs every PSF under all three borders; on 64 x 520 the
two widest PSFs have a case of their own per border, to keep every case short (test_wide_psfs_on_a_row_of_tiles)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import blur_double as BD
from conftest import ROOT
from guarded import GuardSet
from rcot_amd import blur as B
from rcot_amd import params as P
from test_blur_cpu import (CACHE_LISTS, bd_chain_np, box, cached_equals_uncached, contents, delta, loader_batches_match_restated_chain)

pytestmark = pytest.mark.gpu

BORDERS = ("replicate", "mirror", "wrap")


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _run(hip, img, q, border, step=1, phase=0, offset=0):
    """one guarded call -> the result on the host.  The destination is poisoned, the source and the PSF are compared afterwards;
    ``offset``: bytes by which src and dst are shifted off their alignment"""
    gs = GuardSet("cuda")
    h, w = img.shape[:2]
    oh, ow = h // step, w // step
    src = gs.empty(img.size + offset, dtype=torch.uint8, name="src")[offset:].view(h, w, 3)
    src.copy_(torch.from_numpy(img))
    dst = gs.empty(oh * ow * 3 + offset, dtype=torch.uint8, name="dst")[offset:].view(oh, ow, 3)
    psf = gs.tensor(torch.from_numpy(np.array(q)), name="psf")                 # a writable copy: psf_q_of hands out views of cached bytes
    got = hip.blur_u8(src, psf, BD.BORDERS[border], step, phase, out=dst)
    gs.check()
    assert got.data_ptr() == dst.data_ptr() and np.array_equal(src.cpu().numpy(), img) and np.array_equal(psf.cpu().numpy(), q)
    return dst.cpu().numpy()


def _psfs(h, w):
    """(name, weights, image kind or None = rotate) for an h x w image: g1.6k7 and m31a77 on the largest shape, everything elsewhere —
    on 64 x 520 the two widest PSFs run in test_wide_psfs_on_a_row_of_tiles"""
    q = B.quantise_psf
    if (h, w) == BIG:
        return [("g1.6k7", B.psf_q_of("g1.6k7"), None), ("m31a77", B.psf_q_of("m31a77"), None)]
    out = [("delta1", q(delta(1, 0, 0)), None), ("g1.6k7", B.psf_q_of("g1.6k7"), None), ("aniso15", q(B.psf_gaussian_aniso(15, 4.0, 1.5, 30)), None),
           ("m15a30", B.psf_q_of("m15a30"), None), ("m31a77", B.psf_q_of("m31a77"), None), ("first31", q(delta(31, 0, 0)), None),
           ("last31", q(delta(31, 30, 30)), None)]
    if (h, w) != ROW_OF_TILES:
        out += WIDE()
    return out


def WIDE():
    return [("g5k31", B.psf_q_of("g5k31"), None), ("box63", B.quantise_psf(box(63)), "sat")]   # box63 on 0 / 255: the largest accumulator


ROW_OF_TILES, BIG = (64, 520), (352, 2064)
SHAPES = [(1, 1), (7, 5), (3, 40), (40, 3), (17, 17), (33, 86), (32, 256), (97, 123), ROW_OF_TILES, BIG]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_equals_the_double_byte_for_byte(hip, shape):
    h, w = shape
    imgs = contents(h, w, 7 * h + w)
    kinds = ("noise", "sat", "smooth")
    n = 0
    for name, q, kind in _psfs(h, w):
        for border in BORDERS:
            k = kind or kinds[n % 3]
            n += 1
            want = BD.blur_np(imgs[k], q, border)
            got = _run(hip, imgs[k], q, border)
            assert got.shape == want.shape and np.array_equal(got, want), (name, border, k, int((got != want).sum()))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("which", [0, 1], ids=["g5k31", "box63"])
def test_wide_psfs_on_a_row_of_tiles(hip, which, border):
    """64 x 520, the shape of test_blur_equals_the_double_byte_for_byte with seven tiles along a row and a last tile of 24 bytes, under
    the two widest PSFs (the largest halo, the largest accumulator): one case per PSF and border"""
    h, w = ROW_OF_TILES
    name, q, kind = WIDE()[which]
    k = kind or ("noise", "sat", "smooth")[BORDERS.index(border)]
    img = contents(h, w, 7 * h + w)[k]
    want = BD.blur_np(img, q, border)
    got = _run(hip, img, q, border)
    assert np.array_equal(got, want), (name, border, k, int((got != want).sum()))


@pytest.mark.parametrize("shape", [(9, 12), (96, 123), (66, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_step_and_phase(hip, shape):
    h, w = shape
    imgs = contents(h, w, 3 * h + w)
    ran = 0
    for step, phase in ((3, 1), (2, 0), (2, 1)):
        if h % step or w % step:
            continue
        for (name, q), border, kind in zip((("g1.6k7", B.psf_q_of("g1.6k7")), ("m15a30", B.psf_q_of("m15a30")), ("g2k15", B.psf_q_of("g2k15"))),
                                           BORDERS, ("noise", "sat", "smooth")):
            want = BD.blur_np(imgs[kind], q, border, step, phase)
            got = _run(hip, imgs[kind], q, border, step, phase)
            assert got.shape == (h // step, w // step, 3) and np.array_equal(got, want), (name, border, step, phase)
            ran += 1
    assert ran >= 3
    if h % 3 == 0 and w % 3 == 0:                                               # the BD protocol's own call
        d = torch.from_numpy(imgs["smooth"]).cuda()
        assert np.array_equal(B.bd_downscale_u8(d, hip).cpu().numpy(), BD.blur_np(imgs["smooth"], B.psf_q_of("g1.6k7"), "replicate", 3, 1))
        assert np.array_equal(B.bd_degrade_u8(d, hip).cpu().numpy(), bd_chain_np(imgs["smooth"]))


def test_refusals_leave_the_output_untouched(hip):
    from rcot_amd import lib
    gs = GuardSet("cuda")
    img = contents(18, 24, 3)["noise"]
    src = gs.tensor(torch.from_numpy(img), name="src")
    dst = gs.empty((18, 24, 3), dtype=torch.uint8, name="dst")
    q = B.psf_q_of("g1.6k7")
    psf = gs.tensor(torch.from_numpy(np.array(q)), name="psf")
    big = gs.empty((65, 65), dtype=torch.int32, name="psf65")
    before = dst.clone()
    call = lambda *a: hip.L.rcot_blur_u8(*a, hip._st())
    p = lambda t: t.data_ptr()
    ok = (p(src), p(dst), 18, 24, p(psf), 7, 0, 1, 0)                            # src, dst, H, W, psf, K, border, step, phase
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    bad = [sub(0, None), sub(1, None), sub(4, None)]                             # a null pointer
    bad += [sub(2, 0), sub(2, -18), sub(3, 0), sub(3, -24)]                      # H or W < 1
    bad += [sub(5, 0), sub(5, -7), sub(5, 6), sub(5, 8), sub(5, 64)]             # K even or < 1
    bad += [sub(6, -1), sub(6, 3), sub(6, 100)]                                  # no such border
    bad += [sub(7, 0), sub(7, -3)]                                               # step < 1
    bad += [sub(8, 1), sub(8, -1), ok[:7] + (3, 3), ok[:7] + (3, -1), ok[:7] + (2, 2)]          # phase outside [0, step)
    bad += [ok[:7] + (4, 0), ok[:7] + (5, 0), ok[:7] + (9, 0), ok[:2] + (20, 24) + ok[4:7] + (3, 1)]   # H or W no multiple of step
    for args in bad:
        assert call(*args) == -1, args
    unsupported = [ok[:4] + (p(big), 65) + ok[6:], ok[:4] + (p(big), 127) + ok[6:],           # K > 63
                   ok[:2] + (26755, 26755) + ok[4:], ok[:2] + (1, 715827883) + ok[4:]]        # 2^31 bytes or more
    for args in unsupported:
        assert call(*args) == lib.EUNSUPPORTED, args
    with pytest.raises(lib.RcotKernelError, match="invalid argument"):
        hip.blur_u8(src, psf, 3)
    with pytest.raises(lib.RcotKernelError, match="invalid argument"):
        hip.blur_u8(src, psf, 0, step=4)
    with pytest.raises(lib.RcotKernelError, match="no kernel for this shape"):
        hip.blur_u8(src, big, 0)
    with pytest.raises(lib.RcotKernelError, match="contiguous"):
        hip.blur_u8(src[:, ::2], psf, 0)                                          # a non-contiguous image
    with pytest.raises(lib.RcotKernelError, match="contiguous"):
        hip.blur_u8(src.permute(1, 0, 2), psf, 0)
    with pytest.raises(lib.RcotKernelError, match="PSF"):
        hip.blur_u8(src, psf.t(), 0)
    with pytest.raises(lib.RcotKernelError, match="PSF"):
        hip.blur_u8(src, psf.float(), 0)
    with pytest.raises(lib.RcotKernelError, match="expected 6 x 8"):
        hip.blur_u8(src, psf, 0, step=3, phase=1, out=dst)
    with pytest.raises(ValueError):
        B.blur_degrade_u8(src, q - 1, "replicate", hip)                          # the weight contract, checked on the host
    gs.check()
    assert torch.equal(dst, before)                                              # nothing was launched
    assert call(*ok) == 0                                                        # the same arguments, whole, run
    assert np.array_equal(dst.cpu().numpy(), BD.blur_np(img, q, "replicate"))
    small = gs.empty((6, 8, 3), dtype=torch.uint8, name="dst3")
    assert call(p(src), p(small), 18, 24, p(psf), 7, 2, 3, 2) == 0               # phase step - 1
    assert np.array_equal(small.cpu().numpy(), BD.blur_np(img, q, "wrap", 3, 2))
    assert call(p(src), p(dst), 1, 18 * 24, p(psf), 7, 1, 1, 0) == 0             # the same bytes as one row
    gs.check()
    assert lib.ABI_VERSION >= 33


def test_determinism_streams_and_alignment(hip):
    img = contents(50, 70, 9)["smooth"]
    for q, border, step, phase in ((B.psf_q_of("g2k15"), "mirror", 1, 0), (B.psf_q_of("m31a77"), "wrap", 1, 0), (B.psf_q_of("g1.6k7"), "replicate", 2, 1)):
        want = BD.blur_np(img, q, border, step, phase)
        d, psf = torch.from_numpy(img).cuda(), B.device_psf(q, hip.device)
        torch.cuda.synchronize()
        outs = []
        for _ in range(2):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append(hip.blur_u8(d, psf, BD.BORDERS[border], step, phase))
            s.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), want) and torch.equal(outs[0], outs[1])
        assert np.array_equal(_run(hip, img, q, border, step, phase, offset=1), want)         # one byte off the alignment
        assert np.array_equal(_run(hip, img, q, border, step, phase, offset=3), want)
    assert np.array_equal(B.blur_degrade_u8(torch.from_numpy(img).cuda(), B.psf_q_of("g1.6")).cpu().numpy(),
                          BD.blur_np(img, B.psf_q_of("g1.6"), "replicate"))                    # the defaults
    assert B.device_psf(B.psf_q_of("g1.6"), hip.device) is B.device_psf(B.psf_q_of("g1.6").copy(), hip.device)


@pytest.mark.parametrize("task", ["blur_g1.6", "blur_m15", "sr_bd_x3"])
def test_folder_loader_on_the_device(hip, tmp_path, task):
    loader_batches_match_restated_chain(tmp_path, hip, task)


@pytest.mark.parametrize("de_type", CACHE_LISTS, ids=lambda d: "+".join(d))
def test_cached_loader_equals_uncached_on_the_device(hip, tmp_path, monkeypatch, de_type):
    count = [0]
    real = hip.blur_u8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(hip, "blur_u8", counted)
    cached_equals_uncached(tmp_path, hip, de_type, lambda: count[0])


def _u8(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("task,cache", [("blur_g1.6", "off"), ("blur_g1.6", "device"), ("sr_bd_x3", "device")])
def test_trainer_cli_blur(tmp_path, task, cache):
    """--de_type blur_g1.6 (resp. sr_bd_x3) on one 64 x 96 image: 5 samples, two iterations of one epoch at P = 32, finite losses"""
    from PIL import Image
    os.makedirs(tmp_path / "sharp")
    Image.fromarray(_u8(60, 64, 96)).save(tmp_path / "sharp" / "a.png")
    env = dict(os.environ, PYTHONPATH=ROOT)
    folder = ["--blur_dir", str(tmp_path / "sharp")] if task != "sr_bd_x3" else ["--sr_dir", str(tmp_path / "sharp")]
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--de_type", task, *folder, "--patch_size", "32",
           "--batchSize", "3", "--nEpochs", "1", "--pairnum", "10000000", "--seed", "4", "--type", "Deblur", "--sigma", "1", "--degset",
           str(tmp_path / "none") + "/", "--tarset", str(tmp_path / "none") + "/", "--data_cache", cache, "--data_cache_gb", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "...total sample ids: 5" in r.stdout and "Epoch 1(0/2)" in r.stdout
    losses = [float(v) for v in re.findall(r"Loss_\w+: ([-+0-9.eEnaif]+)", r.stdout)]
    assert len(losses) >= 2 and np.isfinite(losses).all(), r.stdout[-2000:]
    lines = re.findall(r"^data cache: (\d+) images, .* (\d+) sr degradations, (\d+) blur degradations$", r.stdout, flags=re.M)
    assert lines == ([("2", "0", "1")] if cache == "device" else []), r.stdout[-2000:]      # the image and its twin, made once
    assert "blur degradations" not in r.stdout or cache == "device"


def test_tester_cli_blur(hip, tmp_path):
    from PIL import Image
    from rcot_amd import tester as TS
    from rcot_amd.compat import shim
    tars = {"a.png": _u8(70, 32, 48), "b.png": _u8(71, 40, 56)}
    os.makedirs(tmp_path / "tar")
    for n, a in tars.items():
        Image.fromarray(a).save(tmp_path / "tar" / n)
    ck = str(tmp_path / "net.pth")
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()}
    torch.save({"epoch": 1, "Tnet": shim().T_net.from_state_dict(prm, decoder=True)}, ck)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres",
                        str(tmp_path / tag / "RES") + "/"]
    raw = lambda tag, sub, n: open(tmp_path / tag / sub / n, "rb").read()
    png = lambda tag, sub, n: np.array(Image.open(tmp_path / tag / sub / n))
    # --degset names a folder that does not exist and is not read
    base = ["--model", ck, "--tarset", str(tmp_path / "tar") + "/", "--degset", str(tmp_path / "nowhere") + "/"]
    r = TS.main(base + dirs("f") + ["--blur", "g1.6", "--savedeg", str(tmp_path / "f" / "DEG")])
    assert r["images"] == 2 and np.isfinite(r["psnr"])
    for n, a in tars.items():
        assert np.array_equal(png("f", "DEG", n), BD.blur_np(a, B.psf_q_of("g1.6"), "replicate")), n     # the "blurred" baseline
        assert np.array_equal(png("f", "TAR", n), a) and png("f", "OUT", n).shape == a.shape
    rd = TS.main(base + dirs("d") + ["--blur", "g1.6", "--metrics", "device"])
    assert rd["images"] == 2
    for key in ("psnr", "ssim", "psnr_best", "ssim_best", "psnr_worst", "ssim_worst"):
        assert abs(rd[key] - r[key]) < 1e-9, (key, rd[key], r[key])
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("d", sub, n) == raw("f", sub, n), (sub, n)
    rw = TS.main(base + dirs("w") + ["--blur", "m15a30", "--blur_border", "wrap", "--savedeg", str(tmp_path / "w" / "DEG")])
    assert rw["images"] == 2 and np.array_equal(png("w", "DEG", "b.png"), BD.blur_np(tars["b.png"], B.psf_q_of("m15a30"), "wrap"))
    # the saved input as --degset, without the flag: the same outputs
    plain = ["--model", ck, "--tarset", str(tmp_path / "tar") + "/", "--degset", str(tmp_path / "f" / "DEG") + "/"]
    r0 = TS.main(plain + dirs("z0"))
    assert r0["images"] == 2 and abs(r0["psnr"] - r["psnr"]) < 1e-9
    for n in tars:
        assert np.array_equal(png("z0", "OUT", n), png("f", "OUT", n)), n
    # BD super-resolution: the targets are cropped to multiples of 3 (30 x 48, 39 x 54), padded for the network
    bd = ["--sr_scale", "3", "--sr_degradation", "bd", "--pad", "reflect"]
    rb = TS.main(base + dirs("b") + bd + ["--savedeg", str(tmp_path / "b" / "DEG")])
    assert rb["images"] == 2
    for n, a in tars.items():
        hr = np.ascontiguousarray(a[:a.shape[0] - a.shape[0] % 3, :a.shape[1] - a.shape[1] % 3])
        assert np.array_equal(png("b", "DEG", n), bd_chain_np(hr)) and np.array_equal(png("b", "TAR", n), hr), n
    rc = TS.main(base + dirs("c") + ["--sr_scale", "3", "--pad", "reflect", "--savedeg", str(tmp_path / "c" / "DEG")])      # bicubic: as before
    assert rc["images"] == 2 and not np.array_equal(png("c", "DEG", "a.png"), png("b", "DEG", "a.png"))
    # the saved BD input as --degset with the cropped targets: identical outputs
    plain_b = ["--model", ck, "--tarset", str(tmp_path / "b" / "TAR") + "/", "--degset", str(tmp_path / "b" / "DEG") + "/", "--pad", "reflect"]
    rz = TS.main(plain_b + dirs("zb"))
    assert rz["images"] == 2 and abs(rz["psnr"] - rb["psnr"]) < 1e-9
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("zb", sub, n) == raw("b", sub, n), (sub, n)
    for flags, word in ((["--blur", "g1.6", "--sr_scale", "3"], "--sr_scale"), (["--blur", "g1.6", "--jpeg_q", "10"], "--jpeg_q"),
                        (["--blur", "g1.6", "--noise_sigma", "25"], "--noise_sigma"), (["--sr_degradation", "bd", "--sr_scale", "2"], "--sr_scale 3")):
        with pytest.raises(SystemExit, match=word) as e:
            TS.main(base + flags)
        assert len(str(e.value).splitlines()) == 1
