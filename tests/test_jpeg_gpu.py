"""GPU tier of the compression-artifact task: rcot_jpeg_roundtrip against the numpy restatement (tests/jpeg_double.py, itself equal to
Pillow on libjpeg-turbo: tests/test_jpeg_cpu.py), byte for byte, on guard-banded, pre-poisoned buffers (tests/guarded.py); its
refusals; determinism and alignment; the folder loader with and without the device cache; the trainer CLI and the tester CLI with the
jpeg flags."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_double as JD
from conftest import ROOT
from guarded import GuardSet
from rcot_amd import jpeg as J
from rcot_amd import params as P
from test_jpeg_cpu import cached_equals_uncached, contents, loader_batches_match_restated_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _run(hip, img, q, sub, offset=0):
    """one guarded call -> the result on the host.  The workspace is exactly rcot_jpeg_ws_bytes long and poisoned, the source is
    compared afterwards; ``offset``: bytes by which src and dst are shifted off their alignment"""
    gs = GuardSet("cuda")
    h, w = img.shape[:2]
    src = gs.empty(img.size + offset, dtype=torch.uint8, name="src")[offset:].view(h, w, 3)
    src.copy_(torch.from_numpy(img))
    dst = gs.empty(img.size + offset, dtype=torch.uint8, name="dst")[offset:].view(h, w, 3)
    ws = gs.empty(max(hip.jpeg_ws_bytes(h, w, sub), 1), dtype=torch.uint8, name="ws")
    got = hip.jpeg_roundtrip(src, q, sub, out=dst, ws=ws)
    gs.check()
    assert got.data_ptr() == dst.data_ptr() and np.array_equal(src.cpu().numpy(), img)
    return dst.cpu().numpy()


# the CPU list without 1 x 1 and 16 x 16; 24 x 1040: many MCUs along a row, an even height that is no multiple of 16; 321 x 481;
# 128 x 2064: 8 x 33 tiles at 4:2:0 and 16 x 33 at 4:4:4 — more workgroups than CUs — with a last tile column of 16 pixels
SHAPES = [(7, 5), (8, 8), (17, 17), (9, 16), (15, 33), (2, 40), (40, 56), (97, 123), (24, 1040), (321, 481), (128, 2064)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_roundtrip_equals_the_double_byte_for_byte(hip, shape):
    h, w = shape
    imgs = contents(h, w, 7 * h + w)
    kinds = ("noise", "sat", "smooth") if h * w <= 100 * 130 else ("sat", "smooth")     # sat: the one that reaches the inverse DCT's clamp
    for sub in (0, 2):
        for q, kind in zip((1, 10, 40, 100), kinds * 2):
            want = JD.roundtrip_np(imgs[kind], q, sub)
            got = _run(hip, imgs[kind], q, sub)
            assert np.array_equal(got, want), (sub, q, kind, int((got != want).sum()))
    if h * w <= 100 * 130:                                                                # every quality on the saturated image
        for sub in (0, 2):
            for q in (1, 10, 40, 100):
                assert np.array_equal(_run(hip, imgs["sat"], q, sub), JD.roundtrip_np(imgs["sat"], q, sub)), (sub, q)


def test_refusals_leave_the_output_untouched(hip):
    gs = GuardSet("cuda")
    img = contents(16, 24, 3)["noise"]
    src = gs.tensor(torch.from_numpy(img), name="src")
    dst = gs.empty((16, 24, 3), dtype=torch.uint8, name="dst")
    need = hip.jpeg_ws_bytes(16, 24, 2)
    assert need > 0 and hip.jpeg_ws_bytes(16, 24, 0) == 0
    ws = gs.empty(need, dtype=torch.uint8, name="ws")
    before, ws_before = dst.clone(), ws.clone()
    call = lambda s, d, H, W, q, sub, w_, n: hip.L.rcot_jpeg_roundtrip(s, d, H, W, q, sub, w_, n, hip._st())
    p = lambda t: t.data_ptr()
    ok = (p(src), p(dst), 16, 24, 10, 2, p(ws), need)
    bad = [ok[:0] + (None,) + ok[1:], ok[:1] + (None,) + ok[2:]]                           # src, dst null
    bad += [ok[:2] + (0,) + ok[3:], ok[:2] + (-4,) + ok[3:], ok[:3] + (0,) + ok[4:], ok[:3] + (-4,) + ok[4:]]       # H, W < 1
    bad += [ok[:4] + (v,) + ok[5:] for v in (0, 101, -1, 1000)]                             # quality outside 1 .. 100
    bad += [ok[:5] + (v,) + ok[6:] for v in (1, 3, -1, 420)]                                # no such subsampling
    bad += [ok[:6] + (None, need), ok[:7] + (need - 1,), ok[:7] + (0,)]                     # 4:2:0: no workspace, one byte short, none
    bad += [ok[:3] + (v,) + ok[4:] for v in (4, 3, 1)]                                      # 4:2:0 with W <= 4
    for args in bad:
        assert call(*args) == -1, args
    for name, fn in (("ws_bytes", lambda: hip.jpeg_ws_bytes(0, 8, 2)), ("ws_bytes", lambda: hip.jpeg_ws_bytes(8, 8, 1)),
                     ("roundtrip", lambda: hip.jpeg_roundtrip(src, 0, 2, out=dst, ws=ws)),
                     ("roundtrip", lambda: hip.jpeg_roundtrip(src[:, :4].contiguous(), 10, 2))):
        from rcot_amd import lib
        with pytest.raises(lib.RcotKernelError, match="invalid argument"):
            fn()
    with pytest.raises(ValueError, match="wider than 4"):
        J.jpeg_degrade_u8(src[:, :4].contiguous(), 10, 2, hip)
    gs.check()
    assert torch.equal(dst, before) and torch.equal(ws, ws_before)                          # nothing was launched
    assert call(*ok) == 0                                                                    # the same arguments, whole, run
    assert call(*(ok[:5] + (0, None, 0))) == 0                                               # 4:4:4 takes no workspace
    assert call(*(ok[:3] + (4, 10, 0, None, 0))) == 0                                        # and any width
    gs.check()
    from rcot_amd import lib
    assert lib.ABI_VERSION >= 32


def test_determinism_streams_and_alignment(hip):
    img = contents(50, 70, 9)["smooth"]
    for sub in (0, 2):
        want = JD.roundtrip_np(img, 10, sub)
        d = torch.from_numpy(img).cuda()
        outs = []
        for _ in range(2):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            ws = torch.empty(max(hip.jpeg_ws_bytes(50, 70, sub), 1), dtype=torch.uint8, device="cuda")      # a workspace per stream
            with torch.cuda.stream(s):
                outs.append(hip.jpeg_roundtrip(d, 10, sub, ws=ws))
            s.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), want) and torch.equal(outs[0], outs[1])
        assert np.array_equal(_run(hip, img, 10, sub, offset=1), want)                      # one byte off the 16-byte alignment
    assert np.array_equal(J.jpeg_degrade_u8(torch.from_numpy(img).cuda(), 10).cpu().numpy(), JD.roundtrip_np(img, 10, 2))   # the defaults


def test_folder_loader_on_the_device(hip, tmp_path):
    loader_batches_match_restated_chain(tmp_path, hip)


@pytest.mark.parametrize("de_type", [["jpeg_q10"], ["jpeg_q10", "jpeg_q40", "denoise_25"]], ids=lambda d: "+".join(d))
def test_cached_loader_equals_uncached_on_the_device(hip, tmp_path, monkeypatch, de_type):
    count = [0]
    real = J.jpeg_degrade_u8

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(J, "jpeg_degrade_u8", counted)
    cached_equals_uncached(tmp_path, hip, de_type, lambda: count[0])


def _u8(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("cache", ["off", "device"])
def test_trainer_cli_jpeg(tmp_path, cache):
    """--de_type jpeg_q10 on one 64 x 96 image: 5 samples, two iterations of one epoch at P = 32, finite losses"""
    from PIL import Image
    os.makedirs(tmp_path / "clean")
    Image.fromarray(_u8(60, 64, 96)).save(tmp_path / "clean" / "a.png")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--de_type", "jpeg_q10", "--jpeg_dir", str(tmp_path / "clean"), "--patch_size", "32",
           "--batchSize", "3", "--nEpochs", "1", "--pairnum", "10000000", "--seed", "4", "--type", "CAR", "--sigma", "1", "--degset",
           str(tmp_path / "none") + "/", "--tarset", str(tmp_path / "none") + "/", "--data_cache", cache, "--data_cache_gb", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "...total sample ids: 5" in r.stdout and "Epoch 1(0/2)" in r.stdout
    losses = [float(v) for v in re.findall(r"Loss_\w+: ([-+0-9.eEnaif]+)", r.stdout)]
    assert len(losses) >= 2 and np.isfinite(losses).all(), r.stdout[-2000:]
    lines = re.findall(r"^data cache: (\d+) images, .* (\d+) sr degradations, (\d+) jpeg degradations$", r.stdout, flags=re.M)
    assert lines == ([("2", "0", "1")] if cache == "device" else []), r.stdout[-2000:]      # the image and its twin, made once


def test_tester_cli_jpeg(hip, tmp_path):
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
    r = TS.main(base + dirs("f") + ["--jpeg_q", "10", "--savedeg", str(tmp_path / "f" / "DEG")])
    assert r["images"] == 2 and np.isfinite(r["psnr"])
    for n, a in tars.items():
        assert np.array_equal(png("f", "DEG", n), JD.roundtrip_np(a, 10, 2)), n            # the "JPEG" baseline = the restated round trip
        assert np.array_equal(png("f", "TAR", n), a) and png("f", "OUT", n).shape == a.shape
    rd = TS.main(base + dirs("d") + ["--jpeg_q", "10", "--metrics", "device"])
    assert rd["images"] == 2
    for key in ("psnr", "ssim", "psnr_best", "ssim_best", "psnr_worst", "ssim_worst"):
        assert abs(rd[key] - r[key]) < 1e-9, (key, rd[key], r[key])
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("d", sub, n) == raw("f", sub, n), (sub, n)
    r4 = TS.main(base + dirs("s") + ["--jpeg_q", "10", "--jpeg_subsampling", "444", "--savedeg", str(tmp_path / "s" / "DEG")])
    assert r4["images"] == 2 and np.array_equal(png("s", "DEG", "b.png"), JD.roundtrip_np(tars["b.png"], 10, 0))
    # the saved input as --degset, without the flag: the same outputs, and --jpeg_q 0 is the flag left out
    plain = ["--model", ck, "--tarset", str(tmp_path / "tar") + "/", "--degset", str(tmp_path / "f" / "DEG") + "/"]
    r0, r1 = TS.main(plain + dirs("z0") + ["--jpeg_q", "0"]), TS.main(plain + dirs("z1"))
    assert r0 == r1 and r0["images"] == 2 and abs(r0["psnr"] - r["psnr"]) < 1e-9
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("z0", sub, n) == raw("z1", sub, n), (sub, n)
        assert np.array_equal(png("z0", "OUT", n), png("f", "OUT", n)), n
