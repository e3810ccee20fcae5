"""GPU tier of the super-resolution task: rcot_resize_axis against the numpy fp32 restatement of its arithmetic, bit for bit, on
guard-banded, pre-poisoned buffers (tests/guarded.py); its refusals; ``imresize`` against the REFERENCE's outputs
(tests/golden/resize.npz); the 8-bit chain; the folder loader, the trainer CLI and the tester CLI with the sr flags."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_double as RD
from conftest import ROOT
from guarded import GuardSet
from rcot_amd import params as P
from rcot_amd import resize as RZ
from test_resize_cpu import loader_batches_match_restated_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _src(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-0.2, 1.2, size=shape).astype(np.float32)


def _run(hip, src, axis, idx, taps, offset=0):
    """one guarded launch -> the result on the host; ``offset``: floats by which src and dst are shifted off their 16-byte alignment"""
    gs = GuardSet("cuda")
    out_len = idx.shape[0]
    oshape = (src.shape[0], out_len, src.shape[2]) if axis == 0 else (src.shape[0], src.shape[1], out_len)
    s = gs.empty(src.size + offset, name="src")[offset:].view(src.shape)
    s.copy_(torch.from_numpy(src))
    d = gs.empty(int(np.prod(oshape)) + offset, name="dst")[offset:].view(oshape)          # poisoned: the band pattern, NaN as fp32
    i = gs.tensor(torch.from_numpy(idx), name="idx")
    t = gs.tensor(torch.from_numpy(taps), name="taps")
    got = hip.resize_axis(s, axis, i, t, out=d)
    gs.check()
    assert got.data_ptr() == d.data_ptr()
    return d.cpu().numpy()


# (planes, H, W), axis, out_len.  The fixture's sizes on both axes (K = 18, 14, 10 shrinking, 6 enlarging; W = 36 takes the float4 rows,
# W = 9 and 5 the scalar ones); odd sizes where nothing is a multiple of 4; one-pixel axes; 259 columns (crosses the 256-wide tile of both
# forms); K = 34 (the 64-tap register form); 40 x 1300 shrunk x4 along the columns (a span of ~1030 pixels: 7 rows per LDS image, several
# images per band); 1028 columns (a second float4 segment of one lane); and the two enlargements of a 339 x 510 x 3 image to DIV2K's
# 1356 x 2040, the sizes the loader runs: thousands of workgroups dealt to the XCDs in runs of rows, 15 image rows per workgroup of the
# column form.
AXIS_CASES = [((3, 48, 36), 0, 12), ((3, 48, 36), 0, 16), ((3, 48, 36), 0, 24), ((3, 48, 36), 1, 9), ((3, 48, 36), 1, 12),
              ((3, 48, 36), 1, 18), ((3, 12, 9), 0, 48), ((3, 12, 9), 1, 36), ((3, 7, 5), 0, 27), ((3, 7, 5), 1, 18),
              ((3, 1, 7), 0, 4), ((3, 1, 7), 1, 21), ((3, 7, 1), 0, 21), ((3, 7, 1), 1, 4),
              ((2, 5, 259), 1, 1036), ((2, 5, 259), 0, 20), ((2, 64, 64), 0, 8), ((2, 64, 64), 1, 8), ((1, 40, 1300), 1, 325),
              ((1, 6, 1028), 0, 3), ((3, 339, 2040), 0, 1356), ((3, 1356, 510), 1, 2040)]


@pytest.mark.parametrize("case", AXIS_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}x{c[0][2]}-axis{c[1]}-{c[2]}")
def test_resize_axis_bit_equal(hip, case):
    shape, axis, out_len = case
    src = _src(sum(shape) + 7 * axis + out_len, shape)
    idx, w, _ = RZ.cubic_taps(shape[1 + axis], out_len)
    taps = w.astype(np.float32)
    want = RD.resize_axis_np(src, axis, idx, taps)
    got = _run(hip, src, axis, idx, taps)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if shape[2] % 4 == 0:                                                      # the same rows off their alignment: the scalar form
        assert np.array_equal(_run(hip, src, axis, idx, taps, offset=1).view(np.uint32), want.view(np.uint32))


def test_resize_axis_clamps_a_malformed_table(hip):
    """indices outside [0, n) are clamped, not read: the result equals the restatement (which clamps), the source's guard bands (NaN as
    fp32) never surface; and a table that is no resampling table — a tile whose span exceeds the LDS image — takes the direct reads"""
    src = _src(5, (2, 12, 9))
    for axis in (0, 1):
        idx, w, _ = RZ.cubic_taps(src.shape[1 + axis], 30)
        idx = idx.copy()
        idx[0, 0], idx[3, 2], idx[7, 5], idx[29, 1] = -5, 10 ** 6, -2 ** 31, 2 ** 31 - 1
        taps = np.ascontiguousarray(np.full_like(w, 0.25) + w, dtype=np.float32)        # every tap counts
        got = _run(hip, src, axis, idx, taps)
        assert np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), RD.resize_axis_np(src, axis, idx, taps).view(np.uint32))
    # outputs that each read 6 pixels of a 600-pixel window, 10 pixels on per output: a span of ~3150 pixels, so two rows per LDS
    # image, two images per band of four rows, and a last band of three rows (images of two rows and of one)
    g = np.random.Generator(np.random.PCG64(8))
    src = _src(9, (1, 11, 3200))
    idx = (np.arange(256)[:, None] * 10 + g.integers(0, 600, size=(256, 6))).astype(np.int32)
    taps = g.uniform(-0.5, 1.0, size=(256, 6)).astype(np.float32)
    got = _run(hip, src, 1, idx, taps)
    assert np.array_equal(got.view(np.uint32), RD.resize_axis_np(src, 1, idx, taps).view(np.uint32))
    g = np.random.Generator(np.random.PCG64(6))
    src = _src(7, (1, 3, 9000))
    idx = g.integers(0, 9000, size=(300, 6)).astype(np.int32)
    idx[0, 0], idx[1, 0] = 0, 8999
    taps = g.uniform(-0.5, 1.0, size=(300, 6)).astype(np.float32)
    got = _run(hip, src, 1, idx, taps)
    assert np.array_equal(got.view(np.uint32), RD.resize_axis_np(src, 1, idx, taps).view(np.uint32))


def test_refusals_leave_the_output_untouched(hip):
    from rcot_amd import lib
    gs = GuardSet("cuda")
    src = gs.tensor(torch.from_numpy(_src(1, (2, 8, 8))), name="src")
    idx_h, w, _ = RZ.cubic_taps(8, 4)
    idx, taps = gs.tensor(torch.from_numpy(idx_h), name="idx"), gs.tensor(torch.from_numpy(w.astype(np.float32)), name="taps")
    wide = gs.full((4, 65), 0, dtype=torch.int32, name="idx65"), gs.full((4, 65), 0.0, name="taps65")
    dst = gs.empty((2, 4, 8), name="dst")
    before = dst.view(torch.int32).clone()
    K = idx_h.shape[1]
    call = lambda s, d, planes, H, W, axis, out_len, i, t, k: hip.L.rcot_resize_axis(s, d, planes, H, W, axis, out_len, i, t, k, hip._st())
    p = lambda t: t.data_ptr()
    EINVAL, EUNSUPPORTED = -1, lib.EUNSUPPORTED
    ok = (p(src), p(dst), 2, 8, 8, 0, 4, p(idx), p(taps), K)
    bad = []
    for pos in (0, 1, 7, 8):                                                    # each pointer null
        bad.append((EINVAL, ok[:pos] + (None,) + ok[pos + 1:]))
    for pos in (2, 3, 4, 6, 9):                                                 # planes, H, W, out_len, K < 1
        bad.append((EINVAL, ok[:pos] + (0,) + ok[pos + 1:]))
        bad.append((EINVAL, ok[:pos] + (-3,) + ok[pos + 1:]))
    bad += [(EINVAL, ok[:5] + (2,) + ok[6:]), (EINVAL, ok[:5] + (-1,) + ok[6:])]          # axis outside {0, 1}
    bad.append((EUNSUPPORTED, ok[:7] + (p(wide[0]), p(wide[1]), 65)))                      # K > 64
    bad.append((EUNSUPPORTED, ok[:3] + (65536, 32768, 0, 4) + ok[7:]))                     # a source plane of 2^31 elements
    bad.append((EUNSUPPORTED, ok[:3] + (8, 1 << 20, 0, 4096) + ok[7:]))                    # a destination plane of 2^32 elements
    bad.append((EUNSUPPORTED, ok[:3] + (1 << 20, 8, 1, 4096) + ok[7:]))
    for want, args in bad:
        assert call(*args) == want, args
    with pytest.raises(lib.RcotKernelError, match="no kernel for this shape"):
        hip.resize_axis(src, 0, *wide, out=dst)
    gs.check()
    assert torch.equal(dst.view(torch.int32), before)                           # nothing was launched
    assert call(*ok) == 0                                                       # and the same arguments, whole, run
    torch.cuda.synchronize()
    gs.check()
    assert bool(torch.isfinite(dst).all())


def test_imresize_vs_reference_fixture(hip, gold):
    """<= 5e-6 on each orientation's sound region (the bound of the fp32 restatement, tests/test_resize_cpu.py), every pixel checked"""
    fx = gold("resize.npz")
    worst = 0.0
    for i, ((H, W), (oh, ow)) in enumerate(RD.CASES):
        x = torch.from_numpy(RD.case_input(i).astype(np.float32) / np.float32(255))[None].cuda()
        got = RZ.imresize(x, oh, ow, hip)
        assert tuple(got.shape) == (1, oh, ow)
        got = got[0].cpu().numpy().astype(np.float64)
        seen = np.zeros((oh, ow), dtype=bool)
        for k, (fr, fc) in enumerate(RD.ORIENTATIONS):
            m = RD.sound_mask(H, W, oh, ow, fr, fc)
            if m.any():
                worst = max(worst, float(np.abs(got - fx[f"ref_{i}"][k])[m].max()))
            seen |= m
        assert seen.all()
    print(f"imresize on the device vs the reference, worst over the sound regions: {worst:.1e}")
    assert worst <= 5e-6


def _u8(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_8bit_chain_bit_equal(hip):
    for seed, (h, w, s) in enumerate([(48, 64, 4), (48, 63, 3), (50, 70, 2), (8, 12, 4)]):
        img = _u8(40 + seed, h, w)
        got = RZ.sr_degrade_u8(torch.from_numpy(img).cuda(), s, hip)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
        assert np.array_equal(got.cpu().numpy(), RD.degrade_u8_np(img, s)), (h, w, s)
    for seed, (h, w, oh, ow) in enumerate([(12, 9, 48, 36), (5, 7, 15, 21), (1, 1, 4, 4)]):
        img = _u8(50 + seed, h, w)
        got = RZ.sr_upscale_u8(torch.from_numpy(img).cuda(), oh, ow, hip)
        assert np.array_equal(got.cpu().numpy(), RD.upscale_u8_np(img, oh, ow)), (h, w, oh, ow)
    with pytest.raises(ValueError, match="multiple of 3"):
        RZ.sr_degrade_u8(torch.from_numpy(_u8(1, 48, 64)).cuda(), 3, hip)


@pytest.mark.parametrize("scale", [4, 3])
def test_folder_loader_on_the_device(hip, tmp_path, scale):
    loader_batches_match_restated_chain(tmp_path, hip, scale)


def test_trainer_cli_sr(tmp_path):
    """--de_type sr_x2 on one 64 x 96 image: 5 samples, 3 iterations of one epoch through the recorded launch plans (the loader's
    launches stay outside them: rcot_amd/data.py asserts it), finite losses, a checkpoint"""
    from PIL import Image
    hr = tmp_path / "hr"
    hr.mkdir()
    Image.fromarray(_u8(60, 64, 96)).save(hr / "a.png")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--de_type", "sr_x2", "--sr_dir", str(hr), "--patch_size", "32", "--batchSize", "2",
           "--nEpochs", "1", "--pairnum", "10000000", "--seed", "4", "--type", "SR", "--sigma", "1", "--degset", str(tmp_path / "none") + "/",
           "--tarset", str(tmp_path / "none") + "/"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "...total sample ids: 5" in r.stdout and "Epoch 1(0/3)" in r.stdout
    losses = [float(v) for v in re.findall(r"Loss_\w+: ([-+0-9.eEnaif]+)", r.stdout)]
    assert len(losses) >= 3 and np.isfinite(losses).all(), r.stdout[-2000:]
    assert os.path.isfile(tmp_path / "checkpoint" / "model_SR__1_1.0.pth")


def test_tester_cli_sr(hip, tmp_path):
    from PIL import Image
    from rcot_amd import tester as TS
    from rcot_amd.compat import shim
    tars = {"a.png": _u8(70, 32, 48), "b.png": _u8(71, 43, 50)}                  # b: cropped to 40 x 48 for x4
    os.makedirs(tmp_path / "tar")
    for n, a in tars.items():
        Image.fromarray(a).save(tmp_path / "tar" / n)
    ck = str(tmp_path / "net.pth")
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()}
    torch.save({"epoch": 1, "Tnet": shim().T_net.from_state_dict(prm, decoder=True)}, ck)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres",
                        str(tmp_path / tag / "RES") + "/"]
    base = ["--model", ck, "--tarset", str(tmp_path / "tar") + "/"]
    raw = lambda tag, sub, n: open(tmp_path / tag / sub / n, "rb").read()
    png = lambda tag, sub, n: np.array(Image.open(tmp_path / tag / sub / n))
    # from the target: --degset names a folder that does not exist and is not read
    r = TS.main(base + dirs("t") + ["--degset", str(tmp_path / "nowhere") + "/", "--sr_scale", "4", "--savedeg", str(tmp_path / "t" / "DEG")])
    assert r["images"] == 2 and np.isfinite(r["psnr"])
    for n, a in tars.items():
        crop = np.ascontiguousarray(a[:a.shape[0] - a.shape[0] % 4, :a.shape[1] - a.shape[1] % 4])
        assert np.array_equal(png("t", "DEG", n), RD.degrade_u8_np(crop, 4)), n                  # the bicubic baseline = the restated chain
        assert np.array_equal(png("t", "TAR", n), crop) and png("t", "OUT", n).shape == crop.shape
    # from LR images made by the module's own `down` mode: the same outputs, byte for byte
    assert RZ.main(["--in", str(tmp_path / "tar"), "--out", str(tmp_path / "lr"), "--scale", "4", "--mode", "down"]) == 2
    assert png("", "lr", "b.png").shape == (10, 12, 3)
    assert np.array_equal(png("", "lr", "a.png"), RD.downscale_u8_np(tars["a.png"], 4))
    r2 = TS.main(base + dirs("l") + ["--degset", str(tmp_path / "lr") + "/", "--sr_scale", "4", "--sr_from", "lr"])
    assert r2["images"] == 2 and r2["psnr"] == r["psnr"]
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("l", sub, n) == raw("t", sub, n), (sub, n)
    # `up` and `degrade` modes of the module against the chain
    assert RZ.main(["--in", str(tmp_path / "lr"), "--out", str(tmp_path / "up"), "--scale", "4", "--mode", "up"]) == 2
    assert RZ.main(["--in", str(tmp_path / "tar"), "--out", str(tmp_path / "dg"), "--scale", "4", "--mode", "degrade"]) == 2
    for n in tars:
        assert raw("", "up", n) == raw("", "dg", n) and np.array_equal(png("", "dg", n), png("t", "DEG", n))
    # --sr_scale 0 is the flag left out
    plain = ["--model", ck, "--tarset", str(tmp_path / "t" / "TAR") + "/", "--degset", str(tmp_path / "t" / "DEG") + "/"]
    r3, r4 = TS.main(plain + dirs("z0") + ["--sr_scale", "0"]), TS.main(plain + dirs("z1"))
    assert r3 == r4 and r3["images"] == 2
    for n in tars:
        for sub in ("OUT", "TAR", "RES"):
            assert raw("z0", sub, n) == raw("z1", sub, n), (sub, n)
