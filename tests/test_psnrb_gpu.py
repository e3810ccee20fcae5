"""GPU tier of PSNR-B and the border shave: rcot_image_blockiness (csrc/quality.hip) against the host's integers
(rcot_amd/quality.py, which tests/test_psnrb_cpu.py holds to a plain double loop) on guard-banded buffers with a poisoned workspace
of exactly the size asked for, its reproducibility, byte alignment, workspace and argument rules, rcot_crop_u8 against the numpy
slice, and the tester CLI with --psnrb / --shave on both metric routes.  (tests/test_quality_gpu.py has no case beyond 2^31 bytes per
image, so there is none here.)"""
import os

import numpy as np
import pytest
import torch

from guarded import GuardSet, poison_workspaces
from rcot_amd import quality as Q
from test_psnrb_cpu import ORIGINS, SIZES as CPU_SIZES, SPACES, random_image

pytestmark = pytest.mark.gpu

BTH, BTW = 32, 63                                 # the kernel's tile (HipBackend.BLOCKINESS_TILE, asserted below)
# the CPU tier's sizes; rows of every byte phase; one tile less / more a pixel in each direction, two and four tiles; one image of
# Rain100L's size
SIZES = CPU_SIZES + [(17, 33), (31, 64), (33, 65), (64, 129)]
SIZES += [(BTH + dy, BTW + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (BTH + dy, BTW + dx) not in SIZES]
SIZES += [(321, 481)]
SENTINEL = -7


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    assert be.BLOCKINESS_TILE == (BTH, BTW)
    return be


def checkerboard(h, w):
    """0 / 255 in every channel, the largest sum a pair can give, and its inverse"""
    c = (((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2) * 255).astype(np.uint8)
    a = np.repeat(c[:, :, None], 3, axis=2)
    return a, 255 - a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(hip, ad, bd, h, w, space, oy, ox, stats, ws, ws_bytes):
    return hip.L.rcot_image_blockiness(ad.data_ptr(), bd.data_ptr(), h, w, space, oy, ox, stats.data_ptr(), ws.data_ptr(), ws_bytes, hip._st())


def _guarded_call(hip, G, ad, bd, h, w, space, oy, ox):
    """one call on guarded buffers: the statistics between two bands, the workspace exactly as long as asked for and full of NaN"""
    planes = 3 if space == "rgb" else 1
    need = hip.image_blockiness_ws_bytes(h, w, space)
    assert need % 8 == 0
    ws = G.empty(need // 4, torch.float32, "ws")                               # the band pattern: NaN as fp32
    stats = G.full((planes, 5), float(SENTINEL), torch.float64, "stats").view(torch.int64)
    assert _raw(hip, ad, bd, h, w, hip.SPACES[space], oy, ox, stats, ws, need) == 0
    return stats.cpu().numpy()


# ------------------------------------------------------------------ 1. the integers against the host
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_blockiness_equals_the_host(hip, size):
    h, w = size
    G = GuardSet("cuda")
    inputs = [("random", random_image(h * 1000 + w, h, w), random_image(h * 1000 + w + 1, h, w)), ("checker", *checkerboard(h, w))]
    for kind, a, b in inputs:
        ad, bd = G.tensor(torch.from_numpy(a), "a"), G.tensor(torch.from_numpy(b), "b")
        for space in SPACES:
            for oy, ox in ORIGINS:
                got = _guarded_call(hip, G, ad, bd, h, w, space, oy, ox)
                want = Q.blockiness_stats(a, b, space, oy, ox)
                assert got.dtype == want.dtype == np.int64 and np.array_equal(got, want), (kind, space, oy, ox, got.tolist(), want.tolist())
                assert Q.psnrb_from_sums(got, h, w, oy, ox) == Q.psnrb_u8(a, b, space, oy, ox)
                if kind == "checker":                                          # every pixel and every pair gives 255^2 (luma: 235 - 16)
                    v2 = (255 if space == "rgb" else 219) ** 2
                    assert got[0].tolist() == [h * w * v2] + [n * v2 for n in Q.blockiness_counts(h, w, oy, ox)]
    G.check()


# ------------------------------------------------------------------ 2. reproducibility, the wrapper
def test_blockiness_is_bitwise_reproducible(hip):
    h, w = 75, 139
    a, b = random_image(1, h, w), random_image(2, h, w)
    ad, bd = _dev(a), _dev(b)
    for space in SPACES:
        ws = torch.zeros(hip.image_blockiness_ws_bytes(h, w, space) // 4, device="cuda")
        first = hip.image_blockiness(ad, bd, space, 3, 5, ws=ws)
        second = hip.image_blockiness(ad, bd, space, 3, 5, ws=ws)
        ws.fill_(float("nan"))                                               # an unrelated launch dirties the workspace
        third = hip.image_blockiness(ad, bd, space, 3, 5, ws=ws)
        poison_workspaces(hip)
        own = hip.image_blockiness(ad, bd, space, 3, 5)                      # the backend's workspace
        assert first.dtype == torch.int64 and tuple(first.shape) == (3 if space == "rgb" else 1, 5)
        for other in (second, third, own):
            assert torch.equal(first, other), space
        assert np.array_equal(first.cpu().numpy(), Q.blockiness_stats(a, b, space, 3, 5))
        assert torch.equal(hip.image_blockiness(ad, bd, space), torch.from_numpy(Q.blockiness_stats(a, b, space)).cuda())


def test_images_at_any_byte_alignment(hip):
    """views that start 1, 2 and 3 bytes into an allocation: the first and the last dword of an image then straddle its ends; the bytes
    around the images are 255, so that one of them picked up by mistake shows"""
    for h, w in ((11, 12), (37, 70), (33, 65)):
        a, b = random_image(h + w, h, w) // 2, random_image(h + w + 1, h, w) // 2
        n = h * w * 3
        for oa, ob in ((1, 3), (2, 0), (3, 2), (0, 1)):
            bufa, bufb = torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda"), torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda")
            av, bv = bufa[oa:oa + n].view(h, w, 3), bufb[ob:ob + n].view(h, w, 3)
            av.copy_(_dev(a))
            bv.copy_(_dev(b))
            assert av.data_ptr() % 4 == oa and bv.data_ptr() % 4 == ob
            for space in SPACES:
                got = hip.image_blockiness(av, bv, space, 3, 5).cpu().numpy()
                assert np.array_equal(got, Q.blockiness_stats(a, b, space, 3, 5)), (h, w, oa, ob, space)


# ------------------------------------------------------------------ 3. workspace and argument rules
def test_workspace_rule(hip):
    from rcot_amd.lib import RcotKernelError
    h, w = 37, 70
    a, b = random_image(5, h, w), random_image(6, h, w)
    ad, bd = _dev(a), _dev(b)
    for space, planes in (("rgb", 3), ("y", 1)):
        need = hip.image_blockiness_ws_bytes(h, w, space)
        assert need == 40 * planes * 2 * 2                                   # ceil(37 / 32) x ceil(70 / 63) tiles
        ws = torch.zeros(need // 4 + 2, device="cuda")
        stats = torch.full((planes, 5), SENTINEL, dtype=torch.int64, device="cuda")
        assert _raw(hip, ad, bd, h, w, hip.SPACES[space], 0, 0, stats, ws, need - 1) == -2
        assert _raw(hip, ad, bd, h, w, hip.SPACES[space], 0, 0, stats, ws[1:], need) == -2      # 4 bytes off an 8-byte boundary
        torch.cuda.synchronize()
        assert bool((stats == SENTINEL).all())                               # nothing was launched
        assert _raw(hip, ad, bd, h, w, hip.SPACES[space], 0, 0, stats, ws, need) == 0
        assert np.array_equal(stats.cpu().numpy(), Q.blockiness_stats(a, b, space))
        with pytest.raises(RcotKernelError, match="workspace too small"):
            hip.image_blockiness(ad, bd, space, ws=ws[: need // 4 - 1])
        assert torch.equal(hip.image_blockiness(ad, bd, space, ws=ws[: need // 4]), stats)


def test_invalid_arguments(hip):
    from rcot_amd.lib import RcotKernelError
    h, w = 12, 20
    ad, bd = _dev(random_image(7, h, w)), _dev(random_image(8, h, w))
    ws = torch.zeros(64, device="cuda")
    stats = torch.full((3, 5), SENTINEL, dtype=torch.int64, device="cuda")
    L, st = hip.L, hip._st()
    for space, oy, ox, hh, ww in ((2, 0, 0, h, w), (-1, 0, 0, h, w), (0, 8, 0, h, w), (0, 0, 8, h, w), (0, -1, 0, h, w), (1, 0, -1, h, w),
                                  (0, 0, 0, 0, w), (0, 0, 0, h, 0), (0, 0, 0, -3, w)):
        assert _raw(hip, ad, bd, hh, ww, space, oy, ox, stats, ws, 256) == -1
    assert L.rcot_image_blockiness(None, bd.data_ptr(), h, w, 0, 0, 0, stats.data_ptr(), ws.data_ptr(), 256, st) == -1
    assert L.rcot_image_blockiness(ad.data_ptr(), None, h, w, 0, 0, 0, stats.data_ptr(), ws.data_ptr(), 256, st) == -1
    assert L.rcot_image_blockiness(ad.data_ptr(), bd.data_ptr(), h, w, 0, 0, 0, None, ws.data_ptr(), 256, st) == -1
    assert L.rcot_image_blockiness(ad.data_ptr(), bd.data_ptr(), h, w, 0, 0, 0, stats.data_ptr(), None, 256, st) == -1
    assert L.rcot_image_blockiness(ad.data_ptr(), bd.data_ptr(), h, w, 0, 0, 0, stats.data_ptr() + 4, ws.data_ptr(), 256, st) == -1    # misaligned
    dst = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
    for y0, x0, hc, wc in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (11, 0, 2, 2), (0, 19, 2, 2), (0, 0, 13, 2), (12, 20, 1, 1)):
        assert L.rcot_crop_u8(ad.data_ptr(), h, w, y0, x0, hc, wc, dst.data_ptr(), st) == -1
    assert L.rcot_crop_u8(None, h, w, 0, 0, 2, 2, dst.data_ptr(), st) == -1 and L.rcot_crop_u8(ad.data_ptr(), h, w, 0, 0, 2, 2, None, st) == -1
    torch.cuda.synchronize()
    assert bool((stats == SENTINEL).all()) and bool((dst == 9).all())
    with pytest.raises(RcotKernelError, match="invalid argument"):
        hip.image_blockiness(ad, bd, "ycbcr")
    with pytest.raises(RcotKernelError, match="invalid argument"):
        hip.image_blockiness(ad, bd, "y", 8, 0)
    with pytest.raises(RcotKernelError, match="expected 12 x 20"):
        hip.image_blockiness(ad, bd[:, :19].contiguous(), "rgb")
    with pytest.raises(RcotKernelError, match="uint8"):
        hip.image_blockiness(ad.float(), bd, "rgb")
    with pytest.raises(RcotKernelError, match="leaves the 12 x 20 image"):
        hip.crop_u8(ad, 1, 1, 12, 5)


# ------------------------------------------------------------------ 4. the crop
def test_crop_u8_equals_the_slice(hip):
    G = GuardSet("cuda")
    for h, w in ((12, 20), (33, 47), (75, 139)):
        img = random_image(h * w, h, w)
        src = G.tensor(torch.from_numpy(img), "src")
        # the whole image; starts at every byte phase of the source (x0 = 0 .. 3) with odd and even row lengths; one pixel; one column
        for y0, x0, hc, wc in ((0, 0, h, w), (1, 1, h - 2, w - 2), (2, 2, h - 4, w - 5), (3, 3, 5, 7), (0, 1, h, 1), (h - 1, w - 1, 1, 1), (5, 0, 1, w)):
            dst = G.full((hc, wc, 3), 7, torch.uint8, "dst")
            assert hip.crop_u8(src, y0, x0, hc, wc, out=dst) is dst
            assert np.array_equal(dst.cpu().numpy(), img[y0:y0 + hc, x0:x0 + wc]), (h, w, y0, x0, hc, wc)
        assert np.array_equal(hip.crop_u8(src, 2, 3, 4, 5).cpu().numpy(), img[2:6, 3:8])
    G.check()
    # destinations that start 1, 2 and 3 bytes into an allocation: the bytes around them stay
    img = random_image(3, 9, 11)
    for off in (1, 2, 3):
        buf = torch.full((7 * 6 * 3 + 8,), 200, dtype=torch.uint8, device="cuda")
        view = buf[off:off + 7 * 6 * 3].view(7, 6, 3)
        hip.crop_u8(_dev(img), 1, 2, 7, 6, out=view)
        got = buf.cpu().numpy()
        assert np.array_equal(got[off:off + 126].reshape(7, 6, 3), img[1:8, 2:8]) and (got[:off] == 200).all() and (got[off + 126:] == 200).all()


# ------------------------------------------------------------------ 5. the tester CLI
TODAY = {"images", "psnr", "ssim", "psnr_best", "psnr_worst", "ssim_best", "ssim_worst", "ssim_window", "color"}


def test_tester_cli_psnrb_and_shave(hip, tmp_path, capsys):
    from PIL import Image
    from rcot_amd import tester as TS
    from rcot_amd.mprnet_hip import MPRNetHip
    from test_quality_gpu import _mparams, _write_pngs
    g = np.random.Generator(np.random.PCG64(9))
    img = lambda h, w: g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    noisy = lambda a: np.clip(a.astype(np.int64) + g.integers(-30, 31, size=a.shape), 0, 255).astype(np.uint8)
    tars = [("a.png", img(40, 52)), ("b.png", img(33, 47))]
    _write_pngs(tmp_path / "deg", [(n, noisy(t)) for n, t in tars])
    _write_pngs(tmp_path / "tar", tars)
    ck = str(tmp_path / "net.pth")
    net = MPRNetHip(backend=hip, seed=0)
    net.load_state_dict(_mparams())
    torch.save({"epoch": 1, "Tnet": {k: v.cpu() for k, v in net.state_dict().items()}, "Fnet": {}, "backbone": "mprnet"}, ck)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres", str(tmp_path / tag / "RES") + "/"]
    base = ["--model", ck, "--degset", str(tmp_path / "deg") + "/", "--tarset", str(tmp_path / "tar") + "/", "--pad", "reflect"]
    flags = ["--psnrb", "--shave", "2", "--color", "y", "--ssim_window", "uniform7"]

    def folder_bytes(tag):
        return {(sub, n): open(tmp_path / tag / sub / n, "rb").read() for sub in ("OUT", "TAR", "RES") for n in sorted(os.listdir(tmp_path / tag / sub))}

    capsys.readouterr()
    runs, report = {}, {}
    for metrics in ("folders", "device"):
        runs[metrics] = TS.main(base + dirs(metrics) + flags + ["--metrics", metrics])
        lines = capsys.readouterr().out.splitlines()
        i = lines.index("metrics: ssim uniform7, color y, psnrb, shave 2")
        assert lines[i + 1].startswith("FID") and lines[i + 2].startswith("PSNR: Averyge") and lines[i + 3].startswith("SSIM: Averyge")
        assert lines[i + 4].startswith("PSNR-B: Averyge") and len(lines) == i + 5
        report[metrics] = lines[i + 2:]
        assert set(runs[metrics]) == TODAY | {"psnrb", "psnrb_best", "psnrb_worst"} and runs[metrics]["images"] == 2
    f, d = runs["folders"], runs["device"]
    print(report)
    assert report["folders"] == report["device"]                               # the same three averages, as printed
    for key in ("psnr", "psnr_best", "psnr_worst", "psnrb", "psnrb_best", "psnrb_worst"):
        assert f[key] == d[key], (key, f[key], d[key])                         # integers under both, one function after them
    for key in ("ssim", "ssim_best", "ssim_worst"):
        assert abs(f[key] - d[key]) < 1e-9, (key, f[key], d[key])
    # and they are the host's figures for the written PNGs, which stay full size, cropped by 2
    ps, ss, pb = [], [], []
    for n, t in tars:
        o = np.array(Image.open(tmp_path / "device" / "OUT" / n))
        assert o.shape == t.shape and np.array_equal(np.array(Image.open(tmp_path / "device" / "TAR" / n)), t)
        tc, oc = Q.shave_u8(t, 2), Q.shave_u8(o, 2)
        ps.append(Q.psnr_u8(tc, oc, "y"))
        ss.append(Q.ssim_windowed(tc, oc, "uniform7", "y"))
        pb.append(Q.psnrb_u8(oc, tc, "y", 2, 2))
    assert d["psnr"] == sum(ps) / 2 and d["psnrb"] == sum(pb) / 2 and abs(d["ssim"] - sum(ss) / 2) < 1e-9
    assert (d["psnrb_best"], d["psnrb_worst"]) == (max(pb), min(pb)) and d["psnrb"] < d["psnr"] + 1e-12
    assert folder_bytes("folders") == folder_bytes("device")

    # PSNR-B beside the reference's own figures (box2, rgb; no shave): the egress kernel's sums stay, the blockiness rides along
    rb = TS.main(base + dirs("box2") + ["--psnrb", "--metrics", "device"])
    printed = capsys.readouterr().out
    assert "metrics:" not in printed and printed.splitlines()[-1].startswith("PSNR-B: Averyge")
    pb0 = [Q.psnrb_u8(np.array(Image.open(tmp_path / "box2" / "OUT" / n)), t, "rgb") for n, t in tars]
    assert rb["psnrb"] == sum(pb0) / 2 and set(rb) == set(f)

    # without the two flags: no PSNR-B line, today's keys, today's figures and files
    r0 = TS.main(base + dirs("default") + ["--metrics", "device"])
    printed = capsys.readouterr().out
    assert "PSNR-B" not in printed and "metrics:" not in printed and set(r0) == TODAY
    want = TS.evaluate_folders(str(tmp_path / "default" / "TAR"), str(tmp_path / "default" / "OUT"))
    for key, v in zip(("psnr", "ssim", "psnr_best", "ssim_best", "psnr_worst", "ssim_worst"), want):
        assert abs(r0[key] - v) < 1e-9, (key, r0[key], v)
        assert rb[key] == r0[key]
    assert folder_bytes("default") == folder_bytes("device") == folder_bytes("box2")
    r1 = TS.main(base + dirs("default_f"))
    assert "PSNR-B" not in capsys.readouterr().out and set(r1) == TODAY

    # an image that the shave empties is skipped up front, on both routes
    for metrics in ("folders", "device"):
        rs = TS.main(base + dirs("s17_" + metrics) + ["--shave", "17", "--ssim_window", "gauss11", "--metrics", metrics])
        assert "skipped: 33 x 47 leaves nothing after --shave 17" in capsys.readouterr().out and rs["images"] == 1
        assert sorted(os.listdir(tmp_path / ("s17_" + metrics) / "OUT")) == ["a.png"]
    # the refusals, before anything is written
    with pytest.raises(SystemExit, match="--shave -1"):
        TS.main(base + dirs("neg") + ["--shave", "-1"])
    with pytest.raises(SystemExit, match="cannot be cropped"):
        TS.main(base + dirs("box2_shave") + ["--shave", "2", "--metrics", "device"])
    assert not os.path.exists(tmp_path / "neg") and not os.path.exists(tmp_path / "box2_shave")
