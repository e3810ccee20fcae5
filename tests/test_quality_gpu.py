"""GPU tier of the standard image-quality figures: rcot_image_quality (csrc/quality.hip) against the numpy restatement of
rcot_amd/quality.py for both windows and both colour spaces, its reproducibility, workspace and argument rules, the integer luma on
the device, and the tester CLI with --ssim_window / --color on both metric routes."""
import os

import numpy as np
import pytest
import torch

from rcot_amd import params as P
from rcot_amd import quality as Q
from test_quality_cpu import PROTOCOLS, image_pairs, tie_triples

pytestmark = pytest.mark.gpu

TH, TW = 16, 32                                   # the kernel's tile (HipBackend.QUALITY_TILE, asserted below)
# A single map position per window; empty maps (6 rows; 10 columns for the 11-tap window); widths that are no multiple of 4, so that
# rows start at every byte phase; one, two and four tiles meeting at a corner, for each window; one image of Rain100L's size.
SIZES = [(7, 7), (11, 11), (6, 40), (40, 10), (11, 12), (37, 70), (75, 139)]
SIZES += [(TH + win - 1 + dy, TW + win - 1 + dx) for win in (7, 11) for dy in (-1, 1) for dx in (-1, 1)]
SIZES += [(321, 481)]


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    assert be.QUALITY_TILE == (TH, TW)
    return be


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. the four sums against the host
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_image_quality_equals_the_host(hip, size):
    """stats[0], [1], [3] exactly; |stats[2] / stats[3] - host| < 1e-10, the bar tests/test_anysize_gpu.py holds the box-window SSIM to
    (two fp64 evaluations of the same map differ by ~1e-15).  Measured on an MI355X over all sizes and inputs here: at most 1.9e-14
    (profiles/quality_metrics.txt, which scripts/bench_quality.py writes from the same shapes)."""
    h, w = size
    worst = 0.0
    for kind, a, b in image_pairs(h * 1000 + w, h, w, extreme=True):
        ad, bd = _dev(a), _dev(b)
        for window, space in PROTOCOLS:
            got = hip.image_quality(ad, bd, window, space).cpu().numpy()
            err, n = Q.sqerr_sums(a, b, space)
            total, count = Q.ssim_sums(a, b, window, space)
            win = Q.WINDOW_SIZE[window]
            assert count == (3 if space == "rgb" else 1) * max(0, h - win + 1) * max(0, w - win + 1)
            assert got[0] == err and got[1] == n and got[3] == count, (kind, window, space, got.tolist(), err, n, count)
            m = Q.quality_metrics(got)
            assert m["psnr"] == Q.psnr_u8(a, b, space)
            if count == 0:
                assert got[2] == 0.0 and np.isnan(m["ssim"])
                continue
            want = Q.ssim_windowed(a, b, window, space)
            d = abs(got[2] / got[3] - want)
            worst = max(worst, d)
            print(f"{h}x{w} {kind} {window} {space}: device {got[2] / got[3]!r} host {want!r} diff {d:.2e}")
            assert d < 1e-10, (kind, window, space)
            assert abs(m["ssim"] - want) < 1e-10
    print(f"{h}x{w}: worst |device - host| SSIM {worst:.3e}")


# ------------------------------------------------------------------ 2. reproducibility
def test_image_quality_is_bitwise_reproducible(hip):
    _, a, b = image_pairs(77, 75, 139)[1]
    ad, bd = _dev(a), _dev(b)
    for window, space in PROTOCOLS:
        ws = torch.zeros(hip.image_quality_ws_bytes(75, 139, space) // 4, device="cuda")
        first = hip.image_quality(ad, bd, window, space, ws=ws)
        second = hip.image_quality(ad, bd, window, space, ws=ws)
        ws.fill_(float("nan"))                                               # an unrelated launch dirties the workspace
        third = hip.image_quality(ad, bd, window, space, ws=ws)
        own = hip.image_quality(ad, bd, window, space)                       # the backend's workspace
        for other in (second, third, own):
            assert torch.equal(first.view(torch.int64), other.view(torch.int64)), (window, space)


def test_images_at_any_byte_alignment(hip):
    """views that start 1, 2 and 3 bytes into an allocation: the first and the last dword of an image then straddle its ends"""
    for h, w in ((11, 12), (37, 70)):
        _, a, b = image_pairs(h + w, h, w)[1]
        n = h * w * 3
        want = {p: hip.image_quality(_dev(a), _dev(b), *p) for p in PROTOCOLS}
        for oa, ob in ((1, 3), (2, 0), (3, 2), (0, 1)):
            bufa, bufb = torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda"), torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda")
            av, bv = bufa[oa:oa + n].view(h, w, 3), bufb[ob:ob + n].view(h, w, 3)
            av.copy_(_dev(a))
            bv.copy_(_dev(b))
            assert av.data_ptr() % 4 == oa and bv.data_ptr() % 4 == ob
            for p in PROTOCOLS:
                assert torch.equal(hip.image_quality(av, bv, *p), want[p]), (h, w, oa, ob, p)


# ------------------------------------------------------------------ 3. workspace and argument rules
def _raw_call(hip, ad, bd, h, w, window, space, stats, ws, ws_bytes):
    return hip.L.rcot_image_quality(ad.data_ptr(), bd.data_ptr(), h, w, window, space, stats.data_ptr(), ws.data_ptr(), ws_bytes, hip._st())


def test_workspace_rule(hip):
    from rcot_amd.lib import RcotKernelError
    h, w = 37, 70
    _, a, b = image_pairs(5, h, w)[1]
    ad, bd = _dev(a), _dev(b)
    for space, planes in (("rgb", 3), ("y", 1)):
        need = hip.image_quality_ws_bytes(h, w, space)
        assert need == 16 * planes * 3 * 3                                   # ceil(37 / 16) x ceil(70 / 32) tiles per plane
        ws = torch.zeros(need // 4 + 2, device="cuda")
        stats = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
        assert _raw_call(hip, ad, bd, h, w, 1, hip.SPACES[space], stats, ws, need - 1) == -2
        assert _raw_call(hip, ad, bd, h, w, 1, hip.SPACES[space], stats, ws[1:], need) == -2      # 4 bytes off an 8-byte boundary
        torch.cuda.synchronize()
        assert bool((stats == -7.0).all())                                   # nothing was launched
        assert _raw_call(hip, ad, bd, h, w, 1, hip.SPACES[space], stats, ws, need) == 0
        assert torch.equal(stats, hip.image_quality(ad, bd, "gauss11", space))
        with pytest.raises(RcotKernelError, match="workspace too small"):
            hip.image_quality(ad, bd, "gauss11", space, ws=ws[: need // 4 - 1])
        assert torch.equal(hip.image_quality(ad, bd, "gauss11", space, ws=ws[: need // 4]), stats)


def test_invalid_arguments(hip):
    from rcot_amd.lib import RcotKernelError
    h, w = 12, 20
    _, a, b = image_pairs(6, h, w)[1]
    ad, bd = _dev(a), _dev(b)
    ws = torch.zeros(64, device="cuda")
    stats = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    for window, space, hh, ww in ((2, 0, h, w), (-1, 0, h, w), (0, 2, h, w), (1, -1, h, w), (0, 0, 0, w), (0, 0, h, 0)):
        assert _raw_call(hip, ad, bd, hh, ww, window, space, stats, ws, 256) == -1
    assert hip.L.rcot_image_quality(None, bd.data_ptr(), h, w, 0, 0, stats.data_ptr(), ws.data_ptr(), 256, hip._st()) == -1
    assert hip.L.rcot_image_quality(ad.data_ptr(), bd.data_ptr(), h, w, 0, 0, None, ws.data_ptr(), 256, hip._st()) == -1
    assert hip.L.rcot_image_quality(ad.data_ptr(), bd.data_ptr(), h, w, 0, 0, stats.data_ptr(), None, 256, hip._st()) == -1
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all())
    for call in (lambda: hip.image_quality(ad, bd, "box2", "rgb"), lambda: hip.image_quality(ad, bd, "gauss11", "ycbcr")):
        with pytest.raises(RcotKernelError, match="invalid argument"):
            call()
    with pytest.raises(RcotKernelError, match="expected 12 x 20"):
        hip.image_quality(ad, _dev(b[:, :19]), "uniform7", "rgb")
    with pytest.raises(RcotKernelError, match="uint8"):
        hip.image_quality(ad.float(), bd, "uniform7", "rgb")
    with pytest.raises(RcotKernelError, match="uint8"):
        hip.image_quality(ad, _dev(b)[:, :, :2], "uniform7", "rgb")


# ------------------------------------------------------------------ 4. the luma plane on the device, ties included
def test_device_luma_is_the_integer_rule(hip):
    ties = tie_triples()
    h, w = 19, 45                                                            # two tile rows, two tile columns, odd row bytes
    g = np.random.Generator(np.random.PCG64(12))
    img = g.integers(0, 256, size=(h * w, 3), dtype=np.uint8)
    img[7:7 + len(ties)] = ties
    img[-2:] = [[0, 0, 0], [255, 255, 255]]
    img = img.reshape(h, w, 3)
    base = np.zeros((h, w, 3), dtype=np.uint8)                               # black has luma 16: the constant-16 plane
    assert int(Q.luma_u8(base)[0, 0]) == 16
    want = int(((Q.luma_u8(img).astype(np.int64) - 16) ** 2).sum())
    for window in ("uniform7", "gauss11"):
        got = hip.image_quality(_dev(img), _dev(base), window, "y").cpu().numpy()
        assert got[0] == want and got[1] == h * w
    # each tie triple on its own: one wrong rounding cannot hide behind another
    col = np.ascontiguousarray(ties.reshape(len(ties), 1, 3))
    zero = np.zeros_like(col)
    one = hip.image_quality(_dev(col), _dev(zero), "uniform7", "y").cpu().numpy()
    assert one[0] == int(((Q.luma_u8(col).astype(np.int64) - 16) ** 2).sum()) and one[3] == 0


# ------------------------------------------------------------------ 5. the tester CLI
def _mparams():
    from rcot_amd import mprnet as MP
    shapes = MP.mprnet_param_shapes()
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params([(n, s) for n, s in shapes if not n.endswith("body.1.weight")], 71, "T").items()}
    for n, _ in shapes:
        if n.endswith("body.1.weight"):
            prm[n] = torch.full((1,), 0.2)
    return prm


def _write_pngs(folder, items):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for name, arr in items:
        Image.fromarray(arr).save(os.path.join(folder, name))


KEYS = ("psnr", "ssim", "psnr_best", "ssim_best", "psnr_worst", "ssim_worst")


def test_tester_cli_protocols(hip, tmp_path, capsys):
    from rcot_amd import tester as TS
    from rcot_amd.mprnet_hip import MPRNetHip
    g = np.random.Generator(np.random.PCG64(9))
    img = lambda h, w: g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    noisy = lambda a: np.clip(a.astype(np.int64) + g.integers(-30, 31, size=a.shape), 0, 255).astype(np.uint8)
    tars = [("a.png", img(40, 52)), ("b.png", img(33, 47))]
    degs = [(n, noisy(t)) for n, t in tars]
    _write_pngs(tmp_path / "deg", degs)
    _write_pngs(tmp_path / "tar", tars)
    ck = str(tmp_path / "net.pth")
    net = MPRNetHip(backend=hip, seed=0)
    net.load_state_dict(_mparams())
    torch.save({"epoch": 1, "Tnet": {k: v.cpu() for k, v in net.state_dict().items()}, "Fnet": {}, "backbone": "mprnet"}, ck)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres", str(tmp_path / tag / "RES") + "/"]
    base = ["--model", ck, "--degset", str(tmp_path / "deg") + "/", "--tarset", str(tmp_path / "tar") + "/", "--pad", "reflect"]

    def folder_bytes(tag):
        return {(sub, n): open(tmp_path / tag / sub / n, "rb").read() for sub in ("OUT", "TAR", "RES") for n in sorted(os.listdir(tmp_path / tag / sub))}

    capsys.readouterr()
    runs = {}
    for window, color in (("gauss11", "y"), ("uniform7", "rgb")):
        for metrics in ("folders", "device"):
            tag = f"{window}_{color}_{metrics}"
            r = TS.main(base + dirs(tag) + ["--ssim_window", window, "--color", color, "--metrics", metrics])
            printed = capsys.readouterr().out
            assert r["images"] == 2 and (r["ssim_window"], r["color"]) == (window, color)
            lines = printed.splitlines()
            i = lines.index(f"metrics: ssim {window}, color {color}")                  # the protocol line, before the three of the report
            assert lines[i + 1].startswith("FID") and lines[i + 2].startswith("PSNR: Averyge") and lines[i + 3].startswith("SSIM: Averyge")
            runs[tag] = r
        f, d = runs[f"{window}_{color}_folders"], runs[f"{window}_{color}_device"]
        for key in KEYS:
            print(window, color, key, f[key], d[key])
            assert abs(f[key] - d[key]) < 1e-9, (window, color, key, f[key], d[key])
        fb = folder_bytes(f"{window}_{color}_folders")
        assert len(fb) == 6 and fb == folder_bytes(f"{window}_{color}_device")
        # and both are the host's figures for the PNGs that were written
        from PIL import Image
        ps, ss = [], []
        for n, t in tars:
            o = np.array(Image.open(tmp_path / f"{window}_{color}_device" / "OUT" / n))
            ps.append(Q.psnr_u8(t, o, color))
            ss.append(Q.ssim_windowed(t, o, window, color))
        assert abs(d["psnr"] - sum(ps) / 2) < 1e-9 and abs(d["ssim"] - sum(ss) / 2) < 1e-9
        assert abs(d["ssim_worst"] - min(ss)) < 1e-9 and abs(d["psnr_best"] - max(ps)) < 1e-9
    assert folder_bytes("gauss11_y_device") == folder_bytes("uniform7_rgb_device")     # the protocol does not touch the images
    assert abs(runs["gauss11_y_device"]["ssim"] - runs["uniform7_rgb_device"]["ssim"]) > 1e-6

    # the default flags: no protocol line, and the figures of the code path as it was (the egress kernel's sums == the folders read back)
    r0 = TS.main(base + dirs("default") + ["--metrics", "device"])
    printed = capsys.readouterr().out
    assert "metrics:" not in printed and (r0["ssim_window"], r0["color"]) == ("box2", "rgb")
    psnr, ssim, pmax, smax, pmin, smin = TS.evaluate_folders(str(tmp_path / "default" / "TAR"), str(tmp_path / "default" / "OUT"))
    for key, want in zip(KEYS, (psnr, ssim, pmax, smax, pmin, smin)):
        assert abs(r0[key] - want) < 1e-9, (key, r0[key], want)
    assert "PSNR: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(psnr, pmax, pmin) in printed
    assert "SSIM: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(ssim, smax, smin) in printed
    assert folder_bytes("default") == folder_bytes("gauss11_y_device")
    r1 = TS.main(base + dirs("default_f"))
    assert "metrics:" not in capsys.readouterr().out
    assert {k: r1[k] for k in KEYS} == dict(zip(KEYS, (psnr, ssim, pmax, smax, pmin, smin))) and set(r1) == set(r0)
    # the reference's map on the luma plane: host only
    ry = TS.main(base + dirs("box2_y") + ["--color", "y"])
    assert "metrics: ssim box2, color y" in capsys.readouterr().out and ry["images"] == 2
    with pytest.raises(SystemExit, match="host only"):
        TS.main(base + dirs("box2_y_d") + ["--color", "y", "--metrics", "device"])
    assert not os.path.exists(tmp_path / "box2_y_d")
