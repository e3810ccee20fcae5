"""GPU tier of tiled / self-ensemble inference: rcot_view_gather and rcot_view_blend against the numpy restatement
(tests/test_tiles_cpu.py), ``restore_views`` against today's ``tester.restore`` and against per-view network calls, the refusals, the
seam property on the device, and the tester CLI with --tile_window / --tile_batch / --ensemble."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr, seeded_tensor
from rcot_amd import tiles as TL
from test_anysize_cpu import quantise
from test_anysize_gpu import _mparams, _tparams, _write_pngs
from test_tiles_cpu import (ALL8, BASE, BLEND_ONLY_EINVAL, EINVAL_CASES, EUNSUPPORTED_CASES, GEOMETRIES, augment, blend_views, check_seams,
                            gather_views, seam_errors)

pytestmark = pytest.mark.gpu

ORIGINS = {"b": (None, [0, 4]), "c": ([0, 4, 8], [0, 4, 8]), "f": ([0, 32], [0, 32, 56]), "g": (None, [0, 8, 16])}     # as the issue states them


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def restormer(hip):
    from rcot_amd.net_restormer import T_net
    net = T_net(decoder=True, backend=hip)
    net.load_state_dict(_tparams(11))
    return net


@pytest.fixture(scope="module")
def mprnet(hip):
    from rcot_amd.mprnet_hip import MPRNetHip
    net = MPRNetHip(backend=hip, seed=0)
    net.load_state_dict(_mparams())
    return net


class Stub:
    """a 'network' for the plumbing: any callable on [n, C, h, w] with the backend the views run on"""

    def __init__(self, be, fn):
        self.be, self.fn, self.seen, self.batches = be, fn, 0, []

    def __call__(self, t):
        y = self.fn(t, self.seen)
        self.seen += t.shape[0]
        self.batches.append(tuple(t.shape))
        return y


def _flat(views):
    return np.concatenate([v.reshape(-1) for v in views])


# ------------------------------------------------------------------ 1. gather and blend == the restatement
@pytest.mark.parametrize("case", list(GEOMETRIES) + ["i"])
def test_gather_and_blend_equal_the_restatement(hip, case):
    H, W, tile, ov, mult, modes = GEOMETRIES["c" if case == "i" else case]
    planes = 6 if case == "i" else 3
    p = TL.plan(H, W, tile, ov, mult, 1)
    ys, xs, Th, Tw = list(p.ys), list(p.xs), p.Th, p.Tw
    if case in ORIGINS:
        assert (ORIGINS[case][0] is None or ys == ORIGINS[case][0]) and xs == ORIGINS[case][1]
    if case in ("a", "d", "e"):
        assert (ys, xs, Th, Tw) == ([0], [0], H, W)
    if case == "f":
        assert len(modes) * len(ys) * len(xs) == 48
    if case == "d":
        assert augment(np.zeros((1, Th, Tw), np.float32), 2).shape == (1, 16, 8)
    img = seeded_tensor(H * 1000 + W, (planes, H, W))
    want = gather_views(img.numpy(), ys, xs, modes, Th, Tw)
    views = hip.view_gather(img.cuda(), ys, xs, modes, Th, Tw)
    assert views.shape == (len(want), planes * Th * Tw)
    assert torch.equal(views.cpu().reshape(-1), torch.from_numpy(_flat(want)))
    # the blend takes views that differ from what was gathered (a network ran in between): independent values, every view its own
    g = np.random.Generator(np.random.PCG64(H + W))
    net_out = [g.uniform(-1.0, 1.0, v.shape).astype(np.float32) for v in want]
    dev = torch.from_numpy(_flat(net_out)).cuda().view(len(want), -1)
    wy, wx = TL.window_taps(Th, ov or 4, "linear"), TL.window_taps(Tw, ov or 4, "linear")
    for taps in (None, (wy, wx)):
        wd = (None, None) if taps is None else tuple(torch.from_numpy(t).cuda() for t in taps)
        got = hip.view_blend(dev, H, W, ys, xs, modes, Th, Tw, *wd)
        ref = blend_views(net_out, planes, H, W, ys, xs, modes, Th, Tw, *(taps or (None, None)))
        assert got.shape == (planes, H, W)
        assert torch.equal(got.cpu(), torch.from_numpy(ref)), (case, "uniform" if taps is None else "linear")
    # gather, then blend: the image again, up to the rounding of n products and n sums per pixel (n <= the view count)
    tol = 2 * (len(want) + 2) * 2.0 ** -24 * float(img.abs().max())
    for wd in ((None, None), (torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda())):
        back = hip.view_blend(views, H, W, ys, xs, modes, Th, Tw, *wd)
        assert float((back.cpu() - img).abs().max()) <= tol
    if len(want) == 1:
        assert torch.equal(hip.view_blend(views, H, W, ys, xs, modes, Th, Tw).cpu(), img)


# ------------------------------------------------------------------ 2. uniform taps, modes {0}, tile_batch 1 == today's restore
@pytest.mark.parametrize("geom", [(24, 24, 16, 12, 4), (40, 56, 32, 8, 8), (8, 12, 8, 4, 4), (72, 96, 40, 8, 8), (20, 28, 12, 4, 4)],
                         ids=lambda g: "x".join(map(str, g)))
def test_uniform_views_equal_todays_restore_stub(hip, geom):
    from rcot_amd import tester as TS
    H, W, tile, ov, mult = geom
    x = seeded_tensor(H + W, (2, 3, H, W), lo=0.0, hi=1.0).cuda()
    net = Stub(hip, lambda t, k: t * 1.5 + 0.25)
    want = TS.restore(net, x, tile, ov, mult)
    calls = len(net.batches)
    got = TL.restore_views(net, x, TL.plan(H, W, tile, ov, mult, 1), "uniform", 1)
    assert torch.equal(got, want)
    assert len(net.batches) - calls == 2 * calls and all(b[0] == 1 for b in net.batches[calls:])       # one view per call, image by image


def test_uniform_views_equal_todays_restore_mprnet(mprnet):
    from rcot_amd import tester as TS
    x = seeded_tensor(75, (1, 3, 40, 56), lo=0.0, hi=1.0).cuda()
    want = TS.restore(mprnet, x, 32, 8, mprnet.size_multiple)
    p = TL.plan(40, 56, 32, 8, mprnet.size_multiple, 1)
    assert p.n_views == 4 and (p.Th, p.Tw) == (32, 32)
    assert torch.equal(TL.restore_views(mprnet, x, p, "uniform", 1), want)
    assert torch.equal(TS.restore(mprnet, x, 32, 8, mprnet.size_multiple, window="uniform", tile_batch=1, ensemble=1), want)


# ------------------------------------------------------------------ 3. refusals
def _backend_call(hip, which, case, sentinel=-7.0):
    """the backend call of BASE changed by ``case`` -> (thunk, the output tensor it must leave untouched)"""
    g = {**BASE, **{k: v for k, v in case.items() if k in BASE}}
    n = max(len(g["modes"]) * len(g["ys"]) * len(g["xs"]), 1)
    per = max(g["planes"], 1) * max(g["Th"], 1) * max(g["Tw"], 1)
    image = lambda fill: torch.full((max(g["planes"], 1) * g["H"] * g["W"] + 4,), fill, device="cuda")
    stack = lambda fill: torch.full((n * per + 4,), fill, device="cuda")
    off = lambda name: 1 if case.get("misalign") == name else 0
    cut_img = lambda t, name: t[off(name):off(name) + max(g["planes"], 1) * g["H"] * g["W"]].view(max(g["planes"], 1), g["H"], g["W"])[:g["planes"]]
    cut_views = lambda t, name: t[off(name):off(name) + n * per].view(n, per)
    geom = (g["ys"], g["xs"], g["modes"], g["Th"], g["Tw"])
    if which == "gather":
        src, dst = cut_img(image(0.5), "data"), cut_views(stack(sentinel), "result")
        return (lambda: hip.view_gather(src, *geom, out=dst)), dst
    src, dst = cut_views(stack(0.5), "data"), cut_img(image(sentinel), "result")
    wy, wx = torch.ones(max(g["Th"], 1) + 4, device="cuda"), torch.ones(max(g["Tw"], 1) + 4, device="cuda")
    wy, wx = wy[off("wy"):off("wy") + max(g["Th"], 1)], wx[off("wx"):off("wx") + max(g["Tw"], 1)]
    taps = case.get("taps")
    wy, wx = (None if taps == "wx" else wy), (None if taps == "wy" else wx)
    if "taps" not in case and case.get("misalign") not in ("wy", "wx"):
        wy = wx = None
    return (lambda: hip.view_blend(src, g["H"], g["W"], *geom, wy, wx, out=dst)), dst


@pytest.mark.parametrize("which", ["gather", "blend"])
def test_refusals(hip, which):
    from rcot_amd.lib import RcotKernelError
    cases = {k: v for k, v in EINVAL_CASES.items() if "null" not in v}          # a tensor always has an address: NULLs are the CPU tier's
    if which == "blend":
        cases.update(BLEND_ONLY_EINVAL)
    kept = []
    for name, case in cases.items():
        call, out = _backend_call(hip, which, case)
        with pytest.raises(RcotKernelError, match="invalid argument|must|expected"):
            call()
        kept.append((name, out))
    for name, case in EUNSUPPORTED_CASES.items():
        call, out = _backend_call(hip, which, case)
        with pytest.raises(RcotKernelError, match="no kernel for this shape"):
            call()
        kept.append((name, out))
    torch.cuda.synchronize()
    for name, out in kept:
        assert bool((out == -7.0).all()), name                                  # nothing was launched
    call, out = _backend_call(hip, which, {})                                   # and BASE itself runs
    call()
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())


# ------------------------------------------------------------------ 4. networks
def _expected(net, x, p, kind):
    """every view cut and mapped with torch on the host, restored on its own at B = 1, blended by the restatement"""
    views = []
    for m in p.modes:
        for y0 in p.ys:
            for x0 in p.xs:
                w = x[0, :, y0:y0 + p.Th, x0:x0 + p.Tw]
                v = torch.rot90(w, m // 2, dims=(1, 2))
                v = (torch.flip(v, dims=(1,)) if m & 1 else v).contiguous()
                views.append(net(v[None].cuda())[0].cpu().numpy())
    return torch.from_numpy(blend_views(views, 3, p.H, p.W, p.ys, p.xs, p.modes, p.Th, p.Tw, TL.window_taps(p.Th, p.ov_y, kind),
                                        TL.window_taps(p.Tw, p.ov_x, kind)))


@pytest.mark.parametrize("which", ["restormer", "mprnet"])
@pytest.mark.parametrize("request_", ["tiles", "ensemble"])
def test_networks_on_views(which, request_, restormer, mprnet):
    net, bar = (restormer, 2e-5) if which == "restormer" else (mprnet, 1e-5)     # the fp32 bars of test_*_any_size_vs_reference
    if request_ == "tiles":
        x = seeded_tensor(75, (1, 3, 40, 56), lo=0.0, hi=1.0)
        p = TL.plan(40, 56, 32, 8, net.size_multiple, 1)
        assert p.shape_classes() == [(0, 4, 32, 32)]                             # four 32 x 32 views
    else:
        x = seeded_tensor(76, (1, 3, 32, 40), lo=0.0, hi=1.0)
        p = TL.plan(32, 40, 0, 8, net.size_multiple, 8)
        assert p.shape_classes() == [(0, 4, 32, 40), (4, 4, 40, 32)]             # the whole image: two shapes of four
    want = _expected(net, x, p, "linear")
    one = TL.restore_views(net, x.cuda(), p, "linear", 1)
    assert torch.equal(one.cpu()[0], want)
    for tb in (0, 3):
        e = relerr(TL.restore_views(net, x.cuda(), p, "linear", tb)[0], want)
        print(f"{which} {request_}: tile_batch {tb} against one view per call: rel err {e:.2e}")
        assert e <= bar


# ------------------------------------------------------------------ 5. seams on the device
def test_seams_on_the_device(hip):
    def blend(kind):
        def run(p, x):
            net = Stub(hip, lambda t, k: t + 0.02 * torch.arange(k, k + t.shape[0], device=t.device, dtype=t.dtype).view(-1, 1, 1, 1))
            return TL.restore_views(net, torch.from_numpy(x)[None].cuda(), p, kind, 0)[0].cpu().numpy()
        return run
    check_seams(seam_errors(blend("uniform")), seam_errors(blend("linear")))
    e = seam_errors(blend("cosine"))
    assert abs(e[23]) < 1e-6 and abs(e[32] - 0.02) < 1e-6 and (np.diff(e) > -1e-6).all() and np.abs(np.diff(e)).max() < 0.01 - 1e-3


# ------------------------------------------------------------------ 6. the tester CLI
@pytest.mark.parametrize("kind", ["mprnet", "restormer"])
def test_tester_cli_views(hip, tmp_path, capsys, kind):
    from PIL import Image
    from rcot_amd import tester as TS
    g = np.random.Generator(np.random.PCG64(9))
    img = lambda h, w: g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    noisy = lambda a: np.clip(a.astype(np.int64) + g.integers(-30, 31, size=a.shape), 0, 255).astype(np.uint8)
    tars = [("a.png", img(40, 56)), ("b.png", img(37, 50)), ("c.png", img(32, 32))]
    degs = [("a.png", noisy(tars[0][1])), ("b.png", noisy(tars[1][1])), ("c.png", img(32, 36))]      # c: shape mismatch, skipped
    _write_pngs(tmp_path / "deg", degs)
    _write_pngs(tmp_path / "tar", tars)
    ck = str(tmp_path / "net.pth")
    if kind == "mprnet":
        from rcot_amd.mprnet_hip import MPRNetHip
        net = MPRNetHip(backend=hip, seed=0)
        net.load_state_dict(_mparams())
        torch.save({"epoch": 1, "Tnet": {k: v.cpu() for k, v in net.state_dict().items()}, "Fnet": {}, "backbone": "mprnet"}, ck)
    else:
        from rcot_amd.compat import shim
        torch.save({"epoch": 1, "Tnet": shim().T_net.from_state_dict(_tparams(31), decoder=True)}, ck)
    net, mult = TS.load_network(ck)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres", str(tmp_path / tag / "RES") + "/"]
    base = ["--model", ck, "--degset", str(tmp_path / "deg") + "/", "--tarset", str(tmp_path / "tar") + "/"]
    png = lambda tag, sub, n: np.array(Image.open(tmp_path / tag / sub / n))
    r = TS.main(base + dirs("v") + ["--tile", "32", "--overlap", "8", "--tile_window", "linear", "--tile_batch", "0", "--ensemble", "8",
                                    "--pad", "reflect", "--metrics", "device"])
    assert r["images"] == 2 and sorted(os.listdir(tmp_path / "v" / "OUT")) == ["a.png", "b.png"]
    Hp, Wp = -(-37 // mult) * mult, -(-50 // mult) * mult
    x = torch.from_numpy(np.ascontiguousarray(degs[1][1].transpose(2, 0, 1))).float().div(255).unsqueeze(0)
    xp = F.pad(x, (0, Wp - 50, 0, Hp - 37), mode="reflect").cuda()
    p = TL.plan(Hp, Wp, 32, 8, mult, 8)
    assert p.n_views == 32 and p.shape_classes() == [(0, 32, 32, 32)]
    y = TL.restore_views(net, xp, p, "linear", 0)
    assert np.array_equal(png("v", "OUT", "b.png"), quantise(y[0, :, :37, :50]))
    assert np.array_equal(png("v", "RES", "b.png"), quantise(((xp - y).cpu() * 2)[0, :, :37, :50]))
    psnr, ssim, pmax, smax, pmin, smin = TS.evaluate_folders(str(tmp_path / "v" / "TAR"), str(tmp_path / "v" / "OUT"))
    for key, want in (("psnr", psnr), ("ssim", ssim), ("psnr_best", pmax), ("ssim_best", smax), ("psnr_worst", pmin), ("ssim_worst", smin)):
        assert abs(r[key] - want) < 1e-9, (key, r[key], want)
    # none of the new flags == the three defaults spelled out, file by file — on the plain path and on the padded one
    for extra in ([], ["--pad", "reflect", "--metrics", "device"]):
        tiled = ["--tile", "32", "--overlap", "8"] + extra
        r0 = TS.main(base + dirs("d0" + str(len(extra))) + tiled)
        r1 = TS.main(base + dirs("d1" + str(len(extra))) + tiled + ["--tile_window", "uniform", "--tile_batch", "1", "--ensemble", "1"])
        assert r0 == r1 and r0["images"] >= 1
        for sub in ("OUT", "RES", "TAR"):
            names = sorted(os.listdir(tmp_path / ("d0" + str(len(extra))) / sub))
            assert names == sorted(os.listdir(tmp_path / ("d1" + str(len(extra))) / sub)) and names
            for n in names:
                assert np.array_equal(png("d0" + str(len(extra)), sub, n), png("d1" + str(len(extra)), sub, n))
    # and the default path is still the equal-weight average: the ramp changes pixels
    assert not np.array_equal(png("d04", "OUT", "b.png"), png("v", "OUT", "b.png"))
    capsys.readouterr()
