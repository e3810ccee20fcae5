"""GPU tier of whole-image validation at any size: the three entry points of csrc/imageio.hip against torch's F.pad, the save_image
chain and the numpy restatement of the statistics (tests/test_anysize_cpu.py), then the padded pipeline — restore_any_size on both
networks against the REFERENCE's outputs on the padded inputs (tests/golden/anysize.npz), evaluate(pad=...) and the tester CLI with
--pad / --metrics device."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr, seeded_tensor
from rcot_amd import params as P
from synth_folders import dataset_tree
from test_anysize_cpu import egress_stats, quantise, synth_pair

pytestmark = pytest.mark.gpu

# (h, w) -> (Hp, Wp).  The first six are the smallest shapes at which these kernels can go wrong: no padding; pad 7 and 1 with reflect
# reaching row 1 and an empty SSIM map; odd row bytes with a 3 x 9 map; the general case at multiples of 8 and of 4; more than one
# workgroup of pixels (partials + final pass).  The last three reach the remaining code paths: padded widths that are no multiple of 4
# (the scalar forms of all three kernels), a row longer than one wave's 256 pixels (the SSIM window across the segment edge, padding
# columns in the second segment), and a segment that holds padding columns only.
SHAPES = [((8, 8), (8, 8)), ((9, 15), (16, 16)), ((13, 19), (16, 24)), ((37, 50), (40, 56)), ((37, 50), (40, 52)), ((70, 90), (72, 96)),
          ((13, 19), (15, 21)), ((12, 300), (16, 304)), ((11, 256), (12, 264))]
_ids = [f"{h}x{w}-{Hp}x{Wp}" for (h, w), (Hp, Wp) in SHAPES]


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _modes(h, w, Hp, Wp):
    return ["reflect", "replicate"] + (["none"] if (Hp, Wp) == (h, w) else [])


def _fpad(x, Hp, Wp, mode):
    h, w = x.shape[-2:]
    return x.clone() if mode == "none" else F.pad(x, (0, Wp - w, 0, Hp - h), mode=mode)


# ------------------------------------------------------------------ 1. ingest and pad2d == F.pad
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_image_ingest_and_pad2d_equal_torch_pad(hip, shape):
    (h, w), (Hp, Wp) = shape
    g = np.random.Generator(np.random.PCG64(h * 1000 + w))
    img = torch.from_numpy(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    planes = seeded_tensor(h + w, (2, 3, h, w))
    for mode in _modes(h, w, Hp, Wp):
        want = _fpad(img.permute(2, 0, 1).float().div(255)[None], Hp, Wp, mode)
        got = hip.image_ingest(img.cuda(), Hp, Wp, mode)
        assert got.shape == (1, 3, Hp, Wp) and torch.equal(got.cpu(), want), mode
        got = hip.pad2d(planes.cuda(), Hp, Wp, mode)
        assert got.shape == (2, 3, Hp, Wp) and torch.equal(got.cpu(), _fpad(planes, Hp, Wp, mode)), mode
    # a view that starts 4 bytes into an allocation: the scalar forms on a shape the vector forms take otherwise
    buf = torch.empty(3 * Hp * Wp + 1, device="cuda")
    got = hip.image_ingest(img.cuda(), Hp, Wp, "replicate", out=buf[1:].view(1, 3, Hp, Wp))
    assert torch.equal(got.cpu(), _fpad(img.permute(2, 0, 1).float().div(255)[None], Hp, Wp, "replicate"))


# ------------------------------------------------------------------ 2. refusals
def test_refusals(hip):
    from rcot_amd.lib import RcotKernelError
    img = torch.zeros(3, 50, 3, dtype=torch.uint8, device="cuda")
    planes = torch.zeros(3, 3, 50, device="cuda")
    out = torch.full((1, 3, 8, 56), -7.0, device="cuda")
    for call in (lambda: hip.image_ingest(img, 8, 56, "reflect", out=out), lambda: hip.pad2d(planes, 8, 56, "reflect", out=out[0])):
        with pytest.raises(RcotKernelError, match="invalid argument"):                 # 5 mirrored rows of a 3-row image
            call()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                                   # nothing was launched
    assert hip.image_ingest(img, 8, 56, "replicate").shape == (1, 3, 8, 56)            # replicate pads the same shape
    assert torch.equal(hip.pad2d(planes, 8, 56, "replicate"), torch.zeros(3, 8, 56, device="cuda"))
    with pytest.raises(RcotKernelError, match="invalid argument"):
        hip.image_ingest(img, 8, 56, "none")                                           # mode 0 pads nothing
    restored, target = synth_pair(1, 70, 90)
    small = torch.empty(4, device="cuda")                                              # 16 bytes; 18 workgroups need 432
    with pytest.raises(RcotKernelError, match="workspace too small"):
        hip.image_egress(torch.from_numpy(restored).cuda(), 70, 90, target=torch.from_numpy(target).cuda(), want_stats=True, ws=small)
    assert hip.image_egress(torch.from_numpy(restored).cuda(), 70, 90, want_out=True, ws=small)[0].shape == (70, 90, 3)   # no statistics, no workspace


# ------------------------------------------------------------------ 3. the 8-bit quantisation of save_image, exactly
@pytest.mark.parametrize("scale", [2, 3])
def test_image_egress_quantisation_is_save_images(hip, scale):
    k = np.arange(256, dtype=np.float64)[:, None]
    delta = np.linspace(-1e-5, 1e-5, 2001)[None, :]
    grid = ((k + 0.5 + delta) / 255.0).astype(np.float32)                   # 512 256 values either side of every rounding boundary
    h, w = grid.shape
    Hp, Wp = h, w + 3                                                       # 2004: the float4 form; the three columns beyond w are ignored
    g = np.random.Generator(np.random.PCG64(scale))
    restored = np.empty((3, Hp, Wp), dtype=np.float32)
    restored[0, :, :w] = grid
    restored[1] = g.uniform(-0.5, 1.5, (Hp, Wp))                            # below 0 and above 1
    restored[1, :4] = np.array([-1e30, -1.0, -1e-8, 0.0, 1.0, 1.0 + 1e-7, 2.0, 1e30], dtype=np.float32).repeat(Wp // 2)[: 4 * Wp].reshape(4, Wp)
    restored[2] = g.uniform(0.0, 1.0, (Hp, Wp))                             # a NaN-free random plane
    restored[0, :, w:] = 9.0
    degraded = np.empty_like(restored)
    degraded[0, :, :w] = grid[::-1, ::-1]                                   # residuals of every size and sign
    degraded[0, :, w:] = -9.0
    degraded[1] = g.uniform(-0.5, 1.5, (Hp, Wp))
    degraded[2] = restored[2] + ((k[:h] + 0.5 + delta) / 255.0 / scale).astype(np.float32).repeat(2, axis=1)[:, :Wp]   # residuals at the boundaries
    rt, dt = torch.from_numpy(restored), torch.from_numpy(degraded)
    out_u8, res_u8, _ = hip.image_egress(rt.cuda(), h, w, degraded=dt.cuda(), res_scale=scale, want_out=True, want_res=True)
    assert np.array_equal(out_u8.cpu().numpy(), quantise(rt[:, :h, :w]))
    assert np.array_equal(res_u8.cpu().numpy(), quantise((dt - rt)[:, :h, :w] * scale))
    # the scalar form (padded width no multiple of 4) gives the same bytes
    out2, res2, _ = hip.image_egress(rt[:, :, :w + 1].contiguous().cuda(), h, w, degraded=dt[:, :, :w + 1].contiguous().cuda(), res_scale=scale,
                                     want_out=True, want_res=True)
    assert torch.equal(out2, out_u8) and torch.equal(res2, res_u8)


# ------------------------------------------------------------------ 4. the statistics against the numpy restatement
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_image_egress_statistics(hip, shape):
    from rcot_amd import tester as TS
    from rcot_amd.wholeimage import image_metrics
    (h, w), (Hp, Wp) = shape
    restored, target = synth_pair(h * 1000 + w, h, w)
    padded = seeded_tensor(h + w, (3, Hp, Wp), lo=-1.0, hi=2.0)             # what lies beyond the image must not count
    padded[:, :h, :w] = torch.from_numpy(restored)
    rd, td = padded.cuda(), torch.from_numpy(target).cuda()
    out_u8, _, stats = hip.image_egress(rd, h, w, target=td, want_out=True, want_stats=True)
    want_u8 = quantise(torch.from_numpy(restored))
    assert np.array_equal(out_u8.cpu().numpy(), want_u8)
    want = egress_stats(restored, target, want_u8)
    got = stats.cpu().numpy()
    print(f"{h}x{w}: device {got.tolist()} restated {want.tolist()}")
    assert got[1] == want[1] and got[3] == want[3] == 3 * max(0, h - 10) * max(0, w - 10)
    assert abs(got[0] - want[0]) <= 1e-12 * want[0]
    m = image_metrics(stats, h, w)
    if want[3]:
        assert abs(got[2] / got[3] - TS.ssim_image(target, want_u8)) < 1e-10
        assert abs(m["ssim"] - TS.ssim_image(target, want_u8)) < 1e-10
    else:
        assert got[2] == 0.0 and np.isnan(m["ssim"])
    assert abs(m["psnr_u8"] - TS.psnr_uint8(target, want_u8)) < 1e-9
    # bitwise reproducible, with and without the 8-bit outputs
    again = hip.image_egress(rd, h, w, target=td, want_out=False, want_stats=True)[2]
    assert torch.equal(again, stats)
    # target == output: zero 8-bit error is an infinite PSNR and an SSIM of one
    same = hip.image_egress(rd, h, w, target=out_u8, want_out=False, want_stats=True)[2]
    ms = image_metrics(same, h, w)
    assert float(same[1]) == 0.0 and ms["psnr_u8"] == float("inf")
    assert np.isnan(ms["ssim"]) if not want[3] else abs(ms["ssim"] - 1.0) < 1e-12


# ------------------------------------------------------------------ 5 / 6. the padded pipeline against the reference
def _tparams(seed):
    return {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), seed, "T").items()}


def _mparams():
    from rcot_amd import mprnet as MP
    shapes = MP.mprnet_param_shapes()
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params([(n, s) for n, s in shapes if not n.endswith("body.1.weight")], 71, "T").items()}
    for n, _ in shapes:
        if n.endswith("body.1.weight"):
            prm[n] = torch.full((1,), 0.2)
    return prm


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_restormer_any_size_vs_reference(prec, gold):
    from rcot_amd import lib
    from rcot_amd.net_restormer import T_net
    from rcot_amd.ops import HipBackend
    from rcot_amd.wholeimage import restore_any_size
    be = HipBackend()
    be.prec = lib.PREC_BF16X3 if prec == "bf16x3" else lib.PREC_FP32
    net = T_net(decoder=True, backend=be)
    net.load_state_dict(_tparams(11))
    fx = gold("anysize.npz")
    B, h, w, Hp, Wp, sx, sp = (int(v) for v in fx["restormer_cfg"])
    assert (B, h, w, Hp, Wp, sp, net.size_multiple) == (1, 37, 50, 40, 56, 11, 8)
    x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(sx))
    for mode in ("reflect", "replicate") if prec == "fp32" else ("reflect",):
        r = restore_any_size(net, x, net.size_multiple, mode)
        assert (r.h, r.w, r.Hp, r.Wp) == (h, w, Hp, Wp) and r.out.shape == (1, 3, Hp, Wp)
        xp = F.pad(x, (0, Wp - w, 0, Hp - h), mode=mode)
        assert torch.equal(r.x.cpu(), xp)
        assert torch.equal(r.out[..., :h, :w], net(xp.cuda())[..., :h, :w])
        e = relerr(r.out[..., :h, :w], torch.from_numpy(fx[f"restormer_{mode}_y"]))
        print(f"[{prec}] 37x50 {mode}-padded to 40x56, cropped: rel err to the reference {e:.2e}")
        assert e < (2e-5 if prec == "fp32" else 1e-4)          # the bars of test_whole_image_with_odd_latent_plane_vs_reference


def test_mprnet_any_size_vs_reference(hip, gold):
    from rcot_amd.mprnet_hip import MPRNetHip
    from rcot_amd.wholeimage import restore_any_size
    net = MPRNetHip(backend=hip, seed=0)
    net.load_state_dict(_mparams())
    assert net.size_multiple == 4
    x = seeded_tensor(75, (1, 3, 38, 54), lo=0.0, hi=1.0)
    r = restore_any_size(net, x, net.size_multiple, "reflect")
    assert (r.Hp, r.Wp) == (40, 56)
    e = relerr(r.out[..., :38, :54], torch.from_numpy(gold("anysize.npz")["mprnet_reflect_y"]))
    print(f"MPRNet 38x54 reflect-padded to 40x56, cropped: rel err to the reference {e:.2e}")
    assert e < 1e-5                                            # the bar of test_mprnet_hip_whole_image_vs_reference


# ------------------------------------------------------------------ 7. evaluate(pad=...)
def test_evaluate_with_padding_counts_every_image(tmp_path, gold):
    from rcot_amd import trainer as TR
    from rcot_amd.net_restormer import T_net
    root = str(tmp_path)
    dataset_tree(root, 1)
    net = T_net(decoder=True)
    net.load_state_dict(_tparams(11))
    degs, tars = sorted(glob.glob(f"{root}/val/input/*")), sorted(glob.glob(f"{root}/val/target/*"))
    two = float(gold("gpu_fixtures.npz")["eval_psnr"].sum())                 # the reference on the two multiple-of-8 images (no padding there)
    third = float(gold("anysize.npz")["eval_psnr_70x90"])                    # and on the 70 x 90 one, reflect-padded to 72 x 96
    got = TR.evaluate(net, degs, tars, pad="reflect")
    print(f"evaluate(pad='reflect') {got:.4f} dB, reference {(two + third) / 3:.4f} dB")
    assert abs(got - (two + third) / 3) <= 0.02                              # the bar of test_evaluate_matches_reference_psnr
    old = TR.evaluate(net, degs, tars)
    assert abs(old - two / 3) <= 0.02 and old == TR.evaluate(net, degs, tars, pad="none")      # without the keyword: the third image is skipped
    assert np.isnan(TR.evaluate(net, [], [], pad="reflect"))


# ------------------------------------------------------------------ 8. the tester CLI
def _write_pngs(folder, items):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for name, arr in items:
        Image.fromarray(arr).save(os.path.join(folder, name))


@pytest.mark.parametrize("kind", ["mprnet", "restormer"])
def test_tester_cli_pad_and_device_metrics(hip, tmp_path, capsys, kind):
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
    assert net.size_multiple == mult == (4 if kind == "mprnet" else 8)
    dirs = lambda tag: ["--save", str(tmp_path / tag / "OUT") + "/", "--savetar", str(tmp_path / tag / "TAR") + "/", "--saveres", str(tmp_path / tag / "RES") + "/"]
    base = ["--model", ck, "--degset", str(tmp_path / "deg") + "/", "--tarset", str(tmp_path / "tar") + "/"]
    png = lambda tag, sub, n: np.array(Image.open(tmp_path / tag / sub / n))
    capsys.readouterr()
    r = TS.main(base + dirs("p") + ["--pad", "reflect", "--metrics", "device"])
    printed = capsys.readouterr().out
    assert r["images"] == 2 and sorted(os.listdir(tmp_path / "p" / "OUT")) == ["a.png", "b.png"]
    assert "differ" in printed                                                  # the mismatched pair is skipped with a message
    out_b = png("p", "OUT", "b.png")
    assert out_b.shape == (37, 50, 3)                                           # the whole image: no crop to a multiple of 4
    Hp, Wp = -(-37 // mult) * mult, -(-50 // mult) * mult
    x = torch.from_numpy(np.ascontiguousarray(degs[1][1].transpose(2, 0, 1))).float().div(255).unsqueeze(0)
    xp = F.pad(x, (0, Wp - 50, 0, Hp - 37), mode="reflect").cuda()
    y = net(xp)
    assert np.array_equal(out_b, quantise(y[0, :, :37, :50]))
    assert np.array_equal(png("p", "RES", "b.png"), quantise(((xp - y).cpu() * 2)[0, :, :37, :50]))
    assert np.array_equal(png("p", "TAR", "b.png"), tars[1][1])                 # the target, uncropped
    # device statistics == the folders read back
    psnr, ssim, pmax, smax, pmin, smin = TS.evaluate_folders(str(tmp_path / "p" / "TAR"), str(tmp_path / "p" / "OUT"))
    for key, want in (("psnr", psnr), ("ssim", ssim), ("psnr_best", pmax), ("ssim_best", smax), ("psnr_worst", pmin), ("ssim_worst", smin)):
        assert abs(r[key] - want) < 1e-9, (key, r[key], want)
    assert "PSNR: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(psnr, pmax, pmin) in printed
    assert "SSIM: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(ssim, smax, smin) in printed
    # --metrics folders on the padded path reports the same numbers from the PNGs
    rf = TS.main(base + dirs("f") + ["--pad", "reflect"])
    assert rf["images"] == 2 and abs(rf["psnr"] - psnr) < 1e-9 and abs(rf["ssim"] - ssim) < 1e-9
    assert np.array_equal(png("f", "OUT", "b.png"), out_b)
    # one 64 x 64 tile covers the padded image: the whole-image call, bit for bit
    r1 = TS.main(base + dirs("t") + ["--pad", "reflect", "--metrics", "device", "--tile", "64"])
    assert r1["images"] == 2 and np.array_equal(png("t", "OUT", "b.png"), out_b) and r1["psnr"] == r["psnr"]
    # the same arguments without --pad: the reference's crop (and, for multiples of 4 that are no multiples of 8, its skip)
    r0 = TS.main(base + dirs("w"))
    if kind == "mprnet":
        assert r0["images"] == 2 and png("w", "OUT", "b.png").shape == (36, 48, 3)
    else:
        assert r0["images"] == 1 and os.listdir(tmp_path / "w" / "OUT") == ["a.png"]
    assert set(r0) == set(r)
    # tester_noise.py's input with padding: no first row / column dropped
    rn = TS.main(base + dirs("n") + ["--noise_sigma", "25", "--pad", "reflect", "--seed", "3", "--metrics", "device"])
    assert rn["images"] == 2 and png("n", "OUT", "b.png").shape == (37, 50, 3) and np.isfinite(rn["psnr"])
