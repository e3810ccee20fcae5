"""CPU tier of whole-image validation at any size (rcot_amd/wholeimage.py, csrc/imageio.hip): the oracle on the padded inputs against
the REFERENCE's outputs (tests/golden/anysize.npz, scripts/make_anysize_fixture.py), the padding geometry, the new CLI flags, and the
numpy restatement of the egress kernel's four statistics — the test double the GPU tier (tests/test_anysize_gpu.py) holds the kernel
to — against the host metrics the CLIs use today."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr, seeded_tensor
from oracle import rcot_oracle as O
from rcot_amd import params as P


# ------------------------------------------------------------------ the test double of rcot_image_egress
def quantise(t: torch.Tensor) -> np.ndarray:
    """trainer.save_image for one image: float [3, h, w] -> uint8 [h, w, 3], every step an fp32 rounding (torch on the CPU)"""
    return t.detach().float().cpu().clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()


def egress_stats(restored: np.ndarray, target: np.ndarray, out_u8: np.ndarray) -> np.ndarray:
    """The four statistics of rcot_image_egress restated in numpy.  restored float32 [3, h, w] (already cropped), target / out_u8
    uint8 [h, w, 3].  Window moments of the SSIM map in integers (exact), the quotient in fp64."""
    h, w = target.shape[:2]
    t_f = (target.astype(np.float32) / np.float32(255.0)).astype(np.float64)                # correctly rounded fp32 divide
    s0 = float(((restored.astype(np.float64).transpose(1, 2, 0) - t_f) ** 2).sum())
    s1 = int(((out_u8.astype(np.int64) - target.astype(np.int64)) ** 2).sum())
    s2, C1, C2 = 0.0, (0.01 * 255) ** 2, (0.03 * 255) ** 2
    if h > 10 and w > 10:
        a, b = out_u8.astype(np.int64), target.astype(np.int64)          # evaluate.ssim(img1 = target, img2 = output) is symmetric in the pair
        win = lambda v: (v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:])[4:-5, 4:-5]      # 2 x 2 window ending at (y, x), cropped [5:-5]
        Sa, Sb, Saa, Sbb, Sab = win(a), win(b), win(a * a), win(b * b), win(a * b)
        mu1, mu2 = 0.25 * Sa, 0.25 * Sb
        s1_, s2_, s12 = 0.25 * Saa - mu1 * mu1, 0.25 * Sbb - mu2 * mu2, 0.25 * Sab - mu1 * mu2
        s2 = float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1_ + s2_ + C2))).sum())
    return np.array([s0, float(s1), s2, 3.0 * max(0, h - 10) * max(0, w - 10)])


def synth_pair(seed, h, w):
    """(restored float32 [3, h, w] with values a little outside [0, 1] too, target uint8 [h, w, 3])"""
    g = np.random.Generator(np.random.PCG64(seed))
    target = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    restored = (target.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0) + g.normal(0, 0.08, (3, h, w)).astype(np.float32))
    return np.ascontiguousarray(restored, dtype=np.float32), target


# ------------------------------------------------------------------ oracle vs the reference on padded inputs
@pytest.mark.parametrize("mode", ["reflect", "replicate"])
def test_oracle_on_padded_input_vs_reference(gold, mode):
    fx = gold("anysize.npz")
    B, h, w, Hp, Wp, sx, sp = (int(v) for v in fx["restormer_cfg"])
    assert (B, h, w, Hp, Wp) == (1, 37, 50, 40, 56)
    prm = {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), sp, "T").items()}
    x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(sx))
    with torch.no_grad():
        y = O.tnet_forward(prm, F.pad(x, (0, Wp - w, 0, Hp - h), mode=mode), True)[..., :h, :w]
    assert relerr(y, torch.from_numpy(fx[f"restormer_{mode}_y"])) < 1e-5          # test_oracle_golden.py::test_tnet_small's bar


def test_fixture_holds_float32_arrays_only(gold):
    fx = gold("anysize.npz")
    assert sorted(fx.files) == ["eval_psnr_70x90", "mprnet_reflect_y", "restormer_cfg", "restormer_reflect_y", "restormer_replicate_y"]
    assert all(fx[k].dtype == np.float32 for k in fx.files)
    assert fx["restormer_reflect_y"].shape == (1, 3, 37, 50) and fx["mprnet_reflect_y"].shape == (1, 3, 38, 54)
    assert 5.0 < float(fx["eval_psnr_70x90"]) < 40.0


# ------------------------------------------------------------------ geometry, attributes, flags
def test_pad_geometry():
    from rcot_amd.wholeimage import pad_geometry
    for mode in ("none", None, "reflect", "replicate"):
        assert pad_geometry(40, 56, 8, mode) == (40, 56) and pad_geometry(40, 56, 4, mode) == (40, 56)      # nothing to pad
    for mode in ("reflect", "replicate"):
        assert pad_geometry(37, 50, 8, mode) == (40, 56)
        assert pad_geometry(37, 50, 4, mode) == (40, 52)
    assert pad_geometry(481, 321, 8, "reflect") == (488, 328)
    with pytest.raises(ValueError, match="reflect"):
        pad_geometry(3, 50, 8, "reflect")                    # 5 mirrored rows wanted, 2 available
    with pytest.raises(ValueError, match="reflect"):
        pad_geometry(50, 3, 8, "reflect")
    assert pad_geometry(3, 50, 8, "replicate") == (8, 56)
    assert pad_geometry(5, 5, 8, "reflect") == (8, 8)        # 3 <= h - 1 = 4
    with pytest.raises(ValueError, match="multiple of 8"):
        pad_geometry(37, 50, 8, "none")
    with pytest.raises(ValueError):
        pad_geometry(37, 50, 8, "circular")


def test_networks_name_their_size_multiple():
    import Net_Restormer
    from rcot_amd.mprnet_hip import MPRNetHip
    from rcot_amd.net_restormer import T_net
    assert T_net.size_multiple == 8 and MPRNetHip.size_multiple == 4
    assert Net_Restormer.T_net.size_multiple == 8            # the checkpoint shim resolves it through the same class


def test_parsers_accept_the_new_flags():
    from rcot_amd import tester as TS
    from rcot_amd import trainer as TR
    d = TS.parser.parse_args([])
    assert d.pad == "none" and d.metrics == "folders"
    o = TS.parser.parse_args(["--pad", "reflect", "--metrics", "device"])
    assert o.pad == "reflect" and o.metrics == "device"
    assert TS.parser.parse_args(["--pad", "replicate"]).pad == "replicate"
    assert TR.parser.parse_args([]).val_pad == "none"
    assert TR.parser.parse_args(["--val_pad", "reflect"]).val_pad == "reflect"
    for p, flag in ((TS.parser, "--pad"), (TS.parser, "--metrics"), (TR.parser, "--val_pad")):
        with pytest.raises(SystemExit):
            p.parse_args([flag, "zeros"])


# ------------------------------------------------------------------ the restated statistics vs the host metrics of today
@pytest.mark.parametrize("h,w", [(13, 19), (37, 50)])
def test_restated_statistics_agree_with_host_metrics(h, w):
    from rcot_amd import tester as TS
    from rcot_amd import trainer as TR
    from rcot_amd.wholeimage import image_metrics
    restored, target = synth_pair(100 + h, h, w)
    out_u8 = quantise(torch.from_numpy(restored))
    s = egress_stats(restored, target, out_u8)
    assert s[3] == 3 * (h - 10) * (w - 10)
    m = image_metrics(s, h, w)
    want_f = TR.psnr(restored.transpose(1, 2, 0), target.astype(np.float32) / 255.0, data_range=1)
    assert abs(m["psnr_float"] - want_f) <= 1e-12 * abs(want_f)
    want_8 = TS.psnr_uint8(target, out_u8)
    assert abs(m["psnr_u8"] - want_8) <= 1e-12 * abs(want_8)
    assert abs(m["ssim"] - TS.ssim_image(target, out_u8)) <= 1e-12


def test_image_metrics_conventions():
    from rcot_amd.wholeimage import image_metrics
    restored, target = synth_pair(7, 9, 15)
    s = egress_stats(restored, target, quantise(torch.from_numpy(restored)))
    assert s[3] == 0 and np.isnan(image_metrics(s, 9, 15)["ssim"])                 # under 11 pixels on a side: an empty map
    m = image_metrics([0.0, 0.0, 27.0, 27.0], 13, 13)
    assert m["psnr_float"] == float("inf") and m["psnr_u8"] == float("inf") and m["ssim"] == 1.0
