"""GPU tier: the validation suite (rcot_amd/valsuite.py) on small folders — 40 x 56 and 56 x 40 images, six per set, a seeded network.

 1. ``--val_batch 1``, a paired set with default keys: per image the figures of the single-folder validation's own steps
    (restore_any_size + image_egress), exactly — the same launches;
 2. sets made on the fly (jpeg_q10, a chain with noise and a seed) against paired sets whose DEGSET the folder tools wrote, exactly;
 3. color=y ssim=gauss11 shave=4 psnrb against ``tester.evaluate_folders`` on the PNGs of the same restored images (integers under PSNR
    and PSNR-B on both sides: equal; SSIM within 1e-9, as tests/test_psnrb_gpu.py compares device and host);
 4. ``--val_batch 0``: the same images in the same groups, every figure equal to the single-image kernels applied to the batched
    call's own output tensor;
 5. the trainer: two epochs with two sets and --save_best, then --resume.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from synth_folders import write_png

pytestmark = pytest.mark.gpu
SIZES = [(40, 56), (56, 40)] * 3


@pytest.fixture(scope="module")
def net():
    from rcot_amd import params as P
    from rcot_amd.net_restormer import T_net
    from rcot_amd.ops import HipBackend
    n = T_net(decoder=True, backend=HipBackend())
    n.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()})
    return n


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """<root>/tar/ six smooth targets, <root>/deg/ their noisy twins (host noise)"""
    root = str(tmp_path_factory.mktemp("valsuite"))
    g = np.random.Generator(np.random.PCG64(2))
    for i, (h, w) in enumerate(SIZES):
        t = np.clip(128 + 70 * np.sin(np.linspace(0, 5 + i, h))[:, None, None] * np.cos(np.linspace(0, 4, w))[None, :, None]
                    + g.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        write_png(f"{root}/tar/{i}.png", t)
        write_png(f"{root}/deg/{i}.png", np.clip(t + g.normal(0, 20, t.shape), 0, 255).astype(np.uint8))
    return root


def _suite(net, sets, batch=1, pad="reflect"):
    from rcot_amd import valsuite as V
    return V.ValSuite(net.be, V.parse_val_sets(sets), net.size_multiple, pad, batch, 1.0, verbose=False)


def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def _same(a, b):
    """two per-image figure lists: equal floats, key for key"""
    assert len(a) == len(b) == len(SIZES)
    for x, y in zip(a, b):
        assert x == y, (x, y)


# ============================================================================= 1
def test_paired_set_equals_the_single_folder_steps(net, tree):
    from rcot_amd.wholeimage import image_metrics, restore_any_size
    be = net.be
    suite = _suite(net, [["noisy", "paired", f"{tree}/tar/", f"{tree}/deg/"]])
    res = suite.run(net)
    r = res["sets"]["noisy"]
    want = []
    for i, (h, w) in enumerate(SIZES):                                  # trainer._evaluate_padded's steps, pair by pair
        rr = restore_any_size(net, torch.from_numpy(_png(f"{tree}/deg/{i}.png")), 8, "reflect")
        tar = torch.from_numpy(_png(f"{tree}/tar/{i}.png")).to(be.device)
        st = be.image_egress(rr.out, h, w, target=tar, want_out=False, want_stats=True)[2]
        want.append(dict(name=f"{i}.png", **image_metrics(st, h, w)))
    _same(r["images"], want)                                            # in the order of the listing
    assert all(np.isfinite(d["psnr_float"]) and np.isfinite(d["ssim"]) for d in want)
    assert r["count"] == 6 and "psnrb" not in r
    for f in ("psnr_float", "psnr_u8", "ssim"):
        v = [d[f] for d in r["images"]]
        assert r[f] == {"mean": sum(v) / 6, "min": min(v), "max": max(v)}
        assert res["mean"][f] == r[f]["mean"]
    assert suite.groups("noisy") == {(40, 56): ["0.png", "2.png", "4.png"], (56, 40): ["1.png", "3.png", "5.png"]}
    assert suite.cache.images == 12 and suite.cache.bytes == 2 * 6 * 3 * 40 * 56


# ============================================================================= 2
def test_sets_made_on_the_fly_equal_the_folder_tools(net, tree, tmp_path):
    from rcot_amd import chain as C
    from rcot_amd import jpeg as J
    assert J.main(["--in", f"{tree}/tar", "--out", f"{tmp_path}/q10", "--quality", "10"]) == 6
    assert C.main(["--in", f"{tree}/tar", "--out", f"{tmp_path}/ch", "--chain", "blur_g1.6+noise_g10+jpeg_q40", "--seed", "3"]) == 6
    assert C.main(["--in", f"{tree}/tar", "--out", f"{tmp_path}/n25", "--chain", "noise_g25", "--seed", "7"]) == 6
    made = _suite(net, [["q10", "jpeg_q10", f"{tree}/tar/"], ["ch", "chain_blur_g1.6+noise_g10+jpeg_q40", f"{tree}/tar/", "seed=3"],
                        ["n25", "denoise_25", f"{tree}/tar/", "seed=7"]])
    paired = _suite(net, [["q10", "paired", f"{tree}/tar/", f"{tmp_path}/q10/"], ["ch", "paired", f"{tree}/tar/", f"{tmp_path}/ch/"],
                          ["n25", "paired", f"{tree}/tar/", f"{tmp_path}/n25/"]])
    for name in ("q10", "ch", "n25"):                                   # the network's input: the tools' bytes
        for a, b in zip(made.sets[name][0], paired.sets[name][0]):
            assert torch.equal(a.deg, b.deg) and torch.equal(a.tar, b.tar), (name, a.name)
    a, b = made.run(net), paired.run(net)
    for name in ("q10", "ch", "n25"):
        _same(a["sets"][name]["images"], b["sets"][name]["images"])
        assert {k: v for k, v in a["sets"][name].items() if k != "task"} == {k: v for k, v in b["sets"][name].items() if k != "task"}
    assert a["mean"] == b["mean"]
    other = _suite(net, [["ch", "chain_blur_g1.6+noise_g10+jpeg_q40", f"{tree}/tar/", "seed=4"]])
    assert not torch.equal(other.sets["ch"][0][0].deg, made.sets["ch"][0][0].deg)               # the seed reaches the noise


# ============================================================================= 3
def test_standard_protocol_equals_evaluate_folders(net, tree, tmp_path):
    from PIL import Image
    from rcot_amd import tester as TS
    from rcot_amd.wholeimage import restore_any_size
    suite = _suite(net, [["y", "paired", f"{tree}/tar/", f"{tree}/deg/", "color=y", "ssim=gauss11", "shave=4", "psnrb"]])
    r = suite.run(net)["sets"]["y"]
    os.makedirs(tmp_path / "out")
    for i, (h, w) in enumerate(SIZES):
        rr = restore_any_size(net, torch.from_numpy(_png(f"{tree}/deg/{i}.png")), 8, "reflect")
        Image.fromarray(net.be.image_egress(rr.out, h, w)[0].cpu().numpy()).save(tmp_path / "out" / f"{i}.png")
    ps, ss, pmax, smax, pmin, smin, pb, pbmax, pbmin = TS.evaluate_folders(f"{tree}/tar", str(tmp_path / "out"), "gauss11", "y", True, 4)
    print("suite", r["psnr_u8"], r["ssim"], r["psnrb"], "folders", (ps, pmax, pmin), (ss, smax, smin), (pb, pbmax, pbmin))
    assert r["count"] == 6
    assert (r["psnr_u8"]["mean"], r["psnr_u8"]["max"], r["psnr_u8"]["min"]) == (ps, pmax, pmin)
    assert (r["psnrb"]["mean"], r["psnrb"]["max"], r["psnrb"]["min"]) == (pb, pbmax, pbmin)
    for got, want in ((r["ssim"]["mean"], ss), (r["ssim"]["max"], smax), (r["ssim"]["min"], smin)):
        assert abs(got - want) < 1e-9, (got, want)
    assert np.isfinite(r["psnr_float"]["mean"])


# ============================================================================= 4
@pytest.mark.parametrize("batch", [0, 2])
def test_batched_calls_same_images_same_groups(net, tree, batch):
    from rcot_amd.quality import psnrb_from_sums, quality_metrics
    from rcot_amd.wholeimage import image_metrics
    be = net.be
    sets = [["noisy", "paired", f"{tree}/tar/", f"{tree}/deg/"],
            ["std", "jpeg_q10", f"{tree}/tar/", "color=y", "ssim=uniform7", "shave=3", "psnrb"]]
    one, many = _suite(net, sets, 1), _suite(net, sets, batch)
    res = many.run(net, keep_outputs=True)
    for name in ("noisy", "std"):
        assert many.groups(name) == one.groups(name)
        r = res["sets"][name]
        calls = r["outputs"]
        assert [len(names) for _, names in calls] == ([3, 3] if batch == 0 else [2, 1, 2, 1])
        assert [n for _, names in calls for n, _, _ in names] == ["0.png", "2.png", "4.png", "1.png", "3.png", "5.png"]     # group by group
        tars = {im.name: im.tar for im in many.sets[name][0]}
        want = []
        for out, names in calls:
            assert out.shape[0] == len(names)
            for slot, (n, h, w) in enumerate(names):
                o, _, st = be.image_egress(out[slot], h, w, target=tars[n], want_out=True, want_stats=True)
                fig = image_metrics(st, h, w)
                if name == "std":
                    t3, o3 = be.crop_u8(tars[n], 3, 3, h - 6, w - 6), be.crop_u8(o, 3, 3, h - 6, w - 6)
                    q = quality_metrics(be.image_quality(t3, o3, "uniform7", "y"))
                    fig.update(psnr_u8=q["psnr"], ssim=q["ssim"],
                               psnrb=psnrb_from_sums(be.image_blockiness(o3, t3, "y", 3, 3).cpu().numpy(), h - 6, w - 6, 3, 3))
                want.append(dict(name=n, **fig))
        _same(r["images"], sorted(want, key=lambda d: d["name"]))
        assert r["count"] == 6 and ("psnrb" in r) == (name == "std")
    assert set(res["mean"]) == {"psnr_float", "psnr_u8", "ssim", "psnrb"}
    assert res["mean"]["psnrb"] == res["sets"]["std"]["psnrb"]["mean"]


# ============================================================================= 5
def _py(args, cwd):
    return subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=600, cwd=cwd,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_trainer_two_epochs_save_best_and_resume(tree, tmp_path):
    from rcot_amd.compat import load_checkpoint
    tmp = str(tmp_path)
    base = ["rcot_amd.trainer", "--synthetic", "--iters", "2", "--batchSize", "1", "--patch_size", "32", "--de_type", "denoise_15", "--seed", "5",
            "--type", "SuiteTest", "--sigma", "1",
            "--val_set", "noisy", "paired", f"{tree}/tar/", f"{tree}/deg/",
            "--val_set", "q10", "jpeg_q10", f"{tree}/tar/", "psnrb", "--save_best", "--val_batch", "0"]
    r1 = _py(base + ["--nEpochs", "2"], tmp)
    assert r1.returncode == 0, r1.stderr[-3000:]
    lines = [json.loads(ln) for ln in open(os.path.join(tmp, "checksample", "SuiteTest", "validation_suite.jsonl"))]
    assert [o["epoch"] for o in lines] == [1, 2] and all(o["weights"] == "raw" for o in lines)
    for o in lines:
        assert set(o["sets"]) == {"noisy", "q10"} and o["sets"]["noisy"]["count"] == o["sets"]["q10"]["count"] == 6
        assert set(o["mean"]) == {"psnr_float", "psnr_u8", "ssim", "psnrb"}
        assert o["mean"]["psnr_float"] == (o["sets"]["noisy"]["psnr_float"]["mean"] + o["sets"]["q10"]["psnr_float"]["mean"]) / 2
    legacy = open(os.path.join(tmp, "checksample", "SuiteTest", "validation_results.txt")).read().splitlines()
    assert legacy == [f"Patchsize 32 Epoch {o['epoch']}, psnr {o['mean']['psnr_float']:.4f}, Batchsize 1" for o in lines]
    assert "validation suite" in r1.stdout and r1.stdout.count("----------validating-----------") == 2
    ck_path = os.path.join(tmp, "checkpoint", "model_SuiteTest__2_1.0.pth")
    best_path = os.path.join(tmp, "checkpoint", "model_SuiteTest__2_1.0_best.pth")
    ck, bk = load_checkpoint(ck_path), load_checkpoint(best_path)
    values = [o["mean"]["psnr_float"] for o in lines]
    want_epoch = 2 if values[1] > values[0] else 1
    assert ck["best"] == {"key": "mean.psnr_float", "value": max(values), "epoch": want_epoch} and ck["epoch"] == 2
    assert bk["best"] == ck["best"] and bk["epoch"] == want_epoch
    # --resume continues the record
    r2 = _py(base + ["--nEpochs", "3", "--resume", ck_path], tmp)
    assert r2.returncode == 0, r2.stderr[-3000:]
    o3 = json.loads(open(os.path.join(tmp, "checksample", "SuiteTest", "validation_suite.jsonl")).read().splitlines()[-1])
    ck3 = load_checkpoint(os.path.join(tmp, "checkpoint", "model_SuiteTest__3_1.0.pth"))
    v3 = o3["mean"]["psnr_float"]
    assert o3["epoch"] == 3
    if v3 > max(values):
        assert ck3["best"] == {"key": "mean.psnr_float", "value": v3, "epoch": 3}
        assert os.path.isfile(os.path.join(tmp, "checkpoint", "model_SuiteTest__3_1.0_best.pth"))
    else:
        assert ck3["best"] == ck["best"] and not os.path.exists(os.path.join(tmp, "checkpoint", "model_SuiteTest__3_1.0_best.pth"))


# ============================================================================= 6
def test_standalone_tool_on_a_checkpoint(net, tree, tmp_path, capsys):
    """python -m rcot_amd.valsuite's ``main`` on a checkpoint that holds the seeded network: the suite's own figures, the table, the JSON line"""
    from rcot_amd import params as P
    from rcot_amd import valsuite as V
    from rcot_amd.compat import shim
    sd = {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()}
    ck = str(tmp_path / "net.pth")
    torch.save({"epoch": 1, "Tnet": shim().T_net.from_state_dict(sd, decoder=True)}, ck)
    sets = [["noisy", "paired", f"{tree}/tar/", f"{tree}/deg/"], ["q10", "jpeg_q10", f"{tree}/tar/", "psnrb", "color=y", "ssim=uniform7"]]
    argv = ["--model", ck, "--val_batch", "2", "--out", str(tmp_path / "out.jsonl")]
    for s in sets:
        argv += ["--val_set"] + s
    obj = V.main(argv)
    printed = capsys.readouterr().out
    want = V.json_ready(_suite(net, sets, 2).run(net))
    assert obj["sets"] == want["sets"] and obj["mean"] == want["mean"] and obj["weights"] == "raw"
    assert json.loads(open(tmp_path / "out.jsonl").read()) == json.loads(json.dumps(obj))
    table = printed[printed.index("validation suite, weights raw"):].splitlines()
    assert [ln.split()[0] for ln in table[2:5]] == ["noisy", "q10", "mean"]
    with pytest.raises(SystemExit, match="Tnet_ema"):
        V.main(argv + ["--weights", "ema"])


# ============================================================================= 7
def test_validate_on_raw_averaged_and_both_weights(net, tree, capsys):
    """``valsuite.validate`` as the trainer calls it: with an average that differs from the raw weights (its buffer scaled), ``ema`` and
    ``both`` report the averaged weights' figures under "sets" / "mean", ``both`` carries the two under "weights", and the raw weights
    are back afterwards"""
    from rcot_amd import valsuite as V
    from rcot_amd.ema import WeightAverage
    suite = _suite(net, [["noisy", "paired", f"{tree}/tar/", f"{tree}/deg/"]], 2)
    raw = V.validate(suite, net, None, None, 1, say=print)
    assert raw["weights"] == "raw" and raw["epoch"] == 1
    avg = WeightAverage(net, 0.9)
    avg.buf.mul_(0.999)
    before = net.store.flat.clone()
    both = V.validate(suite, net, avg, "both", 2, "ema0.9")
    ema = V.validate(suite, net, avg, "ema", 3, "ema0.9")
    only_raw = V.validate(suite, net, avg, "raw", 4, "ema0.9")
    assert torch.equal(net.store.flat, before)
    assert set(both["weights"]) == {"raw", "ema"} and both["weights"]["raw"]["sets"] == raw["sets"] == only_raw["sets"]
    assert both["sets"] == both["weights"]["ema"]["sets"] == ema["sets"] and ema["weights"] == "ema0.9"
    assert both["mean"]["psnr_float"] != raw["mean"]["psnr_float"]
    out = capsys.readouterr().out
    assert out.count("validation suite, weights raw") == 2 and out.count("validation suite, weights ema0.9") == 2
    assert V.validate(suite, net, None, None, 5, say=lambda s: None)["sets"] == raw["sets"]      # and the raw figures are what they were


# ============================================================================= 8
def test_sr_and_blur_sets_on_the_mprnet_backbone(tree):
    """sr_x2, sr_bd_x3 (cropped to multiples of 3, then padded to the backbone's multiple 4) and blur_g1.6 sets through MPRNetHip at two
    images per call: the resident twins are ``degrade.degrade_file_u8``'s, every image is processed, the figures are finite"""
    from rcot_amd import degrade as D
    from rcot_amd import valsuite as V
    from rcot_amd.mprnet_hip import MPRNetHip
    mp = MPRNetHip(seed=0)
    specs = V.parse_val_sets([["x2", "sr_x2", f"{tree}/tar/", "shave=2", "color=y", "ssim=gauss11"], ["bd", "sr_bd_x3", f"{tree}/tar/"],
                              ["blur", "blur_g1.6", f"{tree}/tar/", "border=mirror"]])
    suite = V.ValSuite(mp.be, specs, mp.size_multiple, "reflect", 2, 1.0, verbose=False)
    assert mp.size_multiple == 4
    for s in specs:
        images, groups = suite.sets[s.name]
        assert len(images) == 6 and sorted(i for g in groups.values() for i in g) == list(range(6))
        clean, deg = D.degrade_file_u8(_png(f"{tree}/tar/1.png"), s.sid, None, mp.be, "target")
        assert np.array_equal(images[1].tar.cpu().numpy(), clean) and np.array_equal(images[1].deg.cpu().numpy(), deg)
        assert (images[1].h, images[1].w) == ((54, 39) if s.name == "bd" else (56, 40))
    assert suite.groups("bd") == {(40, 56): ["0.png", "2.png", "4.png"], (56, 40): ["1.png", "3.png", "5.png"]}
    res = suite.run(mp)
    for s in specs:
        r = res["sets"][s.name]
        assert r["count"] == 6 and all(np.isfinite(r[f][k]) for f in ("psnr_float", "psnr_u8", "ssim") for k in ("mean", "min", "max")), r
