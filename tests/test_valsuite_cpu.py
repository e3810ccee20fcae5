"""CPU tier: the host side of the validation suite (rcot_amd/valsuite.py) — ``--val_set`` parsing and every refusal, grouping by padded
shape, the budget, ``--save_best`` — and the host checks of the two batched image entry points (rcot_amd/ops.py)."""
import argparse
import os

import numpy as np
import pytest
import torch

from rcot_amd import valsuite as V
from synth_folders import write_png


def _refused(tokens, *pieces):
    with pytest.raises(SystemExit) as e:
        V.parse_val_sets(tokens if tokens and isinstance(tokens[0], list) else [tokens])
    msg = str(e.value)
    for p in pieces:
        assert p in msg, (p, msg)
    return msg


# ============================================================================= --val_set
def test_parse_paired_and_defaults():
    s, = V.parse_val_sets([["rain", "paired", "val/target/", "val/input/"]])
    assert (s.name, s.task, s.kind, s.tarset, s.degset) == ("rain", "paired", "paired", "val/target/", "val/input/")
    assert (s.color, s.ssim, s.shave, s.psnrb, s.seed, s.border, s.subsampling) == ("rgb", "box2", 0, False, 0, "replicate", "420")
    assert not s.standard and not s.needs_u8 and s.sid is None


def test_parse_made_sets_carry_the_fields_of_the_task_table():
    from rcot_amd import chain as C
    specs = V.parse_val_sets([["n25", "denoise_25", "t/"], ["x3", "sr_x3", "t/", "shave=3", "ssim=gauss11", "color=y"],
                              ["bd", "sr_bd_x3", "t/"], ["q10", "jpeg_q10", "t/", "psnrb", "subsampling=444"],
                              ["blur", "blur_g1.6", "t/", "border=mirror"],
                              ["ch", "chain_blur_g1.6+noise_g10+jpeg_q40", "t/", "seed=3", "ssim=uniform7"]])
    by = {s.name: s for s in specs}
    assert all(s.kind == "made" and s.degset is None for s in specs)
    assert by["n25"].sid["chain"][0] == C.parse_spec("noise_g25")                 # denoise_<sigma> is the chain noise_g<sigma>
    assert by["x3"].sid == {"sr": 3} and (by["x3"].shave, by["x3"].ssim, by["x3"].color) == (3, "gauss11", "y") and by["x3"].needs_u8
    assert by["bd"].sid == {"sr": 3, "bd": True}
    assert by["q10"].sid == {"jpeg": (10, 0)} and by["q10"].psnrb and by["q10"].needs_u8 and not by["q10"].standard
    assert by["blur"].sid == {"blur": ("g1.6", "mirror")}
    assert by["ch"].sid["chain"] == (C.parse_spec("blur_g1.6+noise_g10+jpeg_q40"), "replicate", 2) and by["ch"].seed == 3
    assert by["ch"].standard


def test_refusals_name_the_set_and_the_piece():
    _refused(["a", "paired", "t/", "d/", "colour=y"], "--val_set a", "key 'colour'", "unknown")
    _refused([["a", "paired", "t/", "d/"], ["a", "jpeg_q10", "t/"]], "--val_set a", "NAME", "given twice")
    _refused(["a", "paired", "t/", "d/", "shave=4"], "--val_set a", "shave=4", "ssim=box2")
    _refused(["a", "paired", "t/", "d/", "shave=4", "ssim=box2"], "--val_set a", "shave=4")
    _refused(["a", "paired", "t/"], "--val_set a", "paired", "needs DEGSET")
    _refused(["a", "jpeg_q10", "t/", "d/"], "--val_set a", "DEGSET 'd/'", "no DEGSET is read")
    _refused(["a", "denoise_25", "t/", "d/"], "--val_set a", "DEGSET 'd/'")
    _refused(["a", "jpeg_q0", "t/"], "--val_set a", "task 'jpeg_q0'")
    _refused(["a", "jpeg_q101", "t/"], "--val_set a", "task 'jpeg_q101'")
    _refused(["a", "chain_blur_g1.6+fog", "t/"], "--val_set a", "task 'chain_blur_g1.6+fog'", "'fog'")
    _refused(["a", "blur_m15", "t/"], "--val_set a", "task 'blur_m15'", "angle")
    _refused(["a", "denoise_x", "t/"], "--val_set a", "task 'denoise_x'", "denoise_<sigma>")
    _refused(["a", "denoise_300", "t/"], "--val_set a", "task 'denoise_300'", "outside 0 .. 255")
    _refused(["a", "derain", "t/"], "--val_set a", "task 'derain'", "expected paired")
    _refused(["a", "paired"], "--val_set a", "NAME TASK TARSET")
    _refused(["a", "paired", "t/", "d/", "e/"], "--val_set a", "argument 'e/'")
    _refused(["a", "paired", "t/", "d/", "color=yuv"], "--val_set a", "color=yuv")
    _refused(["a", "paired", "t/", "d/", "ssim=gauss7"], "--val_set a", "ssim=gauss7")
    _refused(["a", "paired", "t/", "d/", "color=y"], "--val_set a", "color=y", "host only")
    _refused(["a", "paired", "t/", "d/", "shave=-1", "ssim=uniform7"], "--val_set a", "shave=-1")
    _refused(["a", "paired", "t/", "d/", "seed=x"], "--val_set a", "seed=x", "integer")
    _refused(["a", "paired", "t/", "d/", "seed=1", "seed=2"], "--val_set a", "key 'seed'", "twice")
    _refused(["a", "jpeg_q10", "t/", "subsampling=422"], "--val_set a", "subsampling=422")
    _refused(["a", "blur_g1.6", "t/", "border=zero"], "--val_set a", "border=zero")
    _refused(["mean", "paired", "t/", "d/"], "--val_set mean", "NAME")
    _refused(["a.b", "paired", "t/", "d/"], "--val_set a.b", "NAME")


def test_an_empty_folder_is_refused(tmp_path):
    os.makedirs(tmp_path / "t")
    os.makedirs(tmp_path / "d")
    spec = V.parse_val_sets([["a", "paired", f"{tmp_path}/t/", f"{tmp_path}/d/"]])
    with pytest.raises(SystemExit, match="--val_set a: TARSET .*no files"):
        V.list_sets(spec)
    write_png(f"{tmp_path}/t/0.png", np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(SystemExit, match="--val_set a: DEGSET .*no files"):
        V.list_sets(spec)
    write_png(f"{tmp_path}/d/0.png", np.zeros((8, 8, 3), np.uint8))
    assert V.list_sets(spec) == {"a": [(0, f"{tmp_path}/t/0.png", f"{tmp_path}/d/0.png")]}


# ============================================================================= geometry, budget
def test_grouping_by_padded_shape():
    sizes = [(40, 56), (56, 40), (37, 50), (40, 56), (3, 9), (50, 33)]
    groups, skipped = V.group_by_shape(sizes, 8, "reflect")
    assert list(groups.items()) == [((40, 56), [0, 2, 3]), ((56, 40), [1, 5])]
    assert [i for i, _ in skipped] == [4] and "reflect" in skipped[0][1]                     # 3 rows cannot mirror 5
    groups, skipped = V.group_by_shape(sizes, 8, "replicate")
    assert groups[(8, 16)] == [4] and not skipped
    groups, skipped = V.group_by_shape(sizes, 8, "none")
    assert list(groups.items()) == [((40, 56), [0, 3]), ((56, 40), [1])] and [i for i, _ in skipped] == [2, 4, 5]
    assert V.chunks([0, 2, 3, 7, 9], 1) == [[0], [2], [3], [7], [9]]
    assert V.chunks([0, 2, 3, 7, 9], 2) == [[0, 2], [3, 7], [9]]
    assert V.chunks([0, 2, 3, 7, 9], 0) == [[0, 2, 3, 7, 9]]


def test_budget_refusal_names_the_gigabytes(tmp_path):
    for i, (h, w) in enumerate(((40, 56), (56, 40), (31, 47))):
        write_png(f"{tmp_path}/t/{i}.png", np.zeros((h, w, 3), np.uint8))
        write_png(f"{tmp_path}/d/{i}.png", np.zeros((h, w, 3), np.uint8))
    specs = V.parse_val_sets([["p", "paired", f"{tmp_path}/t/", f"{tmp_path}/d/"], ["x3", "sr_x3", f"{tmp_path}/t/"]])
    listing = V.list_sets(specs)
    full = 2 * 3 * (40 * 56 + 56 * 40 + 31 * 47)
    x3 = 2 * 3 * (39 * 54 + 54 * 39 + 30 * 45)                                                # cropped to multiples of 3 first
    assert V.bytes_needed(specs, listing) == full + x3
    assert V.check_budget(specs, listing, 1.0) == full + x3
    huge = lambda path: (40000, 50000)
    with pytest.raises(SystemExit) as e:
        V.check_budget(specs, listing, 8.0, size_of=huge)
    need = 2 * 3 * 3 * (40000 * 50000 + 39999 * 49998) / 2 ** 30
    assert f"{need:.3f} GiB" in str(e.value) and "--val_cache_gb is 8" in str(e.value) and "2 set(s), 6 files" in str(e.value)


# ============================================================================= --save_best
def _result(a, b, pb=None):
    fig = lambda v: {"mean": v, "min": v - 1, "max": v + 1}
    sets = {"a": {"task": "paired", "count": 2, "psnr_float": fig(a), "psnr_u8": fig(a), "ssim": fig(0.5)},
            "b": {"task": "jpeg_q10", "count": 2, "psnr_float": fig(b), "psnr_u8": fig(b), "ssim": fig(0.7)}}
    if pb is not None:
        sets["b"]["psnrb"] = fig(pb)
    return {"sets": sets, "mean": V.mean_over_sets(sets)}


def test_save_best_key_and_the_improve_keep_logic():
    specs = V.parse_val_sets([["a", "paired", "t/", "d/"], ["b", "jpeg_q10", "t/", "psnrb"]])
    assert V.parse_best_key("mean.psnr_float", specs) == ("mean", "psnr_float")
    assert V.parse_best_key("b.psnrb", specs) == ("b", "psnrb") and V.parse_best_key("mean.psnrb", specs) == ("mean", "psnrb")
    for bad, piece in (("psnr_float", "<set|mean>.<figure>"), ("c.ssim", "a, b, mean"), ("a.lpips", "'lpips'"), ("a.psnrb", "psnrb")):
        with pytest.raises(SystemExit) as e:
            V.parse_best_key(bad, specs)
        assert f"--save_best {bad}" in str(e.value) and piece in str(e.value)
    r = _result(30.0, 20.0, 19.0)
    assert r["mean"] == {"psnr_float": 25.0, "psnr_u8": 25.0, "ssim": 0.6, "psnrb": 19.0}      # psnrb: over the sets that report it
    best = V.Best("mean.psnr_float", "mean", "psnr_float")
    assert best.update(r, 1) and best.state_dict() == {"key": "mean.psnr_float", "value": 25.0, "epoch": 1}
    assert not best.update(_result(30.0, 20.0), 2) and best.epoch == 1                         # equal: kept
    assert not best.update(_result(29.0, 20.0), 3)
    assert not best.update(_result(float("nan"), 40.0), 4)                                      # NaN never wins
    assert best.update(_result(31.0, 20.0), 5) and (best.value, best.epoch) == (25.5, 5)
    other = V.Best("b.psnrb", "b", "psnrb")
    assert other.update(r, 1) and other.value == 19.0
    # --resume: the record continues under the same key, starts over under another
    again = V.Best("mean.psnr_float", "mean", "psnr_float")
    assert again.load_state_dict(best.state_dict()) is None and (again.value, again.epoch) == (25.5, 5)
    assert not again.update(_result(30.5, 20.0), 6)
    note = other.load_state_dict(best.state_dict())
    assert "mean.psnr_float" in note and other.value == 19.0
    assert V.Best("a.ssim", "a", "ssim").load_state_dict(None) is None
    assert V.best_path("checkpoint/model_x__2_1.0.pth") == "checkpoint/model_x__2_1.0_best.pth"


def test_table_and_json():
    r = _result(30.0, 20.0, 19.0)
    r["sets"]["a"]["images"] = [{"name": "0.png"}]
    t = V.format_table(r, ", weights raw")
    assert t.splitlines()[0] == "validation suite, weights raw" and "psnrb" in t.splitlines()[1]
    assert [ln.split()[0] for ln in t.splitlines()[2:]] == ["a", "b", "mean"] and " 25.0000" in t.splitlines()[-1]
    j = V.json_ready(r)
    assert "images" not in j["sets"]["a"] and j["mean"]["psnr_float"] == 25.0 and j["sets"]["b"]["psnrb"]["mean"] == 19.0


# ============================================================================= the trainer's flags
def test_without_val_set_the_options_are_what_they_were():
    from rcot_amd import trainer as TR
    o = TR.parser.parse_args([])
    assert (o.val_set, o.val_batch, o.val_cache_gb, o.save_best, o.val_pad) == (None, 8, 8.0, None, "none")
    assert V.check_flags(o) == [] and o.val_pad == "none"
    o = TR.parser.parse_args(["--val_pad", "replicate"])
    assert V.check_flags(o) == [] and o.val_pad == "replicate"
    for flags, name in ((["--save_best"], "save_best"), (["--val_batch", "4"], "val_batch"), (["--val_cache_gb", "2"], "val_cache_gb")):
        with pytest.raises(SystemExit, match=f"--{name} .*needs --val_set"):
            V.check_flags(TR.parser.parse_args(flags))


def test_with_val_sets_the_trainer_flags(monkeypatch):
    from rcot_amd import trainer as TR
    argv = ["--val_set", "a", "paired", "t/", "d/", "--val_set", "q", "jpeg_q10", "t/", "psnrb", "--save_best", "--val_batch", "0"]
    o = TR.parser.parse_args(argv)
    assert o.val_set == [["a", "paired", "t/", "d/"], ["q", "jpeg_q10", "t/", "psnrb"]] and o.save_best == "mean.psnr_float"
    explicit = TR.parser.parse_args(argv, namespace=argparse.Namespace(val_pad=None)).val_pad is not None
    specs = V.check_flags(o, explicit_pad=explicit)
    assert [s.name for s in specs] == ["a", "q"] and o.val_pad == "reflect" and not explicit  # reflect once a set is given
    o = TR.parser.parse_args(argv + ["--val_pad", "replicate", "--save_best", "q.psnrb"])
    explicit = TR.parser.parse_args(argv + ["--val_pad", "replicate"], namespace=argparse.Namespace(val_pad=None)).val_pad is not None
    V.check_flags(o, explicit_pad=explicit)
    assert explicit and o.val_pad == "replicate" and o.save_best == "q.psnrb"
    with pytest.raises(SystemExit, match="--save_best a.psnrb"):
        V.check_flags(TR.parser.parse_args(argv + ["--save_best", "a.psnrb"]))
    with pytest.raises(SystemExit, match="--val_batch -1"):
        V.check_flags(TR.parser.parse_args(argv + ["--val_batch", "-1"]))
    with pytest.raises(SystemExit, match="--val_cache_gb 0"):
        V.check_flags(TR.parser.parse_args(argv + ["--val_cache_gb", "0"]))
    with pytest.raises(SystemExit, match="--val_set needs the HIP path"):
        V.check_flags(TR.parser.parse_args(argv), stock_mprnet=True)
    monkeypatch.setenv("RCOT_MPRNET_STOCK", "1")                                               # the stock-ops trainer path, with or without a GPU
    with pytest.raises(SystemExit, match="--val_set needs the HIP path"):
        TR.main(["--synthetic", "--iters", "1", "--nEpochs", "1", "--backbone", "mprnet"] + argv)


# ============================================================================= the host checks of the batched entry points
def test_batched_entry_points_check_their_rows_on_the_host():
    from rcot_amd.ops import HipBackend, check_egress_rows, check_ingest_rows
    cpu = torch.device("cpu")
    u8 = lambda h, w: torch.zeros(h, w, 3, dtype=torch.uint8)
    imgs = [u8(13, 21), u8(16, 24), u8(9, 17)]
    out = torch.zeros(3, 3, 16, 24)
    check_ingest_rows(imgs, 16, 24, "reflect", out, cpu)
    check_ingest_rows(imgs, 16, 24, "replicate", None, cpu)
    for bad, kw, piece in (([], {}, "1 .. 65535 rows"), (imgs, {"mode": "wrap"}, "padding mode 'wrap'"), (imgs, {"mode": "none"}, "row 0: none cannot pad"),
                           (imgs, {"Hp": 24, "out": None}, "row 2: reflect cannot pad 9 x 17 to 24 x 24"),     # 15 > 8
                           (imgs, {"Wp": 20, "out": None}, "row 0: reflect cannot pad"),
                           (imgs[:2] + [u8(9, 18)[:, :17]], {}, "row 2: the image must be a contiguous"),
                           (imgs[:2] + [torch.zeros(9, 17, 3)], {}, "row 2"), (imgs, {"out": torch.zeros(2, 3, 16, 24)}, "out must be")):
        a = dict(Hp=16, Wp=24, mode="reflect", out=out)
        a.update(kw)
        with pytest.raises(ValueError) as e:
            check_ingest_rows(bad, a["Hp"], a["Wp"], a["mode"], a["out"], cpu)
        assert piece in str(e.value), (piece, str(e.value))
    sizes = [(13, 21), (16, 24), (9, 17)]
    check_egress_rows(out, sizes, imgs, [True, False, True], True, cpu)
    check_egress_rows(out, sizes, None, [True] * 3, False, cpu)
    for a, piece in (((out, [], imgs, [], True), "1 .. 65535"), ((out[:2], sizes, imgs, [True] * 3, True), "restored must be"),
                     ((out, [(13, 21), (17, 24), (9, 17)], imgs, [True] * 3, True), "row 1: 17 x 24 is no crop"),
                     ((out, sizes, [imgs[0], imgs[0], imgs[2]], [True] * 3, True), "row 1: the target is 13 x 21"),
                     ((out, sizes, None, [True] * 3, True), "3 targets"), ((out, sizes, None, [True, False, True], False), "row 1: neither")):
        with pytest.raises(ValueError) as e:
            check_egress_rows(*a, cpu)
        assert piece in str(e.value), (piece, str(e.value))
    assert HipBackend.image_egress_batch_ws_bytes(3, 16, 24) == 24 * 3 * 4 * 1
    assert HipBackend.image_egress_batch_ws_bytes(68, 328, 488) == 24 * 68 * 82 * 2
