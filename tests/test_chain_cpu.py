"""CPU tier of the degradation chains (rcot_amd/chain.py): the grammar and its refusals, ``canonical``, the stage seeds, the order of a
chain sample's draws in the loader's per-sample stream (replayed with ``random.Random``), the sample list, and the up-front refusals of
the command lines.  No kernel runs here: the loader works on a recording backend."""
import os
import random
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from rcot_amd import chain as C

GOOD = {
    "chain_blur_g1.6+noise_g10+jpeg_q40": (("blur", "g1.6"), ("noise", "g", 10.0, 10.0), ("jpeg", 40, 40)),
    "chain_noise_gray0-55": (("noise", "gray", 0.0, 55.0),),
    "chain_sr_x2+noise_pg0.5x2+jpeg_q10-40": (("sr", 2), ("noise", "pg", 0.5, 2.0), ("jpeg", 10, 40)),
    "chain_blur_m15": (("blur", "m15"),),
}


def test_the_grammar_accepts_and_canonical_round_trips():
    for name, spec in GOOD.items():
        assert C.parse_de_type(name) == spec, name
        assert C.canonical(spec) == name and C.parse_de_type(C.canonical(spec)) == spec
        assert C.parse_spec(name) == C.parse_spec(name[len("chain_"):]) == spec            # the tools take both spellings
    for name in ("chain_noise_g2.50", "chain_noise_g0.00001-7.25+blur_a4x1r30k15+sr_x4+sr_x3", "chain_jpeg_q1-100+noise_gray255"):
        spec = C.parse_de_type(name)                                                      # other digits, the same stages
        assert C.parse_de_type(C.canonical(spec)) == spec, name
    assert C.canonical(C.parse_de_type("chain_noise_g2.50")) == "chain_noise_g2.5"
    for name in ("jpeg_q10", "blur_g1.6", "sr_x2", "sr_bd_x3", "denoise_25", "derain", "single"):
        assert C.parse_de_type(name) is None                                              # not chains: left to their own parsers
    six = "chain_" + "+".join(["jpeg_q10"] * 6)
    assert len(C.parse_de_type(six)) == 6


@pytest.mark.parametrize("name, stage", [
    ("chain_blur_g1.6+sr_bd_x3", "sr_bd_x3"),                       # no BD stage
    ("chain_blur_g1.6+chain_noise_g10", "chain_noise_g10"),         # no chain inside a chain
    ("chain_blur_g1.6++jpeg_q10", ""),                              # empty stages
    ("chain_", ""),
    ("chain_jpeg_q10+", ""),
    ("chain_" + "+".join(f"jpeg_q{q}" for q in (10, 20, 30, 40, 50, 60, 70)), "jpeg_q70"),       # a seventh stage
    ("chain_blur_g1-2", "blur_g1-2"),                               # ranges on any other parameter
    ("chain_blur_m15a10-50", "blur_m15a10-50"),
    ("chain_sr_x2-4", "sr_x2-4"),
    ("chain_noise_pg0.1-0.5x2", "noise_pg0.1-0.5x2"),
    ("chain_noise_pg1x2-3", "noise_pg1x2-3"),
    ("chain_jpeg_q40-10", "jpeg_q40-10"),                           # ranges that are not lo < hi, values outside their intervals
    ("chain_jpeg_q10-10", "jpeg_q10-10"),
    ("chain_jpeg_q0", "jpeg_q0"),
    ("chain_jpeg_q10-101", "jpeg_q10-101"),
    ("chain_noise_g20-5", "noise_g20-5"),
    ("chain_noise_g256", "noise_g256"),
    ("chain_noise_gray0-300", "noise_gray0-300"),
    ("chain_noise_g-5", "noise_g-5"),
    ("chain_sr_x5", "sr_x5"),
    ("chain_blur_g0", "blur_g0"),
    ("chain_jpeg_q10+denoise_25", "denoise_25"),                    # other tasks are no stages
    ("chain_noise_s0.1", "noise_s0.1"),
])
def test_malformed_chains_are_refused_naming_the_stage(name, stage):
    with pytest.raises(SystemExit) as e:
        C.parse_de_type(name)
    assert f"stage {stage!r}" in str(e.value) and name in str(e.value)
    assert len(str(e.value).splitlines()) == 1


def test_what_a_chain_needs():
    p = C.parse_de_type
    assert C.cacheable(p("chain_blur_g1.6+jpeg_q30")) and C.cacheable(p("chain_sr_x2+blur_m15a30"))
    for name in ("chain_blur_g1.6+noise_g10+jpeg_q40", "chain_jpeg_q10-40", "chain_blur_m15", "chain_noise_pg0.5x2", "chain_noise_g0"):
        assert not C.cacheable(p(name)), name
    assert C.needs_draws(p("chain_blur_m15")) and not C.needs_draws(p("chain_noise_g10")) and C.has_noise(p("chain_noise_g10"))
    assert [C.size_multiple(p(n)) for n in ("chain_jpeg_q10", "chain_sr_x3", "chain_sr_x2+sr_x4", "chain_sr_x2+sr_x3")] == [1, 3, 4, 6]


def test_stage_seeds():
    """the documented step: ((seed XOR (k + 1)) * 0xD1342543DE82EF95) mod 2^64 — injective in the seed for a fixed k, and no two stages
    of a chain share a seed or sit a small multiple of the counter increment apart"""
    for seed in (0, 1, 5, 2 ** 63 - 1, 0x123456789ABCDEF):
        seeds = [C.stage_seed(seed, k) for k in range(6)]
        assert seeds == [((seed ^ (k + 1)) * 0xD1342543DE82EF95) % 2 ** 64 for k in range(6)]
        assert len(set(seeds)) == 6 and seed not in seeds
        inc_inv = pow(0x9E3779B97F4A7C15, -1, 2 ** 64)
        for a in range(6):
            for b in range(a):                                        # seeds[a] - seeds[b] = j * increment has no |j| < 2^40
                j = (seeds[a] - seeds[b]) * inc_inv % 2 ** 64
                assert min(j, 2 ** 64 - j) > 2 ** 40, (seed, a, b)
    assert len({C.stage_seed(s, 1) for s in range(1000)}) == 1000


# ------------------------------------------------------------------ the loader's draws, on a recording backend
def _png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(a).save(path)
    return a


class Recorder:
    """a backend that launches nothing: ``patch_prep`` keeps its scalar arguments"""
    device = torch.device("cpu")
    _plan = None

    def __init__(self):
        self.preps = []

    def patch_prep(self, clean_img, deg_img, y0, x0, P, mode, sigma, seed, deg_out, clean_out):
        self.preps.append((tuple(clean_img.shape), deg_img is not None, y0, x0, mode, sigma, seed))
        deg_out.zero_()
        clean_out.zero_()


def _folder(root):
    sizes = {"a": (48, 64), "b": (50, 70), "c": (66, 81)}
    for i, (n, (h, w)) in enumerate(sizes.items()):
        _png(f"{root}/clean/{n}.png", h, w, 90 + i)
    return Namespace(de_type=[], chain_dir=f"{root}/clean/", jpeg_dir=f"{root}/clean/", patch_size=32)


def test_draw_order_in_the_loaders_stream(tmp_path, monkeypatch):
    from rcot_amd import data as D
    from rcot_amd import jpeg as J
    name = "chain_blur_m15+noise_g5-20+sr_x3+jpeg_q20-40+noise_pg0.5x2"
    args = _folder(str(tmp_path))
    chained = []
    monkeypatch.setattr(C, "chain_degrade_u8", lambda img, spec, draws, border, sub, be: chained.append((spec, draws, border, sub)) or img.clone())
    monkeypatch.setattr(J, "jpeg_degrade_u8", lambda img, q, sub, be: img.clone())
    rec_c, rec_j = Recorder(), Recorder()
    seed, B = 11, 4
    lc = D.FolderLoader(Namespace(**{**vars(args), "de_type": [name]}), B, seed=seed, backend=rec_c)
    lj = D.FolderLoader(Namespace(**{**vars(args), "de_type": ["jpeg_q10"]}), B, seed=seed, backend=rec_j)
    assert len(lc) == len(lj) == 4                                    # 15 samples / 4
    names_of = {}
    for epoch in (1, 2):
        names_of[epoch] = [n for ([names, _], _, _) in lc for n in names]
        assert names_of[epoch] == [n for ([names, _], _, _) in lj for n in names] and len(names_of[epoch]) == 15
    assert len(rec_c.preps) == len(rec_j.preps) == len(chained) == 30
    # sr_x3 in the chain: the image is cropped to a multiple of 16, then of 3, as an sr_x3 sample's; jpeg_q10 stops at 16
    shape_c = {"a": (48, 63, 3), "b": (48, 63, 3), "c": (63, 78, 3)}
    shape_j = {"a": (48, 64, 3), "b": (48, 64, 3), "c": (64, 80, 3)}
    pos = 0
    for epoch in (1, 2):
        for k in range(15):
            n = names_of[epoch][k]
            got_c, got_j = rec_c.preps[pos], rec_j.preps[pos]
            assert got_c[0] == shape_c[n] and got_j[0] == shape_j[n]
            # replay: one stream per (seed, epoch, global position); the three common draws first, as every task draws them
            for got, (H, W, _) in ((got_c, got_c[0]), (got_j, got_j[0])):
                rng = random.Random((seed * 1_000_003 + epoch) * 2_147_483_659 + k)
                want = (rng.randint(0, H - 32), rng.randint(0, W - 32), rng.randint(1, 7), 0.0, rng.getrandbits(63))
                assert got[1] and got[2:] == want, (epoch, k)
                if got is got_c:                                      # then the chain's own, in stage order
                    spec, draws, border, sub = chained[pos]
                    assert spec == C.parse_de_type(name) and (border, sub) == ("replicate", 2)
                    assert draws.seed == want[4]
                    assert draws.values == (rng.randint(0, 179), rng.uniform(5.0, 20.0), None, rng.randint(20, 40), None), (epoch, k)
            pos += 1
    # a chain without an sr stage decodes to the jpeg_q10 sample's size: its three common draws ARE that sample's, position by position
    rec_p = Recorder()
    lp = D.FolderLoader(Namespace(**{**vars(args), "de_type": ["chain_noise_g5-20"]}), B, seed=seed, backend=rec_p)
    for _ in lp:
        pass
    assert rec_p.preps == rec_j.preps[:15]
    assert [d.values for _, d, _, _ in chained[30:]] != [] and all(5.0 <= d.values[0] <= 20.0 for _, d, _, _ in chained[30:])


def test_file_draws_are_a_function_of_seed_and_index():
    spec = C.parse_de_type("chain_blur_m15+noise_gray0-55+jpeg_q10-40")
    rng = random.Random(3 * 2_147_483_659 + 7)
    want = C.Draws(rng.getrandbits(63), (rng.randint(0, 179), rng.uniform(0.0, 55.0), rng.randint(10, 40)))
    assert C.file_draws(spec, 3, 7) == want == C.file_draws(spec, 3, 7)
    assert C.file_draws(spec, 3, 8) != want and C.file_draws(spec, 4, 7) != want


# ------------------------------------------------------------------ the sample list
def test_sample_ids(tmp_path):
    from rcot_amd import data as D
    args = _folder(str(tmp_path))
    files = [f"{tmp_path}/clean/{n}.png" for n in "abc"]
    one = Namespace(**{**vars(args), "de_type": ["chain_blur_g1.6+noise_g10+jpeg_q40"], "blur_border": "mirror", "jpeg_subsampling": "444"})
    ids = D.build_sample_ids(one)
    spec = C.parse_de_type(one.de_type[0])
    assert ids == [{"file": f, "de": 7, "gt": None, "chain": (spec, "mirror", 0)} for f in files] * 5       # `single`, x5
    assert D.FolderLoader._decode(ids[1])[0].shape == (48, 64, 3)
    assert D.FolderLoader._file_keys(ids[1]) == [((files[1], "crop16"), files[1], 0)]
    sr = D.build_sample_ids(Namespace(**{**vars(args), "de_type": ["chain_sr_x3+jpeg_q10"]}))
    assert all(s["sr"] == 3 and s["chain"][1:] == ("replicate", 2) for s in sr) and len(sr) == 15
    assert D.FolderLoader._decode(sr[1])[0].shape == (48, 63, 3)                                          # as an sr_x3 sample is decoded
    assert D.FolderLoader._file_keys(sr[1]) == [((files[1], "crop16", "mod", 3), files[1], 3)]
    mixed = D.build_sample_ids(Namespace(**{**vars(args), "de_type": ["chain_noise_g10", "jpeg_q10", "chain_blur_m15"]}))
    assert [("jpeg" in s, s.get("chain", (None,))[0]) for s in mixed[::15]] == \
        [(True, None), (False, C.parse_de_type("chain_noise_g10")), (False, C.parse_de_type("chain_blur_m15"))]
    with pytest.raises(SystemExit, match="--chain_dir"):
        D.build_sample_ids(Namespace(**{**vars(one), "chain_dir": None}))
    with pytest.raises(SystemExit, match="stage 'sr_bd_x3'"):
        D.build_sample_ids(Namespace(**{**vars(one), "de_type": ["chain_sr_bd_x3"]}))
    with pytest.raises(SystemExit, match="--blur_border"):
        D.build_sample_ids(Namespace(**{**vars(one), "blur_border": "zero"}))


def test_sample_ids_without_chains_are_what_they_were(tmp_path):
    """a --de_type list without chains: the list, written out here, that the loader built before there were chains"""
    from rcot_amd import data as D
    from rcot_amd.blur import parse_de_type as blur_spec
    root = str(tmp_path)
    for i in range(2):
        _png(f"{root}/Denoise/d{i}.png", 40 + i, 52, 40 + i)
        _png(f"{root}/hr/h{i}.png", 48, 48, 50 + i)
        _png(f"{root}/single/degraded/s{i}.png", 32, 32, 60 + i)
        _png(f"{root}/single/target/s{i}.png", 32, 32, 70 + i)
    _png(f"{root}/clean/a.png", 48, 64, 80)
    os.makedirs(f"{root}/lists/noisy")
    open(f"{root}/lists/noisy/denoise.txt", "w").write("d0.png\nd1.png\n")
    args = Namespace(de_type=["denoise_25", "single", "sr_x2", "jpeg_q10", "blur_g1.6", "blur_m15", "sr_bd_x3"], data_file_dir=f"{root}/lists/",
                     denoise_dir=f"{root}/Denoise/", single_dir=f"{root}/single", sr_dir=f"{root}/hr", jpeg_dir=f"{root}/clean",
                     blur_dir=f"{root}/clean", chain_dir=None, patch_size=32)
    want = [{"file": f"{root}/Denoise/d{i}.png", "de": 1, "gt": None} for i in range(2)] * 5
    want += [{"file": f"{root}/single/degraded/s{i}.png", "de": 7, "gt": f"{root}/single/target/s{i}.png"} for i in range(2)] * 5
    want += [{"file": f"{root}/hr/h{i}.png", "de": 7, "gt": None, "sr": 2} for i in range(2)] * 5
    want += [{"file": f"{root}/clean/a.png", "de": 7, "gt": None, "jpeg": (10, 2)}] * 5
    want += [{"file": f"{root}/clean/a.png", "de": 5, "gt": None, "blur": (blur_spec(t), "replicate")} for t in ("blur_g1.6", "blur_m15")
             for _ in range(5)]
    want += [{"file": f"{root}/hr/h{i}.png", "de": 7, "gt": None, "sr": 3, "bd": True} for i in range(2)] * 5
    assert D.build_sample_ids(args) == want
    # and a chain goes behind all of them
    both = D.build_sample_ids(Namespace(**{**vars(args), "de_type": ["chain_jpeg_q10"] + args.de_type, "chain_dir": f"{root}/clean"}))
    assert both[:len(want)] == want and len(both) == len(want) + 5 and all("chain" in s for s in both[len(want):])


def test_cache_report_is_unchanged_without_chain_samples():
    from rcot_amd.imagecache import DeviceImageCache
    c = DeviceImageCache(Recorder(), 1 << 20)
    assert c.chain_degradations == 0 and c.report().endswith("0 misses, 0 sr degradations")
    c.chain_degradations = 2
    assert c.report().endswith("0 sr degradations, 2 chain degradations")


# ------------------------------------------------------------------ the command lines refuse up front (no GPU is touched)
def test_command_lines_refuse_up_front(tmp_path):
    args = _folder(str(tmp_path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    one_line = lambda r, word: r.returncode != 0 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run("rcot_amd.trainer", "--de_type", "chain_blur_g1.6+sr_bd_x3", "--chain_dir", args.chain_dir)
    assert one_line(r, "stage 'sr_bd_x3'"), r.stderr[-2000:]
    r = run("rcot_amd.trainer", "--de_type", "chain_blur_g1.6+jpeg_q30")
    assert one_line(r, "--chain_dir"), r.stderr[-2000:]
    r = run("rcot_amd.trainer", "--de_type", "chain_blur_g1.6+jpeg_q30", "--chain_dir", args.chain_dir, "--synthetic")
    assert one_line(r, "--synthetic"), r.stderr[-2000:]
    for flag in (["--jpeg_q", "10"], ["--sr_scale", "2"], ["--blur", "g1.6"], ["--noise_sigma", "25"]):
        r = run("rcot_amd.tester", "--chain", "noise_g10", *flag)
        assert one_line(r, "--chain makes the network's input from the target"), (flag, r.stderr[-2000:])
    r = run("rcot_amd.tester", "--chain", "noise_g10+chain_jpeg_q10")
    assert one_line(r, "stage 'chain_jpeg_q10'"), r.stderr[-2000:]
    r = run("rcot_amd.chain", "--in", args.chain_dir, "--out", str(tmp_path / "out"), "--chain", "noise_g10+")
    assert one_line(r, "stage ''") and not os.path.exists(tmp_path / "out"), r.stderr[-2000:]
