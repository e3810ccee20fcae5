"""CPU tier of PSNR-B and the border shave (rcot_amd/quality.py): the vectorised sums and the pair counts against a plain double loop
over pixels at every block-grid origin, the degenerate sizes, the closed form on an image of constant 8 x 8 blocks, the grid origin
after a shift, a real JPEG round trip, and the tester's two flags on the folder route.  ``SIZES``, ``ORIGINS`` and ``loop_stats`` are
shared with tests/test_psnrb_gpu.py."""
import math

import numpy as np
import pytest

from rcot_amd import quality as Q

SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 7), (8, 8), (9, 9), (15, 17), (16, 16), (24, 40)]
ORIGINS = [(0, 0), (3, 5), (7, 7)]
SPACES = ("rgb", "y")


def random_image(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def loop_stats(a, space, oy, ox):
    """(sums [planes][4], counts [4]) of the issue's definition, one pixel pair at a time in Python integers"""
    p = Q.planes_u8(a, space).tolist()
    h, w = len(p[0]), len(p[0][0])
    sums, counts = [[0, 0, 0, 0] for _ in p], [0, 0, 0, 0]
    for y in range(h):
        for x in range(w):
            if x + 1 < w:
                k = 0 if (x + ox) % 8 == 7 else 1
                counts[k] += 1
                for s, pl in zip(sums, p):
                    s[k] += (pl[y][x] - pl[y][x + 1]) ** 2
            if y + 1 < h:
                k = 2 if (y + oy) % 8 == 7 else 3
                counts[k] += 1
                for s, pl in zip(sums, p):
                    s[k] += (pl[y][x] - pl[y + 1][x]) ** 2
    return sums, counts


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_sums_and_counts_equal_the_double_loop(size):
    h, w = size
    a = random_image(h * 100 + w, h, w)
    for space in SPACES:
        for oy, ox in ORIGINS:
            sums, counts = loop_stats(a, space, oy, ox)
            got = Q.blockiness_sums(a, space, oy, ox)
            assert got.dtype == np.int64 and got.shape == (3 if space == "rgb" else 1, 4)
            assert got.tolist() == sums, (space, oy, ox)
            assert list(Q.blockiness_counts(h, w, oy, ox)) == counts, (oy, ox)
            assert counts[0] + counts[1] == h * (w - 1) and counts[2] + counts[3] == w * (h - 1)
    assert np.array_equal(Q.blockiness_sums(a, "rgb"), Q.blockiness_sums(a, "rgb", 0, 0))
    for bad in ((8, 0), (0, -1)):
        with pytest.raises(ValueError):
            Q.blockiness_sums(a, "rgb", *bad)
        with pytest.raises(ValueError):
            Q.blockiness_counts(h, w, *bad)


def test_degenerate_sizes_have_no_blocking_effect():
    # w = 8, one column of blocks at origin 0: x + 1 exists only for x <= 6, so no horizontal border pair; h = 8 alike
    assert Q.blockiness_counts(8, 8, 0, 0) == (0, 56, 0, 56)
    a, b = random_image(1, 8, 8), random_image(2, 8, 8)
    for space in SPACES:
        st = Q.blockiness_stats(a, b, space)
        for row in st:
            assert Q.bef_from_sums(row[1:], 8, 8) == 0.0
        assert Q.psnrb_u8(a, b, space) == pytest.approx(np.mean([10 * math.log10(255.0 ** 2 / (int(r[0]) / 64)) for r in st]), abs=1e-12)
    # a single row or column: min(h, w) < 2, the logarithm's argument would be 1
    for h, w in ((1, 1), (1, 9), (9, 1), (1, 40)):
        a, b = random_image(3, h, w), random_image(4, h, w)
        for oy, ox in ORIGINS:
            for space in SPACES:
                st = Q.blockiness_stats(a, b, space, oy, ox)
                assert all(Q.bef_from_sums(r[1:], h, w, oy, ox) == 0.0 for r in st)
                assert math.isfinite(Q.psnrb_u8(a, b, space, oy, ox))
    # no inner pair either way: 2 x 2 at origin (7, 7) has border pairs only
    assert Q.blockiness_counts(2, 2, 7, 7) == (2, 0, 2, 0)
    assert Q.bef_from_sums(Q.blockiness_sums(random_image(5, 2, 2), "y", 7, 7)[0], 2, 2, 7, 7) == 0.0


def blocks_image(seed=11):
    """64 x 64, constant 8 x 8 blocks of random grey levels, and the 8 x 8 table of the levels"""
    v = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(8, 8), dtype=np.int64)
    img = np.repeat(np.repeat(v, 8, axis=0), 8, axis=1).astype(np.uint8)
    return np.repeat(img[:, :, None], 3, axis=2), v


def test_constant_blocks_closed_form():
    img, v = blocks_image()
    dh, dv = int(((v[:, :-1] - v[:, 1:]) ** 2).sum()), int(((v[:-1, :] - v[1:, :]) ** 2).sum())
    got = Q.blockiness_sums(img, "rgb")
    assert got.tolist() == [[8 * dh, 0, 8 * dv, 0]] * 3                       # every step lies on a border, 8 pixels long
    assert Q.blockiness_counts(64, 64) == (64 * 7, 64 * 56, 64 * 7, 64 * 56)
    d_b = (8 * dh + 8 * dv) / (2 * 64 * 7)                                     # D_C = 0
    bef = Q.bef_from_sums(got[0], 64, 64)
    assert bef > 0 and bef == pytest.approx((3.0 / 6.0) * d_b, rel=1e-15)      # log2 8 / log2 64
    target = np.clip(img.astype(np.int64) + np.random.Generator(np.random.PCG64(3)).integers(-9, 10, size=img.shape), 0, 255).astype(np.uint8)
    for space in SPACES:
        assert Q.psnrb_u8(img, target, space) < Q.psnr_u8(img, target, space)
    mse = ((img.astype(np.int64) - target) ** 2).mean(axis=(0, 1))
    assert Q.psnrb_u8(img, target, "rgb") == pytest.approx(np.mean([10 * math.log10(255.0 ** 2 / (m + bef)) for m in mse]), abs=1e-12)
    # the steps of the TARGET play no part: a flat restored image has no blocking effect, whatever it is compared with
    flat = np.full_like(img, 128)
    assert Q.psnrb_u8(flat, img, "rgb") == pytest.approx(Q.psnr_u8(flat, img, "rgb"), abs=1e-12)      # (equal channels: pooled == mean)
    assert Q.psnrb_u8(img, flat, "rgb") < Q.psnr_u8(img, flat, "rgb")


def test_grid_origin_follows_a_shift():
    img, _ = blocks_image(12)
    sub = np.ascontiguousarray(img[3:, 5:])
    moved = Q.blockiness_sums(sub, "rgb", 3, 5)
    # the pairs of the unshifted image that lie inside the crop, classified where the codec put them
    p = Q.planes_u8(img, "rgb")
    dh, dv = (p[:, 3:, 5:-1] - p[:, 3:, 6:]) ** 2, (p[:, 3:-1, 5:] - p[:, 4:, 5:]) ** 2
    xb, yb = np.arange(5, 63) % 8 == 7, np.arange(3, 63) % 8 == 7
    want = np.stack([dh[:, :, xb].sum((1, 2)), dh[:, :, ~xb].sum((1, 2)), dv[:, yb].sum((1, 2)), dv[:, ~yb].sum((1, 2))], axis=1)
    assert np.array_equal(moved, want) and (moved[:, 1] == 0).all() and (moved[:, 3] == 0).all() and (moved[:, 0] > 0).all()
    wrong = Q.blockiness_sums(sub, "rgb", 0, 0)                                # the grid laid from the crop's own corner
    assert (wrong[:, 0] < moved[:, 0]).all() and (wrong[:, 2] < moved[:, 2]).all()
    assert np.array_equal(wrong[:, 0] + wrong[:, 1], moved[:, 0] + moved[:, 1])
    # the shave keeps the grid: shave_u8 by n with origin n % 8
    for n in (2, 8, 11):
        s = Q.shave_u8(img, n)
        got = Q.blockiness_sums(s, "y", n % 8, n % 8)
        assert got[0, 1] == 0 and got[0, 3] == 0 and got[0, 0] > 0


def test_identical_images_give_inf():
    flat = np.full((16, 24, 3), 90, dtype=np.uint8)
    for space in SPACES:
        assert Q.psnrb_u8(flat, flat, space) == float("inf")
        assert Q.psnrb_from_sums([[0, 0, 0, 0, 0]] * (3 if space == "rgb" else 1), 16, 24) == float("inf")
    img, _ = blocks_image()
    assert math.isfinite(Q.psnrb_u8(img, img, "y"))                            # no error, but a blocking effect: finite


def test_jpeg_blocks_show_in_the_luma():
    import jpeg_double as JD
    from test_jpeg_cpu import contents
    clean = contents(64, 96, 5)["smooth"]
    coded = JD.pil_roundtrip(clean, 10, 2)
    bef = lambda im: Q.bef_from_sums(Q.blockiness_sums(im, "y")[0], 64, 96)
    print(f"BEF (y) of the smooth image {bef(clean)!r}, after JPEG quality 10 {bef(coded)!r}")
    assert bef(coded) > 0 and bef(clean) < bef(coded)
    assert Q.psnrb_u8(coded, clean, "y") < Q.psnr_u8(coded, clean, "y")


def test_shave():
    img = random_image(7, 12, 20)
    assert np.array_equal(Q.shave_u8(img, 0), img)
    assert np.array_equal(Q.shave_u8(img, 3), img[3:9, 3:17]) and Q.shave_u8(img, 5).shape == (2, 10, 3)
    for n in (-1, 6, 10):
        with pytest.raises(ValueError, match=f"shave {n}"):
            Q.shave_u8(img, n)


def test_evaluate_folders_and_flags(tmp_path, capsys):
    from PIL import Image
    from rcot_amd import tester as TS
    from test_quality_cpu import image_pairs
    pairs = [image_pairs(8, 33, 47)[1], image_pairs(9, 40, 52)[1]]
    for d in ("t", "o"):
        (tmp_path / d).mkdir()
    for i, (_, a, b) in enumerate(pairs):
        Image.fromarray(a).save(tmp_path / "t" / f"{i}.png")
        Image.fromarray(b).save(tmp_path / "o" / f"{i}.png")
    t, o = str(tmp_path / "t"), str(tmp_path / "o")
    # the defaults: what the function returned before it had the keywords
    ps, ss = [TS.psnr_uint8(a, b) for _, a, b in pairs], [TS.ssim_image(a, b) for _, a, b in pairs]
    today = (sum(ps) / 2, sum(ss) / 2, max(ps), max(ss), min(ps), min(ss))
    assert TS.evaluate_folders(t, o) == today == TS.evaluate_folders(t, o, "box2", "rgb", psnrb=False, shave=0)
    # --psnrb --shave 2 on the luma: the host functions on the cropped pairs, the restored image first
    got = TS.evaluate_folders(t, o, "uniform7", "y", psnrb=True, shave=2)
    cut = [(Q.shave_u8(a, 2), Q.shave_u8(b, 2)) for _, a, b in pairs]
    ps, ss = [Q.psnr_u8(a, b, "y") for a, b in cut], [Q.ssim_windowed(a, b, "uniform7", "y") for a, b in cut]
    pb = [Q.psnrb_u8(b, a, "y", 2, 2) for a, b in cut]
    assert got == (sum(ps) / 2, sum(ss) / 2, max(ps), max(ss), min(ps), min(ss), sum(pb) / 2, max(pb), min(pb))
    assert TS.evaluate_folders(t, o, psnrb=True)[:6] == today
    # a shave that empties the smaller image: one line naming its size, the other image alone is the mean
    capsys.readouterr()
    one = TS.evaluate_folders(t, o, "uniform7", "y", shave=17)
    assert "skipped: 33 x 47 leaves nothing after --shave 17" in capsys.readouterr().out
    a, b = Q.shave_u8(pairs[1][1], 17), Q.shave_u8(pairs[1][2], 17)
    assert a.shape == (6, 18, 3) and one[0] == Q.psnr_u8(a, b, "y") and np.isnan(one[1])    # 6 rows: an empty 7 x 7 map
    # the flags, and the refusals before anything touches a GPU or the checkpoint
    opt = TS.parser.parse_args([])
    assert opt.psnrb is False and opt.shave == 0
    opt = TS.parser.parse_args(["--psnrb", "--shave", "4"])
    assert opt.psnrb is True and opt.shave == 4
    with pytest.raises(SystemExit, match="--shave -1"):
        TS.main(["--model", "/nonexistent/model.pth", "--shave", "-1"])
    with pytest.raises(SystemExit, match="cannot be cropped"):
        TS.main(["--model", "/nonexistent/model.pth", "--shave", "2", "--metrics", "device"])
    # the report: the PSNR-B line and keys only when asked for
    r = TS._report(1.0, 0.5, 2.0, 0.6, 0.5, 0.4, 3)
    out = capsys.readouterr().out
    assert "PSNR-B" not in out and "metrics:" not in out and "psnrb" not in r
    r = TS._report(1.0, 0.5, 2.0, 0.6, 0.5, 0.4, 3, "uniform7", "y", (30.0, 31.0, 29.0), 2)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "metrics: ssim uniform7, color y, psnrb, shave 2" and lines[3].startswith("SSIM: Averyge")
    assert lines[4] == "PSNR-B: Averyge 30.00000,   best 31.00000,   worst 29.00000"
    assert (r["psnrb"], r["psnrb_best"], r["psnrb_worst"]) == (30.0, 31.0, 29.0)
