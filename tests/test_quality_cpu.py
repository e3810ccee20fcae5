"""CPU tier of the standard image-quality figures (rcot_amd/quality.py): the numpy restatement of the two SSIM protocols against skimage's
own route through scipy.ndimage (skimage itself is not a dependency), the integer BT.601 luma, the Gaussian taps, the inf / NaN
conventions and the tester's two flags.  The inputs made here (``image_pairs``) are shared with tests/test_quality_gpu.py."""
import numpy as np
import pytest

from rcot_amd import quality as Q

SIZES = [(7, 7), (11, 11), (11, 12), (37, 70), (75, 139), (321, 481)]
PROTOCOLS = [(wn, sp) for wn in ("uniform7", "gauss11") for sp in ("rgb", "y")]


def image_pairs(seed: int, h: int, w: int, extreme: bool = False):
    """[(kind, a, b)]: two unrelated random images; an image and itself plus integer noise in +-20, clipped; a flat image against itself
    with one pixel changed by 1; with ``extreme`` also all-0 against all-255"""
    g = np.random.Generator(np.random.PCG64(seed))
    a = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    c = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + g.integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
    flat = np.full((h, w, 3), 117, dtype=np.uint8)
    flat1 = flat.copy()
    flat1[h // 2, w // 2, 1] += 1
    out = [("random", a, c), ("noise", a, b), ("flat", flat, flat1)]
    if extreme:
        out.append(("extreme", np.zeros((h, w, 3), dtype=np.uint8), np.full((h, w, 3), 255, dtype=np.uint8)))
    return out


def tie_triples():
    """every (R, G, B) whose luma numerator sits exactly between two integers, n % 255000 == 127500, found by enumerating (R, B) and
    solving the congruence for G"""
    r, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    out = []
    for gch in range(256):
        n = 65481 * r + 128553 * gch + 24966 * b
        rr, bb = np.nonzero(n % 255000 == 127500)
        out += [(int(x), gch, int(y)) for x, y in zip(rr, bb)]
    return np.array(out, dtype=np.uint8)


def scipy_route(a, b, window, space):
    """skimage.metrics.structural_similarity's arithmetic on the planes of the space: scipy.ndimage filters of the five fp64 planes over
    the whole image, the crop by (win - 1) // 2, the mean (per plane, then over the planes)"""
    from scipy import ndimage as ndi
    win = Q.WINDOW_SIZE[window]
    cov_norm = 49.0 / 48.0 if window == "uniform7" else 1.0
    filt = (lambda x: ndi.uniform_filter(x, size=7)) if window == "uniform7" else (lambda x: ndi.gaussian_filter(x, sigma=1.5, truncate=3.5))
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    means = []
    for x, y in zip(Q.planes_u8(a, space).astype(np.float64), Q.planes_u8(b, space).astype(np.float64)):
        ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        p = (win - 1) // 2
        means.append(S[p:S.shape[0] - p, p:S.shape[1] - p].mean())
    return float(np.mean(means))


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_ssim_windowed_equals_the_scipy_route(size):
    h, w = size
    for window, space in PROTOCOLS:
        if h < Q.WINDOW_SIZE[window]:
            continue                                                         # 7 x 7: the uniform window only
        for kind, a, b in image_pairs(h * 1000 + w, h, w):
            got, want = Q.ssim_windowed(a, b, window, space), scipy_route(a, b, window, space)
            print(f"{h}x{w} {window} {space} {kind}: {got!r} scipy {want!r} diff {abs(got - want):.2e}")
            assert abs(got - want) < 1e-12, (window, space, kind)


def test_luma_is_the_integer_rule():
    black, white = np.zeros((1, 1, 3), dtype=np.uint8), np.full((1, 1, 3), 255, dtype=np.uint8)
    assert Q.luma_u8(black)[0, 0] == 16 and Q.luma_u8(white)[0, 0] == 235
    ties = tie_triples()
    assert len(ties) == 194                                                  # of the 2^24 colour triples
    n = ties.astype(np.int64) @ np.array([65481, 128553, 24966])
    y = Q.luma_u8(ties[None])
    assert y.dtype == np.uint8 and y.shape == (1, len(ties))
    assert np.array_equal(y[0], 16 + (n - 127500) // 255000 + 1)             # n = 255000 q + 127500 -> q + 1: every tie rounds up
    g = np.random.Generator(np.random.PCG64(5))
    img = g.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    fl = 16 + (65.481 * img[..., 0] + 128.553 * img[..., 1] + 24.966 * img[..., 2]) / 255.0
    assert np.abs(Q.luma_u8(img).astype(np.float64) - fl).max() <= 0.5 + 1e-9     # the rounding of the BT.601 float form
    assert Q.luma_u8(img).min() >= 16 and Q.luma_u8(img).max() <= 235


def test_window_weights():
    wt = Q.window_weights("gauss11")
    x = np.arange(-5, 6, dtype=np.float64)
    f = np.exp(-x * x / (2 * 1.5 * 1.5))
    assert wt.dtype == np.float64 and wt.shape == (11,)
    assert abs(float(np.sum(wt)) - 1.0) <= np.finfo(np.float64).eps          # 1 ulp
    assert np.array_equal(wt, wt[::-1])
    assert np.allclose(wt, f / f.sum(), rtol=4 * np.finfo(np.float64).eps, atol=0)
    assert np.array_equal(Q.window_weights("uniform7"), np.full(7, 1.0 / 7.0))
    with pytest.raises(ValueError):
        Q.window_weights("box2")


def test_identity_and_empty_maps():
    _, a, b = image_pairs(3, 40, 52)[1]
    for window, space in PROTOCOLS:
        assert abs(Q.ssim_windowed(a, a, window, space) - 1.0) <= 1e-15
        assert Q.psnr_u8(a, a, space) == float("inf")
        for h, w in ((6, 40), (40, 10)):
            if window == "uniform7" and w >= 7 and h >= 7:
                continue                                                     # 40 x 10 holds 7 x 7 windows
            s, n = Q.ssim_sums(a[:h, :w], b[:h, :w], window, space)
            assert (s, n) == (0.0, 0) and np.isnan(Q.ssim_windowed(a[:h, :w], b[:h, :w], window, space))
            e, m = Q.sqerr_sums(a[:h, :w], b[:h, :w], space)
            r = Q.quality_metrics([e, m, s, n])
            assert np.isnan(r["ssim"]) and np.isfinite(r["psnr"]) and m == (3 if space == "rgb" else 1) * h * w
    assert Q.ssim_sums(a[:40, :10], b[:40, :10], "uniform7", "y")[1] == 34 * 4
    assert Q.quality_metrics([0.0, 30.0, 0.0, 0.0]) == dict(psnr=float("inf"), ssim=pytest.approx(float("nan"), nan_ok=True))


def test_rgb_psnr_is_the_testers_and_box2_is_its_map():
    from rcot_amd import tester as TS
    _, a, b = image_pairs(4, 33, 47)[1]
    assert Q.psnr_u8(a, b, "rgb") == TS.psnr_uint8(a, b)
    assert Q.ssim_windowed(a, b, "box2", "rgb") == TS.ssim_image(a, b)
    ya, yb = Q.luma_u8(a), Q.luma_u8(b)
    assert Q.ssim_windowed(a, b, "box2", "y") == TS.ssim_plane(ya, yb)
    err = np.mean((ya.astype(np.float64) - yb.astype(np.float64)) ** 2)
    assert abs(Q.psnr_u8(a, b, "y") - 10 * np.log10(255.0 ** 2 / err)) < 1e-12


def test_tester_flags():
    from rcot_amd import tester as TS
    opt = TS.parser.parse_args([])
    assert (opt.ssim_window, opt.color) == ("box2", "rgb") and not TS._standard(opt)
    opt = TS.parser.parse_args(["--ssim_window", "gauss11", "--color", "y"])
    assert (opt.ssim_window, opt.color) == ("gauss11", "y") and TS._standard(opt)
    with pytest.raises(SystemExit):
        TS.parser.parse_args(["--ssim_window", "gauss7"])
    # the 2 x 2 map on the luma plane is host-only: refused before anything touches a GPU or the checkpoint
    with pytest.raises(SystemExit, match="host only"):
        TS.main(["--model", "/nonexistent/model.pth", "--color", "y", "--metrics", "device"])


def test_evaluate_folders_protocols(tmp_path):
    from PIL import Image
    from rcot_amd import tester as TS
    pairs = [image_pairs(8, 33, 47)[1], image_pairs(9, 40, 52)[1]]
    for d in ("t", "o"):
        (tmp_path / d).mkdir()
    for i, (_, a, b) in enumerate(pairs):
        Image.fromarray(a).save(tmp_path / "t" / f"{i}.png")
        Image.fromarray(b).save(tmp_path / "o" / f"{i}.png")
    old = TS.evaluate_folders(str(tmp_path / "t"), str(tmp_path / "o"))
    assert old == TS.evaluate_folders(str(tmp_path / "t"), str(tmp_path / "o"), "box2", "rgb")
    assert old[1] == np.mean([TS.ssim_image(a, b) for _, a, b in pairs])
    got = TS.evaluate_folders(str(tmp_path / "t"), str(tmp_path / "o"), "gauss11", "y")
    ps = [Q.psnr_u8(a, b, "y") for _, a, b in pairs]
    ss = [Q.ssim_windowed(a, b, "gauss11", "y") for _, a, b in pairs]
    assert got == (sum(ps) / 2, sum(ss) / 2, max(ps), max(ss), min(ps), min(ss))
