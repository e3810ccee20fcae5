"""GPU tier of the whole-image noise kernel rcot_noise_u8 (csrc/noise.hip) on guard-banded, pre-poisoned buffers (tests/guarded.py):
exactness (copy at zero parameters, determinism, in place, the byte path of unaligned pointers against the 16-byte path, shared
deviates of ``gray``), its refusals, the rule against a float64 restatement of the counter-based deviate, the statistics of the three
models with bars of 5 standard errors computed from sigma and N, and an image of more than 2^31 bytes."""
import numpy as np
import pytest
import torch

from guarded import GuardSet
from rcot_amd import lib

pytestmark = pytest.mark.gpu

# 1 x 1: the smallest image; 3 x 5: fewer bytes than one thread's run of 48; 33 x 47: a ragged tail, rows no multiple of anything;
# 64 x 64: whole runs only; 256 x 256: more than one workgroup, the size of the statistics
SHAPES = [(1, 1), (3, 5), (33, 47), (64, 64), (256, 256)]
MODELS = [("g", 25.0, 0.0), ("gray", 25.0, 0.0), ("pg", 0.5, 2.0)]


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _img(h, w, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _run(hip, img, model, p0, p1, seed, inplace=False, offset=0):
    """one guarded call -> the result on the host; ``inplace``: dst is src; ``offset``: bytes by which src and dst are shifted off their
    16-byte alignment.  Out of place the source is compared afterwards."""
    gs = GuardSet("cuda")
    h, w = img.shape[:2]
    src = gs.empty(img.size + offset, dtype=torch.uint8, name="src")[offset:].view(h, w, 3)
    src.copy_(torch.from_numpy(img))
    dst = src if inplace else gs.empty(img.size + offset, dtype=torch.uint8, name="dst")[offset:].view(h, w, 3)
    got = hip.noise_u8(src, model, p0, p1, seed, out=dst)
    gs.check()
    assert got.data_ptr() == dst.data_ptr()
    if not inplace:
        assert np.array_equal(src.cpu().numpy(), img)
    return dst.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exactness(hip, shape):
    h, w = shape
    img = _img(h, w, 13 * h + w)
    for model, p0, p1 in MODELS:
        a = _run(hip, img, model, p0, p1, 77)
        assert a.shape == img.shape and a.dtype == np.uint8
        assert np.array_equal(_run(hip, img, model, p0, p1, 77), a), model                  # same seed, same bytes
        assert not np.array_equal(_run(hip, img, model, p0, p1, 78), a), model              # another seed, other bytes
        assert not np.array_equal(a, img), model
        assert np.array_equal(_run(hip, img, model, p0, p1, 77, inplace=True), a), model    # dst == src
        for off in (1, 4):                                                                  # the byte path gives the bytes of the runs
            assert np.array_equal(_run(hip, img, model, p0, p1, 77, offset=off), a), (model, off)
            assert np.array_equal(_run(hip, img, model, p0, p1, 77, inplace=True, offset=off), a), (model, off)
        # zero parameters copy the image
        assert np.array_equal(_run(hip, img, model, 0.0, 0.0, 77), img), model
        assert np.array_equal(_run(hip, img, model, 0.0, 0.0, 77, inplace=True), img), model
    assert np.array_equal(_run(hip, img, "g", 0.0, 3.0, 77), img)                           # p1 is not read by g and gray
    # gray on an image with R = G = B gives R = G = B
    grey = np.repeat(img[:, :, :1], 3, axis=2)
    out = _run(hip, grey, "gray", 25.0, 0.0, 5)
    assert np.array_equal(out[:, :, 0], out[:, :, 1]) and np.array_equal(out[:, :, 0], out[:, :, 2])
    if h * w >= 15:
        out = _run(hip, grey, "g", 25.0, 0.0, 5)
        assert not np.array_equal(out[:, :, 0], out[:, :, 1])


def test_refusals_leave_the_output_untouched(hip):
    gs = GuardSet("cuda")
    src = gs.tensor(torch.from_numpy(_img(16, 24, 3)), name="src")
    dst = gs.empty((16, 24, 3), dtype=torch.uint8, name="dst")
    before = dst.clone()
    call = lambda s, d, H, W, m, p0, p1: hip.L.rcot_noise_u8(s, d, H, W, m, p0, p1, 9, hip._st())
    ok = (src.data_ptr(), dst.data_ptr(), 16, 24, 0, 10.0, 0.0)
    nan, inf = float("nan"), float("inf")
    bad = [(None,) + ok[1:], ok[:1] + (None,) + ok[2:]]                                      # src, dst null
    bad += [ok[:2] + (v,) + ok[3:] for v in (0, -4)] + [ok[:3] + (v,) + ok[4:] for v in (0, -4)]            # H, W < 1
    bad += [ok[:4] + (v,) + ok[5:] for v in (-1, 3, 100)]                                    # no such model
    for m in (0, 1, 2):
        bad += [ok[:4] + (m, v, 1.0) for v in (-1.0, -1e-30, nan, inf, -inf)]                # p0 negative or not finite
        bad += [ok[:4] + (m, 1.0, v) for v in (-1.0, -1e-30, nan, inf, -inf)]                # p1 negative or not finite
    bad += [ok[:4] + (m, v, 0.0) for m in (0, 1) for v in (255.5, 1000.0)]                   # p0 above 255 for g and gray
    for args in bad:
        assert call(*args) == -1, args
    for fn in (lambda: hip.noise_u8(src, "g", -1.0, 0.0, 1, out=dst), lambda: hip.noise_u8(src, "poisson", 1.0, 0.0, 1, out=dst),
               lambda: hip.noise_u8(src, "gray", 256.0, 0.0, 1, out=dst)):
        with pytest.raises(lib.RcotKernelError, match="invalid argument"):
            fn()
    with pytest.raises(lib.RcotKernelError):
        hip.noise_u8(src.float(), "g", 1.0, 0.0, 1)
    gs.check()
    assert torch.equal(dst, before)                                                          # nothing was launched
    for args in (ok, ok[:4] + (0, 255.0, 0.0), ok[:4] + (2, 300.0, 0.0), ok[:4] + (2, 0.0, 300.0)):         # legal, pg above 255 included
        assert call(*args) == 0, args
    gs.check()
    assert not torch.equal(dst, before) and lib.ABI_VERSION >= 34


# ------------------------------------------------------------------ the rule, restated in float64
def _randn64(seed, idx):
    """counter_randn of csrc/common.h with exact integers and float64 functions"""
    m = (1 << 64) - 1
    z = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & m) + np.uint64(0x9E3779B97F4A7C15) * (z + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    u1 = (((z >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0) / 16777217.0
    u2 = ((z >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


@pytest.mark.parametrize("model, p0, p1", MODELS + [("g", 5.0, 0.0)], ids=lambda v: str(v))
def test_the_rule_against_a_float64_restatement(hip, model, p0, p1):
    """out = trunc(clip(v + s z)) with the documented counter of each model.  The kernel evaluates z with the fp32 hardware logarithm
    and cosine (absolute error of the order of 1e-6 each) and rounds the product and the sum to fp32 (2^-24 relative of at most 400): v +
    s z is off by less than 25 * 1e-5 + 5e-5 < 5e-4, so a byte differs from the float64 restatement only where v + s z lies that close to
    an integer — a fraction below 2 * 5e-4 = 1e-3 of the bytes, asserted as 5e-3 — and then by exactly 1."""
    h, w = 33, 47
    img = _img(h, w, 3)
    pix = np.arange(h * w, dtype=np.uint64).reshape(h, w, 1)
    idx = np.repeat(pix, 3, axis=2) if model == "gray" else pix * np.uint64(3) + np.arange(3, dtype=np.uint64)
    seed = 0xFEDCBA9876543210                                       # the top bit set: the seed travels as an unsigned 64-bit value
    v = img.astype(np.float64)
    s = np.sqrt(p0 * v + p1 * p1) if model == "pg" else p0
    want = np.clip(v + s * _randn64(seed, idx), 0, 255).astype(np.uint8)
    got = _run(hip, img, model, p0, p1, seed)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{model}: {int((diff != 0).sum())} of {diff.size} bytes differ from the float64 restatement, max {int(diff.max())}")
    assert diff.max() <= 1 and (diff != 0).mean() <= 5e-3


# ------------------------------------------------------------------ statistics: every bar is 5 standard errors from sigma and N
def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("sigma", [5.0, 25.0])
def test_statistics_of_g_and_gray(hip, sigma):
    """a constant image of 128: out - 128 has the mean -0.5 (the truncation) and the variance sigma^2 + 1/12"""
    img = np.full((256, 256, 3), 128, dtype=np.uint8)
    var = sigma * sigma + 1.0 / 12.0
    g, g2, gray = _run(hip, img, "g", sigma, 0.0, 1001), _run(hip, img, "g", sigma, 0.0, 1002), _run(hip, img, "gray", sigma, 0.0, 1003)
    assert np.array_equal(gray[:, :, 0], gray[:, :, 1]) and np.array_equal(gray[:, :, 0], gray[:, :, 2])
    for name, out in (("g", g), ("gray", gray[:, :, 0])):          # gray: one deviate per pixel, N = 256^2
        e = out.astype(np.float64) - 128.0
        N = e.size
        assert N == (3 if name == "g" else 1) * 256 * 256
        print(f"{name} sigma {sigma}: mean {e.mean():+.5f} (bar {5 * np.sqrt(var / N):.5f} around -0.5), var {e.var():.4f} "
              f"(bar {5 * np.sqrt(2.0 / N) * var:.4f} around {var:.4f}), min {out.min()}, max {out.max()}")
        assert out.min() > 0 and out.max() < 255, name             # sigma 25 clips with probability < 2e-7 per byte: nothing is masked
        assert abs(e.mean() + 0.5) <= 5 * np.sqrt(var / N), name
        assert abs(e.var() - var) <= 5 * np.sqrt(2.0 / N) * var, name
    pairs = {"R and G under g": (g[:, :, 0], g[:, :, 1]), "G and B under g": (g[:, :, 1], g[:, :, 2]),
             "horizontal neighbours (g)": (g[:, :-1, :], g[:, 1:, :]), "horizontal neighbours (gray)": (gray[:, :-1, 0], gray[:, 1:, 0]),
             "vertical neighbours (g)": (g[:-1], g[1:]), "two seeds": (g, g2)}
    for name, (a, b) in pairs.items():
        c = _corr(a, b)
        print(f"{name} sigma {sigma}: correlation {c:+.5f} (bar {5 / np.sqrt(a.size):.5f})")
        assert abs(c) <= 5 / np.sqrt(a.size), name


def test_statistics_of_pg(hip):
    """a = 0.5, b = 2 on an image whose left half is 40 and right half 200: the variances are 24 + 1/12 and 104 + 1/12"""
    img = np.empty((256, 256, 3), dtype=np.uint8)
    img[:, :128], img[:, 128:] = 40, 200
    out = _run(hip, img, "pg", 0.5, 2.0, 2001).astype(np.float64)
    N = 3 * 256 * 128
    sd = []
    for name, e, v, var in (("left", out[:, :128], 40.0, 24.0 + 1.0 / 12.0), ("right", out[:, 128:], 200.0, 104.0 + 1.0 / 12.0)):
        e = e - v
        assert e.size == N
        print(f"pg {name}: mean {e.mean():+.5f} (bar {5 * np.sqrt(var / N):.5f} around -0.5), var {e.var():.4f} "
              f"(bar {5 * np.sqrt(2.0 / N) * var:.4f} around {var:.4f})")
        assert abs(e.mean() + 0.5) <= 5 * np.sqrt(var / N), name
        assert abs(e.var() - var) <= 5 * np.sqrt(2.0 / N) * var, name
        sd.append(np.sqrt(e.var()))
    # a sample standard deviation has the relative standard error 1 / sqrt(2 N); the ratio of two independent ones sqrt(2) times that
    want = np.sqrt((104.0 + 1.0 / 12.0) / (24.0 + 1.0 / 12.0))
    print(f"pg: ratio of the standard deviations {sd[1] / sd[0]:.5f} (bar {5 * want / np.sqrt(N):.5f} around {want:.5f})")
    assert abs(sd[1] / sd[0] - want) <= 5 * want / np.sqrt(N)


# ------------------------------------------------------------------ beyond 2^31 bytes
def test_an_image_beyond_2_31_bytes(hip):
    """21846 x 32768 pixels are 2^31 + 65536 bytes: the last row starts below byte 2^31 and ends above it, and the grid is at its cap, so
    every thread strides.  The last row is noised (not left a copy) with the statistics of the model, the first row has the bytes of a
    one-row image of the same width (the counters of row 0 do not depend on the height).  About 4.3 GB of device memory."""
    h, w, sigma = 21846, 32768, 25.0
    assert 3 * h * w > 2 ** 31 and 3 * (h - 1) * w < 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip("less than 6 GiB of free device memory")
    src = torch.full((h, w, 3), 128, dtype=torch.uint8, device="cuda")
    dst = torch.full((h, w, 3), 128, dtype=torch.uint8, device="cuda")
    hip.noise_u8(src, "g", sigma, 0.0, 31, out=dst)
    torch.cuda.synchronize()
    first, last, mid = dst[0].cpu().numpy(), dst[-1].cpu().numpy(), dst[h // 2].cpu().numpy()
    assert bool((src[-1] == 128).all()) and bool((src[0] == 128).all())
    del src, dst
    small = hip.noise_u8(torch.full((1, w, 3), 128, dtype=torch.uint8, device="cuda"), "g", sigma, 0.0, 31)
    assert np.array_equal(first, small[0].cpu().numpy())
    var, N = sigma * sigma + 1.0 / 12.0, 3 * w
    for name, row in (("last", last), ("middle", mid)):
        e = row.astype(np.float64) - 128.0
        print(f"{name} row: {float((row != 128).mean()):.4f} of the bytes changed, mean {e.mean():+.4f}, var {e.var():.3f}")
        assert (row != 128).mean() > 0.9, name                     # P(out == 128) is 1 / (25 sqrt(2 pi)) = 1.6 %
        assert abs(e.mean() + 0.5) <= 5 * np.sqrt(var / N) and abs(e.var() - var) <= 5 * np.sqrt(2.0 / N) * var, name
        assert not np.array_equal(row, first), name
    assert abs(_corr(last, mid)) <= 5 / np.sqrt(N)
