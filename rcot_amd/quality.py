"""The standard SSIM protocols and Y-channel PSNR / SSIM of published restoration tables, restated in numpy fp64 on host arrays; the
device computes the same sums in csrc/quality.hip (rcot_image_quality, ``HipBackend.image_quality``).

The reference's own figure (evaluate.py:53-73, what ``rcot_amd.tester`` prints by default) is a 2 x 2 box window cropped [5:-5] and cannot
be compared with any published number.  The protocols here can:

* ``uniform7`` / ``rgb`` — skimage's default ``structural_similarity`` per channel, the AirNet / PromptIR protocol (the reference's
  util/val_utils.py:50-66);
* ``gauss11`` — the 11 x 11, sigma 1.5 Gaussian window of the original SSIM paper, basicsr's ``calculate_ssim`` and MATLAB-style scripts;
* ``y`` — either of them, and PSNR, on the luma plane of YCbCr, as deraining tables (Rain100L) are reported.

Definitions.  Both metrics act on two uint8 HWC images ``a``, ``b`` of equal shape [h, w, 3]: the 8-bit values that land in the PNGs,
data range 255.

Colour space: ``rgb`` — the three channels are three planes.  ``y`` — one plane, the 8-bit luma of ITU-R BT.601 as MATLAB's ``rgb2ycbcr``
/ basicsr's ``bgr2ycbcr(y_only)`` give it for uint8 input, defined in integers so that it has one answer:
``n = 65481 R + 128553 G + 24966 B``, ``Y = 16 + (n + 127500) // 255000`` (round-half-up; 16..235).  The float form
``rint(16 + (65.481 R + 128.553 G + 24.966 B) / 255)`` is not the definition: 194 of the 2^24 colour triples are exact ties, and its fp64
evaluation differs from the integer rule on 107 triples.

Window: ``uniform7`` — 7 taps of 1/7 per axis, ``cov_norm = 49/48`` (skimage's defaults, ``use_sample_covariance=True``).  ``gauss11`` — 11
taps ``exp(-x^2 / (2 1.5^2))``, x = -5..5, normalised to sum 1, ``cov_norm = 1`` (``cv2.getGaussianKernel(11, 1.5)``, basicsr, skimage with
``gaussian_weights=True, use_sample_covariance=False``).  ``box2`` names the reference's own map (``tester.ssim_image``) and is kept here
only so that it can be asked for on the luma plane.

The window is applied separably to a, b, a^2, b^2, ab, giving ux, uy, uxx, uyy, uxy; ``vx = cov_norm (uxx - ux^2)``, vy and vxy alike;
``C1 = (0.01 255)^2``, ``C2 = (0.03 255)^2``; ``S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2))``.  S is evaluated only
where the whole window lies inside the image — (h - win + 1)(w - win + 1) positions per plane, which is skimage's crop by (win - 1) / 2
and basicsr's [5:-5], so no border rule is involved.  The metric is the mean of S over all positions of all planes (every plane has the
same count, so this is the mean of the per-channel means); when h < win or w < win the map is empty: sum 0, count 0, metric NaN.

PSNR is ``10 log10(255^2 / mean((a - b)^2))`` over the planes of the chosen space, ``inf`` at zero error (in ``rgb``: ``tester.psnr_uint8``).

PSNR-B (``psnrb_u8``; the device's sums: rcot_image_blockiness, ``HipBackend.image_blockiness``) and the border shave of SR tables
(``shave_u8``; rcot_crop_u8) are defined at the end of this file.
"""
from __future__ import annotations

import math
import warnings

import numpy as np

WINDOWS = ("box2", "uniform7", "gauss11")
SPACES = ("rgb", "y")
WINDOW_SIZE = {"uniform7": 7, "gauss11": 11}
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def luma_u8(img: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] RGB -> uint8 [h, w]: the integer BT.601 luma of the module docstring"""
    v = np.asarray(img).astype(np.int64)
    n = 65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2]
    return (16 + (n + 127500) // 255000).astype(np.uint8)


def window_weights(window: str) -> np.ndarray:
    """The taps of one axis, fp64.  The Gaussian's are summed in index order, as the host side of rcot_image_quality does."""
    if window == "uniform7":
        return np.full(7, 1.0 / 7.0)
    if window == "gauss11":
        g = [math.exp(-float(x * x) / (2.0 * 1.5 * 1.5)) for x in range(-5, 6)]
        s = 0.0
        for v in g:
            s += v
        return np.array([v / s for v in g], dtype=np.float64)
    raise ValueError(f"window {window!r}: expected 'uniform7' or 'gauss11'")


def planes_u8(img: np.ndarray, space: str) -> np.ndarray:
    """uint8 [h, w, 3] -> int64 [planes, h, w] of the colour space"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected a uint8 [h, w, 3] image")
    if space == "rgb":
        return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.int64)
    if space == "y":
        return luma_u8(img).astype(np.int64)[None]
    raise ValueError(f"color space {space!r}: expected one of {SPACES}")


def _valid_filter(p: np.ndarray, window: str) -> np.ndarray:
    """[h, w] -> [h - win + 1, w - win + 1]: the separable window at the positions where it lies inside the plane.  uniform7: integer window
    sums (exact) divided by 49 once; gauss11: fp64, rows then columns."""
    win = WINDOW_SIZE[window]
    h, w = p.shape
    if window == "uniform7":
        c = np.zeros((h + 1, w + 1), dtype=np.int64)
        c[1:, 1:] = p.cumsum(0).cumsum(1)
        return (c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]) / 49.0
    wt = window_weights(window)
    f = p.astype(np.float64)
    hz = sum(wt[k] * f[:, k:w - win + 1 + k] for k in range(win))
    return sum(wt[k] * hz[k:h - win + 1 + k, :] for k in range(win))


def ssim_sums(im1: np.ndarray, im2: np.ndarray, window: str, space: str):
    """(sum of the SSIM map over all planes, its position count) — stats[2], stats[3] of rcot_image_quality"""
    if window not in WINDOW_SIZE:
        raise ValueError(f"window {window!r}: expected 'uniform7' or 'gauss11'")
    a, b = planes_u8(im1, space), planes_u8(im2, space)
    if a.shape != b.shape:
        raise ValueError("the two images differ in shape")
    win = WINDOW_SIZE[window]
    _, h, w = a.shape
    if h < win or w < win:
        return 0.0, 0
    cov_norm = 49.0 / 48.0 if window == "uniform7" else 1.0
    total = 0.0
    for x, y in zip(a, b):
        ux, uy = _valid_filter(x, window), _valid_filter(y, window)
        uxx, uyy, uxy = _valid_filter(x * x, window), _valid_filter(y * y, window), _valid_filter(x * y, window)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        total += float(s.sum())
    return total, a.shape[0] * (h - win + 1) * (w - win + 1)


def ssim_windowed(im1: np.ndarray, im2: np.ndarray, window: str, space: str) -> float:
    """SSIM of two uint8 [h, w, 3] images under ``window`` ("uniform7" | "gauss11"; "box2": the reference's map, ``tester.ssim_image``, on
    the planes of the space) and ``space`` ("rgb" | "y"); NaN for an empty map"""
    if window == "box2":
        from .tester import ssim_plane
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # numpy's mean of an empty map: the NaN is the documented result
            return float(np.mean([ssim_plane(x, y) for x, y in zip(planes_u8(im1, space), planes_u8(im2, space))]))
    total, count = ssim_sums(im1, im2, window, space)
    return total / count if count else float("nan")


def sqerr_sums(im1: np.ndarray, im2: np.ndarray, space: str):
    """(sum of (a - b)^2 over the planes, its element count), exact integers — stats[0], stats[1] of rcot_image_quality"""
    a, b = planes_u8(im1, space), planes_u8(im2, space)
    if a.shape != b.shape:
        raise ValueError("the two images differ in shape")
    return int(((a - b) ** 2).sum()), int(a.size)


def psnr_u8(im1: np.ndarray, im2: np.ndarray, space: str) -> float:
    e, n = sqerr_sums(im1, im2, space)
    return quality_metrics([e, n, 0.0, 0])["psnr"]


def quality_metrics(stats) -> dict:
    """``stats``: the four numbers of rcot_image_quality -> dict(psnr, ssim): inf at zero error, NaN for an empty SSIM map"""
    s = [float(v) for v in (stats.tolist() if hasattr(stats, "tolist") else stats)]
    err = s[0] / s[1] if s[1] else float("nan")
    return dict(psnr=float("inf") if err == 0.0 else 10.0 * math.log10(255.0 * 255.0 / err),
                ssim=s[2] / s[3] if s[3] else float("nan"))


# ------------------------------------------------------------------------------- PSNR-B and the border shave
# PSNR-B (Yim & Bovik, "Quality assessment of deblocked images", IEEE TIP 2011; basicsr's ``calculate_psnrb``) adds a blocking-effect
# factor (BEF) to the mean squared error: how much stronger the steps of the RESTORED image ``a`` across the borders of the codec's
# 8 x 8 blocks are than its steps elsewhere.  The block grid has an origin (oy, ox), each 0 .. 7: the position of the image's first pixel
# inside the grid — 0 for a whole image, ``n % 8`` after ``n`` pixels were shaved from every side, so that the borders stay where the
# codec put them.  For one plane p of a: the horizontal pair (y, x), (y, x + 1), 0 <= x <= w - 2, is a border pair when
# (x + ox) % 8 == 7 and an inner pair otherwise; D_hb, D_hi are the sums of (p[y, x] - p[y, x + 1])^2 over the two classes and N_hb, N_hi
# their pair counts; the vertical pairs give D_vb, D_vi, N_vb, N_vi with oy.  N_b = N_hb + N_vb, N_i = N_hi + N_vi; BEF = 0 when either is
# 0 or min(h, w) < 2, else with D_B = (D_hb + D_vb) / N_b and D_C = (D_hi + D_vi) / N_i: BEF = (log2 8 / log2 min(h, w)) (D_B - D_C) when
# D_B > D_C (decided in exact integers), else 0.  PSNR-B of the plane = 10 log10(255^2 / (mean (a - b)^2 + BEF)), inf at a zero
# denominator; PSNR-B of the image = the mean over the planes (basicsr's per-channel mean; ``psnr_u8`` pools the planes instead).
# With origin 0 and h, w multiples of 8 this is basicsr's calculate_psnrb and the MATLAB original (the ratio is the same on the 0 .. 1 and
# the 0 .. 255 scale).  At other sizes basicsr's border counts are inconsistent with the pairs it sums (``arange(7, W - 1, 8)`` against
# ``W // 8 - 1``); the rule here counts the pairs that exist.
BLOCK = 8


def shave_u8(img: np.ndarray, n: int) -> np.ndarray:
    """[h, w, ...] -> [h - 2n, w - 2n, ...]: ``n`` pixels off every side (SR tables shave ``scale`` pixels before PSNR / SSIM)"""
    if n < 0:
        raise ValueError(f"shave {n}: expected an integer >= 0")
    h, w = img.shape[:2]
    if n and (h <= 2 * n or w <= 2 * n):
        raise ValueError(f"shave {n}: nothing is left of {h} x {w} pixels")
    return img[n:h - n, n:w - n]


def _origin(oy: int, ox: int):
    if not (0 <= oy < BLOCK and 0 <= ox < BLOCK):
        raise ValueError(f"block-grid origin ({oy}, {ox}): expected 0 .. {BLOCK - 1} each")


def blockiness_counts(h: int, w: int, oy: int = 0, ox: int = 0):
    """(N_hb, N_hi, N_vb, N_vi): the pairs that exist in an h x w plane under the grid origin (oy, ox).  With origin 0 and h, w
    multiples of 8 these are basicsr's (and the MATLAB original's) counts; at other sizes basicsr's border counts are inconsistent
    with the pairs it sums (``arange(7, W - 1, 8)`` against ``W // 8 - 1``), and this rule counts the pairs that exist."""
    _origin(oy, ox)
    nxb = sum(1 for x in range(w - 1) if (x + ox) % BLOCK == BLOCK - 1)
    nyb = sum(1 for y in range(h - 1) if (y + oy) % BLOCK == BLOCK - 1)
    n_hb, n_vb = h * nxb, w * nyb
    return n_hb, h * (w - 1) - n_hb, n_vb, w * (h - 1) - n_vb


def blockiness_sums(a: np.ndarray, space: str, oy: int = 0, ox: int = 0) -> np.ndarray:
    """int64 [planes, 4]: (D_hb, D_hi, D_vb, D_vi) of every plane of ``a`` — stats[:, 1:] of rcot_image_blockiness"""
    _origin(oy, ox)
    p = planes_u8(a, space)
    _, h, w = p.shape
    dh, dv = (p[:, :, :-1] - p[:, :, 1:]) ** 2, (p[:, :-1, :] - p[:, 1:, :]) ** 2
    xb, yb = (np.arange(w - 1) + ox) % BLOCK == BLOCK - 1, (np.arange(h - 1) + oy) % BLOCK == BLOCK - 1
    return np.stack([dh[:, :, xb].sum(axis=(1, 2)), dh[:, :, ~xb].sum(axis=(1, 2)),
                     dv[:, yb, :].sum(axis=(1, 2)), dv[:, ~yb, :].sum(axis=(1, 2))], axis=1).astype(np.int64)


def bef_from_sums(sums, h: int, w: int, oy: int = 0, ox: int = 0) -> float:
    """the blocking-effect factor of one plane from its (D_hb, D_hi, D_vb, D_vi)"""
    d_hb, d_hi, d_vb, d_vi = (int(v) for v in sums)
    n_hb, n_hi, n_vb, n_vi = blockiness_counts(h, w, oy, ox)
    n_b, n_i, d_b, d_c = n_hb + n_vb, n_hi + n_vi, d_hb + d_vb, d_hi + d_vi
    if n_b == 0 or n_i == 0 or min(h, w) < 2 or d_b * n_i <= d_c * n_b:
        return 0.0
    return (math.log2(BLOCK) / math.log2(min(h, w))) * (d_b / n_b - d_c / n_i)


def psnrb_from_sums(stats, h: int, w: int, oy: int = 0, ox: int = 0) -> float:
    """``stats``: integers [planes][5], per plane (sum (a - b)^2, D_hb, D_hi, D_vb, D_vi) — what rcot_image_blockiness writes -> PSNR-B,
    the mean over the planes.  The host path and the device path both end here, so they print the same floats."""
    rows = stats.tolist() if hasattr(stats, "tolist") else stats
    out = []
    for row in rows:
        den = int(row[0]) / (h * w) + bef_from_sums(row[1:5], h, w, oy, ox)
        out.append(float("inf") if den == 0.0 else 10.0 * math.log10(255.0 * 255.0 / den))
    return sum(out) / len(out)


def blockiness_stats(a: np.ndarray, b: np.ndarray, space: str, oy: int = 0, ox: int = 0) -> np.ndarray:
    """int64 [planes, 5]: the host's restatement of rcot_image_blockiness (``a`` is the restored image, ``b`` the target)"""
    pa, pb = planes_u8(a, space), planes_u8(b, space)
    if pa.shape != pb.shape:
        raise ValueError("the two images differ in shape")
    return np.concatenate([((pa - pb) ** 2).sum(axis=(1, 2))[:, None], blockiness_sums(a, space, oy, ox)], axis=1).astype(np.int64)


def psnrb_u8(a: np.ndarray, b: np.ndarray, space: str, oy: int = 0, ox: int = 0) -> float:
    """PSNR-B of the restored uint8 [h, w, 3] image ``a`` against the target ``b`` on the planes of ``space``"""
    return psnrb_from_sums(blockiness_stats(a, b, space, oy, ox), a.shape[0], a.shape[1], oy, ox)
