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
