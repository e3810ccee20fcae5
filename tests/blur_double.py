"""TEST DOUBLE — not part of the product, never imported by rcot_amd/.

The PSF blur restated in numpy from the rule in the header comment of rcot_amd/csrc/blur.hip: integer weights q (int32 [K][K], K odd,
q >= 0, sum 2^22), a correlation, acc = sum_i sum_j q[i][j] src[by(y + i - r)][bx(x + j - r)], out = (acc + 2^21) >> 22, the border maps
replicate / mirror / wrap valid at any distance, and the sampling dst[oy][ox] = out[oy step + phase][ox step + phase].  Everything is
computed in int64 and acc + 2^21 is ASSERTED to stay below 2^31 (the kernel works in 32-bit integers).  ``BlurDouble`` is the CPU double
of the backend for the folder loader, the folder CLI and the BD chain."""
import numpy as np
import torch

from jpeg_double import JpegDouble
from resize_double import ResizeDouble

I64 = np.int64
BORDERS = {"replicate": 0, "mirror": 1, "wrap": 2}


def border_index(p, n, border):
    """b(p) of the rule for an int64 array of positions on an axis of length n"""
    p = np.asarray(p, dtype=I64)
    border = BORDERS.get(border, border)
    if border == 0:
        return np.clip(p, 0, n - 1)
    if border == 2:
        return np.mod(p, n)                                  # numpy's mod is the mathematical one
    assert border == 1
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    m = np.mod(p, period)
    return np.where(m < n, m, period - m)


def blur_np(img, q, border, step=1, phase=0):
    """img uint8 [H, W, 3], q int [K, K] -> uint8 [H / step, W / step, 3] by the rule"""
    img, q = np.asarray(img), np.asarray(q).astype(I64)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    K = q.shape[0]
    assert q.shape == (K, K) and K % 2 == 1 and (q >= 0).all() and int(q.sum()) == 1 << 22
    H, W = img.shape[:2]
    assert step >= 1 and 0 <= phase < step and H % step == 0 and W % step == 0
    r = (K - 1) // 2
    oh, ow = H // step, W // step
    # the image with its halo of r, gathered once through the border maps: big[y + r][x + r] = src[by(y)][bx(x)]
    iy = border_index(np.arange(-r, H + r, dtype=I64), H, border)
    ix = border_index(np.arange(-r, W + r, dtype=I64), W, border)
    big = img[np.ix_(iy, ix)].astype(I64)
    acc = np.zeros((oh, ow, 3), dtype=I64)
    for i in range(K):
        for j in range(K):
            if q[i, j]:                                      # the output at (oy step + phase, ox step + phase) reads big[.. + i][.. + j]
                acc += q[i, j] * big[phase + i:phase + i + (oh - 1) * step + 1:step, phase + j:phase + j + (ow - 1) * step + 1:step]
    acc += 1 << 21
    assert acc.size == 0 or (int(acc.min()) >= 0 and int(acc.max()) < (1 << 31)), "the accumulator leaves 31 bits"
    out = acc >> 22
    assert out.size == 0 or int(out.max()) <= 255
    return out.astype(np.uint8)


class BlurDouble(JpegDouble, ResizeDouble):
    """``TorchDouble`` with the method ``rcot_amd.blur`` calls, restated on the CPU, on top of the doubles of the bicubic chain (the BD
    degradation enlarges with it) and of the JPEG task (mixed task lists; the cached loader's one-launch batch as a loop over
    ``patch_prep``); ``blurs`` counts the whole-image blurs"""

    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.blurs = 0

    def blur_u8(self, img, psf_dev, border, step=1, phase=0, out=None):
        self.blurs += 1
        r = torch.from_numpy(blur_np(img.numpy(), psf_dev.numpy(), int(border), int(step), int(phase)))
        if out is not None:
            out.copy_(r)
            return out
        return r
