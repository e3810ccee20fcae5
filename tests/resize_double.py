"""TEST DOUBLE — not part of the product, never imported by rcot_amd/.

Restatements of the resize kernel's arithmetic and of the 8-bit super-resolution chain in numpy, shared by tests/test_resize_cpu.py
and tests/test_resize_gpu.py, the ``TorchDouble`` extended by the three backend methods the chain calls, and the accessors of
tests/golden/resize.npz (scripts/make_resize_fixture.py).
"""
from __future__ import annotations

import numpy as np
import torch

from host_double import TorchDouble
from rcot_amd import resize as RZ

#: (H, W) -> (out_h, out_w), the cases of tests/golden/resize.npz in its order
CASES = [((48, 36), (12, 9)), ((48, 36), (16, 12)), ((48, 36), (24, 18)), ((12, 9), (48, 36)), ((16, 12), (48, 36)),
         ((24, 18), (48, 36)), ((20, 28), (5, 7)), ((5, 7), (20, 28)), ((7, 5), (27, 18)), ((40, 24), (10, 6)), ((24, 40), (96, 160))]
#: the four orientations of the fixture: (rows flipped, columns flipped)
ORIENTATIONS = [(False, False), (True, False), (False, True), (True, True)]


def case_input(i: int) -> np.ndarray:
    """the seeded uint8 [H, W] input of case ``i`` (the fixture stores it too; the tests compare)"""
    (H, W), _ = CASES[i]
    return np.random.Generator(np.random.PCG64(9100 + i)).integers(0, 256, size=(H, W), dtype=np.uint8)


def flip(a: np.ndarray, fr: bool, fc: bool) -> np.ndarray:
    """rows / columns of the last two axes reversed"""
    if fr:
        a = a[..., ::-1, :]
    if fc:
        a = a[..., :, ::-1]
    return a


def sound_mask(H: int, W: int, out_h: int, out_w: int, fr: bool, fc: bool) -> np.ndarray:
    """bool [out_h, out_w]: the outputs whose unmirrored taps are all >= 0 along both axes when the resize runs on the image flipped
    by (fr, fc) — where the reference's border deviation does not reach — in the coordinates of the result flipped back"""
    rows = RZ.cubic_taps(H, out_h)[2] >= 0
    cols = RZ.cubic_taps(W, out_w)[2] >= 0
    if H == out_h:
        rows[:] = True
    if W == out_w:
        cols[:] = True
    return flip(rows[:, None] & cols[None, :], fr, fc)


# ------------------------------------------------------------------ the kernel's arithmetic
def resize_axis_np(src: np.ndarray, axis: int, idx: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """src [planes, H, W] -> the resize along ``axis`` (0 rows, 1 columns) in the dtype of ``src``:
    acc = 0; for k ascending: acc = acc + taps[o, k] * src[idx[o, k]], each product and each sum rounded.  Indices are clamped."""
    n = src.shape[1 + axis]
    taps = taps.astype(src.dtype)
    idx = np.clip(idx, 0, n - 1)
    out_len, K = idx.shape
    shape = (src.shape[0], out_len, src.shape[2]) if axis == 0 else (src.shape[0], src.shape[1], out_len)
    acc = np.zeros(shape, dtype=src.dtype)
    for k in range(K):
        if axis == 0:
            acc = acc + taps[:, k][None, :, None] * src[:, idx[:, k], :]
        else:
            acc = acc + taps[:, k][None, None, :] * src[:, :, idx[:, k]]
    return acc


def imresize_np(x: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """x [planes, H, W] (float32: the kernel's arithmetic with fp32 taps; float64: the rule itself) -> [planes, out_h, out_w]"""
    H, W = x.shape[-2:]
    for axis in RZ.axis_order(H, W, out_h, out_w):
        n_in, n_out = ((H, out_h), (W, out_w))[axis]
        idx, taps, _ = RZ.cubic_taps(n_in, n_out)
        x = resize_axis_np(x, axis, idx, taps.astype(np.float32) if x.dtype == np.float32 else taps)
    return x


def imresize_matrix(x: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """fp64 application of ``cubic_taps`` as dense matrices (a second route through the tables: BLAS summation order)"""
    H, W = x.shape[-2:]
    x = x.astype(np.float64)
    for axis in RZ.axis_order(H, W, out_h, out_w):
        n_in, n_out = ((H, out_h), (W, out_w))[axis]
        idx, taps, _ = RZ.cubic_taps(n_in, n_out)
        M = np.zeros((n_out, n_in))
        np.add.at(M, (np.repeat(np.arange(n_out), idx.shape[1]), idx.ravel()), taps.ravel())
        x = np.einsum("oh,phw->pow", M, x) if axis == 0 else np.einsum("ow,phw->pho", M, x)
    return x


# ------------------------------------------------------------------ the 8-bit chain
def ingest_np(u8: np.ndarray, dtype=np.float32) -> np.ndarray:
    """uint8 [h, w, 3] -> [3, h, w] / 255 (correctly rounded in ``dtype``): rcot_image_ingest, mode none"""
    return np.ascontiguousarray(u8.transpose(2, 0, 1)).astype(dtype) / dtype(255)


def quant8_np(x: np.ndarray) -> np.ndarray:
    """[3, h, w] -> uint8 [h, w, 3]: clamp(0, 1), * 255, + 0.5, clamp(0, 255), truncate, each step rounded in the dtype of ``x``
    (out_u8 of rcot_image_egress)"""
    t = x.dtype.type
    a = np.clip(np.clip(x, t(0), t(1)) * t(255) + t(0.5), t(0), t(255))
    return np.ascontiguousarray(a.astype(np.uint8).transpose(1, 2, 0))


def upscale_u8_np(lr_u8: np.ndarray, out_h: int, out_w: int, dtype=np.float32) -> np.ndarray:
    return quant8_np(imresize_np(ingest_np(lr_u8, dtype), out_h, out_w))


def downscale_u8_np(hr_u8: np.ndarray, s: int, dtype=np.float32) -> np.ndarray:
    H, W = hr_u8.shape[:2]
    return quant8_np(imresize_np(ingest_np(hr_u8, dtype), H // s, W // s))


def degrade_u8_np(hr_u8: np.ndarray, s: int, dtype=np.float32) -> np.ndarray:
    """shrink, quantise, enlarge, quantise: rcot_amd.resize.sr_degrade_u8 restated"""
    H, W = hr_u8.shape[:2]
    return upscale_u8_np(downscale_u8_np(hr_u8, s, dtype), H, W, dtype)


# ------------------------------------------------------------------ the backend double
class ResizeDouble(TorchDouble):
    """``TorchDouble`` with the three methods ``rcot_amd.resize`` calls, restated on the CPU in fp32"""

    def resize_axis(self, src, axis, idx, taps, out=None):
        lead = src.shape[:-2]
        a = src.reshape(-1, *src.shape[-2:]).numpy()
        r = torch.from_numpy(resize_axis_np(a, axis, idx.numpy(), taps.numpy()))
        r = r.reshape(*lead, *r.shape[-2:])
        if out is not None:
            out.copy_(r)
            return out
        return r

    def image_ingest(self, img, Hp, Wp, mode, out=None):
        assert mode in (None, "none") and tuple(img.shape[:2]) == (Hp, Wp)
        r = torch.from_numpy(ingest_np(img.numpy()))[None]
        if out is not None:
            out.copy_(r.reshape(out.shape))
            return out
        return r

    def image_egress(self, restored, h, w, degraded=None, target=None, res_scale=2.0, want_out=True, want_res=False, want_stats=False,
                     ws=None):
        assert want_out and not want_res and not want_stats
        x = restored.reshape(3, *restored.shape[-2:]).numpy()[:, :h, :w]
        return torch.from_numpy(quant8_np(x)), None, None
