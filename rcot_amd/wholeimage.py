"""Whole images of ANY size through the networks: pad bottom / right to the network's size multiple on the device, run, and let the
egress kernel crop, quantise and measure (csrc/imageio.hip: rcot_image_ingest, rcot_pad2d, rcot_image_egress).

The reference's validation (trainer.py:195-198) and testers (tester.py:77-84, tester_noise.py:84-86) skip or trim every image whose
height or width the network's resampling stages do not divide — 481 x 321 (Rain100L, BSD68) and the arbitrary sizes of SOTS / Urban100
among them.  The usual remedy for Restormer-class networks is used here: pad to the next multiple, restore, crop.  The multiple is read
from the network (``size_multiple``: 8 for ``T_net``, 4 for ``MPRNetHip``).  Opt-in: ``--val_pad`` of rcot_amd.trainer, ``--pad`` /
``--metrics device`` of rcot_amd.tester; without them both run the reference's rules unchanged.

Only four numbers per image come back to the host (``image_metrics``): the squared-error sums under the float PSNR of ``trainer.psnr``
and the 8-bit PSNR of ``tester.psnr_uint8``, and the sum and element count of the SSIM map of ``tester.ssim_image``.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

PAD_MODES = ("none", "reflect", "replicate")


class Restored(NamedTuple):
    """``out`` / ``x``: the network's output and its (padded) input, float [1, 3, Hp, Wp] on the device; the image is their top-left h x w"""
    out: torch.Tensor
    x: torch.Tensor
    h: int
    w: int
    Hp: int
    Wp: int


def pad_geometry(h: int, w: int, mult: int, mode) -> tuple:
    """(Hp, Wp): h and w rounded up to multiples of ``mult``.  Raises ValueError where ``mode`` cannot pad that far: "none" pads nothing,
    "reflect" mirrors without repeating the border pixel and so reaches at most h - 1 rows / w - 1 columns (torch's rule)."""
    mode = "none" if mode is None else mode
    if mode not in PAD_MODES:
        raise ValueError(f"padding mode {mode!r}: expected one of {PAD_MODES}")
    if h <= 0 or w <= 0 or mult <= 0:
        raise ValueError(f"{h} x {w}: an image needs at least one pixel (size multiple {mult})")
    Hp, Wp = (h + mult - 1) // mult * mult, (w + mult - 1) // mult * mult
    if mode == "none" and (Hp, Wp) != (h, w):
        raise ValueError(f"{h} x {w} is not a multiple of {mult} (the network's resampling levels) and no padding was asked for")
    if mode == "reflect" and (Hp - h > h - 1 or Wp - w > w - 1):
        raise ValueError(f"{h} x {w}: reflect padding to {Hp} x {Wp} needs {max(Hp - h, Wp - w)} mirrored pixels, more than the image "
                         f"has beside its border (use replicate)")
    return Hp, Wp


def restore_any_size(net, x_or_u8, mult: int, pad, tile: int = 0, overlap: int = 32, window: str = "uniform", tile_batch: int = 1,
                     ensemble: int = 1) -> Restored:
    """Pad (``pad``: "none" | "reflect" | "replicate"), then ``net`` on the padded image — whole, or as the overlapping tiles of
    ``tester.restore``, with its ``window`` / ``tile_batch`` / ``ensemble`` — WITHOUT cropping: rcot_image_egress crops.  ``x_or_u8``: a uint8 [h, w, 3] image (goes through
    rcot_image_ingest) or a float [1, 3, h, w] / [3, h, w] tensor (rcot_pad2d); host tensors are copied to the network's device."""
    from .tester import restore
    be = net.be
    x = x_or_u8.to(be.device)
    if x.dtype == torch.uint8:
        h, w = x.shape[:2]
        Hp, Wp = pad_geometry(h, w, mult, pad)
        xp = be.image_ingest(x.contiguous(), Hp, Wp, pad)
    else:
        h, w = x.shape[-2:]
        Hp, Wp = pad_geometry(h, w, mult, pad)
        x = x.reshape(1, 3, h, w).contiguous()
        xp = x if (Hp, Wp) == (h, w) else be.pad2d(x, Hp, Wp, pad)
    return Restored(restore(net, xp, tile, overlap, mult, None, window, tile_batch, ensemble), xp, h, w, Hp, Wp)


def image_metrics(stats, h: int, w: int) -> dict:
    """``stats``: the four numbers of rcot_image_egress for an h x w image -> psnr_float (``trainer.psnr``, data range 1), psnr_u8
    (``tester.psnr_uint8``) and ssim (``tester.ssim_image``), with their conventions: inf at zero error, NaN for an empty SSIM map
    (images under 11 pixels on a side: numpy's mean of nothing)."""
    s = [float(v) for v in (stats.tolist() if hasattr(stats, "tolist") else stats)]
    n = 3.0 * h * w
    ef, e8 = s[0] / n, s[1] / n
    return dict(psnr_float=float("inf") if ef == 0.0 else 10.0 * math.log10(1.0 / ef),
                psnr_u8=float("inf") if e8 == 0.0 else 10.0 * math.log10(255.0 * 255.0 / e8),
                ssim=s[2] / s[3] if s[3] else float("nan"))
