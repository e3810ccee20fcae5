"""MATLAB-rule bicubic resize on the device, and the degradation of the super-resolution task built on it.

The reference's README lists DIV2K super-resolution next to the other tasks: "the LR images undergo bicubic rescaling to match the
dimensions of their respective high-resolution counterparts".  That degradation is ``sr_degrade_u8``: shrink by s, quantise to 8 bits
(what a saved LR PNG holds), enlarge by s, quantise (what a saved upscaled PNG holds).  The resampling rule — MATLAB's
``imresize(..., 'bicubic')`` with antialiasing — is defined in the header comment of csrc/resize.hip; ``cubic_taps`` evaluates it into
the two tables ``rcot_resize_axis`` applies.  (The reference's unused util/imresize.py follows the same rule except along the top and
left borders: DESIGN.md section 5.)

    python -m rcot_amd.resize --in DIR --out DIR --scale S --mode degrade|down|up

writes PNG folders: ``down`` the LR set of an HR folder, ``up`` an LR folder enlarged by S, ``degrade`` both in one go (the trainer's
``--degset`` validation folder of an SR run).  ``degrade`` and ``down`` crop an image at the top left to a multiple of S first.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch


def cubic(x: np.ndarray) -> np.ndarray:
    """the cubic convolution kernel with a = -0.5"""
    a = np.abs(x)
    a2, a3 = a * a, a * a * a
    return np.where(a <= 1, 1.5 * a3 - 2.5 * a2 + 1, np.where(a <= 2, -0.5 * a3 + 2.5 * a2 - 4 * a + 2, 0.0))


def cubic_taps(n_in: int, n_out: int):
    """The rule for one axis of input length ``n_in`` and output length ``n_out`` -> (idx int32 [n_out, K] mirrored into [0, n_in),
    taps float64 [n_out, K] with rows that sum to 1, first_unmirrored int64 [n_out]: each row's lowest tap position before mirroring)"""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"cubic_taps: lengths must be positive, got {n_in} -> {n_out}")
    s = n_out / n_in
    kw = 4.0 if s >= 1 else 4.0 / s
    K = int(math.ceil(kw)) + 2
    u = np.arange(1, n_out + 1, dtype=np.float64) / s + 0.5 * (1 - 1 / s)
    first = np.floor(u - kw / 2).astype(np.int64) - 1
    pos = first[:, None] + np.arange(K, dtype=np.int64)[None, :]             # 0-based input pixels, before mirroring
    x = u[:, None] - pos - 1
    w = cubic(x) if s >= 1 else s * cubic(s * x)
    w = w / w.sum(axis=1, keepdims=True)
    j = np.mod(pos, 2 * n_in)                                               # numpy's mod is the mathematical one
    idx = np.where(j >= n_in, 2 * n_in - 1 - j, j)
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w), first


_TABLES = {}


def device_taps(n_in: int, n_out: int, device):
    """the tables of ``cubic_taps`` on ``device`` (idx int32, taps rounded to float32), made once per (n_in, n_out)"""
    key = (str(device), int(n_in), int(n_out))
    if key not in _TABLES:
        idx, w, _ = cubic_taps(n_in, n_out)
        _TABLES[key] = (torch.from_numpy(idx).to(device), torch.from_numpy(w.astype(np.float32)).to(device))
    return _TABLES[key]


def axis_order(H: int, W: int, out_h: int, out_w: int):
    """the axes a resize visits: the smaller scale first, rows first on a tie; an axis whose length stays is left alone (its table
    is the identity)"""
    order = [0, 1] if out_h / H <= out_w / W else [1, 0]
    return [a for a in order if (H, W)[a] != (out_h, out_w)[a]]


def imresize(x: torch.Tensor, out_h: int, out_w: int, backend=None) -> torch.Tensor:
    """x float [planes, H, W] on the device -> [planes, out_h, out_w]: one ``rcot_resize_axis`` launch per axis"""
    if backend is None:
        from .ops import default_backend
        backend = default_backend()
    H, W = x.shape[-2:]
    for axis in axis_order(H, W, out_h, out_w):
        n_in, n_out = ((H, out_h), (W, out_w))[axis]
        idx, taps = device_taps(n_in, n_out, backend.device)
        x = backend.resize_axis(x, axis, idx, taps)
    return x


def _quantise(x: torch.Tensor, backend) -> torch.Tensor:
    """float [3, h, w] -> uint8 [h, w, 3] by the rule of rcot_image_egress (clamp, * 255, + 0.5, truncate: MATLAB's rounding of
    positive values)"""
    h, w = x.shape[-2:]
    return backend.image_egress(x, h, w, want_out=True)[0]


def sr_upscale_u8(lr_u8: torch.Tensor, out_h: int, out_w: int, backend=None) -> torch.Tensor:
    """uint8 [h, w, 3] on the device -> uint8 [out_h, out_w, 3]: the bicubic baseline of an LR image"""
    if backend is None:
        from .ops import default_backend
        backend = default_backend()
    h, w = lr_u8.shape[:2]
    x = backend.image_ingest(lr_u8, h, w, "none").view(3, h, w)
    return _quantise(imresize(x, out_h, out_w, backend), backend)


def sr_downscale_u8(hr_u8: torch.Tensor, s: int, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] with H, W multiples of ``s`` -> the LR image uint8 [H / s, W / s, 3]"""
    if backend is None:
        from .ops import default_backend
        backend = default_backend()
    H, W = hr_u8.shape[:2]
    s = int(s)
    if s < 1 or H % s or W % s or H < s or W < s:
        raise ValueError(f"super-resolution x{s}: the image must be a positive multiple of {s} in both directions, got {H} x {W}")
    x = backend.image_ingest(hr_u8, H, W, "none").view(3, H, W)
    return _quantise(imresize(x, H // s, W // s, backend), backend)


def sr_degrade_u8(hr_u8: torch.Tensor, s: int, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] on the device, H and W multiples of ``s`` -> uint8 [H, W, 3]: ingest, shrink to H/s x W/s, 8-bit quantisation,
    ingest, enlarge to H x W, quantisation — what a saved LR PNG, enlarged and saved again, holds"""
    H, W = hr_u8.shape[:2]
    return sr_upscale_u8(sr_downscale_u8(hr_u8, s, backend), H, W, backend)


def modcrop(img: np.ndarray, s: int) -> np.ndarray:
    """the top-left part of an [H, W, ...] array whose sides are multiples of ``s``"""
    h, w = img.shape[0], img.shape[1]
    return img[:h - h % s, :w - w % s]


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="bicubic LR / upscaled PNG folders for the super-resolution task (MATLAB's imresize rule)")
    parser.add_argument("--in", dest="src", required=True, type=str, help="folder of input images")
    parser.add_argument("--out", dest="dst", required=True, type=str, help="folder the PNGs are written to")
    parser.add_argument("--scale", required=True, type=int, help="integer scale factor S >= 2")
    parser.add_argument("--mode", choices=["degrade", "down", "up"], default="degrade",
                        help="down: HR -> LR (H/S x W/S); up: LR -> enlarged by S; degrade: down then up, at the HR size")
    opt = parser.parse_args(argv)
    if opt.scale < 2:
        raise SystemExit(f"--scale {opt.scale}: the scale factor must be an integer >= 2")
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: rcot_amd.resize runs the HIP path only")
    from PIL import Image
    from .ops import default_backend
    be, s = default_backend(), opt.scale
    os.makedirs(opt.dst, exist_ok=True)
    done = 0
    for name in sorted(os.listdir(opt.src)):
        path = os.path.join(opt.src, name)
        if not os.path.isfile(path):
            continue
        img = np.array(Image.open(path).convert("RGB"))
        if opt.mode != "up":
            img = modcrop(img, s)
            if img.shape[0] < s or img.shape[1] < s:
                print(f"  skipped: {name} is smaller than {s} x {s}")
                continue
        d = torch.from_numpy(np.ascontiguousarray(img)).to(be.device)
        if opt.mode == "degrade":
            out = sr_degrade_u8(d, s, be)
        elif opt.mode == "down":
            out = sr_downscale_u8(d, s, be)
        else:
            out = sr_upscale_u8(d, img.shape[0] * s, img.shape[1] * s, be)
        Image.fromarray(out.cpu().numpy()).save(os.path.join(opt.dst, os.path.splitext(name)[0] + ".png"))
        done += 1
    print(f"{opt.mode} x{s}: {done} image(s) written to {opt.dst}")
    return done


if __name__ == "__main__":
    main()
