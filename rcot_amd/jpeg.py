"""The degradation of the compression-artifact task (the CAR rows, q = 10 / 20 / 30 / 40, of restoration tables): a baseline JPEG round
trip on the device.

Entropy coding is lossless, so an image that is saved as a JPEG and loaded again differs from the original only by colour conversion,
chroma subsampling, the integer DCT, quantisation and their inverses.  ``jpeg_degrade_u8`` applies exactly those steps
(``rcot_jpeg_roundtrip``; the rule is defined in the header comment of csrc/jpeg.hip) and gives, byte for byte, what

    Image.open(BytesIO(<the image saved with quality=Q, subsampling=S>))

holds with Pillow on libjpeg-turbo.  No bitstream is produced or parsed.

    python -m rcot_amd.jpeg --in DIR --out DIR --quality Q [--subsampling 420|444]

writes the degraded images of a folder as PNGs (the trainer's ``--degset`` validation folder of a ``jpeg_q<Q>`` run).
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch

# Annex K of the JPEG standard, in natural (row-major) order
LUMA_BASE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
             100, 103, 99)
CHROMA_BASE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32

SUBSAMPLING = {"420": 2, "444": 0}                          # the flag's spelling -> PIL's ``subsampling`` number
_DE_TYPE = re.compile(r"jpeg_q([0-9]+)\Z")


def check_quality(quality) -> int:
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be an integer in 1 .. 100, got {quality!r}")
    return q


def check_subsampling(subsampling) -> int:
    if subsampling not in (0, 2):
        raise ValueError(f"JPEG subsampling must be 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
    return int(subsampling)


def quant_tables(quality: int):
    """(luminance, chrominance): two lists of 64 divisors in natural order for ``quality`` in 1 .. 100 — the scaled Annex K tables,
    ``Image.quantization`` of a file saved with that quality"""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (LUMA_BASE, CHROMA_BASE))


def parse_de_type(name: str):
    """``jpeg_q<Q>`` -> Q; None for a name of another task; ValueError for a malformed name or a quality outside 1 .. 100"""
    if not name.startswith("jpeg"):
        return None
    m = _DE_TYPE.match(name)
    if not m:
        raise ValueError(f"--de_type {name}: the compression-artifact tasks are named jpeg_q<Q> with Q in 1 .. 100 (jpeg_q10, jpeg_q40)")
    q = int(m.group(1))
    if not 1 <= q <= 100:
        raise ValueError(f"--de_type {name}: the quality must be in 1 .. 100")
    return q


def jpeg_degrade_u8(img_u8: torch.Tensor, quality: int, subsampling: int = 2, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] on the device -> uint8 [H, W, 3]: the image after a baseline JPEG round trip at ``quality`` with ``subsampling``
    0 (4:4:4) or 2 (4:2:0, PIL's default; needs W > 4)"""
    if backend is None:
        from .ops import default_backend
        backend = default_backend()
    quality, subsampling = check_quality(quality), check_subsampling(subsampling)
    if subsampling == 2 and img_u8.shape[1] <= 4:
        raise ValueError(f"JPEG 4:2:0 round trip: the image must be wider than 4 pixels, got {img_u8.shape[0]} x {img_u8.shape[1]} "
                         f"(a codec switches to another upsampling rule there)")
    return backend.jpeg_roundtrip(img_u8, quality, subsampling)


def main(argv=None, backend=None):
    """``backend``: the backend to run on (default: the process's HIP backend; a GPU is required then)"""
    import argparse
    parser = argparse.ArgumentParser(description="JPEG-degraded PNG folders for the compression-artifact task (baseline round trip)")
    parser.add_argument("--in", dest="src", required=True, type=str, help="folder of clean images")
    parser.add_argument("--out", dest="dst", required=True, type=str, help="folder the PNGs are written to")
    parser.add_argument("--quality", required=True, type=int, help="JPEG quality 1 .. 100")
    parser.add_argument("--subsampling", choices=sorted(SUBSAMPLING), default="420", help="chroma subsampling (420 = PIL's default)")
    opt = parser.parse_args(argv)
    if not 1 <= opt.quality <= 100:
        raise SystemExit(f"--quality {opt.quality}: the quality must be in 1 .. 100")
    if backend is None:
        if not torch.cuda.is_available():
            raise SystemExit("No GPU found: rcot_amd.jpeg runs the HIP path only")
        from .ops import default_backend
        backend = default_backend()
    return degrade_folder(opt.src, opt.dst, opt.quality, SUBSAMPLING[opt.subsampling], backend)


def degrade_folder(src: str, dst: str, quality: int, subsampling: int, be) -> int:
    """every image file of ``src`` -> ``dst``/<name>.png after the round trip; returns the number written"""
    from PIL import Image
    os.makedirs(dst, exist_ok=True)
    done = 0
    for name in sorted(os.listdir(src)):
        path = os.path.join(src, name)
        if not os.path.isfile(path):
            continue
        img = np.array(Image.open(path).convert("RGB"))
        if subsampling == 2 and img.shape[1] <= 4:
            print(f"  skipped: {name} is not wider than 4 pixels")
            continue
        out = jpeg_degrade_u8(torch.from_numpy(np.ascontiguousarray(img)).to(be.device), quality, subsampling, be)
        Image.fromarray(out.cpu().numpy()).save(os.path.join(dst, os.path.splitext(name)[0] + ".png"))
        done += 1
    print(f"jpeg q{quality} {'4:2:0' if subsampling == 2 else '4:4:4'}: {done} image(s) written to {dst}")
    return done


if __name__ == "__main__":
    main()
