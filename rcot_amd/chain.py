"""Degradation chains: the whole-image degradations of the other tasks composed, with noise between them and parameters that may be drawn
per sample — blur -> noise -> JPEG, the "practical" order of DnCNN-3, of the first-order model of BSRGAN / Real-ESRGAN and of the
composite-degradation benchmarks, and what an all-in-one or blind model is trained on.

    chain_<stage>+<stage>+...           1 .. 6 stages, applied left to right to the WHOLE image; every stage keeps the image size

    blur_<spec>                         rcot_amd/blur.py's PSF grammar (g1.6, g2k15, a4x1r30, m15a30); m<L> without an angle draws whole
                                        degrees 0 .. 179 per sample
    sr_x2 | sr_x3 | sr_x4               bicubic down, 8 bits, up, 8 bits (rcot_amd.resize.sr_degrade_u8)
    jpeg_q<Q> | jpeg_q<Qlo>-<Qhi>       baseline JPEG round trip (rcot_amd.jpeg.jpeg_degrade_u8); a range draws an integer quality uniformly
                                        from Qlo .. Qhi, both included, 1 <= Qlo < Qhi <= 100
    noise_g<s> | noise_g<lo>-<hi>       white Gaussian noise of sigma s (8-bit units), channels independent; a range draws a real sigma
                                        uniformly from [lo, hi], 0 <= lo < hi <= 255
    noise_gray<s> | noise_gray<lo>-<hi> the same with one deviate shared by R, G and B of a pixel
    noise_pg<a>x<b>                     heteroscedastic Gaussian (Poisson-Gaussian) noise: variance a v + b^2 at the pixel value v

    chain_blur_g1.6+noise_g10+jpeg_q40      chain_noise_gray0-55      chain_sr_x2+noise_pg0.5x2+jpeg_q10-40      chain_blur_m15

Nothing else is a stage: no sr_bd_x3, no chain inside a chain, no empty stage, no range on any other parameter.  ``parse_de_type``
refuses all of that up front with a SystemExit that names the stage.

The stages are the existing entry points, called in order — ``blur_degrade_u8``, ``sr_degrade_u8``, ``jpeg_degrade_u8`` — and the one new
kernel ``rcot_noise_u8`` (csrc/noise.hip, where the noise rule is defined) through ``backend.noise_u8``; nothing is restated here.

Per-sample values.  ``draw(spec, rng, seed)`` takes what the chain draws from a ``random.Random`` stream IN STAGE ORDER — ``rng.randint(0,
179)`` for a motion PSF without an angle, ``rng.randint(Qlo, Qhi)`` for a ranged quality, ``rng.uniform(lo, hi)`` for a ranged sigma,
nothing for a fixed stage — and keeps the sample's noise seed.  The training loader calls it AFTER its three common draws (crop origin,
mode, noise seed), so every other task's draws stay what they are.

Noise seeds.  The noise stage at position k (0-based, counted over ALL stages of the chain) runs with

    stage_seed(seed, k) = ((seed XOR (k + 1)) * 0xD1342543DE82EF95) mod 2^64

one XOR-multiply step with an odd constant (a bijection of the 64-bit seed for every k).  The kernel's counter stream of a seed s is
mix64(s + 0x9e3779b97f4a7c15 (idx + 1)): seeds that differed by a small multiple of that increment would give shifted copies of one
noise field, which the multiplication rules out, so two noise stages of one chain are independent.

    python -m rcot_amd.chain --in DIR --out DIR --chain SPEC [--seed S] [--border replicate|mirror|wrap] [--subsampling 420|444]

writes the degraded images of a folder as PNGs (the trainer's ``--degset`` validation folder of a chain run).  The per-file values come
from ``file_draws(spec, S, index)`` — ``random.Random(S * 2_147_483_659 + index)``, index = the file's position in the sorted folder
listing; first the noise seed (``getrandbits(63)``), then the chain's draws — the rule of the tester's ``--chain``, so both write the same
bytes for the same seed.
"""
from __future__ import annotations

import collections
import glob
import math
import os
import random
import re

import numpy as np
import torch

MAX_STAGES = 6
PREFIX = "chain_"
GRAMMAR = ("a chain is chain_<stage>+<stage>+... with 1 .. 6 stages, each one of blur_<spec> (rcot_amd/blur.py's PSF grammar), sr_x2 | sr_x3 | "
           "sr_x4, jpeg_q<Q> | jpeg_q<Qlo>-<Qhi> (1 <= Qlo < Qhi <= 100), noise_g<s> | noise_gray<s> (s or <lo>-<hi> in 0 .. 255) and "
           "noise_pg<a>x<b>: chain_blur_g1.6+noise_g10+jpeg_q40, chain_noise_gray0-55, chain_sr_x2+noise_pg0.5x2+jpeg_q10-40")

_NUM = r"[0-9]+(?:\.[0-9]+)?"
_SR = re.compile(r"sr_x([234])\Z")
_JPEG = re.compile(r"jpeg_q([0-9]+)(?:-([0-9]+))?\Z")
_NOISE = re.compile(rf"noise_(gray|g)({_NUM})(?:-({_NUM}))?\Z")
_NOISE_PG = re.compile(rf"noise_pg({_NUM})x({_NUM})\Z")
_SEED_MUL = 0xD1342543DE82EF95
_MASK = (1 << 64) - 1

# what a sample brings to its chain: the noise seed and one value per stage (None for a stage that draws nothing)
Draws = collections.namedtuple("Draws", "seed values")


# ------------------------------------------------------------------ the grammar
def _refuse(name: str, stage: str, why: str):
    raise SystemExit(f"--de_type {name}: stage {stage!r} {why}; {GRAMMAR}")


def _parse_stage(name: str, stage: str) -> tuple:
    """one stage -> ("blur", spec) | ("sr", k) | ("jpeg", Qlo, Qhi) | ("noise", "g" | "gray", lo, hi) | ("noise", "pg", a, b); a fixed
    quality or sigma is the range lo == hi"""
    if stage == "":
        _refuse(name, stage, "is empty")
    if stage.startswith("chain"):
        _refuse(name, stage, "is a chain inside a chain")
    if stage.startswith("blur_"):
        from .blur import parse_psf
        try:
            parse_psf(stage[5:])
        except ValueError as e:
            _refuse(name, stage, f"is no blur stage ({e})")
        return ("blur", stage[5:])
    m = _SR.match(stage)
    if m:
        return ("sr", int(m.group(1)))
    m = _JPEG.match(stage)
    if m:
        lo = int(m.group(1))
        hi = lo if m.group(2) is None else int(m.group(2))
        if not (1 <= lo <= 100 and 1 <= hi <= 100):
            _refuse(name, stage, "has a quality outside 1 .. 100")
        if m.group(2) is not None and not lo < hi:
            _refuse(name, stage, "has a quality range that is not Qlo < Qhi")
        return ("jpeg", lo, hi)
    m = _NOISE.match(stage)
    if m:
        lo = float(m.group(2))
        hi = lo if m.group(3) is None else float(m.group(3))
        if not (0 <= lo <= 255 and 0 <= hi <= 255):
            _refuse(name, stage, "has a sigma outside 0 .. 255")
        if m.group(3) is not None and not lo < hi:
            _refuse(name, stage, "has a sigma range that is not lo < hi")
        return ("noise", m.group(1), lo, hi)
    m = _NOISE_PG.match(stage)
    if m:
        a, b = float(m.group(1)), float(m.group(2))
        if not (math.isfinite(a) and math.isfinite(b) and a <= 3.0e38 and b <= 1.0e19):      # a and b^2 are fp32 in the kernel
            _refuse(name, stage, "has a parameter that is no finite fp32 value")
        return ("noise", "pg", a, b)
    _refuse(name, stage, "is no stage of a chain")


def parse_de_type(name: str):
    """``chain_<stage>+...`` -> the tuple of its stage records; None for a name of another task; SystemExit, naming the stage, for
    anything malformed"""
    if not name.startswith("chain"):
        return None
    if not name.startswith(PREFIX):
        raise SystemExit(f"--de_type {name}: {GRAMMAR}")
    stages = name[len(PREFIX):].split("+")
    if len(stages) > MAX_STAGES:
        _refuse(name, stages[MAX_STAGES], f"is stage {MAX_STAGES + 1} of {len(stages)}: a chain has at most {MAX_STAGES}")
    return tuple(_parse_stage(name, s) for s in stages)


def parse_spec(text: str) -> tuple:
    """the ``--chain`` flag of the tools: the stages with or without the ``chain_`` prefix"""
    text = str(text)
    return parse_de_type(text if text.startswith(PREFIX) else PREFIX + text)


def _num(x) -> str:
    return np.format_float_positional(float(x), trim="-")                   # the shortest digits that read back as x, no exponent


def canonical(spec) -> str:
    """a name that ``parse_de_type`` reads back as ``spec``"""
    out = []
    for st in spec:
        if st[0] == "blur":
            out.append("blur_" + st[1])
        elif st[0] == "sr":
            out.append(f"sr_x{st[1]}")
        elif st[0] == "jpeg":
            out.append(f"jpeg_q{st[1]}" + ("" if st[1] == st[2] else f"-{st[2]}"))
        elif st[1] == "pg":
            out.append(f"noise_pg{_num(st[2])}x{_num(st[3])}")
        else:
            out.append(f"noise_{st[1]}{_num(st[2])}" + ("" if st[2] == st[3] else f"-{_num(st[3])}"))
    return PREFIX + "+".join(out)


# ------------------------------------------------------------------ what a chain needs and draws
def _stage_draws(st) -> bool:
    if st[0] == "blur":
        from .blur import needs_angle
        return needs_angle(st[1])
    if st[0] == "jpeg":
        return st[1] != st[2]
    return st[0] == "noise" and st[1] != "pg" and st[2] != st[3]


def has_noise(spec) -> bool:
    return any(st[0] == "noise" for st in spec)


def needs_draws(spec) -> bool:
    """some stage takes a value per sample"""
    return any(_stage_draws(st) for st in spec)


def cacheable(spec) -> bool:
    """the degraded twin of an image is the same for every sample: no noise stage, nothing drawn"""
    return not has_noise(spec) and not needs_draws(spec)


def size_multiple(spec) -> int:
    """the sides of an image must be multiples of this: the least common multiple of the scales of the chain's sr_x<k> stages (1 without one)"""
    m = 1
    for st in spec:
        if st[0] == "sr":
            m = m * st[1] // math.gcd(m, st[1])
    return m


def draw(spec, rng: random.Random, seed: int) -> Draws:
    """the chain's own draws from ``rng``, in stage order (module docstring); ``seed``: the sample's noise seed"""
    values = []
    for st in spec:
        if not _stage_draws(st):
            values.append(None)
        elif st[0] == "blur":
            values.append(rng.randint(0, 179))
        elif st[0] == "jpeg":
            values.append(rng.randint(st[1], st[2]))
        else:
            values.append(rng.uniform(st[2], st[3]))
    return Draws(int(seed), tuple(values))


def file_draws(spec, seed: int, index: int) -> Draws:
    """the values of the ``index``-th file of a sorted folder under ``--seed seed``: the rule of the folder tool and of the tester"""
    rng = random.Random(int(seed) * 2_147_483_659 + int(index))
    nseed = rng.getrandbits(63)
    return draw(spec, rng, nseed)


def stage_seed(seed: int, k: int) -> int:
    """the seed of the noise stage at position ``k`` of a chain (module docstring)"""
    return (((int(seed) & _MASK) ^ (int(k) + 1)) * _SEED_MUL) & _MASK


# ------------------------------------------------------------------ on the device
def chain_degrade_u8(img_u8: torch.Tensor, spec, draws: Draws, border: str = "replicate", subsampling: int = 2, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] on the device -> uint8 [H, W, 3]: the stages of ``spec`` applied left to right with the per-sample values
    ``draws`` (``draw`` / ``file_draws``).  ``border``: the rule of the blur stages; ``subsampling`` (PIL's number): of the JPEG stages.
    H and W must be multiples of ``size_multiple(spec)``.  The input is left as it is."""
    from . import blur as B
    from . import jpeg as J
    from . import resize as R
    be = B._backend(backend)
    if len(draws.values) != len(spec):
        raise ValueError(f"chain_degrade_u8: {len(spec)} stages, {len(draws.values)} drawn values")
    x = img_u8
    for k, (st, v) in enumerate(zip(spec, draws.values)):
        if st[0] == "blur":
            x = B.blur_degrade_u8(x, B.psf_q_of(st[1], v), border, be)
        elif st[0] == "sr":
            x = R.sr_degrade_u8(x, st[1], be)
        elif st[0] == "jpeg":
            x = J.jpeg_degrade_u8(x, st[1] if v is None else v, subsampling, be)
        else:
            p0, p1 = (st[2], st[3]) if st[1] == "pg" else (st[2] if v is None else v, 0.0)
            x = be.noise_u8(x, st[1], p0, p1, stage_seed(draws.seed, k), out=None if x is img_u8 else x)
    return x                                                # (every stage writes a tensor of its own: never the input)


def degrade_file_u8(img: np.ndarray, spec, seed: int, index: int, border: str, subsampling: int, be):
    """one file of a folder: uint8 [H, W, 3] on the host -> (clean, degraded) uint8 arrays of one size — the image cropped at the top
    left to a multiple of ``size_multiple(spec)``, and its chain under ``file_draws(spec, seed, index)`` — or None, with a message,
    for an image a stage cannot take"""
    from . import degrade                                   # the step of every whole-image task; the tester's too
    return degrade.degrade_file_u8(img, degrade.BY_FIELD["chain"].fields(spec, border, subsampling), file_draws(spec, seed, index), be)


# ------------------------------------------------------------------ the folder CLI
def main(argv=None, backend=None):
    """``backend``: the backend to run on (default: the process's HIP backend; a GPU is required then)"""
    import argparse
    from .blur import BORDERS
    from .jpeg import SUBSAMPLING
    parser = argparse.ArgumentParser(description="PNG folders degraded by a chain of blur, bicubic, JPEG and noise stages")
    parser.add_argument("--in", dest="src", required=True, type=str, help="folder of clean images")
    parser.add_argument("--out", dest="dst", required=True, type=str, help="folder the PNGs are written to")
    parser.add_argument("--chain", required=True, type=str, help="the stages, with or without the chain_ prefix: blur_g1.6+noise_g10+jpeg_q40")
    parser.add_argument("--seed", type=int, default=0, help="seed of the per-file values (noise, ranged parameters, motion angles)")
    parser.add_argument("--border", choices=sorted(BORDERS), default="replicate", help="the border rule of the blur stages")
    parser.add_argument("--subsampling", choices=sorted(SUBSAMPLING), default="420", help="chroma subsampling of the JPEG stages")
    opt = parser.parse_args(argv)
    spec = parse_spec(opt.chain)
    if backend is None:
        if not torch.cuda.is_available():
            raise SystemExit("No GPU found: rcot_amd.chain runs the HIP path only")
        from .ops import default_backend
        backend = default_backend()
    return degrade_folder(opt.src, opt.dst, spec, opt.seed, opt.border, SUBSAMPLING[opt.subsampling], backend)


def degrade_folder(src: str, dst: str, spec, seed: int, border: str, subsampling: int, be) -> int:
    """every image file of ``src`` -> ``dst``/<name>.png after the chain; returns the number written"""
    from PIL import Image
    os.makedirs(dst, exist_ok=True)
    done = 0
    for index, path in enumerate(sorted(glob.glob(os.path.join(src, "*")))):       # the tester's listing: the index is the file's there
        if not os.path.isfile(path):
            continue
        pair = degrade_file_u8(np.array(Image.open(path).convert("RGB")), spec, seed, index, border, subsampling, be)
        if pair is None:
            continue
        Image.fromarray(pair[1]).save(os.path.join(dst, os.path.splitext(os.path.basename(path))[0] + ".png"))
        done += 1
    print(f"{canonical(spec)} seed {seed}: {done} image(s) written to {dst}")
    return done


if __name__ == "__main__":
    main()
