"""The degradations of the deblurring tasks and of the "BD" protocol of super-resolution tables: a whole image blurred on the device by a
per-call point-spread function (``rcot_blur_u8``; the rule — integer weights that sum to 2^22, a correlation, three border maps, an
optional sampling of the output — is defined in the header comment of csrc/blur.hip).

PSFs are float64 [K, K] arrays with K odd, no negative entry and the sum 1: ``psf_gaussian``, ``psf_gaussian_aniso`` and ``psf_motion``
make them, ``quantise_psf`` turns one into the int32 weights the kernel takes, ``parse_psf`` reads the spec grammar of the command lines

    g<sigma>[k<K>]                  isotropic Gaussian, 0 < sigma <= 10, K = 2 ceil(3 sigma) + 1 unless given          g1.6  g2k15
    a<s1>x<s2>r<deg>[k<K>]          anisotropic Gaussian, axes s1, s2, rotated by whole degrees 0 .. 179               a4x1r30  a3x1.5r120k15
    m<L>[a<deg>]                    linear motion of odd length L in 3 .. 63 at whole degrees 0 .. 179; without an angle the training
                                    loader draws one per sample                                                          m15  m15a30

``blur_degrade_u8`` is the blur, ``bd_degrade_u8`` the BD degradation of scale 3 (Gaussian 7 x 7, sigma 1.6, every third pixel from the
centre of each 3 x 3 cell, then the bicubic enlargement of rcot_amd/resize.py back to the HR size).

    python -m rcot_amd.blur --in DIR --out DIR --psf SPEC [--border replicate|mirror|wrap] [--mode blur|bd]

writes the degraded images of a folder as PNGs (the trainer's ``--degset`` validation folder of a ``blur_<spec>`` or ``sr_bd_x3`` run);
``--mode bd`` ignores ``--psf`` and crops an image at the top left to a multiple of 3 first.

The motion rule is this module's own (MATLAB's fspecial('motion') rasterises a line another way); no byte equality with it is claimed.
"""
from __future__ import annotations

import functools
import math
import os
import re

import numpy as np
import torch

WEIGHT_BITS = 22                                            # a PSF's integer weights sum to 2^22
KMAX = 63                                                   # the largest side rcot_blur_u8 takes
BORDERS = {"replicate": 0, "mirror": 1, "wrap": 2}          # the flag's spelling -> the ``border`` number of rcot_blur_u8
GRAMMAR = ("a PSF is g<sigma>[k<K>] (0 < sigma <= 10), a<s1>x<s2>r<deg>[k<K>] or m<L>[a<deg>] (L odd in 3 .. 63), with K odd in 1 .. 63 "
           "and whole degrees in 0 .. 179: g1.6, g2k15, a4x1r30, m15, m15a30")
BD_SPEC, BD_SCALE = "g1.6k7", 3

_NUM = r"([0-9]+(?:\.[0-9]+)?)"
_G = re.compile(rf"g{_NUM}(?:k([0-9]+))?\Z")
_A = re.compile(rf"a{_NUM}x{_NUM}r([0-9]+)(?:k([0-9]+))?\Z")
_M = re.compile(r"m([0-9]+)(?:a([0-9]+))?\Z")


# ------------------------------------------------------------------ PSF builders
def _side(K) -> int:
    k = int(K)
    if k != K or k < 1 or k % 2 == 0:
        raise ValueError(f"a PSF has an odd side K >= 1, got {K!r}")
    return k


def _normalised(h: np.ndarray) -> np.ndarray:
    s = h.sum()
    if not s > 0:
        raise ValueError("the PSF has no mass inside its grid")
    return h / s


def _cos_sin(deg) -> tuple:
    """cos and sin of whole degrees, exact at the multiples of 90 (so that a horizontal or vertical PSF has no stray mass)"""
    d = deg % 360
    exact = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}
    if d in exact:
        return exact[d]
    th = math.radians(d)
    return math.cos(th), math.sin(th)


def psf_gaussian(K: int, sigma: float) -> np.ndarray:
    """exp(-(x^2 + y^2) / (2 sigma^2)) on the centred K x K grid, values below eps * max zeroed, normalised: fspecial('gaussian')'s rule"""
    K = _side(K)
    if not sigma > 0:
        raise ValueError(f"psf_gaussian: sigma must be positive, got {sigma!r}")
    r = (K - 1) // 2
    y, x = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    h = np.exp(-(x * x + y * y) / (2.0 * float(sigma) ** 2))
    h[h < np.finfo(np.float64).eps * h.max()] = 0.0
    return _normalised(h)


def psf_gaussian_aniso(K: int, s1: float, s2: float, deg: float) -> np.ndarray:
    """exp(-(u^2 / s1^2 + v^2 / s2^2) / 2) with u = x cos t + y sin t, v = -x sin t + y cos t on the centred grid, normalised"""
    K = _side(K)
    if not (s1 > 0 and s2 > 0):
        raise ValueError(f"psf_gaussian_aniso: both widths must be positive, got {s1!r}, {s2!r}")
    r = (K - 1) // 2
    y, x = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    c, s = _cos_sin(deg)
    u, v = x * c + y * s, -x * s + y * c
    return _normalised(np.exp(-0.5 * (u * u / float(s1) ** 2 + v * v / float(s2) ** 2)))


def psf_motion(L: int, deg: float) -> np.ndarray:
    """linear motion of odd length L at ``deg`` degrees (counter-clockwise from the x axis; rows grow downwards): 8 L + 1 points t equally
    spaced on [-(L - 1) / 2, (L - 1) / 2], each at (x, y) = (c + t cos, c - t sin) with c = (L - 1) / 2, each splatting unit mass
    bilinearly onto its four neighbours (those outside the grid are dropped); normalised"""
    K = _side(L)
    c = (K - 1) / 2.0
    t = np.linspace(-c, c, 8 * K + 1)
    co, si = _cos_sin(deg)
    x, y = c + t * co, c - t * si
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    h = np.zeros((K, K), dtype=np.float64)
    for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
        ok = (yy >= 0) & (yy < K) & (xx >= 0) & (xx < K)
        np.add.at(h, (yy[ok], xx[ok]), w[ok])
    return _normalised(h)


def quantise_psf(h) -> np.ndarray:
    """float64 [K, K] (K odd, h >= 0, sum 1) -> int32 [K, K], no weight negative, sum 2^22: floor(h 2^22), the remainder as +1 to the
    taps with the largest fractional parts, ties to the lower row-major index"""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 2 or h.shape[0] != h.shape[1] or h.shape[0] % 2 == 0:
        raise ValueError(f"quantise_psf: expected an odd-sided square PSF, got the shape {h.shape}")
    if not np.isfinite(h).all() or (h < 0).any():
        raise ValueError("quantise_psf: a PSF has no negative and no non-finite entry")
    if abs(float(h.sum()) - 1.0) > 1e-9:
        raise ValueError(f"quantise_psf: a PSF sums to 1, this one to {float(h.sum())!r}")
    one = 1 << WEIGHT_BITS
    t = h.ravel() * float(one)
    q = np.floor(t).astype(np.int64)
    rest = one - int(q.sum())
    if not 0 <= rest <= q.size:
        raise ValueError(f"quantise_psf: the weights are {rest} short of 2^{WEIGHT_BITS} after rounding down")
    order = np.argsort(-(t - q), kind="stable")
    q[order[:rest]] += 1
    return check_psf_q(q.reshape(h.shape).astype(np.int32))


def check_psf_q(q) -> np.ndarray:
    """the weight contract of rcot_blur_u8, checked on the host: int32 [K, K], K odd in 1 .. 63, every weight >= 0, sum 2^22"""
    q = np.asarray(q)
    if q.dtype != np.int32 or q.ndim != 2 or q.shape[0] != q.shape[1] or q.shape[0] % 2 == 0 or q.shape[0] > KMAX:
        raise ValueError(f"PSF weights are int32 [K, K] with K odd in 1 .. {KMAX}, got {q.dtype} {q.shape}")
    if (q < 0).any() or int(q.sum(dtype=np.int64)) != 1 << WEIGHT_BITS:
        raise ValueError(f"PSF weights are >= 0 and sum to 2^{WEIGHT_BITS}; these sum to {int(q.sum(dtype=np.int64))}")
    return np.ascontiguousarray(q)


# ------------------------------------------------------------------ the spec grammar
def _odd_side(text, default: int, spec: str) -> int:
    K = default if text is None else int(text)
    if K % 2 == 0 or not 1 <= K <= KMAX:
        raise ValueError(f"PSF spec {spec!r}: K = {K} is not odd in 1 .. {KMAX}; {GRAMMAR}")
    return K


def _width(text, spec: str) -> float:
    s = float(text)
    if not 0 < s <= 10:
        raise ValueError(f"PSF spec {spec!r}: a width must be in (0, 10]; {GRAMMAR}")
    return s


def _angle(text, spec: str) -> int:
    d = int(text)
    if not 0 <= d <= 179:
        raise ValueError(f"PSF spec {spec!r}: the angle must be whole degrees in 0 .. 179; {GRAMMAR}")
    return d


def parse_psf(spec: str) -> tuple:
    """the spec grammar -> ("g", sigma, K) | ("a", s1, s2, deg, K) | ("m", L, deg or None); ValueError, one line that names the grammar,
    for anything else"""
    spec = str(spec)
    m = _G.match(spec)
    if m:
        s = _width(m.group(1), spec)
        return ("g", s, _odd_side(m.group(2), 2 * math.ceil(3 * s) + 1, spec))
    m = _A.match(spec)
    if m:
        s1, s2 = _width(m.group(1), spec), _width(m.group(2), spec)
        return ("a", s1, s2, _angle(m.group(3), spec), _odd_side(m.group(4), 2 * math.ceil(3 * max(s1, s2)) + 1, spec))
    m = _M.match(spec)
    if m:
        L = int(m.group(1))
        if L % 2 == 0 or not 3 <= L <= KMAX:
            raise ValueError(f"PSF spec {spec!r}: the length L = {L} is not odd in 3 .. {KMAX}; {GRAMMAR}")
        return ("m", L, None if m.group(2) is None else _angle(m.group(2), spec))
    raise ValueError(f"PSF spec {spec!r} is malformed: {GRAMMAR}")


def needs_angle(spec: str) -> bool:
    """a motion PSF without an angle: whoever uses it draws one"""
    p = parse_psf(spec)
    return p[0] == "m" and p[2] is None


def psf_of(spec: str, angle=None) -> np.ndarray:
    """the float64 PSF of a spec; ``angle`` (whole degrees) for a motion spec that names none"""
    p = parse_psf(spec)
    if p[0] == "g":
        return psf_gaussian(p[2], p[1])
    if p[0] == "a":
        return psf_gaussian_aniso(p[4], p[1], p[2], p[3])
    deg = p[2] if p[2] is not None else angle
    if deg is None:
        raise ValueError(f"PSF spec {spec!r} names no angle: pass one")
    return psf_motion(p[1], int(deg))


@functools.lru_cache(maxsize=4096)
def _psf_bytes(spec: str, angle) -> tuple:
    q = quantise_psf(psf_of(spec, angle))
    return q.shape[0], q.tobytes()


def psf_q_of(spec: str, angle=None) -> np.ndarray:
    """the int32 weights of a spec (made once per (spec, angle))"""
    K, raw = _psf_bytes(str(spec), None if angle is None else int(angle))
    return np.frombuffer(raw, dtype=np.int32).reshape(K, K)


def parse_de_type(name: str):
    """``blur_<spec>`` -> spec; None for a name of another task; ValueError for a malformed name"""
    if not name.startswith("blur"):
        return None
    if not name.startswith("blur_"):
        raise ValueError(f"--de_type {name}: the deblurring tasks are named blur_<spec>; {GRAMMAR}")
    try:
        parse_psf(name[5:])
    except ValueError as e:
        raise ValueError(f"--de_type {name}: {e}") from None
    return name[5:]


# ------------------------------------------------------------------ on the device
_DEVICE_PSFS = {}


def device_psf(psf_q, device) -> torch.Tensor:
    """the weights on ``device`` as int32 [K, K], checked against the contract and uploaded once per (device, PSF bytes).  Nothing is
    ever dropped: the tasks here use a few PSFs (``blur_m<L>`` at most 180, of 16 KB at the most); a caller that streams arbitrary PSFs
    through ``blur_degrade_u8`` grows this table without limit and should call ``backend.blur_u8`` with tensors of its own"""
    q = np.asarray(psf_q)
    key = (str(device), q.shape, q.dtype.str, q.tobytes())
    t = _DEVICE_PSFS.get(key)
    if t is None:
        t = _DEVICE_PSFS[key] = torch.from_numpy(check_psf_q(q).copy()).to(device)
    return t


def _backend(backend):
    if backend is None:
        from .ops import default_backend
        backend = default_backend()
    return backend


def check_border(border) -> int:
    if border not in BORDERS:
        raise ValueError(f"the border rule is one of {', '.join(BORDERS)}, got {border!r}")
    return BORDERS[border]


def blur_degrade_u8(img_u8: torch.Tensor, psf_q, border: str = "replicate", backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] on the device -> uint8 [H, W, 3]: every channel correlated with the int32 weights ``psf_q`` (``quantise_psf``)"""
    be = _backend(backend)
    return be.blur_u8(img_u8, device_psf(psf_q, be.device), check_border(border))


def bd_downscale_u8(hr_u8: torch.Tensor, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] with H, W multiples of 3 -> the LR image uint8 [H / 3, W / 3, 3] of the BD protocol: Gaussian 7 x 7, sigma 1.6,
    replicated border, the centre pixel of each 3 x 3 cell"""
    be = _backend(backend)
    H, W = hr_u8.shape[:2]
    s = BD_SCALE
    if H % s or W % s or H < s or W < s:
        raise ValueError(f"BD degradation: the image must be a positive multiple of {s} in both directions, got {H} x {W}")
    return be.blur_u8(hr_u8, device_psf(psf_q_of(BD_SPEC), be.device), BORDERS["replicate"], step=s, phase=s // 2)


def bd_degrade_u8(hr_u8: torch.Tensor, backend=None) -> torch.Tensor:
    """uint8 [H, W, 3] on the device, H and W multiples of 3 -> uint8 [H, W, 3]: ``bd_downscale_u8``, then the bicubic baseline
    ``resize.sr_upscale_u8`` of that LR image back to H x W"""
    from .resize import sr_upscale_u8
    be = _backend(backend)
    H, W = hr_u8.shape[:2]
    return sr_upscale_u8(bd_downscale_u8(hr_u8, be), H, W, be)


# ------------------------------------------------------------------ the folder CLI
def main(argv=None, backend=None):
    """``backend``: the backend to run on (default: the process's HIP backend; a GPU is required then)"""
    import argparse
    parser = argparse.ArgumentParser(description="blurred PNG folders for the deblurring tasks, or the BD degradation of super-resolution")
    parser.add_argument("--in", dest="src", required=True, type=str, help="folder of sharp images")
    parser.add_argument("--out", dest="dst", required=True, type=str, help="folder the PNGs are written to")
    parser.add_argument("--psf", default=None, type=str, help="the PSF spec (g1.6, g2k15, a4x1r30, m15a30); not read with --mode bd")
    parser.add_argument("--border", choices=sorted(BORDERS), default="replicate", help="the border rule of the blur")
    parser.add_argument("--mode", choices=["blur", "bd"], default="blur",
                        help="blur: the image blurred by --psf; bd: Gaussian 7 x 7 sigma 1.6, every third pixel, bicubic x3 back (the image "
                             "is cropped at the top left to a multiple of 3)")
    opt = parser.parse_args(argv)
    psf_q = None
    if opt.mode == "blur":
        if opt.psf is None:
            raise SystemExit("--mode blur needs --psf SPEC: " + GRAMMAR)
        try:
            if needs_angle(opt.psf):
                raise ValueError(f"PSF spec {opt.psf!r}: a folder is blurred with one fixed angle, m<L>a<deg>; {GRAMMAR}")
            psf_q = psf_q_of(opt.psf)
        except ValueError as e:
            raise SystemExit(str(e))
    if backend is None:
        if not torch.cuda.is_available():
            raise SystemExit("No GPU found: rcot_amd.blur runs the HIP path only")
        from .ops import default_backend
        backend = default_backend()
    return degrade_folder(opt.src, opt.dst, psf_q, opt.border, backend, opt.psf if psf_q is not None else None)


def degrade_folder(src: str, dst: str, psf_q, border: str, be, label=None) -> int:
    """every image file of ``src`` -> ``dst``/<name>.png blurred by ``psf_q``, or BD-degraded when ``psf_q`` is None; returns the number
    written"""
    from PIL import Image
    from .resize import modcrop
    os.makedirs(dst, exist_ok=True)
    done = 0
    for name in sorted(os.listdir(src)):
        path = os.path.join(src, name)
        if not os.path.isfile(path):
            continue
        img = np.array(Image.open(path).convert("RGB"))
        if psf_q is None:
            img = modcrop(img, BD_SCALE)
            if img.shape[0] < BD_SCALE or img.shape[1] < BD_SCALE:
                print(f"  skipped: {name} is smaller than {BD_SCALE} x {BD_SCALE}")
                continue
        d = torch.from_numpy(np.ascontiguousarray(img)).to(be.device)
        out = bd_degrade_u8(d, be) if psf_q is None else blur_degrade_u8(d, psf_q, border, be)
        Image.fromarray(out.cpu().numpy()).save(os.path.join(dst, os.path.splitext(name)[0] + ".png"))
        done += 1
    print(f"{'bd x3' if psf_q is None else f'blur {label} {border}'}: {done} image(s) written to {dst}")
    return done


if __name__ == "__main__":
    main()
