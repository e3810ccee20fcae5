"""Whole-image inference behind the CLI of the reference's testers (tester.py, tester_noise.py), on the HIP kernels.

    python -m rcot_amd.tester --model checkpoint/model_X__N_S.pth --degset dir/ --tarset dir/ --save OUT/ --savetar TAR/ --saveres RES/
                              [--noise_sigma 50] [--tile 512 --overlap 32] [--tile_window linear --tile_batch 0] [--ensemble 8]

Same walk as the reference (tester.py:56-113, tester_noise.py:65-115): sorted ``glob(degset + "*")`` / ``glob(tarset + "*")`` pairs,
RGB, [0, 1] floats, pairs of different shapes skipped; ``tester.py`` crops rows / columns from the END until H and W are multiples
of 4 (:77-84), ``tester_noise.py`` — chosen with ``--noise_sigma`` — drops the FIRST row and column when either is not (:84-86,
kept as is: an odd size stays unusable, and is skipped here with a message where the reference would fail inside the network) and
adds N(0, (sigma / 255)^2) noise to the degraded image (:93-101, numpy's global generator there; ``--seed`` here).  The network is what
the checkpoint holds: a pickled ``Net_Restormer.T_net`` object (the reference's and this package's Restormer checkpoints,
rcot_amd/compat.py) or the state_dict form of ``--backbone mprnet`` runs (``{"backbone": "mprnet"}`` -> ``MPRNetHip``).  Outputs: the
restored image, the target and the scaled residual (x2 resp. x3 with noise, :109 / :111) as PNGs under the three folders, then
PSNR / SSIM over the two folders as ``evaluate.calculate_evaluation_floder`` computes them (evaluate.py:43-106; cv2 and skimage are
not in this image, so both metrics are restated in numpy from their definitions: PSNR = skimage's for uint8 images, SSIM = the
script's own 2 x 2 box-window form).  FID (tester.py:115-118) needs a pretrained Inception network and is not computed.

Superset: ``--pad reflect|replicate`` restores the WHOLE image at any size: it is padded at the bottom and right to the network's size
multiple on the device, restored and cropped back (rcot_amd/wholeimage.py); neither crop above is applied, and a pair is skipped only for
a shape mismatch or when reflect cannot pad it.  ``--metrics device`` takes the three PNGs and both metrics from the egress kernel
(rcot_image_egress: same 8-bit values, same sums) instead of writing the folders and reading them back.

Superset: ``--tile T`` processes the image as overlapping T x T tiles (``--overlap`` pixels, averaged where tiles overlap) for sizes
one does not want to hold whole; the default is the reference's whole-image call.  Restormer takes H, W multiples of 8 (its three
PixelUnshuffle stages; the reference raises on other sizes), MPRNet multiples of 4.

Superset: ``--tile_window linear|cosine``, ``--tile_batch N`` and ``--ensemble 8`` run the tiles as *views* on the device
(rcot_amd/tiles.py; csrc/views.hip: rcot_view_gather, rcot_view_blend): the tiles are cut by one kernel, the network takes N of them per
call (0: all tiles of one shape; tiles of one size are a batch), and one kernel blends them with a separable window that ramps across
the overlap — the equal-weight average of ``--tile`` alone leaves a step at every overlap border, because neighbouring tiles disagree
there.  ``--ensemble 8`` is the geometric self-ensemble of restoration tables' "+" rows: the mean of aug^-1(T(aug(x))) over the 8
dihedral maps of the reference's data_augmentation, per tile, or of the whole image without ``--tile`` (two shapes of four views, one of
eight for a square image).  With none of the three given, ``--tile`` runs as before, bit for bit.

Superset: ``--ssim_window uniform7|gauss11`` and ``--color y`` report the figures of published tables instead of the reference's own
(rcot_amd/quality.py): uniform7 = skimage's default structural_similarity (the AirNet / PromptIR protocol, the reference's
util/val_utils.py:50-66), gauss11 = the 11 x 11, sigma 1.5 Gaussian window (basicsr, MATLAB-style scripts), y = PSNR and SSIM on the
BT.601 luma (deraining tables).  ``--metrics folders`` computes them on the host from the PNGs read back, ``--metrics device`` with
rcot_image_quality on the 8-bit images already on the device.  A line naming the protocol is printed before the report.  The defaults
(box2, rgb) print what the reference prints.

Superset: ``--sr_scale S`` evaluates super-resolution (the reference's README: "the LR images undergo bicubic rescaling to match the
dimensions of their respective high-resolution counterparts"): the network's input is the bicubic degradation made on the device
(rcot_amd/resize.py; MATLAB's imresize rule, csrc/resize.hip).  ``--sr_from target`` (default) makes it from the target — cropped at the
top left to a multiple of S, shrunk, quantised to 8 bits, enlarged, quantised; ``--degset`` is not read.  ``--sr_from lr`` reads the
h x w LR images from ``--degset``, enlarges them by S and crops the target at the top left to hS x wS (targets smaller than that, or
larger by S or more in either direction, are skipped with a message).  ``--savedeg DIR`` writes the 8-bit network input — the bicubic
baseline every SR table starts with.  The padding, tiling, ensemble and metrics flags combine with these as before (``--color y
--ssim_window gauss11`` is the protocol of SR tables); ``--sr_scale 0`` leaves everything as it was.

Superset: ``--jpeg_q Q`` evaluates compression-artifact reduction (the CAR rows of restoration tables, Q = 10 / 20 / 30 / 40): the
network's input is the whole target after a baseline JPEG round trip at quality Q made on the device (rcot_amd/jpeg.py,
csrc/jpeg.hip: byte for byte what Pillow on libjpeg-turbo holds after saving and loading it; ``--jpeg_subsampling 420|444``, default
420 as PIL's); ``--degset`` is not read.  ``--savedeg DIR`` writes that input, the "JPEG" baseline row.  The padding, tiling, ensemble
and metrics flags combine with it as before; it is refused together with ``--sr_scale`` or ``--noise_sigma``; ``--jpeg_q 0`` (the
default) leaves everything as it was.

Superset: ``--blur SPEC`` evaluates deblurring from sharp images alone: the network's input is the whole target blurred on the device by
the PSF of the spec (rcot_amd/blur.py's grammar: g1.6, g2k15, a4x1r30, m15a30; csrc/blur.hip) under ``--blur_border
replicate|mirror|wrap``; ``--degset`` is not read.  ``--savedeg DIR`` writes that input, the "blurred" baseline row.  It is refused
together with ``--sr_scale``, ``--jpeg_q`` or ``--noise_sigma``.  ``--sr_degradation bd`` (with ``--sr_scale 3 --sr_from target`` only)
replaces the bicubic shrink of the SR input by the BD protocol — Gaussian 7 x 7, sigma 1.6, every third pixel — before the same bicubic
enlargement; the default ``bicubic`` is the path above.  With neither flag everything runs as before.

Superset: ``--chain SPEC`` evaluates a degradation chain (rcot_amd/chain.py's grammar, with or without the ``chain_`` prefix:
blur_g1.6+noise_g10+jpeg_q40): the network's input is the whole target — cropped at the top left to a multiple of the scale of an
``sr_x<k>`` stage — after the stages, made on the device under ``--blur_border`` and ``--jpeg_subsampling``; ``--degset`` is not read.
The noise seed and the drawn values of a file (ranged parameters, motion angles) come from ``random.Random`` seeded by ``--seed`` and the
file's index in the sorted ``--tarset`` listing (``chain.file_draws``), so a table row is reproducible and ``--savedeg DIR`` writes the
bytes ``python -m rcot_amd.chain`` writes for the same seed (after the degradation ``--pad none`` still crops both images to a multiple
of 4, as for every task; the folder tool does not).  It is refused together with ``--sr_scale``, ``--jpeg_q``, ``--blur`` or
``--noise_sigma``.

Superset: ``--psnrb`` also reports PSNR-B (Yim & Bovik 2011, basicsr's ``calculate_psnrb``; rcot_amd/quality.py), the figure the CAR rows
of restoration tables carry next to PSNR and SSIM: one more line after the SSIM line, in the colour space of ``--color``, from the PNGs
with ``--metrics folders`` and from rcot_image_blockiness on the 8-bit images already on the device with ``--metrics device``.
``--shave N`` crops N pixels from every side of both 8-bit images before PSNR, SSIM and PSNR-B, as SR tables do with N = the scale (the
PNGs stay full size; PSNR-B keeps the codec's block grid, origin N mod 8; an image with nothing left is skipped with a message).  With
``--metrics device`` the crop is rcot_crop_u8 and needs ``--ssim_window uniform7|gauss11``: the egress kernel's own sums cannot be cropped.
SR tables: ``--shave <scale> --color y --ssim_window gauss11``; CAR tables: ``--psnrb --color y``.  With neither flag everything runs as
before.

Superset: ``--weights ema`` restores with the averaged weights that ``rcot_amd.trainer --ema`` saves under "Tnet_ema" (either backbone); it
exits with a message naming the key when the checkpoint has none.  The default ``raw`` reads "Tnet" as before.
"""
from __future__ import annotations

import argparse
import glob
import math
import os

import numpy as np
import torch

parser = argparse.ArgumentParser(description="RCOT evaluation on MI355X (tester.py / tester_noise.py flags)")
parser.add_argument("--cuda", action="store_true", help="accepted for CLI compatibility (the HIP path always runs on the GPU)")
parser.add_argument("--model", default="./checkpoint/model_Dehazing__99_10.0.pth", type=str, help="model path")
parser.add_argument("--degset", default="./datasets/Dehazing/outdoor/hazy/", type=str, help="degraded data")
parser.add_argument("--tarset", default="./datasets/Dehazing/outdoor/gt/", type=str, help="target data")
parser.add_argument("--saveres", default="./results/Dehazing/RES/", type=str, help="savepath, Default: residual")
parser.add_argument("--save", default="./results/Dehazing/OUT/", type=str, help="savepath, Default: results")
parser.add_argument("--savetar", default="./results/Dehazing/TAR/", type=str, help="savepath, Default: targets")
parser.add_argument("--gpus", default="0", type=str, help="gpu ids (accepted, ignored: one process, current device)")
parser.add_argument("--noise_sigma", type=float, default=None, help="tester_noise.py: add N(0, sigma^2) (8-bit scale) to the degraded image")
parser.add_argument("--seed", type=int, default=0, help="seed of the added noise")
parser.add_argument("--tile", type=int, default=0, help="superset: tile size (0 = whole image, the reference's behaviour)")
parser.add_argument("--overlap", type=int, default=32, help="superset: tile overlap in pixels")
parser.add_argument("--tile_window", choices=["uniform", "linear", "cosine"], default="uniform",
                    help="superset: weights of a tile where tiles overlap: uniform = equal (the plain average); linear / cosine = a ramp "
                         "across the overlap (no step at the overlap borders)")
parser.add_argument("--tile_batch", type=int, default=1, help="superset: tiles per network call (0 = all tiles of one shape)")
parser.add_argument("--ensemble", type=int, choices=[1, 8], default=1,
                    help="superset: 8 = geometric self-ensemble, the mean over the 8 dihedral views (per tile, or of the whole image)")
parser.add_argument("--pad", choices=["none", "reflect", "replicate"], default="none",
                    help="superset: pad bottom / right to the network's size multiple, restore the whole image, crop back (none = the "
                         "reference's crops and skips)")
parser.add_argument("--metrics", choices=["folders", "device"], default="folders",
                    help="superset: folders = PSNR / SSIM read back from the written PNGs (the reference's way); device = PNGs and metrics "
                         "from the egress kernel's 8-bit outputs and sums")
parser.add_argument("--ssim_window", choices=["box2", "uniform7", "gauss11"], default="box2",
                    help="superset: box2 = the reference's 2 x 2 window (evaluate.py); uniform7 = skimage's default SSIM (AirNet / PromptIR "
                         "tables); gauss11 = the 11 x 11, sigma 1.5 Gaussian window (basicsr / MATLAB-style)")
parser.add_argument("--color", choices=["rgb", "y"], default="rgb",
                    help="superset: y = PSNR / SSIM on the BT.601 luma of YCbCr (deraining tables) instead of the three RGB planes")
parser.add_argument("--sr_scale", type=int, default=0,
                    help="superset: super-resolution by this integer factor: the network's input is the bicubic degradation made on the "
                         "device (rcot_amd/resize.py); 0 = off, everything as before")
parser.add_argument("--sr_from", choices=["target", "lr"], default="target",
                    help="superset, with --sr_scale S: target = degrade the target (cropped at the top left to a multiple of S; --degset is "
                         "not read); lr = --degset holds the h x w low-resolution images, enlarged by S, the target is cropped to hS x wS")
parser.add_argument("--jpeg_q", type=int, default=0,
                    help="superset: compression-artifact reduction: the network's input is the target after a baseline JPEG round trip at "
                         "this quality (1 .. 100) made on the device (rcot_amd/jpeg.py; --degset is not read); 0 = off, everything as before")
parser.add_argument("--jpeg_subsampling", choices=["420", "444"], default="420",
                    help="superset, with --jpeg_q: chroma subsampling of the round trip (420 = PIL's default)")
parser.add_argument("--blur", default=None, type=str,
                    help="superset: deblurring: the network's input is the target blurred on the device by this PSF spec (rcot_amd/blur.py: "
                         "g1.6, g2k15, a4x1r30, m15a30; --degset is not read); off by default, everything as before")
parser.add_argument("--blur_border", choices=["replicate", "mirror", "wrap"], default="replicate",
                    help="superset, with --blur: the border rule of the blur")
parser.add_argument("--sr_degradation", choices=["bicubic", "bd"], default="bicubic",
                    help="superset, with --sr_scale 3 --sr_from target: bd = Gaussian 7 x 7 sigma 1.6 and every third pixel instead of the "
                         "bicubic shrink (the BD rows of SR tables); bicubic = the path as before")
parser.add_argument("--chain", default=None, type=str,
                    help="superset: a degradation chain: the network's input is the target after these stages made on the device "
                         "(rcot_amd/chain.py: blur_g1.6+noise_g10+jpeg_q40; --degset is not read; --seed seeds the per-file values); off by "
                         "default, everything as before")
parser.add_argument("--weights", choices=["raw", "ema"], default="raw",
                    help="superset: ema = the averaged weights of a checkpoint written with rcot_amd.trainer --ema (its \"Tnet_ema\" key); "
                         "raw = \"Tnet\", everything as before")
parser.add_argument("--psnrb", action="store_true",
                    help="superset: also report PSNR-B (PSNR with the blocking-effect factor of Yim & Bovik 2011; the CAR rows of "
                         "restoration tables) in the colour space of --color")
parser.add_argument("--shave", type=int, default=0,
                    help="superset: crop this many pixels from every side of both 8-bit images before PSNR, SSIM and PSNR-B (SR tables: "
                         "the scale); the written PNGs stay full size; 0 = off, everything as before")
parser.add_argument("--savedeg", default=None, type=str, help="superset: also write the 8-bit network input (with --sr_scale: the bicubic "
                                                             "baseline) as PNGs under this folder")


# ------------------------------------------------------------------------------- metrics (evaluate.py)
def psnr_uint8(im1: np.ndarray, im2: np.ndarray) -> float:
    """skimage.metrics.peak_signal_noise_ratio for uint8 images (data range 255), as evaluate.py:84 calls it"""
    err = float(np.mean((im1.astype(np.float64) - im2.astype(np.float64)) ** 2))
    return float("inf") if err == 0.0 else 10.0 * math.log10(255.0 * 255.0 / err)


def _box2(a: np.ndarray) -> np.ndarray:
    """cv2.filter2D with the 2 x 2 window of cv2.getGaussianKernel(2, 1) (both taps 0.5; anchor at the window centre (1, 1): the taps
    sit at offsets -1 and 0), cropped [5:-5] as evaluate.py:54-60 does — the border handling never reaches the crop"""
    s = 0.25 * (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:])          # s[y-1, x-1] = window ending at (y, x), y, x >= 1
    return s[4:-5, 4:-5]


def ssim_plane(img1: np.ndarray, img2: np.ndarray) -> float:
    """evaluate.ssim (:43-63) for one 2-D plane in [0, 255]"""
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    mu1, mu2 = _box2(a), _box2(b)
    s1, s2, s12 = _box2(a * a) - mu1 * mu1, _box2(b * b) - mu2 * mu2, _box2(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(m.mean())


def ssim_image(im1: np.ndarray, im2: np.ndarray) -> float:
    """``ssim(im1, im2)`` as evaluate.py:86 calls its own function on H x W x 3 arrays: filter2D works per channel, the mean runs
    over everything"""
    return float(np.mean([ssim_plane(im1[:, :, c], im2[:, :, c]) for c in range(im1.shape[2])]))


def _standard(opt) -> bool:
    """a protocol other than the reference's own was asked for"""
    return opt.ssim_window != "box2" or opt.color != "rgb"


def _nothing_left(h: int, w: int, shave: int) -> bool:
    """``--shave``: an h x w image that the crop would empty is skipped, with this one line"""
    if h > 2 * shave and w > 2 * shave:
        return False
    print(f"  skipped: {h} x {w} leaves nothing after --shave {shave}")
    return True


def evaluate_folders(path1: str, path2: str, ssim_window: str = "box2", color: str = "rgb", psnrb: bool = False, shave: int = 0):
    """evaluate.calculate_evaluation_floder (:65-106): mean / best / worst PSNR and SSIM over the sorted file pairs; with another
    ``ssim_window`` / ``color`` the protocols of rcot_amd/quality.py.  ``path1`` holds the targets, ``path2`` the restored images.
    ``shave``: that many pixels come off every side of both images first (a pair with nothing left is skipped with a message and does
    not count).  ``psnrb``: three more values follow the six, mean / best / worst PSNR-B of the restored images on the planes of
    ``color``, with the block-grid origin ``shave % 8``."""
    from PIL import Image
    if (ssim_window, color) == ("box2", "rgb"):
        psnr, ssim = psnr_uint8, ssim_image
    else:
        from . import quality as Q
        psnr, ssim = (lambda x, y: Q.psnr_u8(x, y, color)), (lambda x, y: Q.ssim_windowed(x, y, ssim_window, color))
    a, b = sorted(os.listdir(path1)), sorted(os.listdir(path2))
    ps, ss, pb, skipped = [], [], [], 0
    for n1, n2 in zip(a, b):
        i1 = np.array(Image.open(os.path.join(path1, n1)).convert("RGB"))
        i2 = np.array(Image.open(os.path.join(path2, n2)).convert("RGB"))
        if shave:
            if _nothing_left(i1.shape[0], i1.shape[1], shave) or _nothing_left(i2.shape[0], i2.shape[1], shave):
                skipped += 1
                continue
            from .quality import shave_u8
            i1, i2 = shave_u8(i1, shave), shave_u8(i2, shave)
        ps.append(psnr(i1, i2))
        ss.append(ssim(i1, i2))
        if psnrb:
            from .quality import psnrb_u8
            pb.append(psnrb_u8(i2, i1, color, shave % 8, shave % 8))
    if not ps:
        nan = float("nan")
        return (nan,) * (9 if psnrb else 6)
    n = len(b) - skipped
    six = sum(ps) / n, sum(ss) / n, max(ps), max(ss), min(ps), min(ss)
    return six + (sum(pb) / n, max(pb), min(pb)) if psnrb else six


# ------------------------------------------------------------------------------- the network of a checkpoint
def load_network(path: str, weights: str = "raw"):
    """-> (callable network on the GPU, multiple its input sizes must have).  ``weights`` "ema": the averaged weights a run with
    ``rcot_amd.trainer --ema`` saved under "Tnet_ema" (a plain state_dict, either backbone) instead of "Tnet"."""
    from .compat import load_checkpoint
    ck = load_checkpoint(path)
    if weights == "ema":
        if not isinstance(ck, dict) or "Tnet_ema" not in ck:
            raise SystemExit(f"--weights ema: {path} has no \"Tnet_ema\" key (it was not written by rcot_amd.trainer --ema); "
                             f"--weights raw reads \"Tnet\"")
        ck = dict(ck, Tnet=dict(ck["Tnet_ema"]))
    if isinstance(ck, dict) and ck.get("backbone") == "mprnet":
        from .mprnet_hip import MPRNetHip
        net = MPRNetHip(seed=0)
        net.load_state_dict(ck["Tnet"])
        return net, 4
    tn = ck["Tnet"]
    if isinstance(tn, dict):                                          # a plain state_dict
        from .compat import shim
        tn = shim().T_net.from_state_dict(tn, decoder=True)
    return tn, 8


def restore(net, x: torch.Tensor, tile: int = 0, overlap: int = 32, mult: int = 8, pad=None, window: str = "uniform", tile_batch: int = 1,
            ensemble: int = 1) -> torch.Tensor:
    """``net(x)`` whole (tile 0), or as overlapping tiles averaged where they overlap.  ``pad`` ("reflect" | "replicate"): any H, W —
    padded to multiples of ``mult`` first, cropped back after (rcot_amd/wholeimage.py).  ``window`` ("linear" | "cosine": a ramp across
    the overlap), ``tile_batch`` (tiles per network call, 0 = all of one shape) or ``ensemble`` (8: the mean over the 8 dihedral views)
    other than their defaults: the same tiles as views on the device (rcot_amd/tiles.py)"""
    _, _, H, W = x.shape
    if pad not in (None, "none"):
        from .wholeimage import restore_any_size
        return restore_any_size(net, x, mult, pad, tile, overlap, window, tile_batch, ensemble).out[:, :, :H, :W].contiguous()
    if (window, tile_batch, ensemble) != ("uniform", 1, 1):
        from .tiles import plan, restore_views
        return restore_views(net, x, plan(H, W, tile, overlap, mult, ensemble), window, tile_batch)
    if not tile or (tile >= H and tile >= W):
        return net(x)
    tile = max(mult, tile // mult * mult)
    step = max(mult, (tile - overlap) // mult * mult)
    acc, cnt = torch.zeros_like(x), torch.zeros(1, 1, H, W, device=x.device)
    ys = sorted({min(y, max(H - tile, 0)) for y in range(0, H, step)})
    xs = sorted({min(c, max(W - tile, 0)) for c in range(0, W, step)})
    for y0 in ys:
        for x0 in xs:
            y1, x1 = min(y0 + tile, H), min(x0 + tile, W)
            acc[:, :, y0:y1, x0:x1] += net(x[:, :, y0:y1, x0:x1].contiguous())
            cnt[:, :, y0:y1, x0:x1] += 1
    return acc / cnt


def _report(psnr, ssim, pmax, smax, pmin, smin, done, ssim_window="box2", color="rgb", psnrb=None, shave=0):
    """``psnrb``: None, or (mean, best, worst) of ``--psnrb``"""
    if (ssim_window, color) != ("box2", "rgb"):
        print(f"metrics: ssim {ssim_window}, color {color}" + (", psnrb" if psnrb is not None else "") + (f", shave {shave}" if shave else ""))
    print("FID value: not computed (needs a pretrained Inception network; tester.py:115-118)")
    print("PSNR: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(psnr, pmax, pmin))
    print("SSIM: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(ssim, smax, smin))
    r = dict(images=done, psnr=psnr, ssim=ssim, psnr_best=pmax, psnr_worst=pmin, ssim_best=smax, ssim_worst=smin,
             ssim_window=ssim_window, color=color)
    if psnrb is not None:
        print("PSNR-B: Averyge {:.5f},   best {:.5f},   worst {:.5f}".format(*psnrb))
        r.update(psnrb=psnrb[0], psnrb_best=psnrb[1], psnrb_worst=psnrb[2])
    return r


def _report_folders(opt, done):
    """the report of ``--metrics folders``: the PNGs read back"""
    v = evaluate_folders(opt.savetar, opt.save, opt.ssim_window, opt.color, opt.psnrb, opt.shave)
    return _report(*v[:6], done, opt.ssim_window, opt.color, v[6:] if opt.psnrb else None, opt.shave)


def _target_task(opt):
    """the whole-image task (a sample's fields, rcot_amd/degrade.py) that makes the network's input from the target — ``--chain``,
    ``--sr_scale S --sr_from target`` (bicubic, or ``--sr_degradation bd``), ``--jpeg_q`` or ``--blur``, which main() lets through one
    at a time — or None"""
    from .degrade import BY_FIELD, blur_border, jpeg_subsampling
    if opt.chain is not None:
        from .chain import parse_spec
        return BY_FIELD["chain"].fields(parse_spec(opt.chain), blur_border(opt), jpeg_subsampling(opt))
    if opt.sr_scale > 0 and opt.sr_from == "target":
        return BY_FIELD["bd"].fields(True) if opt.sr_degradation == "bd" else BY_FIELD["sr"].fields(opt.sr_scale)
    if opt.jpeg_q > 0:
        return BY_FIELD["jpeg"].fields(opt.jpeg_q, jpeg_subsampling(opt))
    if opt.blur is not None:
        return BY_FIELD["blur"].fields(opt.blur, blur_border(opt))
    return None


def _sr_from_lr(deg: np.ndarray, tar: np.ndarray, S: int, be):
    """``--sr_scale S --sr_from lr``: (network input, target) as uint8 [H, W, 3] arrays of one size, or None (with a message) for a
    pair that is skipped.  ``deg`` is the h x w LR image: it is enlarged to hS x wS, and the target is cropped to that at the top left
    — it may be larger by less than S in either direction (what the crop to a multiple of S removed when the LR image was made)"""
    from .resize import sr_upscale_u8
    H, W = deg.shape[0] * S, deg.shape[1] * S
    if tar.shape[0] < H or tar.shape[1] < W or tar.shape[0] - H >= S or tar.shape[1] - W >= S:
        print(f"  skipped: LR {deg.shape[0]} x {deg.shape[1]} times {S} is {H} x {W}, the target is {tar.shape[0]} x {tar.shape[1]}")
        return None
    lr = torch.from_numpy(np.ascontiguousarray(deg)).to(be.device)
    return sr_upscale_u8(lr, H, W, be).cpu().numpy(), np.ascontiguousarray(tar[:H, :W])


def _main_any_size(opt, net):
    """``--pad`` other than none and / or ``--metrics device``: ingest (or pad2d for the noisy float input), the network on the padded
    image, and the egress kernel for the crop, the three 8-bit images and the statistics.  The size multiple is the network's own."""
    from PIL import Image
    from .chain import file_draws
    from .degrade import degrade_file_u8
    from .wholeimage import image_metrics, pad_geometry, restore_any_size
    be, mult = net.be, net.size_multiple
    padded = opt.pad != "none"
    device_metrics = opt.metrics == "device"
    standard = _standard(opt)                                         # rcot_image_quality instead of the egress kernel's own sums
    proto = (opt.ssim_window, opt.color)
    tar_list = sorted(glob.glob(opt.tarset + "*"))
    task = _target_task(opt)                                          # the input is made from the target: --degset is not read
    deg_list = tar_list if task is not None else sorted(glob.glob(opt.degset + "*"))
    rng = np.random.default_rng(opt.seed)
    noisy = opt.noise_sigma is not None
    N, og = opt.shave, opt.shave % 8                                  # the shave and the block-grid origin it leaves
    sizes, stats, bstats = [], [], []
    for index, (deg_name, tar_name) in enumerate(zip(deg_list, tar_list)):
        name = os.path.basename(tar_name)
        print("Processing ", deg_name)
        deg, tar = np.array(Image.open(deg_name).convert("RGB")), np.array(Image.open(tar_name).convert("RGB"))
        if task is not None:                                          # (a chain's per-file values: the rule of its folder tool)
            drawn = file_draws(task["chain"][0], opt.seed, index) if "chain" in task else None
            # the wording of a skip is each flag's own: --chain speaks as its folder tool does (the size after the crop, no noun), the
            # other three name the "target" at the size it was read
            pair = degrade_file_u8(tar, task, drawn, be, "" if "chain" in task else "target")
            if pair is None:
                continue
            tar, deg = pair
        elif opt.sr_scale > 0:
            pair = _sr_from_lr(deg, tar, opt.sr_scale, be)
            if pair is None:
                continue
            deg, tar = pair
        if deg.shape != tar.shape:
            print(f"  skipped: degraded {deg.shape[0]} x {deg.shape[1]} and target {tar.shape[0]} x {tar.shape[1]} differ")
            continue
        h, w = deg.shape[:2]
        if not padded:                                                # the reference's crops (tester.py:77-84, tester_noise.py:84-86)
            if noisy:
                if (h % 4) or (w % 4):
                    deg, tar = deg[1:h, 1:w], tar[1:h, 1:w]
            else:
                deg, tar = deg[:h - h % 4, :w - w % 4], tar[:h - h % 4, :w - w % 4]
            h, w = deg.shape[:2]
        try:
            pad_geometry(h, w, mult, opt.pad)
        except ValueError as e:
            print(f"  skipped: {e}")
            continue
        if N and _nothing_left(h, w, N):
            continue
        tar_d = torch.from_numpy(np.ascontiguousarray(tar)).to(be.device)
        if opt.savedeg:
            Image.fromarray(np.ascontiguousarray(deg)).save(os.path.join(opt.savedeg, name))
        if noisy:                                                     # the noise is drawn on the host (numpy's generator, as the reference)
            x = torch.from_numpy(np.ascontiguousarray(deg.transpose(2, 0, 1))).float().div(255).unsqueeze(0)
            x = x + torch.from_numpy(rng.normal(size=tar.transpose(2, 0, 1).shape) * opt.noise_sigma / 255.0).float()
        else:
            x = torch.from_numpy(np.ascontiguousarray(deg))
        r = restore_any_size(net, x, mult, opt.pad, opt.tile, opt.overlap, opt.tile_window, opt.tile_batch, opt.ensemble)
        out_u8, res_u8, st = be.image_egress(r.out, h, w, degraded=r.x, target=tar_d, res_scale=3.0 if noisy else 2.0, want_out=True,
                                             want_res=True, want_stats=device_metrics and not standard)
        tar_m, out_m = tar_d, out_u8                                  # the pair the metrics see: shaved on the device
        if device_metrics and N:
            tar_m, out_m = be.crop_u8(tar_d, N, N, h - 2 * N, w - 2 * N), be.crop_u8(out_u8, N, N, h - 2 * N, w - 2 * N)
        if device_metrics and standard:
            st = be.image_quality(tar_m, out_m, opt.ssim_window, opt.color)
        if device_metrics and opt.psnrb:
            bstats.append(be.image_blockiness(out_m, tar_m, opt.color, og, og))
        Image.fromarray(res_u8.cpu().numpy()).save(os.path.join(opt.saveres, name))
        Image.fromarray(out_u8.cpu().numpy()).save(os.path.join(opt.save, name))
        Image.fromarray(np.ascontiguousarray(tar)).save(os.path.join(opt.savetar, name))
        sizes.append((h, w))
        stats.append(st)
    if not device_metrics:
        return _report_folders(opt, len(sizes))
    if not sizes:
        nan = float("nan")
        return _report(nan, nan, nan, nan, nan, nan, 0, *proto, (nan, nan, nan) if opt.psnrb else None, N)
    pb = None
    if opt.psnrb:                                                     # the five integers per plane ride behind the four numbers, as bits
        from .quality import psnrb_from_sums
        both = torch.stack([torch.cat([s, b.view(torch.float64).flatten()]) for s, b in zip(stats, bstats)]).cpu().numpy()
        host, ints = both[:, :4].tolist(), np.ascontiguousarray(both[:, 4:]).view(np.int64).reshape(len(sizes), -1, 5)
        v = [psnrb_from_sums(i, h - 2 * N, w - 2 * N, og, og) for i, (h, w) in zip(ints, sizes)]
        pb = (sum(v) / len(v), max(v), min(v))
    else:
        host = torch.stack(stats).cpu().tolist()                      # four numbers per image, read once
    if standard:
        from .quality import quality_metrics
        m = [quality_metrics(s) for s in host]
        ps, ss = [v["psnr"] for v in m], [v["ssim"] for v in m]
    else:
        m = [image_metrics(s, h, w) for s, (h, w) in zip(host, sizes)]
        ps, ss = [v["psnr_u8"] for v in m], [v["ssim"] for v in m]
    return _report(sum(ps) / len(ps), sum(ss) / len(ss), max(ps), max(ss), min(ps), min(ss), len(sizes), *proto, pb, N)


def main(argv=None):
    from PIL import Image
    from .trainer import save_image
    opt = parser.parse_args(argv)
    if opt.ssim_window == "box2" and opt.color == "y" and opt.metrics == "device":
        raise SystemExit("--ssim_window box2 with --color y (the reference's 2 x 2 map on the luma plane) is computed on the host only: "
                         "use --metrics folders, or --ssim_window uniform7 | gauss11")
    if opt.shave < 0:
        raise SystemExit(f"--shave {opt.shave}: the number of pixels cropped from every side must be an integer >= 0 (0 = off)")
    if opt.shave > 0 and opt.metrics == "device" and opt.ssim_window == "box2":
        raise SystemExit("--shave with --metrics device crops the 8-bit images for rcot_image_quality; --ssim_window box2 comes from the "
                         "egress kernel's own sums, which cannot be cropped: use --ssim_window uniform7 | gauss11, or --metrics folders")
    if opt.jpeg_q < 0 or opt.jpeg_q > 100:
        raise SystemExit(f"--jpeg_q {opt.jpeg_q}: the quality must be in 1 .. 100 (0 = off)")
    if opt.jpeg_q > 0 and (opt.sr_scale > 0 or opt.noise_sigma is not None):
        raise SystemExit("--jpeg_q makes the network's input from the target: it cannot be combined with --sr_scale or --noise_sigma")
    if opt.blur is not None:
        from .blur import GRAMMAR, needs_angle, parse_psf
        if opt.sr_scale > 0 or opt.jpeg_q > 0 or opt.noise_sigma is not None:
            raise SystemExit("--blur makes the network's input from the target: it cannot be combined with --sr_scale, --jpeg_q or "
                             "--noise_sigma")
        try:
            parse_psf(opt.blur)
            if needs_angle(opt.blur):
                raise ValueError(f"PSF spec {opt.blur!r}: an evaluation blurs with one fixed angle, m<L>a<deg>; {GRAMMAR}")
        except ValueError as e:
            raise SystemExit(f"--blur: {e}")
    if opt.chain is not None:
        if opt.sr_scale > 0 or opt.jpeg_q > 0 or opt.blur is not None or opt.noise_sigma is not None:
            raise SystemExit("--chain makes the network's input from the target: it cannot be combined with --sr_scale, --jpeg_q, --blur "
                             "or --noise_sigma")
        from .chain import parse_spec
        parse_spec(opt.chain)                                         # a malformed chain is refused here, naming the stage
    if opt.sr_degradation == "bd" and (opt.sr_scale != 3 or opt.sr_from != "target"):
        raise SystemExit("--sr_degradation bd is the BD protocol of scale 3 made from the target: it needs --sr_scale 3 --sr_from target")
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: rcot_amd.tester runs the HIP path only")
    if opt.sr_scale < 0 or opt.sr_scale == 1:
        raise SystemExit(f"--sr_scale {opt.sr_scale}: the scale factor must be an integer >= 2 (0 = off)")
    for d in (opt.save, opt.savetar, opt.saveres) + ((opt.savedeg,) if opt.savedeg else ()):
        os.makedirs(d, exist_ok=True)
    net, mult = load_network(opt.model, opt.weights)
    if opt.pad != "none" or opt.metrics == "device" or opt.sr_scale > 0 or opt.jpeg_q > 0 or opt.blur is not None or opt.chain is not None:
        return _main_any_size(opt, net)
    deg_list, tar_list = sorted(glob.glob(opt.degset + "*")), sorted(glob.glob(opt.tarset + "*"))
    rng = np.random.default_rng(opt.seed)
    noisy = opt.noise_sigma is not None
    done = 0
    for deg_name, tar_name in zip(deg_list, tar_list):
        name = os.path.basename(tar_name)
        print("Processing ", deg_name)
        deg, tar = np.array(Image.open(deg_name).convert("RGB")), np.array(Image.open(tar_name).convert("RGB"))
        shape1, shape2 = deg.shape, tar.shape
        h, w = deg.shape[:2]
        if noisy:
            if (h % 4) or (w % 4):                                    # tester_noise.py:84-86
                deg, tar = deg[1:h, 1:w], tar[1:h, 1:w]
        else:
            deg, tar = deg[:h - h % 4, :w - w % 4], tar[:h - h % 4, :w - w % 4]      # tester.py:77-84
        if shape1 != shape2:
            continue
        h, w = deg.shape[:2]
        if h % mult or w % mult or h == 0 or w == 0:
            print(f"  skipped: {h} x {w} is not a multiple of {mult} (the network's resampling levels)")
            continue
        if opt.shave and _nothing_left(h, w, opt.shave):
            continue
        x = torch.from_numpy(np.ascontiguousarray(deg.transpose(2, 0, 1))).float().div(255).unsqueeze(0)
        if noisy:
            x = x + torch.from_numpy(rng.normal(size=tar.transpose(2, 0, 1).shape) * opt.noise_sigma / 255.0).float()
        gt = torch.from_numpy(np.ascontiguousarray(tar.transpose(2, 0, 1))).float().div(255).unsqueeze(0)
        if opt.savedeg:
            Image.fromarray(np.ascontiguousarray(deg)).save(os.path.join(opt.savedeg, name))
        xd = x.cuda()
        out = restore(net, xd, opt.tile, opt.overlap, mult, None, opt.tile_window, opt.tile_batch, opt.ensemble)
        res = (xd - out).cpu()
        save_image(res * (3 if noisy else 2), os.path.join(opt.saveres, name))
        save_image(out.cpu(), os.path.join(opt.save, name))
        save_image(gt, os.path.join(opt.savetar, name))
        done += 1
    return _report_folders(opt, done)


if __name__ == "__main__":
    main()
