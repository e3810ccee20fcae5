"""The validation suite: any number of named validation sets, each a folder of targets and a task that says where the degraded twin
comes from, resident on the device as 8-bit images and measured there — the trainer's ``--val_set`` / ``--val_batch`` /
``--val_cache_gb`` / ``--save_best``, and ``python -m rcot_amd.valsuite`` for a checkpoint.

    --val_set NAME TASK TARSET [DEGSET] [key=value ...]          (any number of times)

    TASK    paired              DEGSET is read; pairs whose shapes differ are skipped with a line, as the single-folder validation does
            denoise_<sigma>     the target with white Gaussian noise of sigma (8-bit units) added and clipped to 8 bits: the chain
                                ``noise_g<sigma>`` (rcot_noise_u8) — the rule the training patches see, not the float noise of
                                ``rcot_amd.tester --noise_sigma``
            sr_x2|3|4, sr_bd_x3, jpeg_q<Q>, blur_<spec>, chain_<...>     any whole-image task of rcot_amd/degrade.py, made from the target
                                (DEGSET is refused; a motion blur needs its angle: one fixed PSF per set)
    keys    color=rgb|y  ssim=box2|uniform7|gauss11  shave=N  psnrb  seed=S  border=replicate|mirror|wrap  subsampling=420|444

The per-file values of a made set (noise seed, ranged qualities and sigmas) are ``chain.file_draws(spec, seed, index)``, index = the
file's place in the sorted listing of TARSET: the network's input is, byte for byte, the folder that ``python -m rcot_amd.chain`` /
``jpeg`` / ``blur`` / ``resize`` writes with the same seed.

Residency.  At set-up every target and every degraded twin is decoded or made ONCE and kept as uint8 [h, w, 3] in a
``DeviceImageCache`` of ``--val_cache_gb`` GiB: a validation set wants one frozen noise realisation, unlike training.  The bytes needed
are known from the image headers, so a suite that does not fit is refused before anything is decoded.  Nothing is streamed per epoch.

Geometry.  Every image is padded at the bottom / right to the network's size multiple (``--val_pad``, reflect unless given; an image
that mode cannot pad is skipped with a line), restored whole and cropped by the egress kernel.  The images of a set are grouped by padded
shape.  ``--val_batch 1``: rcot_image_ingest, the network, rcot_image_egress per image — the launches of the single-folder validation.
``--val_batch N`` / ``0`` (a whole group): up to N images of a group in one rcot_image_ingest_batch, ONE network call and one
rcot_image_egress_batch.  The default is 8: on 68 images of 321 x 481 one validation takes 2.03 s against 2.47 s at 1 (the network's lower
levels stop being bound by launches; profiles/valsuite.txt), and a whole group is no faster.  No tiles, no self-ensemble.

Figures per set, each as mean / min / max over the ``count`` images processed: ``psnr_float`` (the reference's validation figure on the
unclamped float output; the divisor is the number of images PROCESSED — the single-folder validation divides by the length of the
listing, skipped files included, and that quirk is not copied), ``psnr_u8`` and ``ssim`` in the set's protocol (from the egress
kernel's own sums for box2 / rgb, from rcot_image_quality on the 8-bit output otherwise; ``shave`` crops both 8-bit images on the device
first), ``psnrb`` when asked for (rcot_image_blockiness).  ``mean`` is the unweighted mean over the sets.  Everything stays on the
device until every set is done; ONE read back per validation.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import types
from typing import NamedTuple, Optional

import torch

FIGURES = ("psnr_float", "psnr_u8", "ssim", "psnrb")
SSIM_WINDOWS = ("box2", "uniform7", "gauss11")
COLORS = ("rgb", "y")
KEYS = ("color", "ssim", "shave", "psnrb", "seed", "border", "subsampling")
USAGE = "--val_set NAME TASK TARSET [DEGSET] [key=value ...]"


class SetSpec(NamedTuple):
    name: str
    task: str                      # as given
    kind: str                      # "paired" | "made"
    sid: Optional[dict]            # a made set: the sample fields of rcot_amd/degrade.py
    tarset: str
    degset: Optional[str]
    color: str
    ssim: str
    shave: int
    psnrb: bool
    seed: int
    border: str
    subsampling: str

    @property
    def standard(self) -> bool:
        """rcot_image_quality instead of the egress kernel's own sums"""
        return self.ssim != "box2" or self.color != "rgb"

    @property
    def needs_u8(self) -> bool:
        return self.standard or self.psnrb or self.shave > 0


# ------------------------------------------------------------------------------- parsing
def _refuse(name, piece, why):
    raise SystemExit(f"--val_set {name}: {piece}: {why}  ({USAGE})")


def _parse_task(name: str, task: str, border: str, subsampling: str):
    """-> (kind, sample fields or None)"""
    from . import blur as B
    from . import chain as C
    from . import degrade as D
    if task == "paired":
        return "paired", None
    opts = types.SimpleNamespace(blur_border=border, jpeg_subsampling=subsampling)
    try:
        if task.startswith("denoise_"):
            try:
                sigma = float(task[len("denoise_"):])
            except ValueError:
                raise ValueError(f"the denoising tasks are named denoise_<sigma> with sigma in 0 .. 255 (denoise_15, denoise_25, denoise_50)")
            if not (math.isfinite(sigma) and 0 <= sigma <= 255):
                raise ValueError(f"sigma {sigma:g} is outside 0 .. 255")
            spec = C.parse_spec("noise_g" + C._num(sigma))
            return "made", D.BY_FIELD["chain"].fields(spec, D.blur_border(opts), D.jpeg_subsampling(opts))
        for t in D.TASKS:
            v = t.parse(task)
            if v is None:
                continue
            if t.field == "blur" and B.needs_angle(v):
                raise ValueError(f"a validation set blurs with one fixed PSF: a motion blur needs its angle, m<L>a<deg>; {B.GRAMMAR}")
            return "made", t.fields(v, *[o(opts) for o in t.options])
    except (ValueError, SystemExit) as e:
        _refuse(name, f"task {task!r}", str(e))
    _refuse(name, f"task {task!r}", "expected paired, denoise_<sigma>, sr_x2|3|4, sr_bd_x3, jpeg_q<Q>, blur_<spec> or chain_<stage>+...")


def parse_val_set(tokens) -> SetSpec:
    """one ``--val_set`` occurrence -> SetSpec; SystemExit naming the set and the piece for anything malformed"""
    from .blur import BORDERS
    from .jpeg import SUBSAMPLING
    tokens = [str(t) for t in tokens]
    pos = [t for t in tokens if "=" not in t and t != "psnrb"]
    keys = [t for t in tokens if "=" in t or t == "psnrb"]
    name = pos[0] if pos else "?"
    if len(pos) < 3:
        _refuse(name, "arguments", f"a set needs NAME TASK TARSET, got {len(pos)} of them")
    if len(pos) > 4:
        _refuse(name, f"argument {pos[4]!r}", "at most NAME TASK TARSET DEGSET come before the keys")
    kv = {}
    for t in keys:
        k, _, v = t.partition("=")
        if k not in KEYS:
            _refuse(name, f"key {k!r}", f"unknown; the keys are {', '.join(KEYS)}")
        if k in kv:
            _refuse(name, f"key {k!r}", "given twice")
        kv[k] = v
    color, ssim = kv.get("color", "rgb"), kv.get("ssim", "box2")
    border, sub = kv.get("border", "replicate"), kv.get("subsampling", "420")
    if color not in COLORS:
        _refuse(name, f"color={color}", f"expected one of {', '.join(COLORS)}")
    if ssim not in SSIM_WINDOWS:
        _refuse(name, f"ssim={ssim}", f"expected one of {', '.join(SSIM_WINDOWS)}")
    if border not in BORDERS:
        _refuse(name, f"border={border}", f"expected one of {', '.join(BORDERS)}")
    if sub not in SUBSAMPLING:
        _refuse(name, f"subsampling={sub}", f"expected one of {', '.join(SUBSAMPLING)}")
    ints = {}
    for k in ("shave", "seed"):
        try:
            ints[k] = int(kv.get(k, "0"))
        except ValueError:
            _refuse(name, f"{k}={kv[k]}", "expected an integer")
        if ints[k] < 0:
            _refuse(name, f"{k}={kv[k]}", "expected an integer >= 0")
    if "psnrb" in kv and kv["psnrb"] not in ("", "1", "0"):
        _refuse(name, f"psnrb={kv['psnrb']}", "psnrb takes no value")
    psnrb = "psnrb" in kv and kv["psnrb"] != "0"
    if ints["shave"] and ssim == "box2":
        _refuse(name, f"shave={ints['shave']}", "the shave crops the 8-bit images for rcot_image_quality; ssim=box2 comes from the egress "
                                                 "kernel's own sums, which cannot be cropped: use ssim=uniform7 or ssim=gauss11")
    if ssim == "box2" and color == "y":
        _refuse(name, "color=y", "the 2 x 2 map on the luma plane is computed on the host only (rcot_amd.tester --metrics folders): use "
                                 "ssim=uniform7 or ssim=gauss11")
    kind, sid = _parse_task(name, pos[1], border, sub)
    degset = pos[3] if len(pos) == 4 else None
    if kind == "paired" and degset is None:
        _refuse(name, "task 'paired'", "needs DEGSET, the folder of degraded images")
    if kind == "made" and degset is not None:
        _refuse(name, f"DEGSET {degset!r}", f"task {pos[1]} makes the degraded images from the targets: no DEGSET is read")
    return SetSpec(name, pos[1], kind, sid, pos[2], degset, color, ssim, ints["shave"], psnrb, ints["seed"], border, sub)


def parse_val_sets(occurrences) -> list:
    """every ``--val_set`` of a command line (argparse: nargs="+", action="append") -> [SetSpec]; names are unique, and ``mean`` is taken"""
    specs = []
    for tokens in occurrences or []:
        s = parse_val_set(tokens)
        if s.name == "mean":
            _refuse(s.name, "NAME", "'mean' names the mean over the sets")
        if "." in s.name:
            _refuse(s.name, "NAME", "a name holds no '.' (--save_best SET.FIGURE)")
        if any(o.name == s.name for o in specs):
            _refuse(s.name, "NAME", "given twice: every set needs a name of its own")
        specs.append(s)
    return specs


def parse_best_key(key: str, specs) -> tuple:
    """``--save_best KEY``, KEY = <set|mean>.<figure> -> (set name or "mean", figure); SystemExit for a set or figure that is not there"""
    where, dot, fig = str(key).rpartition(".")
    names = [s.name for s in specs]
    if not dot or where not in names + ["mean"]:
        raise SystemExit(f"--save_best {key}: expected <set|mean>.<figure> with a set of {', '.join(names + ['mean'])}")
    if fig not in FIGURES:
        raise SystemExit(f"--save_best {key}: figure {fig!r} is not one of {', '.join(FIGURES)}")
    if fig == "psnrb" and not any(s.psnrb for s in specs if where in ("mean", s.name)):
        raise SystemExit(f"--save_best {key}: no set behind {where!r} reports psnrb (give it the key psnrb)")
    return where, fig


def add_arguments(parser, standalone: bool = False) -> None:
    parser.add_argument("--val_set", nargs="+", action="append", default=None, metavar="ARG",
                        help="a validation set: NAME TASK TARSET [DEGSET] [key=value ...]; TASK = paired (DEGSET is read), denoise_<sigma>, "
                             "or any whole-image task (sr_x2|3|4, sr_bd_x3, jpeg_q<Q>, blur_<spec>, chain_<...>) made from the targets on "
                             "the device; keys: color=rgb|y ssim=box2|uniform7|gauss11 shave=N psnrb seed=S border=... subsampling=...; "
                             "any number of sets (rcot_amd/valsuite.py)" + ("" if standalone else "; without it: --degset / --tarset as before"))
    parser.add_argument("--val_batch", type=int, default=8,
                        help="with --val_set: images of one padded shape per network call (1 = one image per call, the launches of the "
                             "single-folder validation; 0 = a whole group; default 8: measured 18 %% faster per validation than 1 on "
                             "321 x 481 images, profiles/valsuite.txt)")
    parser.add_argument("--val_cache_gb", type=float, default=8.0,
                        help="with --val_set: budget in GiB of the resident 8-bit images (targets and degraded twins); a suite that does not "
                             "fit is refused before training starts")
    if not standalone:
        parser.add_argument("--save_best", nargs="?", const="mean.psnr_float", default=None, metavar="KEY",
                            help="with --val_set: when KEY = <set|mean>.<figure> (default mean.psnr_float) improves, the checkpoint just written "
                                 "is also saved as ..._best.pth; the checkpoint carries \"best\": {key, value, epoch}")


def check_flags(o, stock_mprnet: bool = False, explicit_pad: bool = True) -> list:
    """The trainer's up-front check: parses the sets (SystemExit naming the set and the piece), refuses the suite's flags where they
    cannot act, and sets ``o.val_pad`` to reflect when sets were given and --val_pad was not.  Returns the SetSpecs ([]: no suite)."""
    specs = parse_val_sets(o.val_set)
    d = argparse.ArgumentParser()
    add_arguments(d)
    d = d.parse_args([])
    if not specs:
        for f in ("val_batch", "val_cache_gb", "save_best"):
            if getattr(o, f) != getattr(d, f):
                raise SystemExit(f"--{f} belongs to the validation suite: it needs --val_set")
        return specs
    if stock_mprnet:
        raise SystemExit("--val_set needs the HIP path; --backbone mprnet without a GPU (or with RCOT_MPRNET_STOCK=1) is the stock-ops loop")
    if o.val_batch < 0:
        raise SystemExit(f"--val_batch {o.val_batch}: images per network call, 0 = a whole group of one padded shape")
    if not (o.val_cache_gb > 0 and math.isfinite(o.val_cache_gb)):
        raise SystemExit(f"--val_cache_gb {o.val_cache_gb}: the budget of the resident validation images, in GiB, must be positive")
    if o.save_best is not None:
        parse_best_key(o.save_best, specs)
    if not explicit_pad:
        o.val_pad = "reflect"
    return specs


# ------------------------------------------------------------------------------- what a suite holds: listing, sizes, budget, groups
def _listing(folder: str) -> list:
    return [p for p in sorted(glob.glob(folder + "*")) if os.path.isfile(p)]      # the trainer's listing of --tarset: a prefix glob


def image_size(path: str) -> tuple:
    """(h, w) from the file's header"""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def list_sets(specs) -> dict:
    """name -> [(index, target path, degraded path or None)]; an empty folder, or a paired set whose folders differ in length, is refused"""
    out = {}
    for s in specs:
        tars = _listing(s.tarset)
        if not tars:
            _refuse(s.name, f"TARSET {s.tarset!r}", "no files")
        degs = [None] * len(tars)
        if s.kind == "paired":
            degs = _listing(s.degset)
            if not degs:
                _refuse(s.name, f"DEGSET {s.degset!r}", "no files")
        out[s.name] = [(i, t, d) for i, (t, d) in enumerate(zip(tars, degs))]
    return out


def bytes_needed(specs, listing, size_of=image_size) -> int:
    """the image bytes the resident suite takes: target and degraded twin of every file, at the size the task keeps (an sr task crops
    to its scale first) — an upper bound where pairs are skipped later"""
    total = 0
    for s in specs:
        m = (s.sid or {}).get("sr", 1)
        for _, tar, _ in listing[s.name]:
            h, w = size_of(tar)
            total += 2 * 3 * (h - h % m) * (w - w % m)
    return total


def check_budget(specs, listing, cache_gb: float, size_of=image_size) -> int:
    need = bytes_needed(specs, listing, size_of)
    if need > int(cache_gb * 2 ** 30):
        raise SystemExit(f"--val_set: the suite needs {need / 2 ** 30:.3f} GiB of resident 8-bit images ({len(specs)} set(s), "
                         f"{sum(len(v) for v in listing.values())} files, targets and degraded twins), --val_cache_gb is {cache_gb:g}: raise "
                         f"it, or validate fewer images (nothing is streamed per epoch)")
    return need


def group_by_shape(sizes, mult: int, pad: str):
    """``sizes``: [(h, w)] -> (groups, skipped): ``groups`` an insertion-ordered dict (Hp, Wp) -> [positions in ``sizes``] by the shape
    ``pad`` brings each image to, ``skipped`` [(position, message)] for the images ``wholeimage.pad_geometry`` refuses"""
    from .wholeimage import pad_geometry
    groups, skipped = {}, []
    for i, (h, w) in enumerate(sizes):
        try:
            groups.setdefault(pad_geometry(h, w, mult, pad), []).append(i)
        except ValueError as e:
            skipped.append((i, str(e)))
    return groups, skipped


def chunks(members, batch: int) -> list:
    """the network calls of one group: ``batch`` images each (0: all of them)"""
    n = len(members) if batch <= 0 else batch
    return [members[i:i + n] for i in range(0, len(members), n)]


# ------------------------------------------------------------------------------- --save_best
class Best:
    """the best value of ``key`` so far: {"key", "value", "epoch"} in the checkpoint"""

    def __init__(self, key: str, where: str, figure: str):
        self.key, self.where, self.figure = key, where, figure
        self.value, self.epoch = None, None

    def figure_of(self, result: dict) -> float:
        v = result["mean"][self.figure] if self.where == "mean" else result["sets"][self.where][self.figure]["mean"]
        return float("nan") if v is None else float(v)

    def update(self, result: dict, epoch: int) -> bool:
        """True when this validation's figure is the best so far (every figure of the suite is better when larger; NaN never wins)"""
        v = self.figure_of(result)
        if math.isnan(v) or (self.value is not None and not v > self.value):
            return False
        self.value, self.epoch = v, int(epoch)
        return True

    def state_dict(self) -> dict:
        return {"key": self.key, "value": self.value, "epoch": self.epoch}

    def load_state_dict(self, st) -> Optional[str]:
        """continue a checkpoint's record; a note for the user when it tracked another key (then it starts over)"""
        if not isinstance(st, dict) or st.get("value") is None:
            return None
        if st.get("key") != self.key:
            return f"holds the best of {st.get('key')}, --save_best tracks {self.key}: starting over"
        self.value, self.epoch = float(st["value"]), st.get("epoch")
        return None


def best_path(path: str) -> str:
    root, ext = os.path.splitext(path)
    return root + "_best" + ext


# ------------------------------------------------------------------------------- the suite on the device
class _Image(NamedTuple):
    index: int
    name: str
    tar: torch.Tensor
    deg: torch.Tensor
    h: int
    w: int


class ValSuite:
    def __init__(self, backend, specs, mult: int, pad: str, batch: int = 8, cache_gb: float = 8.0, verbose: bool = True):
        from .imagecache import DeviceImageCache
        self.be, self.specs, self.mult, self.pad, self.batch = backend, list(specs), int(mult), pad, int(batch)
        self.say = print if verbose else (lambda *a, **k: None)
        listing = list_sets(self.specs)
        need = check_budget(self.specs, listing, cache_gb)
        self.cache = DeviceImageCache(backend, int(cache_gb * 2 ** 30))
        self.sets = {}                                                    # name -> (images, groups)
        if any(s.task.startswith("denoise_") for s in self.specs):
            self.say("validation suite: denoise_<sigma> adds the noise to the 8-bit target and clips to 8 bits (rcot_noise_u8, the rule of "
                     "the training patches), not the float noise of rcot_amd.tester --noise_sigma")
        self.say("validation suite: psnr_float is the mean over the images processed (the single-folder validation divides by the length of "
                 "the listing, skipped files included)")
        for s in self.specs:
            self.sets[s.name] = self._load(s, listing[s.name])
        self.say(f"validation suite: {len(self.specs)} set(s), {sum(len(v[0]) for v in self.sets.values())} image pairs resident, "
                 f"{self.cache.bytes / 2 ** 20:.1f} MiB of {cache_gb:g} GiB ({need / 2 ** 20:.1f} MiB by the headers), pad {self.pad}, "
                 f"{'a whole group' if self.batch <= 0 else self.batch} image(s) per network call")

    # -------------------------------------------------------------- set-up: decode once, degrade once, keep
    def _keep(self, key, arr):
        import numpy as np
        t = self.cache.offer(key, torch.from_numpy(np.ascontiguousarray(arr)).to(self.be.device))
        assert key in self.cache, key                                   # the budget was checked against the headers
        return t

    def _load(self, s: SetSpec, files):
        import numpy as np
        from PIL import Image
        from .chain import file_draws
        from .degrade import degrade_file_u8
        images = []
        for index, tar_name, deg_name in files:
            tar = np.array(Image.open(tar_name).convert("RGB"))
            if s.kind == "paired":
                deg = np.array(Image.open(deg_name).convert("RGB"))
                if deg.shape != tar.shape:
                    self.say(f"validation set {s.name}: {deg_name} skipped: degraded {deg.shape[0]} x {deg.shape[1]} and target "
                             f"{tar.shape[0]} x {tar.shape[1]} differ")
                    continue
            else:
                drawn = file_draws(s.sid["chain"][0], s.seed, index) if "chain" in s.sid else None
                pair = degrade_file_u8(tar, s.sid, drawn, self.be, "target")
                if pair is None:
                    self.say(f"validation set {s.name}: {tar_name} skipped")
                    continue
                tar, deg = pair
            h, w = tar.shape[:2]
            if s.shave and (h <= 2 * s.shave or w <= 2 * s.shave):
                self.say(f"validation set {s.name}: {tar_name} skipped: {h} x {w} leaves nothing after shave={s.shave}")
                continue
            images.append(_Image(index, os.path.basename(tar_name), self._keep((s.name, index, "tar"), tar),
                                 self._keep((s.name, index, "deg"), deg), h, w))
        groups, skipped = group_by_shape([(im.h, im.w) for im in images], self.mult, self.pad)
        for i, why in skipped:
            self.say(f"validation set {s.name}: {images[i].name} skipped: {why}")
        return images, groups

    def groups(self, name: str) -> dict:
        """(Hp, Wp) -> the file names of the group, in processing order"""
        images, groups = self.sets[name]
        return {k: [images[i].name for i in v] for k, v in groups.items()}

    # -------------------------------------------------------------- one validation
    def _restore_chunk(self, net, ims, Hp, Wp, needs_u8):
        """-> [(out_u8 or None, stats [4])] per image, and the network's output tensor [n, 3, Hp, Wp]"""
        be = self.be
        if self.batch == 1:
            from .wholeimage import restore_any_size
            res = []
            for im in ims:
                r = restore_any_size(net, im.deg, self.mult, self.pad)
                o, _, st = be.image_egress(r.out, im.h, im.w, target=im.tar, want_out=needs_u8, want_stats=True)
                res.append((o, st))
            return res, None
        xb = be.image_ingest_batch([im.deg for im in ims], Hp, Wp, self.pad)
        out = net(xb)
        outs, stats = be.image_egress_batch(out, [(im.h, im.w) for im in ims], [im.tar for im in ims], want_out=needs_u8, want_stats=True)
        return [(o, stats[i]) for i, o in enumerate(outs)], out

    def run(self, net, keep_outputs: bool = False) -> dict:
        """every set through ``net`` -> {"sets": {name: {...}}, "mean": {...}}; per set "count", "task", the figures as {"mean", "min",
        "max"} and "images": the per-image figures in the order of the listing (the means are summed in that order).  ``keep_outputs``: also "outputs" per set, the network's output
        tensor of every batched call with the images it held [(tensor [n, 3, Hp, Wp], [(name, h, w)])] (the tests read it)."""
        from .quality import psnrb_from_sums, quality_metrics
        from .wholeimage import image_metrics
        be = self.be
        parts, layout, kept = [], [], {}
        for s in self.specs:
            images, groups = self.sets[s.name]
            N, og = s.shave, s.shave % 8
            for (Hp, Wp), members in groups.items():
                for chunk in chunks(members, self.batch):
                    ims = [images[i] for i in chunk]
                    res, out = self._restore_chunk(net, ims, Hp, Wp, s.needs_u8)
                    if keep_outputs and out is not None:
                        kept.setdefault(s.name, []).append((out, [(im.name, im.h, im.w) for im in ims]))
                    for im, (o, st) in zip(ims, res):
                        vec = [st]
                        if s.needs_u8:
                            tar_m, out_m = im.tar, o
                            if N:
                                tar_m = be.crop_u8(im.tar, N, N, im.h - 2 * N, im.w - 2 * N)
                                out_m = be.crop_u8(o, N, N, im.h - 2 * N, im.w - 2 * N)
                            if s.standard:
                                vec.append(be.image_quality(tar_m, out_m, s.ssim, s.color))
                            if s.psnrb:
                                vec.append(be.image_blockiness(out_m, tar_m, s.color, og, og).view(torch.float64).flatten())
                        parts += vec
                        layout.append((s, im))
        host = torch.cat(parts).cpu() if parts else torch.zeros(0, dtype=torch.float64)      # the ONE read back of a validation
        sets, at = {s.name: {"task": s.task, "count": 0, "images": []} for s in self.specs}, 0
        for s, im in layout:
            fig = image_metrics(host[at:at + 4].tolist(), im.h, im.w)
            at += 4
            if s.standard:
                q = quality_metrics(host[at:at + 4].tolist())
                at += 4
                fig["psnr_u8"], fig["ssim"] = q["psnr"], q["ssim"]
            if s.psnrb:
                planes = 3 if s.color == "rgb" else 1
                ints = host[at:at + 5 * planes].contiguous().view(torch.int64).view(planes, 5).numpy()
                at += 5 * planes
                fig["psnrb"] = psnrb_from_sums(ints, im.h - 2 * s.shave, im.w - 2 * s.shave, s.shave % 8, s.shave % 8)
            sets[s.name]["images"].append((im.index, dict(name=im.name, **fig)))
        for s in self.specs:
            r = sets[s.name]
            r["images"] = [d for _, d in sorted(r["images"], key=lambda p: p[0])]      # in the order of the listing, whatever the groups were
            r["count"] = len(r["images"])
            for f in FIGURES:
                if f == "psnrb" and not s.psnrb:
                    continue
                v = [im[f] for im in r["images"]]
                nan = float("nan")
                r[f] = {"mean": sum(v) / len(v), "min": min(v), "max": max(v)} if v else {"mean": nan, "min": nan, "max": nan}
            if keep_outputs:
                r["outputs"] = kept.get(s.name, [])
        return {"sets": sets, "mean": mean_over_sets(sets)}


def mean_over_sets(sets: dict) -> dict:
    """the unweighted mean over the sets of every figure's set mean (psnrb: over the sets that report it)"""
    out = {}
    for f in FIGURES:
        v = [r[f]["mean"] for r in sets.values() if f in r]
        if v:
            out[f] = sum(v) / len(v)
    return out


# ------------------------------------------------------------------------------- output
def format_table(result: dict, title: str = "") -> str:
    has_b = any("psnrb" in r for r in result["sets"].values())
    cell = lambda d: f"{d['mean']:8.4f} [{d['min']:8.4f}, {d['max']:8.4f}]"
    wide = max([len(n) for n in result["sets"]] + [4])
    tw = max([len(r["task"]) for r in result["sets"].values()] + [4])
    head = f"{'set':<{wide}}  {'task':<{tw}}  {'n':>4}  {'psnr_float mean [min, max]':<30}  {'psnr_u8':<30}  {'ssim':<30}"
    lines = ([f"validation suite{title}"] if title is not None else []) + [head + (f"  {'psnrb':<30}" if has_b else "")]
    for n, r in result["sets"].items():
        line = f"{n:<{wide}}  {r['task']:<{tw}}  {r['count']:>4}  {cell(r['psnr_float']):<30}  {cell(r['psnr_u8']):<30}  {cell(r['ssim']):<30}"
        lines.append(line + (f"  {cell(r['psnrb']):<30}" if "psnrb" in r else ""))
    m = result["mean"]
    pad30 = lambda f: f"{m[f]:8.4f}{'':22}" if f in m else f"{'':30}"
    lines.append(f"{'mean':<{wide}}  {'':<{tw}}  {len(result['sets']):>4}  {pad30('psnr_float')}  {pad30('psnr_u8')}  {pad30('ssim')}"
                 + (f"  {pad30('psnrb')}" if has_b else ""))
    return "\n".join(lines)


def json_ready(result: dict) -> dict:
    """the figures of a validation without the per-image lists and tensors"""
    return {"sets": {n: {k: v for k, v in r.items() if k not in ("images", "outputs")} for n, r in result["sets"].items()},
            "mean": dict(result["mean"])}


def append_jsonl(path: str, obj: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(obj) + "\n")


def validate(suite: ValSuite, net, avg=None, val_weights: Optional[str] = None, epoch=None, weights_name: str = "ema", say=print) -> dict:
    """One validation as the trainer runs it: on the raw weights, on the averaged ones (``avg``: a WeightAverage; ``val_weights`` "ema"),
    or on both — then the averaged weights' figures are the deciding ones ("sets" / "mean") and "weights" holds both.  Prints the
    table(s) and returns the JSON object of validation_suite.jsonl."""
    if avg is None or val_weights == "raw":
        res = suite.run(net)
        say(format_table(res, "" if avg is None else ", weights raw"))
        return {"epoch": epoch, "weights": "raw", **json_ready(res)}
    both = {}
    if val_weights == "both":
        raw = suite.run(net)
        say(format_table(raw, ", weights raw"))
        both["raw"] = json_ready(raw)
    with avg.applied():
        res = suite.run(net)
    say(format_table(res, f", weights {weights_name}"))
    if val_weights == "both":
        both["ema"] = json_ready(res)
        return {"epoch": epoch, "weights": both, **json_ready(res)}
    return {"epoch": epoch, "weights": weights_name, **json_ready(res)}


# ------------------------------------------------------------------------------- python -m rcot_amd.valsuite
def main(argv=None):
    parser = argparse.ArgumentParser(description="The validation suite of rcot_amd.trainer for a checkpoint (rcot_amd/valsuite.py)")
    parser.add_argument("--model", required=True, type=str, help="checkpoint path (either backbone)")
    parser.add_argument("--weights", choices=["raw", "ema"], default="raw", help="ema = the averaged weights (\"Tnet_ema\")")
    parser.add_argument("--val_pad", choices=["none", "reflect", "replicate"], default="reflect",
                        help="padding to the network's size multiple (none: images of other sizes are skipped)")
    parser.add_argument("--out", default=None, type=str, help="append the JSON object of this validation to FILE")
    add_arguments(parser, standalone=True)
    opt = parser.parse_args(argv)
    specs = parse_val_sets(opt.val_set)
    if not specs:
        raise SystemExit(f"rcot_amd.valsuite needs at least one {USAGE}")
    if opt.val_batch < 0:
        raise SystemExit(f"--val_batch {opt.val_batch}: images per network call, 0 = a whole group of one padded shape")
    listing = list_sets(specs)
    check_budget(specs, listing, opt.val_cache_gb)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: rcot_amd.valsuite runs the HIP path only")
    from .tester import load_network
    net, _ = load_network(opt.model, opt.weights)
    suite = ValSuite(net.be, specs, net.size_multiple, opt.val_pad, opt.val_batch, opt.val_cache_gb)
    res = suite.run(net)
    print(format_table(res, f", weights {opt.weights}"))
    obj = {"epoch": None, "model": opt.model, "weights": opt.weights, **json_ready(res)}
    if opt.out:
        append_jsonl(opt.out, obj)
    return obj


if __name__ == "__main__":
    main()
