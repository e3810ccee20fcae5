"""The whole-image degradation tasks in one table: the task families whose sample is a clean image that is degraded AS A WHOLE on the
device before a patch is cut — ``sr_x<k>``, ``jpeg_q<Q>``, ``blur_<spec>``, ``sr_bd_x3`` and ``chain_<...>``.  The loader
(rcot_amd/data.py), the trainer's flag check and the tester's input step read everything they need to know about a family from its
entry; the grammars and the device entry points stay in the task's own module (resize.py, jpeg.py, blur.py, chain.py), which are
looked up there at call time.

A sample of such a task is the dict ``{"file", "de", "gt": None, **task.fields(value, *options)}``; ``task_of`` finds the entry from the
fields a sample carries.  Per sample, after the loader's three common draws, ``task.draw`` takes what the family draws from the
sample's stream, ``task.key`` names the degraded twin in the device cache (None: the twin is made per sample) and ``task.make`` makes
it."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import blur as B
from . import chain as C
from . import jpeg as J
from . import resize as R


def blur_border(args) -> str:
    """--blur_border replicate | mirror | wrap (default replicate)"""
    v = str(getattr(args, "blur_border", None) or "replicate")
    if v not in B.BORDERS:
        raise SystemExit(f"--blur_border {v}: expected replicate, mirror or wrap")
    return v


def jpeg_subsampling(args) -> int:
    """--jpeg_subsampling 420 | 444 (default 420) as PIL's number"""
    v = str(getattr(args, "jpeg_subsampling", None) or "420")
    if v not in J.SUBSAMPLING:
        raise SystemExit(f"--jpeg_subsampling {v}: expected 420 or 444")
    return J.SUBSAMPLING[v]


def _sr_scale(name: str):
    from .data import SR_SCALE                              # (data.py imports this module: the two names are read when a list is parsed)
    return SR_SCALE.get(name)


def _is_bd(name: str):
    from .data import SR_BD
    return True if name == SR_BD else None


def _chain_fields(spec, border, sub) -> dict:
    m = C.size_multiple(spec)                               # "sr": the decode (and the cached HR image) of sr_x<m>
    return {"chain": (spec, border, sub), **({"sr": m} if m > 1 else {})}


def _chain_key(sid: dict):
    spec, border, sub = sid["chain"]                        # a chain with noise or drawn values runs for every sample
    return (sid["file"], "chain", C.canonical(spec), border, sub) if C.cacheable(spec) else None


def _chain_has_420(sid: dict) -> bool:
    return sid["chain"][2] == 2 and any(st[0] == "jpeg" for st in sid["chain"][0])


def _blur_angle(sid: dict, rng, nseed):
    return rng.randint(0, 179) if B.needs_angle(sid["blur"][0]) else None       # a motion PSF without an angle draws whole degrees


def _blur_key(sid: dict):
    return None if B.needs_angle(sid["blur"][0]) else (sid["file"], "blur", *sid["blur"])       # a drawn angle: made per sample, not kept


# field      the sample field that marks the family (and the entry's name)
# parse      --de_type name -> the task's value, None for a name of another family; ValueError / SystemExit for a malformed one
# once       the family's names count once each, in sorted order, however --de_type lists them (else: in its order, as often as listed)
# folder     the flag of its image folder; noun: what "needs --<folder> DIR, a flat folder of <noun>" calls the images
# label      the reference's task label of its samples
# options    the readers of the option flags it takes (--blur_border, --jpeg_subsampling), in the order they are checked
# fields     (value, *options) -> the fields of a sample id
# needs_wide sample -> a 4:2:0 JPEG stage runs: the image must be wider than 4 pixels
# draw       (sample, rng, noise seed) -> what the family draws per sample, after the common draws (None: nothing)
# key        sample -> the cache key of the degraded twin, None for a twin that depends on the draw
# make       (device image, sample, drawn, backend) -> the degraded twin
# counter    the cache counter a twin counts under
Task = collections.namedtuple("Task", "field parse once folder noun label options fields needs_wide draw key make counter")
_nothing = lambda sid, rng, nseed: None
_any_width = lambda sid: False

TASKS = (
    Task(field="sr", parse=_sr_scale, once=True, folder="sr_dir", noun="high-resolution images", label="single", options=(),
         fields=lambda s: {"sr": s},
         needs_wide=_any_width, draw=_nothing,
         key=lambda sid: (sid["file"], "sr", sid["sr"]),
         make=lambda a, sid, drawn, be: R.sr_degrade_u8(a, sid["sr"], be), counter="sr"),
    Task(field="jpeg", parse=J.parse_de_type, once=False, folder="jpeg_dir", noun="clean images", label="single", options=(jpeg_subsampling,),
         fields=lambda q, sub: {"jpeg": (q, sub)},
         needs_wide=lambda sid: sid["jpeg"][1] == 2, draw=_nothing,
         key=lambda sid: (sid["file"], "jpeg", *sid["jpeg"]),
         make=lambda a, sid, drawn, be: J.jpeg_degrade_u8(a, *sid["jpeg"], be), counter="jpeg"),
    Task(field="blur", parse=B.parse_de_type, once=False, folder="blur_dir", noun="sharp images", label="deblur", options=(blur_border,),
         fields=lambda spec, border: {"blur": (spec, border)},
         needs_wide=_any_width, draw=_blur_angle,
         key=_blur_key,
         make=lambda a, sid, drawn, be: B.blur_degrade_u8(a, B.psf_q_of(sid["blur"][0], drawn), sid["blur"][1], be), counter="blur"),
    # the BD protocol of scale 3: "sr": 3 — the decode and the cached HR image of sr_x3
    Task(field="bd", parse=_is_bd, once=True, folder="sr_dir", noun="high-resolution images", label="single", options=(),
         fields=lambda _: {"sr": 3, "bd": True},
         needs_wide=_any_width, draw=_nothing,
         key=lambda sid: (sid["file"], "bd", 3),
         make=lambda a, sid, drawn, be: B.bd_degrade_u8(a, be), counter="blur"),
    # the noise stages run on seeds derived from the sample's noise seed, which the draw carries
    Task(field="chain", parse=C.parse_de_type, once=False, folder="chain_dir", noun="clean images", label="single",
         options=(blur_border, jpeg_subsampling),
         fields=_chain_fields,
         needs_wide=_chain_has_420, draw=lambda sid, rng, nseed: C.draw(sid["chain"][0], rng, nseed),
         key=_chain_key,
         make=lambda a, sid, drawn, be: C.chain_degrade_u8(a, sid["chain"][0], drawn, *sid["chain"][1:], be), counter="chain"),
)
BY_FIELD = {t.field: t for t in TASKS}
_PRECEDENCE = ("chain", "bd", "blur", "sr", "jpeg")         # a chain or BD sample carries "sr" too


def task_of(sid: dict):
    """the entry of a sample, None for a sample of a reference task"""
    for f in _PRECEDENCE:
        if sid.get(f):
            return BY_FIELD[f]
    return None


def named(task: Task, de_type) -> list:
    """the (name, value) of the family's tasks in a --de_type list, in its order; SystemExit for a malformed name"""
    out = []
    for t in de_type:
        try:
            v = task.parse(t)
        except ValueError as e:
            raise SystemExit(str(e))
        if v is not None:
            out.append((t, v))
    return out


def folder(task: Task, args, de_type: str) -> str:
    root = getattr(args, task.folder, None)
    if root is None:
        raise SystemExit(f"--de_type {de_type} needs --{task.folder} DIR, a flat folder of {task.noun}")
    return root


def degrade_file_u8(img: np.ndarray, sid: dict, drawn, be, noun: str = ""):
    """one file of an evaluation folder: uint8 [H, W, 3] on the host -> (clean, degraded) uint8 arrays of one size — the image cropped
    at the top left to the task's size multiple, and its degradation under ``drawn``, made on the device — or None, with a message,
    for an image a stage cannot take.  ``noun`` ("target"): the message names the file as it was read; without: as it was cropped"""
    m = sid.get("sr", 1)
    given = f"{noun} {img.shape[0]} x {img.shape[1]}"
    img = np.ascontiguousarray(img[:img.shape[0] - img.shape[0] % m, :img.shape[1] - img.shape[1] % m])
    shown = given if noun else f"{img.shape[0]} x {img.shape[1]}"
    if img.shape[0] < m or img.shape[1] < m:
        print(f"  skipped: {shown} is smaller than the scale factor {m}")
        return None
    task = task_of(sid)
    if img.shape[1] <= 4 and task.needs_wide(sid):
        print(f"  skipped: {shown} is not wider than 4 pixels (4:2:0)")
        return None
    return img, task.make(torch.from_numpy(img).to(be.device), sid, drawn, be).cpu().numpy()
