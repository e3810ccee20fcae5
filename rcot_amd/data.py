"""Folder-driven training data with the contract of the reference's ``TrainDataset`` + ``DataLoader``
(util/dataset_utils.py:27-281, trainer.py:132-135): batches ``([names, de_id], degraded, clean)`` of fp32 CHW patches in
[0, 1].  The host keeps what needs a file system and an image decoder — the sample lists (:63-169, same list files,
same replication factors, same clean/ground-truth naming rules :198-213) and PIL decoding — and hands every decoded uint8
image to ONE device kernel (``rcot_patch_prep``) that crops, applies the dihedral augmentation, adds the Gaussian noise of
the denoise_* tasks and converts to CHW float (rcot_amd/csrc/dataprep.hip).  The sr_x2 / sr_x3 / sr_x4 tasks (``--sr_dir``) degrade
the whole HR image on the device first (rcot_amd/resize.py) and hand both images to the same kernel; the jpeg_q<Q> tasks (``--jpeg_dir``)
do the same with a baseline JPEG round trip (rcot_amd/jpeg.py), the blur_<spec> tasks (``--blur_dir``) and sr_bd_x3 with a PSF blur
(rcot_amd/blur.py), the chain_<stage>+... tasks (``--chain_dir``) with a chain of those stages and whole-image noise (rcot_amd/chain.py).
The reference does those steps with PIL/numpy on the host at ``num_workers=0`` (trainer.py:32,134).

``FolderLoader(..., cache=DeviceImageCache(...))`` (the trainer's ``--data_cache device``, rcot_amd/imagecache.py) keeps every decoded
image — and the degraded twin of an HR image — on the device after its first use and cuts a whole batch from the resident images in ONE
launch (``rcot_patch_prep_batch``); the batches are the uncached loader's, bit for bit.

Randomness: the reference leaves python's ``random`` and numpy unseeded; here every draw (epoch
shuffle, crop origin, augmentation mode 1..7, noise seed, then the angle of a blur_m<L> sample or the draws of a chain) comes from one
``random.Random(seed, epoch)`` stream indexed by the GLOBAL sample position, so a run is reproducible and the union of the ranks'
shards does not depend on the world size.
"""
from __future__ import annotations

import os
import random
from typing import List, Sequence

import numpy as np
import torch

DE_DICT = {"denoise_15": 0, "denoise_25": 1, "denoise_50": 2, "derain": 3, "dehaze": 4, "deblur": 5, "lowlight": 6,
           "single": 7}                                   # util/dataset_utils.py:40
NOISE_SIGMA = {0: 15.0, 1: 25.0, 2: 50.0}                  # util/degradation_utils.py:29-40
# superset: super-resolution (the reference's README lists DIV2K next to the other tasks and has no loader for it).  The sample is an
# HR image, the degradation is made on the device (rcot_amd/resize.py: bicubic down by s, 8 bits, up by s, 8 bits), the label is the
# reference's `single` — how the reference would see a pre-made SR folder
SR_SCALE = {"sr_x2": 2, "sr_x3": 3, "sr_x4": 4}
# superset: compression-artifact reduction, --de_type jpeg_q<Q> for any Q in 1 .. 100 (the CAR rows of restoration tables use 10, 20,
# 30, 40).  The sample is a clean image from --jpeg_dir, the degradation — a baseline JPEG round trip of the whole image — is made on the
# device (rcot_amd/jpeg.py), the label is `single` again
# superset: deblurring from sharp images alone, --de_type blur_<spec> (rcot_amd/blur.py's PSF grammar: blur_g1.6, blur_g2k15, blur_m15a30,
# blur_m15).  The sample is a sharp image from --blur_dir, the WHOLE image is blurred on the device, the label is the reference's `deblur`.
# A motion PSF without an angle draws whole degrees per sample.  sr_bd_x3 is the "BD" row of super-resolution tables (Gaussian 7 x 7,
# sigma 1.6, every third pixel, bicubic x3 back): an HR image from --sr_dir, decoded as sr_x3 decodes it, the label `single`
SR_BD = "sr_bd_x3"


def blur_tasks(de_type: Sequence[str]) -> List[tuple]:
    """the (name, PSF spec) of every blur_<spec> task of a --de_type list, in its order; SystemExit for a malformed name"""
    from .blur import parse_de_type
    out = []
    for t in de_type:
        try:
            spec = parse_de_type(t)
        except ValueError as e:
            raise SystemExit(str(e))
        if spec is not None:
            out.append((t, spec))
    return out


def blur_border(args) -> str:
    """--blur_border replicate | mirror | wrap (default replicate)"""
    from .blur import BORDERS
    v = str(getattr(args, "blur_border", None) or "replicate")
    if v not in BORDERS:
        raise SystemExit(f"--blur_border {v}: expected replicate, mirror or wrap")
    return v


def blur_dir_or_exit(args, de_type: str) -> str:
    root = getattr(args, "blur_dir", None)
    if root is None:
        raise SystemExit(f"--de_type {de_type} needs --blur_dir DIR, a flat folder of sharp images")
    return root


def jpeg_tasks(de_type: Sequence[str]) -> List[tuple]:
    """the (name, quality) of every jpeg_q<Q> task of a --de_type list, in its order; SystemExit for a malformed name or quality"""
    from .jpeg import parse_de_type
    out = []
    for t in de_type:
        try:
            q = parse_de_type(t)
        except ValueError as e:
            raise SystemExit(str(e))
        if q is not None:
            out.append((t, q))
    return out


def jpeg_subsampling(args) -> int:
    """--jpeg_subsampling 420 | 444 (default 420) as PIL's number"""
    from .jpeg import SUBSAMPLING
    v = str(getattr(args, "jpeg_subsampling", None) or "420")
    if v not in SUBSAMPLING:
        raise SystemExit(f"--jpeg_subsampling {v}: expected 420 or 444")
    return SUBSAMPLING[v]


def jpeg_dir_or_exit(args, de_type: str) -> str:
    root = getattr(args, "jpeg_dir", None)
    if root is None:
        raise SystemExit(f"--de_type {de_type} needs --jpeg_dir DIR, a flat folder of clean images")
    return root


def chain_tasks(de_type: Sequence[str]) -> List[tuple]:
    """the (name, stage records) of every chain_<stage>+... task of a --de_type list, in its order; SystemExit, naming the stage, for a
    malformed chain"""
    from .chain import parse_de_type
    out = []
    for t in de_type:
        spec = parse_de_type(t)
        if spec is not None:
            out.append((t, spec))
    return out


def chain_dir_or_exit(args, de_type: str) -> str:
    root = getattr(args, "chain_dir", None)
    if root is None:
        raise SystemExit(f"--de_type {de_type} needs --chain_dir DIR, a flat folder of clean images")
    return root


def crop_to_multiple(img: np.ndarray, base: int = 16) -> np.ndarray:
    """util/image_utils.py:59-64 crop_img: centre-crop H and W to multiples of ``base``."""
    h, w = img.shape[0], img.shape[1]
    ch, cw = h % base, w % base
    return img[ch // 2:h - ch + ch // 2, cw // 2:w - cw + cw // 2, :]


def rain_gt_name(rainy_name: str) -> str:
    """util/dataset_utils.py:198-200."""
    return rainy_name.split("rainy")[0] + "gt/norain-" + rainy_name.split("rain-")[-1]


def nonhazy_name(hazy_name: str) -> str:
    """util/dataset_utils.py:202-207."""
    dir_name = hazy_name.split("synthetic")[0] + "original/"
    name = hazy_name.split("/")[-1].split("_")[0]
    return dir_name + name + "." + hazy_name.split(".")[-1]


def build_sample_ids(args) -> List[dict]:
    """The reference's ``_init_ids`` + ``_merge_ids`` (util/dataset_utils.py:63-228): one dict per sample with the file of
    the (degraded or clean) image, the task label and, for paired tasks, the ground-truth file."""
    de_type = list(args.de_type)
    ids: List[dict] = []
    if any(t in de_type for t in ("denoise_15", "denoise_25", "denoise_50")):
        ref = os.path.join(args.data_file_dir, "noisy/denoise.txt")
        listed = set(l.strip() for l in open(ref))
        clean = [args.denoise_dir + n for n in sorted(os.listdir(args.denoise_dir)) if n.strip() in listed]
        for t, lab in (("denoise_15", 0), ("denoise_25", 1), ("denoise_50", 2)):
            if t in de_type:
                ids += [{"file": c, "de": lab, "gt": None} for c in clean] * 5          # :87-101 (x5)
    if "derain" in de_type:
        rs = os.path.join(args.data_file_dir, "rainy/rainTrain.txt")
        files = [args.derain_dir + l.strip() for l in open(rs)]
        ids += [{"file": f, "de": 3, "gt": rain_gt_name(f)} for f in files] * 360       # :122-127 (x360)
    if "dehaze" in de_type:
        hz = os.path.join(args.data_file_dir, "hazy/hazy_outside.txt")
        files = [args.dehaze_dir + l.strip() for l in open(hz)]
        ids += [{"file": f, "de": 4, "gt": nonhazy_name(f)} for f in files]             # :106-116
    for t, lab, attr, sub_d, sub_c, rep in (("deblur", 5, "deblur_dir", "blur/", "sharp/", 5),
                                             ("lowlight", 6, "lowlight_dir", "low/", "high/", 20),
                                             ("single", 7, "single_dir", "degraded/", "target/", 5)):
        if t in de_type:
            root = getattr(args, attr, None)
            if root is None:
                raise SystemExit(f"--de_type {t} needs --{attr} (the reference never defines that flag either: "
                                 f"util/dataset_utils.py:134-169 reads args.{attr})")
            names = sorted(os.listdir(os.path.join(root, sub_c if t == "deblur" else sub_d)))
            ids += [{"file": os.path.join(root, sub_d, n), "de": lab, "gt": os.path.join(root, sub_c, n)} for n in names] * rep
    for t, scale in SR_SCALE.items():
        if t in de_type:
            root = sr_dir_or_exit(args, t)
            names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
            ids += [{"file": os.path.join(root, n), "de": DE_DICT["single"], "gt": None, "sr": scale} for n in names] * 5   # x5: `single`'s factor
    for t, quality in jpeg_tasks(de_type):
        root = jpeg_dir_or_exit(args, t)
        sub = jpeg_subsampling(args)
        names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
        ids += [{"file": os.path.join(root, n), "de": DE_DICT["single"], "gt": None, "jpeg": (quality, sub)} for n in names] * 5
    for t, spec in blur_tasks(de_type):
        root = blur_dir_or_exit(args, t)
        border = blur_border(args)
        names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
        ids += [{"file": os.path.join(root, n), "de": DE_DICT["deblur"], "gt": None, "blur": (spec, border)} for n in names] * 5
    if SR_BD in de_type:                                                    # "sr": 3 — the decode and the cached HR image of sr_x3
        root = sr_dir_or_exit(args, SR_BD)
        names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
        ids += [{"file": os.path.join(root, n), "de": DE_DICT["single"], "gt": None, "sr": 3, "bd": True} for n in names] * 5
    for t, spec in chain_tasks(de_type):                                    # "sr": the decode (and the cached image) of sr_x<k>
        from .chain import size_multiple
        root = chain_dir_or_exit(args, t)
        how = (spec, blur_border(args), jpeg_subsampling(args))
        names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
        extra = {"sr": size_multiple(spec)} if size_multiple(spec) > 1 else {}
        ids += [{"file": os.path.join(root, n), "de": DE_DICT["single"], "gt": None, "chain": how, **extra} for n in names] * 5
    return ids


def sr_dir_or_exit(args, de_type: str) -> str:
    root = getattr(args, "sr_dir", None)
    if root is None:
        raise SystemExit(f"--de_type {de_type} needs --sr_dir DIR, a flat folder of high-resolution images")
    return root


def _read_rgb(path: str) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


class FolderLoader:
    """Iterable over one epoch of shuffled batches (``len`` = batches per epoch of the GLOBAL batch size), sharded over
    ranks by global sample position.  Yields device tensors."""

    def __init__(self, args, local_batch: int, seed: int = 0, rank: int = 0, world: int = 1, backend=None, threads: int = 0, cache=None):
        """``threads`` (the reference's --threads / DataLoader num_workers, trainer.py:32,134): decode workers.  The files of
        the NEXT batches are read and decoded in a thread pool while the current iteration runs (PIL releases the GIL while it
        decodes); 0 still prefetches with one worker — decoding never sits on the training thread's critical path."""
        # ``cache`` (a rcot_amd.imagecache.DeviceImageCache on the backend's device, or None): None is the route above, launch for
        # launch.  With a cache every file is decoded and uploaded once and stays on the device, the pool decodes only the files of
        # coming batches that are not resident yet, and a batch is ONE rcot_patch_prep_batch launch — the same draws from the same
        # per-sample streams, so the batches are the uncached loader's bit for bit (``_iter_cached``).
        self.cache = cache
        self.args, self.B, self.P = args, local_batch, args.patch_size
        self.threads = max(1, int(threads or 0))
        self.depth = 2                                                      # batches decoded ahead
        self.seed, self.rank, self.world = seed, rank, world
        self.ids = build_sample_ids(args)
        if not self.ids:
            raise SystemExit("no training samples found: check --de_type and the *_dir / --data_file_dir flags")
        if rank == 0:
            print(f"...total sample ids: {len(self.ids)}")                 # util/dataset_utils.py:228
        if backend is None:
            from .ops import default_backend
            backend = default_backend()
        self.be = backend
        self.epoch = 0

    def __len__(self):
        g = self.B * self.world
        if self.world > 1:
            return len(self.ids) // g           # every rank must take part in every all-reduce: the ragged tail is dropped
        return (len(self.ids) + g - 1) // g                                  # DataLoader(drop_last=False)

    def set_epoch(self, epoch: int):
        """the next __iter__ yields epoch ``epoch`` (1-based): shuffle order, crops, augmentations and noise seeds are functions of
        (seed, epoch), so a run resumed at --start_epoch continues the stream instead of replaying epoch 1"""
        self.epoch = int(epoch) - 1

    @staticmethod
    def _decode(sid: dict):
        """worker thread: read + decode + crop to a multiple of 16 (util/image_utils.py:59-64)"""
        img = crop_to_multiple(_read_rgb(sid["file"]), 16)
        if sid.get("sr"):                                                   # then to a multiple of the scale, at the top left (x3 only)
            img = img[:img.shape[0] - img.shape[0] % sid["sr"], :img.shape[1] - img.shape[1] % sid["sr"]]
        gt = crop_to_multiple(_read_rgb(sid["gt"]), 16) if sid["gt"] is not None else None
        return np.ascontiguousarray(img), (None if gt is None else np.ascontiguousarray(gt))

    def _sample(self, rng: random.Random, sid: dict, deg_out, clean_out, decoded=None):
        P = self.P
        img, gt = decoded if decoded is not None else self._decode(sid)
        H, W = img.shape[0], img.shape[1]
        if H < P or W < P or (gt is not None and gt.shape != img.shape):
            raise ValueError(f"{sid['file']}: {H}x{W} is smaller than the {P}x{P} patch or differs from its ground truth")
        y0, x0 = rng.randint(0, H - P), rng.randint(0, W - P)
        mode = rng.randint(1, 7)                                            # random_augmentation: always 1..7
        nseed = rng.getrandbits(63)
        dev = self.be.device
        a = torch.from_numpy(img).to(dev, non_blocking=True)
        if sid.get("chain"):  # a degradation chain: every stage sees the WHOLE image; its own draws follow the three common ones
            assert getattr(self.be, "_plan", None) is None
            self.be.patch_prep(a, self._chained(rng, sid, a, nseed), y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)
        elif sid.get("bd"):   # super-resolution, BD protocol: blurred, sampled and enlarged again as a whole
            from .blur import bd_degrade_u8
            assert getattr(self.be, "_plan", None) is None
            self.be.patch_prep(a, bd_degrade_u8(a, self.be), y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)
        elif sid.get("blur"):  # deblurring: the WHOLE image is blurred, so a patch sees real neighbours and no border rule inside the image
            assert getattr(self.be, "_plan", None) is None
            self.be.patch_prep(a, self._blurred(rng, sid, a), y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)
        elif sid.get("sr"):   # super-resolution: the file is the HR image; the WHOLE image is degraded, so the crop sees real neighbours
            from .resize import sr_degrade_u8
            assert getattr(self.be, "_plan", None) is None                  # loader launches stay outside recorded launch plans
            self.be.patch_prep(a, sr_degrade_u8(a, sid["sr"], self.be), y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)
        elif sid.get("jpeg"):  # compression artifacts: the WHOLE image makes the round trip, so a crop sees block borders at any phase
            from .jpeg import jpeg_degrade_u8
            assert getattr(self.be, "_plan", None) is None
            self.be.patch_prep(a, jpeg_degrade_u8(a, *sid["jpeg"], self.be), y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)
        elif gt is None:      # denoise_*: the file IS the clean image, the degradation is synthetic noise
            self.be.patch_prep(a, None, y0, x0, P, mode, NOISE_SIGMA[sid["de"]], nseed, deg_out, clean_out)
        else:
            g = torch.from_numpy(gt).to(dev, non_blocking=True)
            self.be.patch_prep(g, a, y0, x0, P, mode, 0.0, nseed, deg_out, clean_out)

    def _blurred(self, rng: random.Random, sid: dict, a):
        """the blurred twin of the device image ``a`` of a blur_<spec> sample; a motion PSF without an angle draws whole degrees from the
        sample's stream — AFTER the crop, mode and noise-seed draws, which therefore are those of every other task"""
        from .blur import blur_degrade_u8, needs_angle, psf_q_of
        spec, border = sid["blur"]
        angle = rng.randint(0, 179) if needs_angle(spec) else None
        return blur_degrade_u8(a, psf_q_of(spec, angle), border, self.be)

    def _chained(self, rng: random.Random, sid: dict, a, nseed: int):
        """the degraded twin of the device image ``a`` of a chain sample: the chain's draws come from the sample's stream in stage
        order, AFTER the crop, mode and noise-seed draws (rcot_amd/chain.py); the noise stages run on seeds derived from ``nseed``"""
        from .chain import chain_degrade_u8, draw
        spec, border, sub = sid["chain"]
        return chain_degrade_u8(a, spec, draw(spec, rng, nseed), border, sub, self.be)

    def __iter__(self):
        if self.cache is not None:
            return self._iter_cached()
        return self._iter_uncached()

    def _iter_uncached(self):
        from concurrent.futures import ThreadPoolExecutor
        self.epoch += 1
        order = list(range(len(self.ids)))
        random.Random(self.seed * 1_000_003 + self.epoch).shuffle(order)      # DataLoader(shuffle=True)
        g = self.B * self.world
        dev = self.be.device
        nb = len(self)
        batch_idx = lambda it: order[it * g + self.rank * self.B:it * g + self.rank * self.B + self.B]
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            pending = {}                                                    # batch -> futures of its decoded files

            def submit(it):
                if it < nb and it not in pending:
                    pending[it] = [pool.submit(self._decode, self.ids[k]) for k in batch_idx(it)]
            for it in range(min(self.depth, nb)):
                submit(it)
            for it in range(nb):
                lo = it * g + self.rank * self.B
                idx = batch_idx(it)
                if not idx:
                    break
                submit(it)
                futs = pending.pop(it)
                submit(it + self.depth)                                     # keep the pool busy while this batch is prepared and trained
                n = len(idx)
                deg = torch.empty(n, 3, self.P, self.P, dtype=torch.float32, device=dev)
                clean = torch.empty_like(deg)
                names, labels = [], []
                for j, k in enumerate(idx):
                    sid = self.ids[k]
                    rng = random.Random((self.seed * 1_000_003 + self.epoch) * 2_147_483_659 + lo + j)
                    self._sample(rng, sid, deg[j], clean[j], futs[j].result())
                    names.append(os.path.basename(sid["gt"] or sid["file"]).split(".")[0])
                    labels.append(sid["de"])
                yield ([names, torch.tensor(labels)], deg, clean)

    # ------------------------------------------------------------------ the cached route (rcot_amd/imagecache.py)
    @staticmethod
    def _file_keys(sid: dict):
        """the files of a sample as (cache key, path, sr scale or 0): the image, then the ground truth of a paired sample"""
        if sid.get("sr"):
            return [((sid["file"], "crop16", "mod", sid["sr"]), sid["file"], sid["sr"])]
        keys = [((sid["file"], "crop16"), sid["file"], 0)]
        if sid["gt"] is not None:
            keys.append(((sid["gt"], "crop16"), sid["gt"], 0))
        return keys

    @staticmethod
    def _decode_file(path: str, s: int) -> np.ndarray:
        """worker thread: what ``_decode`` does to one file"""
        img = crop_to_multiple(_read_rgb(path), 16)
        if s:
            img = img[:img.shape[0] - img.shape[0] % s, :img.shape[1] - img.shape[1] % s]
        return np.ascontiguousarray(img)

    def _iter_cached(self):
        from concurrent.futures import ThreadPoolExecutor
        self.epoch += 1
        cache = self.cache
        order = list(range(len(self.ids)))
        random.Random(self.seed * 1_000_003 + self.epoch).shuffle(order)
        g = self.B * self.world
        dev = self.be.device
        nb = len(self)
        P = self.P
        batch_idx = lambda it: order[it * g + self.rank * self.B:it * g + self.rank * self.B + self.B]
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            inflight = {}                                                   # key -> future of a file that is being decoded
            asked = set()

            def submit(it):
                if it < nb and it not in asked:
                    asked.add(it)
                    for k in batch_idx(it):
                        for key, path, s in self._file_keys(self.ids[k]):
                            if key not in cache and key not in inflight:
                                inflight[key] = pool.submit(self._decode_file, path, s)

            def resident(key, path, s, local):
                """the device image of a file: from the cache, from this batch's transients, else decoded (by the pool, as a rule)"""
                t = cache.lookup(key)
                if t is None:
                    t = local.get(key)
                if t is None:
                    fut = inflight.pop(key, None)
                    img = fut.result() if fut is not None else self._decode_file(path, s)
                    t = local[key] = cache.offer(key, torch.from_numpy(img).to(dev, non_blocking=True))
                return t

            for it in range(min(self.depth, nb)):
                submit(it)
            for it in range(nb):
                lo = it * g + self.rank * self.B
                idx = batch_idx(it)
                if not idx:
                    break
                submit(it)
                submit(it + self.depth)
                n = len(idx)
                deg = torch.empty(n, 3, P, P, dtype=torch.float32, device=dev)
                clean = torch.empty_like(deg)
                names, labels, rows, local = [], [], [], {}
                for j, k in enumerate(idx):
                    sid = self.ids[k]
                    rng = random.Random((self.seed * 1_000_003 + self.epoch) * 2_147_483_659 + lo + j)
                    imgs = [resident(key, path, s, local) for key, path, s in self._file_keys(sid)]
                    a, gt = imgs[0], (imgs[1] if len(imgs) > 1 else None)
                    H, W = a.shape[0], a.shape[1]
                    if H < P or W < P or (gt is not None and gt.shape != a.shape):
                        raise ValueError(f"{sid['file']}: {H}x{W} is smaller than the {P}x{P} patch or differs from its ground truth")
                    y0, x0 = rng.randint(0, H - P), rng.randint(0, W - P)   # the draws of _sample, in its order
                    mode = rng.randint(1, 7)
                    nseed = rng.getrandbits(63)
                    if sid.get("chain"):
                        from .chain import cacheable, canonical
                        spec, border, sub = sid["chain"]
                        if cacheable(spec):                                 # no noise, nothing drawn: one twin per image
                            key = (sid["file"], "chain", canonical(spec), border, sub)
                            d = cache.lookup(key)
                            if d is None:
                                d = local.get(key)
                            if d is None:
                                d = local[key] = cache.offer(key, self._chained(rng, sid, a, nseed))
                                cache.chain_degradations += 1
                        else:                                               # noise or per-sample values: the chain runs for every sample
                            d = self._chained(rng, sid, a, nseed)
                        rows.append((a, d, y0, x0, mode, 0.0, nseed))
                    elif sid.get("bd"):
                        key = (sid["file"], "bd", 3)
                        d = cache.lookup(key)
                        if d is None:
                            d = local.get(key)
                        if d is None:
                            from .blur import bd_degrade_u8
                            d = local[key] = cache.offer(key, bd_degrade_u8(a, self.be))
                            cache.blur_degradations += 1
                        rows.append((a, d, y0, x0, mode, 0.0, nseed))
                    elif sid.get("blur"):
                        from .blur import needs_angle
                        if needs_angle(sid["blur"][0]):                    # an angle per sample: the twin is made per sample, not kept
                            d = self._blurred(rng, sid, a)
                        else:
                            key = (sid["file"], "blur", *sid["blur"])
                            d = cache.lookup(key)
                            if d is None:
                                d = local.get(key)
                            if d is None:
                                d = local[key] = cache.offer(key, self._blurred(rng, sid, a))
                                cache.blur_degradations += 1
                        rows.append((a, d, y0, x0, mode, 0.0, nseed))
                    elif sid.get("sr"):
                        key = (sid["file"], "sr", sid["sr"])
                        d = cache.lookup(key)
                        if d is None:
                            d = local.get(key)
                        if d is None:
                            from .resize import sr_degrade_u8
                            d = local[key] = cache.offer(key, sr_degrade_u8(a, sid["sr"], self.be))
                            cache.sr_degradations += 1
                        rows.append((a, d, y0, x0, mode, 0.0, nseed))
                    elif sid.get("jpeg"):
                        key = (sid["file"], "jpeg", *sid["jpeg"])
                        d = cache.lookup(key)
                        if d is None:
                            d = local.get(key)
                        if d is None:
                            from .jpeg import jpeg_degrade_u8
                            d = local[key] = cache.offer(key, jpeg_degrade_u8(a, *sid["jpeg"], self.be))
                            cache.jpeg_degradations += 1
                        rows.append((a, d, y0, x0, mode, 0.0, nseed))
                    elif gt is None:
                        rows.append((a, None, y0, x0, mode, NOISE_SIGMA[sid["de"]], nseed))
                    else:
                        rows.append((gt, a, y0, x0, mode, 0.0, nseed))
                    names.append(os.path.basename(sid["gt"] or sid["file"]).split(".")[0])
                    labels.append(sid["de"])
                self.be.patch_prep_batch(rows, P, deg, clean)
                yield ([names, torch.tensor(labels)], deg, clean)
