"""Folder-driven training data with the contract of the reference's ``TrainDataset`` + ``DataLoader``
(util/dataset_utils.py:27-281, trainer.py:132-135): batches ``([names, de_id], degraded, clean)`` of fp32 CHW patches in
[0, 1].  The host keeps what needs a file system and an image decoder — the sample lists (:63-169, same list files,
same replication factors, same clean/ground-truth naming rules :198-213) and PIL decoding — and hands every decoded uint8
image to ONE device kernel (``rcot_patch_prep``) that crops, applies the dihedral augmentation, adds the Gaussian noise of
the denoise_* tasks and converts to CHW float (rcot_amd/csrc/dataprep.hip).  The whole-image tasks — sr_x<k>, jpeg_q<Q>, blur_<spec>,
sr_bd_x3 and chain_<stage>+... — degrade the whole clean image on the device first and hand both images to the same kernel; what a
family parses, reads, draws, keeps and calls is ONE entry of the table in rcot_amd/degrade.py, and this file has one arm for all of them.
The reference does those steps with PIL/numpy on the host at ``num_workers=0`` (trainer.py:32,134).

``FolderLoader(..., cache=DeviceImageCache(...))`` (the trainer's ``--data_cache device``, rcot_amd/imagecache.py) keeps every decoded
image — and the degraded twin a table entry gives a cache key — on the device after its first use and cuts a whole batch from the
resident images in ONE launch (``rcot_patch_prep_batch``); the batches are the uncached loader's, bit for bit.  Both routes take the
common draws (``_draws``) and resolve a sample to its images (``_resolve``) through the same two functions, over the same epoch
skeleton (``_epoch``); they differ in where an image comes from and in the launch.

Randomness: the reference leaves python's ``random`` and numpy unseeded; here every draw (epoch
shuffle, crop origin, augmentation mode 1..7, noise seed, then the angle of a blur_m<L> sample or the draws of a chain) comes from one
``random.Random(seed, epoch)`` stream indexed by the GLOBAL sample position, so a run is reproducible and the union of the ranks'
shards does not depend on the world size.
"""
from __future__ import annotations

import os
import random
from typing import List

import numpy as np
import torch

from . import degrade

DE_DICT = {"denoise_15": 0, "denoise_25": 1, "denoise_50": 2, "derain": 3, "dehaze": 4, "deblur": 5, "lowlight": 6,
           "single": 7}                                   # util/dataset_utils.py:40
NOISE_SIGMA = {0: 15.0, 1: 25.0, 2: 50.0}                  # util/degradation_utils.py:29-40
# supersets, all degraded as WHOLE images on the device (rcot_amd/degrade.py has the table of the five families):
# super-resolution (the reference's README lists DIV2K next to the other tasks and has no loader for it): the sample is an HR image from
# --sr_dir, degraded by rcot_amd/resize.py (bicubic down by s, 8 bits, up by s, 8 bits); the label is the reference's `single` — how the
# reference would see a pre-made SR folder
SR_SCALE = {"sr_x2": 2, "sr_x3": 3, "sr_x4": 4}
# the "BD" row of super-resolution tables (Gaussian 7 x 7, sigma 1.6, every third pixel, bicubic x3 back): an HR image from --sr_dir,
# decoded as sr_x3 decodes it, the label `single`.  (jpeg_q<Q>: rcot_amd/jpeg.py; blur_<spec>: rcot_amd/blur.py; chain_<...>: rcot_amd/chain.py)
SR_BD = "sr_bd_x3"


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
    for task in degrade.TASKS:                                              # the whole-image tasks: sr, jpeg, blur, bd, chain
        tasks = degrade.named(task, de_type)
        for t, value in (sorted(set(tasks)) if task.once else tasks):
            root = degrade.folder(task, args, t)
            fields = task.fields(value, *(read(args) for read in task.options))
            names = sorted(n for n in os.listdir(root) if os.path.isfile(os.path.join(root, n)))
            ids += [{"file": os.path.join(root, n), "de": DE_DICT[task.label], "gt": None, **fields} for n in names] * 5   # x5: `single`'s factor
    return ids


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
        # what a sample id says about every sample made from it, worked out once: its name, the cache keys of its files, its whole-image
        # task (or None) and the cache key of its degraded twin (or None) — the cached route spends its time on the host
        self._static = [(os.path.basename(sid["gt"] or sid["file"]).split(".")[0], self._file_keys(sid), task, task and task.key(sid))
                        for sid in self.ids for task in (degrade.task_of(sid),)]

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
        """worker thread: read + decode + crop to a multiple of 16 (util/image_utils.py:59-64), then (``s``: the scale of an sr_x<s> image
        or of a chain's sr stages) to a multiple of ``s`` at the top left (x3 and x6 only)"""
        img = crop_to_multiple(_read_rgb(path), 16)
        if s:
            img = img[:img.shape[0] - img.shape[0] % s, :img.shape[1] - img.shape[1] % s]
        return np.ascontiguousarray(img)

    @staticmethod
    def _decode(sid: dict):
        """worker thread: the decoded files of a sample as (image, ground truth or None)"""
        files = [FolderLoader._decode_file(path, s) for _, path, s in FolderLoader._file_keys(sid)]
        return files[0], (files[1] if len(files) > 1 else None)

    def _draws(self, rng: random.Random, sid: dict, shape, gt_shape):
        """the common draws of a sample, the first of its stream whatever its task: crop origin, augmentation mode, noise seed"""
        P, (H, W) = self.P, shape[:2]
        if H < P or W < P or (gt_shape is not None and gt_shape != shape):
            raise ValueError(f"{sid['file']}: {H}x{W} is smaller than the {P}x{P} patch or differs from its ground truth")
        y0, x0 = rng.randint(0, H - P), rng.randint(0, W - P)
        mode = rng.randint(1, 7)                                            # random_augmentation: always 1..7
        return y0, x0, mode, rng.getrandbits(63)

    def _resolve(self, rng: random.Random, sid: dict, task, a, gt, nseed: int, twin=None, key=None):
        """a sample's device images ``a`` and ``gt`` (or None) -> (clean image, degraded image or None, noise sigma): what patch_prep
        takes.  A whole-image task (rcot_amd/degrade.py) degrades the WHOLE image, so a patch sees real neighbours, block borders at
        any phase and no border rule inside the image; its own draws follow the common ones.  ``task``: the sample's entry of that
        table, or None.  ``twin(key, make, counter)``: the cached route's keeper of degraded twins, asked where the task gives the twin
        a ``key``; else the twin is made here"""
        if task is not None:
            if twin is None:
                assert getattr(self.be, "_plan", None) is None              # loader launches stay outside recorded launch plans
            make = lambda: task.make(a, sid, task.draw(sid, rng, nseed), self.be)      # (a kept twin depends on no draw: none is taken)
            return a, (make() if key is None else twin(key, make, task.counter)), 0.0
        if gt is None:                                                      # denoise_*: the file IS the clean image, the degradation is synthetic noise
            return a, None, NOISE_SIGMA[sid["de"]]
        return gt, a, 0.0

    def _sample(self, rng: random.Random, sid: dict, deg_out, clean_out, decoded=None):
        img, gt = decoded if decoded is not None else self._decode(sid)
        y0, x0, mode, nseed = self._draws(rng, sid, img.shape, None if gt is None else gt.shape)
        up = lambda x: None if x is None else torch.from_numpy(x).to(self.be.device, non_blocking=True)
        clean, deg, sigma = self._resolve(rng, sid, degrade.task_of(sid), up(img), up(gt), nseed)
        self.be.patch_prep(clean, deg, y0, x0, self.P, mode, sigma, nseed, deg_out, clean_out)

    def _epoch(self):
        """the next epoch as a list of (global position of the rank's first sample, the rank's sample indices) per batch, and the
        number the seed of a sample's stream is its global position above"""
        self.epoch += 1
        order = list(range(len(self.ids)))
        random.Random(self.seed * 1_000_003 + self.epoch).shuffle(order)      # DataLoader(shuffle=True)
        g, batches = self.B * self.world, []
        for it in range(len(self)):
            lo = it * g + self.rank * self.B
            if not order[lo:lo + self.B]:
                break
            batches.append((lo, order[lo:lo + self.B]))
        return batches, (self.seed * 1_000_003 + self.epoch) * 2_147_483_659

    def _outputs(self, idx):
        """the names and labels of a batch and its two output tensors"""
        deg = torch.empty(len(idx), 3, self.P, self.P, dtype=torch.float32, device=self.be.device)
        return [[self._static[k][0] for k in idx], torch.tensor([self.ids[k]["de"] for k in idx])], deg, torch.empty_like(deg)

    def __iter__(self):
        if self.cache is not None:
            return self._iter_cached()
        return self._iter_uncached()

    def _iter_uncached(self):
        from concurrent.futures import ThreadPoolExecutor
        batches, stream = self._epoch()
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            pending = {}                                                    # batch -> futures of its decoded files

            def submit(it):
                if it < len(batches) and it not in pending:
                    pending[it] = [pool.submit(self._decode, self.ids[k]) for k in batches[it][1]]
            for it in range(min(self.depth, len(batches))):
                submit(it)
            for it, (lo, idx) in enumerate(batches):
                submit(it)
                futs = pending.pop(it)
                submit(it + self.depth)                                     # keep the pool busy while this batch is prepared and trained
                head, deg, clean = self._outputs(idx)
                for j, k in enumerate(idx):
                    self._sample(random.Random(stream + lo + j), self.ids[k], deg[j], clean[j], futs[j].result())
                yield (head, deg, clean)

    def _iter_cached(self):
        """the cached route (rcot_amd/imagecache.py): the same draws from the same streams, the images from the device"""
        from concurrent.futures import ThreadPoolExecutor
        cache, dev = self.cache, self.be.device
        batches, stream = self._epoch()
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            inflight = {}                                                   # key -> future of a file that is being decoded
            asked = set()
            local = {}                                                      # the batch's transients: images the budget did not take

            def submit(it):
                if it < len(batches) and it not in asked:
                    asked.add(it)
                    for k in batches[it][1]:
                        for key, path, s in self._static[k][1]:
                            if key not in cache and key not in inflight:
                                inflight[key] = pool.submit(self._decode_file, path, s)

            def kept(key, make, counter=None):
                """the device image of ``key``: from the cache, from this batch's transients, else made, offered and counted"""
                t = cache.lookup(key)
                if t is None:
                    t = local.get(key)
                if t is None:
                    t = local[key] = cache.offer(key, make())
                    if counter is not None:
                        cache.count(counter)
                return t

            def decoded(key, path, s):
                """the upload of a file: decoded by the pool, as a rule"""
                fut = inflight.pop(key, None)
                return torch.from_numpy(fut.result() if fut is not None else self._decode_file(path, s)).to(dev, non_blocking=True)

            for it in range(min(self.depth, len(batches))):
                submit(it)
            for it, (lo, idx) in enumerate(batches):
                submit(it)
                submit(it + self.depth)
                head, deg, clean = self._outputs(idx)
                rows = []
                local.clear()
                for j, k in enumerate(idx):
                    sid, rng = self.ids[k], random.Random(stream + lo + j)
                    _, files, task, twin_key = self._static[k]
                    imgs = [kept(key, lambda: decoded(key, path, s)) for key, path, s in files]
                    a, gt = imgs[0], (imgs[1] if len(imgs) > 1 else None)
                    y0, x0, mode, nseed = self._draws(rng, sid, a.shape, None if gt is None else gt.shape)
                    clean_img, deg_img, sigma = self._resolve(rng, sid, task, a, gt, nseed, kept, twin_key)
                    rows.append((clean_img, deg_img, y0, x0, mode, sigma, nseed))
                self.be.patch_prep_batch(rows, self.P, deg, clean)
                yield (head, deg, clean)
