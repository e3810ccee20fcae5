"""A device-resident training set: every image of the training folders decoded once and kept in HBM as uint8 [H, W, 3], so that
``FolderLoader(..., cache=...)`` (rcot_amd/data.py) cuts a whole batch from resident images in one launch (``patch_prep_batch``)
instead of decoding, uploading and — for the super-resolution tasks — degrading the files of every sample again.

Keys (a file's: ``FolderLoader._file_keys``; a twin's: the ``key`` of its family's entry in rcot_amd/degrade.py, which also names the
entry point that makes it and the counter it counts under)
    (path, "crop16")            a decoded file after ``crop_to_multiple(..., 16)``
    (path, "crop16", "mod", s)  the HR image of an ``sr_x<s>`` sample after the further top-left crop to a multiple of ``s``
    (path, "sr", s)             its degraded twin, made ONCE by ``rcot_amd.resize.sr_degrade_u8``
    (path, "jpeg", Q, S)        the twin of a ``jpeg_q<Q>`` sample (its clean image is the plain ``(path, "crop16")``), made ONCE by
                                ``rcot_amd.jpeg.jpeg_degrade_u8`` with subsampling S (PIL's number: 2 = 4:2:0, 0 = 4:4:4)
    (path, "blur", spec, border) the twin of a ``blur_<spec>`` sample whose PSF is fixed (clean image: ``(path, "crop16")``), made ONCE by
                                ``rcot_amd.blur.blur_degrade_u8``; a motion PSF that draws its angle per sample has no resident twin
    (path, "bd", 3)             the twin of an ``sr_bd_x3`` sample (HR image: ``(path, "crop16", "mod", 3)``, shared with ``sr_x3``),
                                made ONCE by ``rcot_amd.blur.bd_degrade_u8``
    (path, "chain", name, border, S) the twin of a ``chain_<...>`` sample whose chain has no noise stage and draws nothing per sample
                                (``rcot_amd.chain.cacheable``; name: ``chain.canonical`` of its stages), made ONCE by
                                ``rcot_amd.chain.chain_degrade_u8``.  Its clean image is ``(path, "crop16")``, or the ``"mod"`` key of
                                ``sr_x<k>`` when the chain has such a stage.  Any other chain keeps the decoded image only and runs
                                for every sample: a noise realisation frozen per image would be learned

Budget: ``budget_bytes`` of image bytes.  An image that would take the total over the budget is not stored: the loader uses it as a
transient tensor for the batch at hand (stream-ordered allocation keeps it alive until the launch has run) and meets it as a miss
again next time.  There is no eviction and no reordering: what is resident depends only on the order of first touches, which the
loader's seed fixes, so a run stays reproducible.

Counters: ``images`` and ``bytes`` resident, ``hits`` and ``misses`` over every resolution of a key, ``sr_degradations`` and
``jpeg_degradations`` made (the report names the latter once there is one), ``blur_degradations``: whole-image blurs kept, BD included
(named once there is one), ``chain_degradations``: twins of deterministic chains kept (named last, once there is one).  The loader
counts a twin where it makes it, through ``count(counter)``.
"""
from __future__ import annotations

import torch


class DeviceImageCache:
    def __init__(self, backend, budget_bytes: int):
        self.be = backend
        self.device = backend.device
        self.budget = max(0, int(budget_bytes))
        self._store = {}
        self.bytes = self.hits = self.misses = self.sr_degradations = self.jpeg_degradations = self.blur_degradations = 0
        self.chain_degradations = 0

    @property
    def images(self) -> int:
        return len(self._store)

    def __contains__(self, key) -> bool:
        return key in self._store

    def keys(self):
        return list(self._store)                      # in the order of storing

    def lookup(self, key):
        """the resident image of ``key`` (a hit) or None (a miss); every call counts as one of the two"""
        t = self._store.get(key)
        if t is None:
            self.misses += 1
        else:
            self.hits += 1
        return t

    def offer(self, key, img: torch.Tensor) -> torch.Tensor:
        """``img`` (uint8 [H, W, 3] on the cache's device) is kept under ``key`` if it fits the budget; returned either way"""
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous() or img.device != self.device:
            raise ValueError(f"DeviceImageCache: {key}: expected a contiguous uint8 [H, W, 3] image on {self.device}")
        if key not in self._store and self.bytes + img.numel() <= self.budget:
            self._store[key] = img
            self.bytes += img.numel()
        return img

    def count(self, counter: str):
        """one more degraded twin made under ``counter``: "sr", "jpeg", "blur" or "chain" (rcot_amd/degrade.py names it per task)"""
        setattr(self, counter + "_degradations", getattr(self, counter + "_degradations") + 1)

    def report(self) -> str:
        return (f"data cache: {self.images} images, {self.bytes / 2 ** 20:.1f} MiB of {self.budget / 2 ** 30:g} GiB, {self.hits} hits, "
                f"{self.misses} misses, {self.sr_degradations} sr degradations"
                + (f", {self.jpeg_degradations} jpeg degradations" if self.jpeg_degradations else "")
                + (f", {self.blur_degradations} blur degradations" if self.blur_degradations else "")
                + (f", {self.chain_degradations} chain degradations" if self.chain_degradations else ""))
