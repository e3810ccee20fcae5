"""Tensor-level front end of the HIP kernels (``HipBackend``).

Every method takes torch tensors / views that live on the MI355X, checks the layout
contract of include/rcot_hip.h, and launches the matching ``rcot_*`` entry point on the
calling thread's current HIP stream.  Outputs are written in place into caller-provided
tensors.  PyTorch is used only for memory (allocation, views) and streams.

There is deliberately no alternative implementation here: constructing a HipBackend
without a GPU or without librcot_hip.so raises.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import os
import struct
import sys

import ctypes as C

import torch

from . import lib as _lib

LN = Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]   # (mu, rs, weight, bias)


ctypes_ll = C.c_longlong


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def check_patch_rows(rows, P: int, deg_out, clean_out) -> None:
    """The host check of ``patch_prep_batch`` (backend-independent: the kernel trusts its table): every row is
    ``(clean_img, deg_img | None, y0, x0, mode, sigma, seed)`` with contiguous uint8 [H, W, 3] images of one shape per pair, a P x P
    window inside the image and a mode in 0..7; ``deg_out`` / ``clean_out`` are contiguous float32 [len(rows), 3, P, P].  Raises
    ValueError naming the first row that fails."""
    P = int(P)
    if P <= 0 or not rows:
        raise ValueError(f"patch_prep_batch: needs at least one row and P > 0, got {len(rows)} row(s), P = {P}")
    for what, t in (("deg_out", deg_out), ("clean_out", clean_out)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (len(rows), 3, P, P):
            raise ValueError(f"patch_prep_batch: {what} must be a contiguous float32 [{len(rows)}, 3, {P}, {P}] tensor, got "
                             f"{t.dtype} {tuple(t.shape)}")
    for b, (clean_img, deg_img, y0, x0, mode, sigma, seed) in enumerate(rows):
        for what, t in (("clean", clean_img), ("degraded", deg_img)):
            if t is None and what == "degraded":
                continue
            if t is None or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
                raise ValueError(f"patch_prep_batch: row {b}: the {what} image must be a contiguous uint8 [H, W, 3] tensor")
            if t.device != deg_out.device:
                raise ValueError(f"patch_prep_batch: row {b}: the {what} image is on {t.device}, the batch on {deg_out.device}")
        H, W = int(clean_img.shape[0]), int(clean_img.shape[1])
        if deg_img is not None and tuple(deg_img.shape) != (H, W, 3):
            raise ValueError(f"patch_prep_batch: row {b}: the degraded image is {tuple(deg_img.shape)}, the clean one {(H, W, 3)}")
        if not (0 <= int(y0) and int(y0) + P <= H and 0 <= int(x0) and int(x0) + P <= W):
            raise ValueError(f"patch_prep_batch: row {b}: the {P} x {P} window at ({y0}, {x0}) leaves the {H} x {W} image")
        if not 0 <= int(mode) <= 7:
            raise ValueError(f"patch_prep_batch: row {b}: mode {mode} is not one of the dihedral maps 0..7")


_PAD_NAMES = ("none", "reflect", "replicate")


def _check_u8_row(what: str, i: int, name: str, t, device):
    if t is None or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
        raise ValueError(f"{what}: row {i}: the {name} must be a contiguous uint8 [h, w, 3] tensor")
    if t.device != device:
        raise ValueError(f"{what}: row {i}: the {name} is on {t.device}, the batch on {device}")


def check_ingest_rows(imgs, Hp: int, Wp: int, mode, out, device) -> None:
    """The host check of ``image_ingest_batch`` (backend-independent: the kernel trusts its table): 1 .. 65535 contiguous uint8
    [h, w, 3] images on ``device`` that ``mode`` pads to Hp x Wp (``wholeimage.pad_geometry``'s rules), and ``out`` (None: not made
    yet) a contiguous float32 tensor of N * 3 * Hp * Wp elements there.  Raises ValueError naming the first row that fails."""
    what = "image_ingest_batch"
    mode = "none" if mode is None else mode
    if mode not in _PAD_NAMES:
        raise ValueError(f"{what}: padding mode {mode!r}: expected one of {_PAD_NAMES}")
    N, Hp, Wp = len(imgs), int(Hp), int(Wp)
    if not 1 <= N <= 65535 or Hp < 1 or Wp < 1:
        raise ValueError(f"{what}: needs 1 .. 65535 rows and a padded shape of at least 1 x 1, got {N} row(s), {Hp} x {Wp}")
    if out is not None and (out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != N * 3 * Hp * Wp or out.device != device):
        raise ValueError(f"{what}: out must be a contiguous float32 [{N}, 3, {Hp}, {Wp}] tensor on {device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    for i, t in enumerate(imgs):
        _check_u8_row(what, i, "image", t, device)
        h, w = int(t.shape[0]), int(t.shape[1])
        ok = h >= 1 and w >= 1 and h <= Hp and w <= Wp
        if mode == "none":
            ok = ok and (h, w) == (Hp, Wp)
        elif mode == "reflect":
            ok = ok and Hp - h <= h - 1 and Wp - w <= w - 1
        if not ok:
            raise ValueError(f"{what}: row {i}: {mode} cannot pad {h} x {w} to {Hp} x {Wp}")


def check_egress_rows(restored, sizes, targets, wants, want_stats: bool, device) -> None:
    """The host check of ``image_egress_batch``: ``restored`` a contiguous float32 [N, 3, Hp, Wp] tensor on ``device``, one (h, w)
    inside Hp x Wp per row, a uint8 [h, w, 3] target per row when statistics are asked for, and something to do for every row (an
    8-bit output or the statistics).  Raises ValueError naming the first row that fails."""
    what = "image_egress_batch"
    N = len(sizes)
    if not 1 <= N <= 65535:
        raise ValueError(f"{what}: needs 1 .. 65535 rows, got {N}")
    if (restored.dtype != torch.float32 or restored.dim() != 4 or not restored.is_contiguous() or restored.shape[0] != N
            or restored.shape[1] != 3 or restored.device != device):
        raise ValueError(f"{what}: restored must be a contiguous float32 [{N}, 3, Hp, Wp] tensor on {device}, got {restored.dtype} "
                         f"{tuple(restored.shape)} on {restored.device}")
    Hp, Wp = int(restored.shape[2]), int(restored.shape[3])
    if len(wants) != N or (want_stats and (targets is None or len(targets) != N)):
        raise ValueError(f"{what}: {N} row(s) need {N} output choices" + (f" and {N} targets" if want_stats else ""))
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if not (1 <= h <= Hp and 1 <= w <= Wp):
            raise ValueError(f"{what}: row {i}: {h} x {w} is no crop of the {Hp} x {Wp} planes")
        if want_stats:
            _check_u8_row(what, i, "target", targets[i], device)
            if tuple(targets[i].shape[:2]) != (h, w):
                raise ValueError(f"{what}: row {i}: the target is {targets[i].shape[0]} x {targets[i].shape[1]}, the crop {h} x {w}")
        elif not wants[i]:
            raise ValueError(f"{what}: row {i}: neither an 8-bit output nor statistics were asked for")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)


def _loaded_hip_runtime() -> str:
    """path of the libamdhip64 this process has already mapped (torch's), so that dlopen hands back that instance; the bare soname
    when it cannot be told (then the loader's search order decides, which is the same file on a stock ROCm image)"""
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                if "libamdhip64" in ln:
                    return ln.split(None, 5)[5].strip()
    except (OSError, IndexError):
        pass
    return "libamdhip64.so"


class _Handover:
    """Stream-to-stream ordering on ONE device with events that carry no system-scope fence (hipEventDisableTiming |
    hipEventDisableSystemFence): `dst` waits for what `src` has enqueued so far.  The schedule hands work between its two streams
    ~400 times per iteration, and the stream that RECORDS pays for every hand-over: 4.2-6.6 us with torch's events (their release is
    system-scope: the L2 write-back a host or peer reader would need) against 2.5-4.2 us with these
    (scripts/micro/event_cost.py, profiles/r06_event_cost.txt).  Both sides are kernels of this process on this device, which a
    device-scope release orders; host reads go through torch's own synchronisation.  One event per hand-over SITE (it is re-recorded
    at every replay: a wait captures the event as it stands when the wait is enqueued)."""
    _hip = None
    FLAGS = 0x2 | 0x20000000         # hipEventDisableTiming | hipEventDisableSystemFence

    def __init__(self):
        cls = _Handover
        if cls._hip is None:
            cls._hip = C.CDLL(_loaded_hip_runtime())   # the HIP runtime torch has mapped: events and streams must come from ONE runtime
            cls._hip.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            cls._hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            cls._hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
            cls._hip.hipEventDestroy.argtypes = [C.c_void_p]
        self.ev = C.c_void_p()
        rc = cls._hip.hipEventCreateWithFlags(C.byref(self.ev), cls.FLAGS)
        if rc != 0:
            raise _lib.RcotKernelError(f"hipEventCreateWithFlags: HIP error {rc}")

    def record(self, src: int):
        rc = self._hip.hipEventRecord(self.ev, src)
        if rc != 0:
            raise _lib.RcotKernelError(f"hipEventRecord: HIP error {rc}")

    def wait(self, dst: int):
        rc = self._hip.hipStreamWaitEvent(dst, self.ev, 0)
        if rc != 0:
            raise _lib.RcotKernelError(f"hipStreamWaitEvent: HIP error {rc}")

    def __call__(self, src: int, dst: int):
        self.record(src)
        self.wait(dst)

    def __del__(self):
        try:
            # (not at interpreter shutdown: the HIP runtime may already be unloading, and the process is about to release everything)
            if self.ev and not sys.is_finalizing():
                self._hip.hipEventDestroy(self.ev)
        except Exception:
            pass

_DEFAULT = {}

#: arithmetic of the big MFMA products by name (include/rcot_hip.h RCOT_PREC_*): "fp32" exact fp32 MFMA; "bf16x3" two-term split,
#: three products (~2^-16 per product); "bf16x6" three-term split, six products: fp32-class results from the bf16 pipe (weight
#: projections on the producer / consumer kernel; everything else runs the exact-fp32 kernels)
PREC_BY_NAME = {"fp32": _lib.PREC_FP32, "bf16x3": _lib.PREC_BF16X3, "bf16x6": _lib.PREC_BF16X6, "bf16x1": _lib.PREC_BF16X1}
_TWO_TERM = (_lib.PREC_BF16X3, _lib.PREC_BF16X1)      # the arithmetics that run on the two-term split kernels and packs
#: ONE default for the product (HipBackend(), trainer.py --prec, bench.py --prec; RCOT_GEMM_PREC overrides): exact fp32, the
#: reference's arithmetic.  bf16x6 gives results as close to fp64 (tests/test_x3_gpu.py::test_x6_is_as_accurate_as_the_fp32_kernel;
#: every parity test holds the fp32 bars in it) 2 % faster end to end, bf16x3 results within the north_star tolerances 15 % faster.
DEFAULT_PREC = "fp32"
#: floats in each of HipBackend._ln_scratch's buffers: the deferred partial rows of one LayerNorm backward, rcot_ln_bwd_rows(B, C, N)
#: rows of 2 C floats (<= 1024 rows x 2 * 512 columns for every B <= 1024; tests/test_ln_forms_cpu.py holds the trainer's shapes to it)
LN_SCRATCH_FLOATS = 1024 * 1024


def default_backend():
    """One shared HipBackend (and workspace) per device for every network of the process."""
    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    if dev not in _DEFAULT:
        _DEFAULT[dev] = HipBackend()
    return _DEFAULT[dev]


class HipBackend:
    """Launches librcot_hip.so kernels.  One instance per device."""

    name = "hip"

    def __init__(self, device: Optional[torch.device] = None, workspace_bytes: int = 256 << 20):
        if not torch.cuda.is_available():
            raise _lib.RcotLibraryError("no HIP device visible: the RCOT hot path has no CPU fallback")
        self.L = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.ws = torch.empty(workspace_bytes // 4, dtype=torch.float32, device=self.device)
        self.ws_bytes = self.ws.numel() * 4
        # arithmetic of the big MFMA products (PREC_BY_NAME above).  RCOT_GEMM_PREC selects the process default (DEFAULT_PREC);
        # set ``backend.prec`` to switch at run time.
        self.prec = PREC_BY_NAME[os.environ.get("RCOT_GEMM_PREC", DEFAULT_PREC)]
        self._poison = os.environ.get("RCOT_POISON", "0") == "1"
        # weight-gradient overlap: leaf kernels of the backward sweep run on a second HIP stream (own split-K workspace)
        # while the data-gradient chain continues; RCOT_OVERLAP=0 keeps everything on one stream
        self.overlap = os.environ.get("RCOT_OVERLAP", "1") != "0"
        self._raw_events = os.environ.get("RCOT_RAW_EVENTS", "1") != "0"   # hand-overs between the two streams on fence-free HIP events (_Handover)
        self.attn_core_maxn = 4096         # largest plane rcot_attn_core_fwd is used on (it takes <= 65536; slower above 4096)
        self.ln_fused = True               # LN statistics made by the projection kernel
        self.prod_stats = True             # LayerNorm statistics made by the epilogue of the product that stores the tensor (round 6)
        self._ev_ring, self._ev_next = [], -1
        # networks built on this backend also keep the THREE-term weight packs of the bf16x6 arithmetic (1.5x the two-term packs,
        # refreshed with them after every optimizer step): on when that arithmetic is the process default
        self.x6_packs = self.prec == _lib.PREC_BF16X6
        self._side = torch.cuda.Stream(device=self.device) if self.overlap else None
        self._ws_side = torch.empty_like(self.ws) if self.overlap else None
        # split-K slabs of weight gradients that wait for block_param_reduce(): their own arena (self.ws is reused by every
        # split-K launch that follows on the same stream)
        # (two generations, like the LayerNorm scratch below: the launch that closes a block reads the slabs on the SIDE stream while
        # the main stream's paired data/weight-gradient launches of the next block already write the other generation)
        self._ws_slabs_gen = [torch.empty_like(self.ws), torch.empty_like(self.ws)]
        self._held = []
        self._pcm_cache = {}                     # padded-plane geometries, operand buffers and index tables of conv_pcm_*
        # entries whose device addresses are baked into recorded launch plans (touched while ``pcm_pinning`` is set: LaunchPlan.record
        # collects them in ``_pcm_touched``): key -> number of live plans that refer to it; _pcm_trim() never evicts them
        self._pcm_pinned = {}
        self._pcm_touched = set()
        self.pcm_pinning = False
        self._plan = None                        # the LaunchPlan being recorded on this backend (rcot_amd/plan.py), else None
        self._side_pending = False
        # deferred LayerNorm parameter-gradient partials of one block (<= 1024 rows x 2*512 columns each), in TWO generations:
        # the launch that closes a block (block_param_reduce) runs on the side stream behind that block's weight-gradient
        # kernels while the main stream is already in the next block, which therefore writes the other generation
        self._ln_scratch = [[torch.empty(LN_SCRATCH_FLOATS, dtype=torch.float32, device=self.device) for _ in range(2)] for _ in range(2)]
        self._ln_rows = 0
        self._gen = 0
        self._gen_event = [None, None]          # side-stream event after the reduce that read generation g
        self._held_gen = [[], []]               # tensors that reduce (and the side kernels before it) still read
        # Side-stream policy: the launch that closes a block (its parameter reduce) runs on the side stream under the next block in
        # bf16x6 only — fp32 77.06 -> 78.04 ms per iteration, bf16x6 73.03 -> 72.48, bf16x3 70.13 -> 70.71
        # (profiles/r06_ab_sched_nofence.txt; the earlier rounds' runs are in NOTES.md)
        self._defer_close_env = os.environ.get("RCOT_DEFER_CLOSE")
        # Early slab sums: the project_out / project_in weight-gradient slabs of a block are added up on the side stream right behind
        # the second of them (slab_sets_reduce), where that stream is idle, so that the closing launch reads the qkv set only.
        # Per iteration, off -> on, five alternating pairs each: fp32 73.31 -> 72.25 ms, bf16x6 70.89 -> 70.14, bf16x3 68.66 -> 68.58
        # (inside its 0.35 ms spread: off; its small planes make their slabs on the main stream anyway) — profiles/early_slab_sums.txt
        self._early_slabs_env = os.environ.get("RCOT_EARLY_SLABS")

    # ------------------------------------------------------------------ leaf-kernel overlap
    @property
    def defer_close(self):
        """the launch that closes a block runs on the side stream under the next block (policy above); RCOT_DEFER_CLOSE=0/1 overrides"""
        if self._defer_close_env is not None:
            return self._defer_close_env != "0"
        return self.prec == _lib.PREC_BF16X6

    @property
    def early_slab_sums(self):
        """the first two weight-gradient slab sets of a block are summed early on the side stream (policy above); RCOT_EARLY_SLABS=0/1 overrides"""
        if self._early_slabs_env is not None:
            return self._early_slabs_env != "0"
        return self.prec in (_lib.PREC_FP32, _lib.PREC_BF16X6)

    def side_run(self, fn, *hold):
        """Run ``fn`` (kernel launches that only READ ``hold`` tensors and WRITE parameter gradients) on the side
        stream, ordered after everything enqueued so far on the current stream.  ``hold`` stays referenced until
        side_join(), so the caching allocator cannot hand those blocks out while the side kernels are pending."""
        if not self.overlap:
            fn()
            return
        self._handover_to_side()
        ws = self.ws
        self.ws = self._ws_side
        try:
            with torch.cuda.stream(self._side):
                fn()
        finally:
            self.ws = ws
        self._held.extend(hold)
        self._side_pending = True

    def side_join(self):
        """The current stream waits for the side stream; the held tensors may be released afterwards."""
        if self._side_pending:
            self._handover_from_side()
            self._side_pending = False
        self._held.clear()
        for g in (0, 1):
            self._gen_event[g] = None
            self._held_gen[g].clear()

    def _new_handover(self):
        """an event for one hand-over site: owned by the launch plan being recorded (re-recorded at every replay), else the next of a
        ring that the eagerly walked schedule re-uses (a wait keeps the state the event had when the wait was enqueued)"""
        if self._plan is not None:
            return _Handover()
        if len(self._ev_ring) < 2048:
            self._ev_ring.append(_Handover())
            return self._ev_ring[-1]
        self._ev_next = (self._ev_next + 1) % len(self._ev_ring)
        return self._ev_ring[self._ev_next]

    def _handover_to_side(self):
        """the side stream waits for what the calling stream has enqueued so far"""
        if self._raw_events:
            h, side, dev = self._new_handover(), self._side.cuda_stream, self._dev_index
            self._host(lambda: h(_raw_stream(dev), side))
        else:
            self._host(lambda: self._side.wait_stream(torch.cuda.current_stream()))

    def _handover_from_side(self):
        """the calling stream waits for what the side stream has enqueued so far"""
        if self._raw_events:
            h, side, dev = self._new_handover(), self._side.cuda_stream, self._dev_index
            self._host(lambda: h(side, _raw_stream(dev)))
        else:
            self._host(lambda: torch.cuda.current_stream().wait_stream(self._side))

    def _host(self, fn):
        """a cross-stream wait / event of the schedule: runs now; while a launch plan is recorded (rcot_amd/plan.py) it is also kept,
        at this position, for every replay"""
        if self._plan is not None:
            self._plan.host_action(fn)
        else:
            fn()

    # ------------------------------------------------------------------ plumbing
    def empty(self, *shape):
        if self._poison:                           # RCOT_POISON=1 (debugging): reads of unwritten memory surface as NaN
            return torch.full(shape, float("nan"), dtype=torch.float32, device=self.device)
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def zeros(self, *shape):
        t = torch.empty(*shape, dtype=torch.float32, device=self.device)
        if t.numel():
            self.fill(t, 0.0)                      # (rcot_fill: no at::native launches from this package, construction included)
        return t

    def _st(self):
        # the raw hipStream_t of the calling thread's current stream on this device.  torch.cuda.current_stream().cuda_stream
        # builds a Stream object per call (device-index resolution, lazy-init checks): 3 400 calls per iteration were a quarter of
        # the host's enqueue time (scripts/host_profile.py)
        return _raw_stream(self._dev_index)

    @staticmethod
    def _chk(t: torch.Tensor, what: str):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise _lib.RcotKernelError(f"{what}: expected a float32 tensor on the HIP device")

    @staticmethod
    def _bcn(t: torch.Tensor, what: str):
        """View as [B, C, N] with unit pixel stride and dense channels; returns (B, C, N, batch_stride)."""
        if t.dim() == 4:
            B, Cc, H, W = t.shape
            N = H * W
            ok = t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == N
        else:
            B, Cc, N = t.shape
            ok = t.stride(2) == 1 and t.stride(1) == N
        if not ok:
            raise _lib.RcotKernelError(f"{what}: channel planes must be dense NCHW")
        return B, Cc, N, t.stride(0)

    # ------------------------------------------------------------------ K-major fast path
    @staticmethod
    def pack_shapes(Co: int, Ci: int):
        """Shapes of the (WT, WP) packs of a [Co, Ci] 1x1 weight (see rcot_pack_weight)."""
        r16, r4 = (lambda v: (v + 15) // 16 * 16), (lambda v: (v + 3) // 4 * 4)
        return (r16(Ci), r4(Co)), (r16(Co), r4(Ci))

    @staticmethod
    def fold_shapes(Co: int, Ci: int):
        """Shapes of the LN-fold pack of a [Co, Ci] 1x1 weight that follows a LayerNorm: (WTf, c12)."""
        r16, r4 = (lambda v: (v + 15) // 16 * 16), (lambda v: (v + 3) // 4 * 4)
        return (r16(Ci), r4(Co)), (2, r4(Co))

    @staticmethod
    def split_shapes(Co: int, Ci: int):
        """Sizes (in floats, 1-D) of the pre-split fragment packs of a [Co, Ci] 1x1 weight: (WTs and WTfs, WPs)."""
        c = lambda v, q: (v + q - 1) // q
        return (c(Ci, 16) * c(Co, 32) * 512,), (c(Co, 16) * c(Ci, 32) * 512,)

    @staticmethod
    def split6_shapes(Co: int, Ci: int):
        """the THREE-term form of split_shapes (bf16x6 arithmetic): 3 KiB records"""
        c = lambda v, q: (v + q - 1) // q
        return (c(Ci, 16) * c(Co, 32) * 768,), (c(Co, 16) * c(Ci, 32) * 768,)

    def pack_weight(self, W, WT, WP, fold=None, split=None, split6=None):
        """``fold`` = (ln_w, ln_b, WTf, c12): also write the LN-folded forward operand; ``split`` = (WTs, WPs, WTfs | None):
        also write the pre-split bf16 fragment packs of the bf16x3 producer / consumer kernel (rcot_pack_weight)."""
        Co, Ci = W.shape
        assert W.stride(1) == 1 and WT.is_contiguous() and WP.is_contiguous()
        assert (tuple(WT.shape), tuple(WP.shape)) == self.pack_shapes(Co, Ci)
        f = (None, None, None, None)
        if fold is not None:
            lnw, lnb, WTf, c12 = fold
            assert (tuple(WTf.shape), tuple(c12.shape)) == self.fold_shapes(Co, Ci) and WTf.is_contiguous() and c12.is_contiguous()
            f = (lnw.data_ptr(), lnb.data_ptr(), WTf.data_ptr(), c12.data_ptr())
        sp = (None, None, None)
        if split is not None:
            st_, sp_ = self.split_shapes(Co, Ci)
            assert tuple(split[0].shape) == st_ and tuple(split[1].shape) == sp_ and (split[2] is None or tuple(split[2].shape) == st_)
            sp = (split[0].data_ptr(), split[1].data_ptr(), _ptr(split[2]))
        s6 = (None, None, None)
        if split6 is not None:
            st6, sp6 = self.split6_shapes(Co, Ci)
            assert tuple(split6[0].shape) == st6 and tuple(split6[1].shape) == sp6 and (split6[2] is None or tuple(split6[2].shape) == st6)
            s6 = (split6[0].data_ptr(), split6[1].data_ptr(), _ptr(split6[2]))
        _lib.check(self.L.rcot_pack_weight(W.data_ptr(), W.stride(0), Co, Ci, WT.data_ptr(), WP.data_ptr(), *f, *sp, *s6, self._st()),
                   "rcot_pack_weight")

    def pack_table(self, items, prec=None):
        """Device descriptors for pack_weights(): items = [(W, WT, WP[, fold[, split[, split6]]]), ...] with fold = (ln_w, ln_b, WTf,
        c12) or None, split = (WTs, WPs, WTfs | None) or None, split6 likewise (pointers must stay valid).  ``prec``: leave out
        the fragment packs that arithmetic never reads (the two-term packs serve bf16x3 only, the three-term packs bf16x6 only) —
        a repack then writes a third (fp32) / half (bf16x3) of the bytes; None = every pack given."""
        rows, c2d, chunk = [], [], 0
        want3 = prec is None or prec in _TWO_TERM
        want6 = prec is None or prec == _lib.PREC_BF16X6
        # the LN-folded operand WTf and its row constants serve the split arithmetics (LayerNorm applied in the epilogue); the exact-fp32
        # kernel normalises the fragments in its loop and reads WT (round 6: a third of the repack's bytes for qkv / project_in less)
        want_fold = prec is None or prec != _lib.PREC_FP32
        r16, r4 = (lambda v: (v + 15) // 16 * 16), (lambda v: (v + 3) // 4 * 4)
        for d, item in enumerate(items):
            W, WT, WP = item[:3]
            fold = item[3] if len(item) > 3 and want_fold else None
            split = item[4] if len(item) > 4 and want3 else None
            split6 = item[5] if len(item) > 5 and want6 else None
            Co, Ci = W.shape
            assert W.stride(1) == 1 and (tuple(WT.shape), tuple(WP.shape)) == self.pack_shapes(Co, Ci)
            nt, np_ = r16(Ci) * r4(Co), r16(Co) * r4(Ci)
            fp = [0, 0, 0, 0]
            sp = [0, 0, 0]
            units = nt + np_
            if fold is not None:
                lnw, lnb, WTf, c12 = fold
                assert (tuple(WTf.shape), tuple(c12.shape)) == self.fold_shapes(Co, Ci)
                fp = [lnw.data_ptr(), lnb.data_ptr(), WTf.data_ptr(), c12.data_ptr()]
                units += nt
            if split is not None:
                (st_,), (sp_,) = self.split_shapes(Co, Ci)
                assert split[0].numel() == st_ and split[1].numel() == sp_ and (split[2] is None or fold is not None)
                sp = [split[0].data_ptr(), split[1].data_ptr(), 0 if split[2] is None else split[2].data_ptr()]
                units += st_ // 8 + sp_ // 8 + (st_ // 8 if split[2] is not None else 0)     # one unit per 32-byte record
            s6 = [0, 0, 0]
            if split6 is not None:
                (st6,), (sp6,) = self.split6_shapes(Co, Ci)
                assert split6[0].numel() == st6 and split6[1].numel() == sp6 and (split6[2] is None or fold is not None)
                s6 = [split6[0].data_ptr(), split6[1].data_ptr(), 0 if split6[2] is None else split6[2].data_ptr()]
                units += st6 // 12 + sp6 // 12 + (st6 // 12 if split6[2] is not None else 0)    # one unit per 48-byte record
            n = (units + 1023) // 1024 + ((r4(Co) + 63) // 64 if fold is not None else 0)
            rows.append([W.data_ptr(), W.stride(0), Co, Ci, WT.data_ptr(), WP.data_ptr(), chunk] + fp + sp + s6 + [0, 0, 0])
            c2d.extend([d] * n)
            chunk += n
        return (torch.tensor(rows, dtype=torch.int64, device=self.device),
                torch.tensor(c2d, dtype=torch.int32, device=self.device)), chunk

    def pack_weights(self, table, nchunks):
        _lib.check(self.L.rcot_pack_weights(table[0].data_ptr(), table[1].data_ptr(), nchunks, self._st()), "rcot_pack_weights")

    @staticmethod
    def kmajor_ok(N: int, K: int, a_rows: int) -> bool:
        return N % 64 == 0 and a_rows >= (K + 15) // 16 * 16

    @staticmethod
    def kmajor_worth(M: int, N: int, Z: int) -> bool:
        """The LDS-DMA kernel has no split-K: take it when its 128x128 or 64x64 tiling yields enough workgroups."""
        return N % 64 == 0 and ((M + 63) // 64) * (N // 64) * Z >= 128

    def gemm_kmajor(self, At, Bm, C, M: int, K: int, R=None, rowscale=None, ln: LN = None, beta: float = 0.0, fold=None,
                    split=None, ln_compute: bool = False):
        """C[zo,zi] (M x N) = A @ LN?(Bm) + rowscale*R + beta*C with A given transposed: At [Zo,Zi,rows>=ceil16(K),>=M]
        (rows >= K zero).  Bm: [Zo,Zi,K,N]; C/R: [Zo,Zi,M,N]; N % 128 == 0.  ``fold`` = (AtF, c12): the LN-folded
        operand (same view geometry as At) and its row constants, used by the bf16x3 kernel when ``ln`` is given;
        ``split``: the pre-split fragment pack of the operand that is multiplied (At, or AtF with ``ln``).
        ``ln_compute``: the (mu, rs) of ``ln`` are OUTPUTS made by the kernel; returns False (nothing launched) when the
        producer/consumer kernel does not take the shape — the caller then runs ln_stats and calls again without it."""
        Zo, Zi, Kb, N = Bm.shape
        assert Kb == K and C.shape[2] == M and At.stride(3) == 1 and Bm.stride(3) == 1 and C.stride(3) == 1
        r = (None, 0, 0, 0)
        if R is not None:
            assert R.stride(3) == 1 and tuple(R.shape) == tuple(C.shape)
            r = (R.data_ptr(), R.stride(2), R.stride(0), R.stride(1))
        s = (None, 0, 0)
        if rowscale is not None:
            assert rowscale.stride(2) == 1
            s = (rowscale.data_ptr(), rowscale.stride(0), rowscale.stride(1))
        mu = rs = lw = lb = None
        sLN = 0
        if ln is not None:
            mu, rs, lw, lb = ln
            sLN = mu.stride(0)
        AtF = c12 = None
        if fold is not None and ln is not None:
            AtF, c12 = fold
            assert tuple(AtF.stride()) == tuple(At.stride()) and c12.is_contiguous()
        rc = self.L.rcot_gemm_kmajor(At.data_ptr(), At.stride(2), At.stride(0), At.stride(1), At.shape[2],
                                     Bm.data_ptr(), Bm.stride(2), Bm.stride(0), Bm.stride(1),
                                     C.data_ptr(), C.stride(2), C.stride(0), C.stride(1),
                                     r[0], r[1], r[2], r[3], s[0], s[1], s[2],
                                     _ptr(mu), _ptr(rs), sLN, 1 if ln_compute else 0, _ptr(lw), _ptr(lb), _ptr(AtF), _ptr(c12),
                                     _ptr(split), Zo, Zi, M, N, K, beta, self.ws.data_ptr(), self.ws_bytes, self.prec, self._st())
        if ln_compute and rc == _lib.EUNSUPPORTED:
            return False
        _lib.check(rc, "rcot_gemm_kmajor")
        return True

    def stats_ok(self, M: int, N: int, B: int) -> bool:
        """gemm_kmajor_stats takes the shape: exact fp32, one row tile holds every channel of its pixels (rcot_gemm_kmajor_stats)"""
        return self.prod_stats and self.prec == _lib.PREC_FP32 and M <= 96 and N % 128 == 0 and self.kmajor_worth(M, N, B)

    def gemm_kmajor_stats(self, At, Bm, C, M: int, K: int, R, stats):
        """C[z] = A[z] Bm[z] + R[z] as gemm_kmajor (no LayerNorm prologue, Zi = 1) AND stats = (mu, rs) [Zo, N]: the WithBias-LayerNorm
        statistics of C over its M rows, from the product's own epilogue (rcot_gemm_kmajor_stats): the LayerNorm that follows needs
        no rcot_ln_stats launch and no statistics pass in its projection kernel."""
        Zo, Zi, Kb, N = Bm.shape
        assert Zi == 1 and Kb == K and C.shape[2] == M and At.stride(3) == 1 and Bm.stride(3) == 1 and C.stride(3) == 1
        r = (None, 0, 0, 0)
        if R is not None:
            assert R.stride(3) == 1 and tuple(R.shape) == tuple(C.shape)
            r = (R.data_ptr(), R.stride(2), R.stride(0), R.stride(1))
        mu, rs = stats
        assert tuple(mu.shape) == (Zo, N) and tuple(rs.shape) == (Zo, N) and mu.stride(1) == 1 and rs.stride(1) == 1 and mu.stride(0) == rs.stride(0)
        _lib.check(self.L.rcot_gemm_kmajor_stats(At.data_ptr(), At.stride(2), At.stride(0), At.stride(1), At.shape[2],
                                                 Bm.data_ptr(), Bm.stride(2), Bm.stride(0), Bm.stride(1),
                                                 C.data_ptr(), C.stride(2), C.stride(0), C.stride(1), r[0], r[1], r[2], r[3],
                                                 mu.data_ptr(), rs.data_ptr(), mu.stride(0), Zo, Zi, M, N, K, self._st()), "rcot_gemm_kmajor_stats")

    def gemm_kmajor_multi(self, items) -> bool:
        """Up to three independent plain products of gemm_kmajor from ONE launch (rcot_gemm_kmajor_multi): items =
        [(At, Bm, C, M, K, R | None, rowscale | None), ...] with the shapes gemm_kmajor takes and a common pixel count.  False (nothing
        launched) when the arithmetic in use runs these products on the split-bf16 kernel: the caller launches them one by one."""
        if self.prec in _TWO_TERM:
            return False
        arr = (_lib.KmajorDesc * len(items))()
        N = items[0][1].shape[3]
        for d, (At, Bm, Cc, M, K, R, rowscale) in zip(arr, items):
            Zo, Zi, Kb, n = Bm.shape
            assert Kb == K and n == N and Cc.shape[2] == M and At.stride(3) == 1 and Bm.stride(3) == 1 and Cc.stride(3) == 1
            d.At, d.lda, d.sAo, d.sAi, d.a_rows = At.data_ptr(), At.stride(2), At.stride(0), At.stride(1), At.shape[2]
            d.Bm, d.ldb, d.sBo, d.sBi = Bm.data_ptr(), Bm.stride(2), Bm.stride(0), Bm.stride(1)
            d.C, d.ldc, d.sCo, d.sCi = Cc.data_ptr(), Cc.stride(2), Cc.stride(0), Cc.stride(1)
            if R is not None:
                assert R.stride(3) == 1 and tuple(R.shape) == tuple(Cc.shape)
                d.R, d.ldr, d.sRo, d.sRi = R.data_ptr(), R.stride(2), R.stride(0), R.stride(1)
            if rowscale is not None:
                assert rowscale.stride(2) == 1
                d.rowscale, d.sSo, d.sSi = rowscale.data_ptr(), rowscale.stride(0), rowscale.stride(1)
            d.Zo, d.Zi, d.M, d.K = Zo, Zi, M, K
        rc = self.L.rcot_gemm_kmajor_multi(arr, len(items), N, self.prec, self._st())
        if rc == _lib.EUNSUPPORTED:
            return False
        _lib.check(rc, "rcot_gemm_kmajor_multi")
        return True

    @staticmethod
    def _bcn_z(t):
        """dense-plane [B,C,H,W] / [B,C,N] view -> [B,1,C,N] (no copy)"""
        if t.dim() == 4:
            t = t.view(t.shape[0], t.shape[1], t.shape[2] * t.shape[3])
        return t.unsqueeze(1)

    @staticmethod
    def _as_z(t, B):
        """[rows, ld] pack -> [B (broadcast), 1, rows, ld]"""
        return t.view(1, 1, *t.shape).expand(B, 1, -1, -1)

    def _split_of(self, packed):
        """the pre-split pack triple (WTs, WPs, WTfs) of ``packed`` that matches the arithmetic in use: the two-term packs for
        bf16x3, the three-term ones (fifth entry of the pack tuple) for bf16x6, None for exact fp32 / absent packs"""
        if self.prec == _lib.PREC_BF16X6:
            return packed[4] if len(packed) > 4 else None
        if self.prec in _TWO_TERM:
            return packed[3] if len(packed) > 3 else None
        return None

    # ------------------------------------------------------------------ 1x1 projections
    def conv1x1_fwd(self, W, X, Y, ln: LN = None, R=None, beta: float = 0.0, packed=None, ln_compute: bool = False, stats=None):
        """Y[b] = W @ LN?(X[b]) (+R[b]) (+beta*Y[b]);  W: [Co,Ci] view with unit inner stride.
        ``packed`` = (WT, WP[, (WTf, c12) | None[, (WTs, WPs, WTfs | None)]]) from pack_weight enables the K-major LDS-DMA
        kernels when N % 64 == 0.  ``ln_compute``: the (mu, rs) tensors of ``ln`` are not yet filled — the projection kernel
        makes them when it can (bf16x3 producer/consumer kernel, unsplit), otherwise ln_stats runs first.
        ``stats`` = (mu, rs) [B, N] (only where stats_ok() holds): the LayerNorm statistics of Y over its channels, made by the
        epilogue of this product (gemm_kmajor_stats)."""
        Co, Ci = W.shape
        B, ci, N, sX = self._bcn(X, "conv1x1_fwd X")
        _, co, _, sY = self._bcn(Y, "conv1x1_fwd Y")
        assert ci == Ci and co == Co and W.stride(1) == 1
        if stats is not None:
            assert ln is None and beta == 0.0 and packed is not None and self.stats_ok(Co, N, B)
            v = self._bcn_z
            return self.gemm_kmajor_stats(self._as_z(packed[0], B), v(X), v(Y), Co, Ci, None if R is None else v(R), stats)
        kmajor = packed is not None and self.kmajor_worth(Co, N, B)
        fold = split = None
        if kmajor:
            if ln is not None and len(packed) > 2 and packed[2] is not None:
                fold = (self._as_z(packed[2][0], B), packed[2][1])
            sp_ = self._split_of(packed)
            if sp_ is not None:
                split = sp_[0] if ln is None else (sp_[2] if fold is not None else None)
        if ln_compute:
            v = self._bcn_z
            made = False
            if self.ln_fused and kmajor:
                if self.prec == _lib.PREC_FP32:
                    # exact fp32: gemm_xx_kernel makes the statistics of its own pixel columns (ln_stats_kernel's arithmetic, bit-identical)
                    made = self.gemm_kmajor(self._as_z(packed[0], B), v(X), v(Y), Co, Ci, R=None if R is None else v(R), ln=ln, beta=beta,
                                            ln_compute=True)
                elif fold is not None and split is not None and Ci % 16 == 0:
                    made = self.gemm_kmajor(self._as_z(packed[0], B), v(X), v(Y), Co, Ci, R=None if R is None else v(R), ln=ln, beta=beta,
                                            fold=fold, split=split, ln_compute=True)
            if made:
                return
            self.ln_stats(X, ln[0], ln[1])
        if kmajor:
            v = self._bcn_z
            self.gemm_kmajor(self._as_z(packed[0], B), v(X), v(Y), Co, Ci, R=None if R is None else v(R), ln=ln,
                             beta=beta, fold=fold, split=split)
            return
        sR = 0
        if R is not None:
            _, cr, _, sR = self._bcn(R, "conv1x1_fwd R")
            assert cr == Co
        mu = rs = lw = lb = None
        if ln is not None:
            mu, rs, lw, lb = ln
        _lib.check(self.L.rcot_conv1x1_fwd(W.data_ptr(), W.stride(0), X.data_ptr(), sX, Y.data_ptr(), sY, B, Ci, Co, N,
                                           _ptr(mu), _ptr(rs), _ptr(lw), _ptr(lb), _ptr(R), sR, beta, self._st()),
                   "rcot_conv1x1_fwd")

    def conv1x1_dgrad(self, W, dY, dX, beta: float = 0.0, packed=None):
        Co, Ci = W.shape
        B, co, N, sdY = self._bcn(dY, "conv1x1_dgrad dY")
        _, ci, _, sdX = self._bcn(dX, "conv1x1_dgrad dX")
        assert ci == Ci and co == Co and W.stride(1) == 1
        if packed is not None and self.kmajor_worth(Ci, N, B):
            sp_ = self._split_of(packed)
            split = sp_[1] if sp_ is not None else None
            return self.gemm_kmajor(self._as_z(packed[1], B), self._bcn_z(dY), self._bcn_z(dX), Ci, Co, beta=beta, split=split)
        _lib.check(self.L.rcot_conv1x1_dgrad(W.data_ptr(), W.stride(0), dY.data_ptr(), sdY, dX.data_ptr(), sdX, B, Ci,
                                             Co, N, beta, self._st()), "rcot_conv1x1_dgrad")

    def conv1x1_wgrad(self, dY, X, dW, ln: LN = None, beta: float = 1.0):
        Co, Ci = dW.shape
        B, co, N, sdY = self._bcn(dY, "conv1x1_wgrad dY")
        _, ci, _, sX = self._bcn(X, "conv1x1_wgrad X")
        assert ci == Ci and co == Co and dW.stride(1) == 1
        mu = rs = lw = lb = None
        if ln is not None:
            mu, rs, lw, lb = ln
        _lib.check(self.L.rcot_conv1x1_wgrad(dY.data_ptr(), sdY, X.data_ptr(), sX, dW.data_ptr(), dW.stride(0), B, Ci,
                                             Co, N, _ptr(mu), _ptr(rs), _ptr(lw), _ptr(lb), beta, self.ws.data_ptr(),
                                             self.ws_bytes, self.prec, self._st()), "rcot_conv1x1_wgrad")

    def conv1x1_wgrad_slabs(self, dY, X, dW, ln: LN = None, region=(0, 1)):
        """The weight gradient of conv1x1_wgrad left as split-K slabs in part ``region`` = (index, count) of the slab arena; returns the descriptor block_param_reduce() takes (it adds the slabs to ``dW``), or None when the shape has
        no slab kernel (the caller then uses conv1x1_wgrad).  rcot_conv1x1_wgrad_slabs."""
        Co, Ci = dW.shape
        B, co, N, sdY = self._bcn(dY, "conv1x1_wgrad_slabs dY")
        _, ci, _, sX = self._bcn(X, "conv1x1_wgrad_slabs X")
        assert ci == Ci and co == Co and dW.stride(1) == 1
        mu = rs = lw = lb = None
        if ln is not None:
            mu, rs, lw, lb = ln
        idx, cnt = region
        self._gen_acquire()
        per = (self._ws_slabs.numel() // cnt) // 64 * 64
        ws = self._ws_slabs[idx * per:(idx + 1) * per]
        S, ld = C.c_int(0), C.c_int(0)
        rc = self.L.rcot_conv1x1_wgrad_slabs(dY.data_ptr(), sdY, X.data_ptr(), sX, B, Ci, Co, N, _ptr(mu), _ptr(rs), _ptr(lw),
                                             _ptr(lb), ws.data_ptr(), per * 4, self.prec, C.byref(S), C.byref(ld), self._st())
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc, "rcot_conv1x1_wgrad_slabs")
        return (ws.data_ptr(), S.value, Co, Ci, ld.value, dW.data_ptr(), dW.stride(0))

    def conv1x1_dgrad_wgrad_slabs(self, W, dY, dX, X, dW, ln: LN = None, packed=None, region=(0, 1)):
        """dX = W^T dY AND the weight gradient of the same dY left as split-K slabs (the descriptor of conv1x1_wgrad_slabs), from
        ONE launch (rcot_conv1x1_dgrad_wgrad_slabs, bf16x3 only).  None (nothing launched) when the shapes / the arithmetic have
        no paired kernel: the caller runs conv1x1_dgrad and conv1x1_wgrad_slabs / conv1x1_wgrad."""
        if self.prec != _lib.PREC_BF16X3 or packed is None or len(packed) < 4 or packed[3] is None:
            return None
        Co, Ci = W.shape
        B, co, N, sdY = self._bcn(dY, "conv1x1_dgrad_wgrad dY")
        _, ci, _, sdX = self._bcn(dX, "conv1x1_dgrad_wgrad dX")
        _, ci2, _, sX = self._bcn(X, "conv1x1_dgrad_wgrad X")
        assert ci == Ci and ci2 == Ci and co == Co and dW.stride(1) == 1 and tuple(dW.shape) == (Co, Ci)
        if not self.kmajor_worth(Ci, N, B):
            return None
        WP, WPs = packed[1], packed[3][1]
        mu = rs = lw = lb = None
        if ln is not None:
            mu, rs, lw, lb = ln
        idx, cnt = region
        self._gen_acquire()
        per = (self._ws_slabs.numel() // cnt) // 64 * 64
        ws = self._ws_slabs[idx * per:(idx + 1) * per]
        S, ld = C.c_int(0), C.c_int(0)
        rc = self.L.rcot_conv1x1_dgrad_wgrad_slabs(WP.data_ptr(), WP.stride(0), WPs.data_ptr(), dY.data_ptr(), sdY, dX.data_ptr(), sdX,
                                                   X.data_ptr(), sX, B, Ci, Co, N, _ptr(mu), _ptr(rs), _ptr(lw), _ptr(lb),
                                                   self.ws.data_ptr(), self.ws_bytes, ws.data_ptr(), per * 4, self.prec, C.byref(S),
                                                   C.byref(ld), self._st())
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc, "rcot_conv1x1_dgrad_wgrad_slabs")
        return (ws.data_ptr(), S.value, Co, Ci, ld.value, dW.data_ptr(), dW.stride(0))

    # ------------------------------------------------------------------ batched small-matrix products
    def bmm_nn(self, A, Bm, C, transA: bool = False, R=None, rowscale=None, beta: float = 0.0):
        """C[zo,zi] = op(A[zo,zi]) @ Bm[zo,zi] + rowscale[zo,zi,:,None]*R[zo,zi] + beta*C.
        A: [Zo,Zi,M,K] ([Zo,Zi,K,M] if transA); Bm: [Zo,Zi,K,N]; C/R: [Zo,Zi,M,N]; rowscale: [Zo,Zi,M]."""
        Zo, Zi, K, N = Bm.shape
        M = C.shape[2]
        assert A.stride(3) == 1 and Bm.stride(3) == 1 and C.stride(3) == 1
        assert tuple(A.shape[2:]) == ((K, M) if transA else (M, K))
        r = (None, 0, 0, 0)
        if R is not None:
            assert R.stride(3) == 1 and tuple(R.shape) == tuple(C.shape)
            r = (R.data_ptr(), R.stride(2), R.stride(0), R.stride(1))
        s = (None, 0, 0)
        if rowscale is not None:
            assert rowscale.stride(2) == 1
            s = (rowscale.data_ptr(), rowscale.stride(0), rowscale.stride(1))
        _lib.check(self.L.rcot_bmm_nn(A.data_ptr(), A.stride(2), A.stride(0), A.stride(1), int(transA),
                                      Bm.data_ptr(), Bm.stride(2), Bm.stride(0), Bm.stride(1),
                                      C.data_ptr(), C.stride(2), C.stride(0), C.stride(1),
                                      r[0], r[1], r[2], r[3], s[0], s[1], s[2],
                                      Zo, Zi, M, N, K, beta, self._st()), "rcot_bmm_nn")

    def bmm_nt(self, A, Bm, C):
        """C[zo,zi] (M x N) = A[zo,zi] (M x K) @ Bm[zo,zi]^T (N x K)."""
        Zo, Zi, M, K = A.shape
        N = Bm.shape[2]
        assert A.stride(3) == 1 and Bm.stride(3) == 1 and C.stride(3) == 1 and Bm.shape[3] == K
        _lib.check(self.L.rcot_bmm_nt(A.data_ptr(), A.stride(2), A.stride(0), A.stride(1),
                                      Bm.data_ptr(), Bm.stride(2), Bm.stride(0), Bm.stride(1),
                                      C.data_ptr(), C.stride(2), C.stride(0), C.stride(1),
                                      Zo, Zi, M, N, K, self.ws.data_ptr(), self.ws_bytes, self.prec, self._st()), "rcot_bmm_nt")

    def bmm_nt_slabs(self, A, Bm):
        """bmm_nt left as split-K slabs in the workspace: (pointer, S, ld) for attn_softmax(), or None when the shape has no slab
        kernel.  The slabs live until the next split-K launch on this stream: consume them with the very next call."""
        Zo, Zi, M, K = A.shape
        N = Bm.shape[2]
        assert A.stride(3) == 1 and Bm.stride(3) == 1 and Bm.shape[3] == K
        S, ld = C.c_int(0), C.c_int(0)
        rc = self.L.rcot_bmm_nt_slabs(A.data_ptr(), A.stride(2), A.stride(0), A.stride(1), Bm.data_ptr(), Bm.stride(2),
                                      Bm.stride(0), Bm.stride(1), Zo, Zi, M, N, K, self.ws.data_ptr(), self.ws_bytes, self.prec,
                                      C.byref(S), C.byref(ld), self._st())
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc, "rcot_bmm_nt_slabs")
        return (self.ws.data_ptr(), S.value, ld.value)

    # ------------------------------------------------------------------ Linear
    def linear_fwd(self, X, W, bias, Y, lrelu: float = 1.0):
        B, i = X.shape
        o = W.shape[0]
        assert X.is_contiguous() and W.is_contiguous() and Y.is_contiguous() and W.shape[1] == i
        _lib.check(self.L.rcot_linear_fwd(X.data_ptr(), W.data_ptr(), _ptr(bias), Y.data_ptr(), B, i, o, lrelu,
                                          self.ws.data_ptr(), self.ws_bytes, self._st()), "rcot_linear_fwd")

    def linear_dgrad(self, dY, W, dX):
        B, o = dY.shape
        i = W.shape[1]
        assert dY.is_contiguous() and W.is_contiguous() and dX.is_contiguous()
        _lib.check(self.L.rcot_linear_dgrad(dY.data_ptr(), W.data_ptr(), dX.data_ptr(), B, i, o, self.ws.data_ptr(),
                                            self.ws_bytes, self._st()), "rcot_linear_dgrad")

    def linear_wgrad(self, dY, X, dW, beta: float = 1.0):
        B, o = dY.shape
        i = X.shape[1]
        assert dY.is_contiguous() and X.is_contiguous() and dW.is_contiguous()
        _lib.check(self.L.rcot_linear_wgrad(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), B, i, o, beta, self._st()),
                   "rcot_linear_wgrad")

    # ------------------------------------------------------------------ dense convolutions
    def conv2d_fwd(self, X, Wt, bias, Y, stride: int, pad: int, lrelu: float = 1.0, cmap: int = 0, R=None, mask=None,
                   mslope: float = 1.0):
        """``mask`` (same shape as Y): the result is stored as ``mask > 0 ? y : y * mslope`` (lrelu_bwd folded into the store)"""
        B, Ci, H, W = X.shape
        Co, _, KH, KW = Wt.shape
        assert X.is_contiguous() and Wt.is_contiguous() and Y.is_contiguous() and (R is None or R.is_contiguous())
        assert mask is None or (mask.is_contiguous() and mask.shape == Y.shape)
        _lib.check(self.L.rcot_conv2d_fwd(X.data_ptr(), Wt.data_ptr(), _ptr(bias), Y.data_ptr(), B, Ci, H, W, Co, KH,
                                          KW, stride, pad, lrelu, cmap, _ptr(R), _ptr(mask), mslope, self.ws.data_ptr(),
                                          self.ws_bytes, self._st()), "rcot_conv2d_fwd")

    def conv2d_dgrad(self, dY, Wt, dX, stride: int, pad: int, beta: float = 0.0, mask=None, mslope: float = 1.0):
        """``mask`` (same shape as dX): dX is stored as ``mask > 0 ? dx : dx * mslope``"""
        B, Ci, H, W = dX.shape
        Co, _, KH, KW = Wt.shape
        assert dY.is_contiguous() and Wt.is_contiguous() and dX.is_contiguous()
        assert mask is None or (mask.is_contiguous() and mask.shape == dX.shape)
        _lib.check(self.L.rcot_conv2d_dgrad(dY.data_ptr(), Wt.data_ptr(), dX.data_ptr(), B, Ci, H, W, Co, KH, KW,
                                            stride, pad, beta, _ptr(mask), mslope, self.ws.data_ptr(), self.ws_bytes, self._st()),
                   "rcot_conv2d_dgrad")

    def conv2d_wgrad(self, dY, X, dWt, stride: int, pad: int, beta: float = 1.0):
        B, Ci, H, W = X.shape
        Co, _, KH, KW = dWt.shape
        assert dY.is_contiguous() and X.is_contiguous() and dWt.is_contiguous()
        _lib.check(self.L.rcot_conv2d_wgrad(dY.data_ptr(), X.data_ptr(), dWt.data_ptr(), B, Ci, H, W, Co, KH, KW,
                                            stride, pad, beta, self.ws.data_ptr(), self.ws_bytes, self._st()),
                   "rcot_conv2d_wgrad")

    # ------------------------------------------------------------------ k3s1 / k4s2 convolutions as bf16x3 K-major products
    @staticmethod
    def conv_pcm_ok(Ci: int, Co: int, k: int, s: int, pad: int, H: int, W: int) -> bool:
        """shapes rcot_conv_pcm takes (the critic's nine inner convolutions): forward and data gradient"""
        if (k, s, pad) == (3, 1, 1):
            return Ci % 16 == 0 and Co % 16 == 0 and W % 4 == 0
        if (k, s, pad) == (4, 2, 1):
            return Ci % 16 == 0 and Co % 16 == 0 and W % 8 == 0 and H % 2 == 0
        return False

    def _pcm_geom(self, B: int, Ho: int, Wo: int, Cd: int, Hd: int, Wd: int, kind: str):
        """Cached per geometry: N (GEMM columns), plane pitch, guard, and the colmap for a dense [B, Cd, Hd, Wd] result.
        kind 'same': result pixel (y, x) = plane position (y + 1, x + 4) (forward, k3 data gradient); 'planes': identity map."""
        key = (B, Ho, Wo, Cd, Hd, Wd, kind)
        g = self._pcm_get(key)
        if g is None:
            import numpy as np
            Wp, Hp = Wo + 8, Ho + 2
            Ps = Hp * Wp
            N = (B * Ps + 255) // 256 * 256
            G = (Wp + 8 + 3) // 4 * 4
            if kind == "planes":
                cm = np.arange(N // 4, dtype=np.int64) * 4
            else:
                n = np.arange(N // 4, dtype=np.int64) * 4
                b, r = n // Ps, n % Ps
                yp, xp = r // Wp, r % Wp
                ok = (b < B) & (yp >= 1) & (yp <= Hd) & (xp >= 4) & (xp < 4 + Wd)
                cm = np.where(ok, b * Cd * Hd * Wd + (yp - 1) * Wd + (xp - 4), -1)
            g = dict(N=N, Wp=Wp, Hp=Hp, Ps=Ps, G=G, colmap=torch.from_numpy(cm.astype(np.int32)).to(self.device), plane=(B, Ho, Wo))
            self._pcm_put(key, g)
        return g

    def _pcm_get(self, key):
        """cache lookup that refreshes the entry's age and notes it for the launch plan being recorded"""
        v = self._pcm_cache.pop(key, None)
        if v is not None:
            self._pcm_cache[key] = v                       # dict order = least recently used first
            if self.pcm_pinning:
                self._pcm_touched.add(key)
        return v

    def _pcm_put(self, key, v):
        if self._plan is not None:
            # a lazily created operand inside a recording would live in the plan's pool and its H2D copies / fills would not be
            # part of the recording: the eager warm-up pass of the same shape and arithmetic must have created it
            raise RuntimeError(f"padded-plane cache entry {key!r} created while a launch plan is being recorded "
                               "(the warm-up pass did not cover this configuration)")
        self._pcm_cache[key] = v
        if self.pcm_pinning:
            self._pcm_touched.add(key)

    def _pcm_trim(self):
        """Geometries, index tables and zeroed operand buffers are cached per shape; a validation folder with many image sizes
        must not grow that without bound.  Called only where no padded operand is pending (start of a forward / weight gradient).
        Evicts the least recently used entries, never one a live launch plan refers to (its address is baked into the recorded
        arguments: freeing it would let the allocator hand the memory to other tensors and later replays would write into them)."""
        if len(self._pcm_cache) <= 192 or self._plan is not None:
            return                                 # (never while a launch plan is being recorded: what the recording has touched so far
                                                   #  is pinned only when it succeeds — ADVICE r5)
        for key in [k for k in self._pcm_cache if k not in self._pcm_pinned and k not in self._pcm_touched]:
            if len(self._pcm_cache) <= 128:
                break
            del self._pcm_cache[key]

    def _pcm_buffer(self, rows: int, g, tag: str = ""):
        """zero-initialised [rows][N + 2 G] operand buffer of ONE plane geometry (B, Ho, Wo): rcot_conv_pcm_prep rewrites only the
        B plane images, so the guards and the tail [B*Ps, N) stay zero only as long as every user of a buffer shares the
        geometry — two geometries may round to the same N (a training level and a tall validation plane)."""
        key = ("buf" + tag, rows) + tuple(g["plane"])
        b = self._pcm_get(key)
        if b is None:
            b = torch.zeros(rows * (g["N"] + 2 * g["G"]) + 64, dtype=torch.float32, device=self.device)
            self._pcm_put(key, b)
        return b

    def conv_pcm_tables(self, Co: int, Ci: int, k: int, kind: str):
        """(rowoff, koff, M, K): A[m][kk] = W.flat[rowoff[m] + koff[kk]] for the operand orders of csrc/conv_pcm.hip.
        kind 'fwd': M = Co, kk = (tap, ci) [k4: (a, b, ij, ci)]; 'dgrad': M = Ci [k4: (ij, ci)], kk = (tap, co) [k4: (a, b, co)]."""
        key = ("tab", Co, Ci, k, kind)
        t = self._pcm_get(key)
        if t is None:
            import numpy as np
            T = k * k
            co, ci = np.arange(Co), np.arange(Ci)
            if k == 3 and kind == "fwd":
                rowoff = co * Ci * T
                koff = (np.arange(T)[:, None] + ci[None, :] * T).reshape(-1)                       # (tap, ci) -> ci*9 + tap
            elif k == 3:
                rowoff = ci * T
                koff = ((T - 1 - np.arange(T))[:, None] + co[None, :] * Ci * T).reshape(-1)        # (tap', co): flipped tap
            elif kind == "fwd":                                                                    # k4 s2: tap (a, b), parity (i, j)
                rowoff = co * Ci * T
                ab = np.array([[a, b] for a in range(2) for b in range(2)])
                ij = np.array([[i, j] for i in range(2) for j in range(2)])
                kk = (2 * ab[:, None, 0] + ij[None, :, 0]) * 4 + (2 * ab[:, None, 1] + ij[None, :, 1])     # [ab][ij] -> ky*4 + kx
                koff = (kk[:, :, None] + ci[None, None, :] * T).reshape(-1)
            else:
                ij = np.array([[i, j] for i in range(2) for j in range(2)])
                rowoff = ((ij[:, 0] * 4 + ij[:, 1])[:, None] + ci[None, :] * T).reshape(-1)       # (ij, ci)
                ab = np.array([[a, b] for a in range(2) for b in range(2)])
                koff = ((2 * ab[:, 0] * 4 + 2 * ab[:, 1])[:, None] + co[None, :] * Ci * T).reshape(-1)     # ((a, b), co)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
            t = (dev(rowoff), dev(koff), int(rowoff.size), int(koff.size))
            self._pcm_put(key, t)
        return t

    def conv_pcm_pack(self, Wt, kind: str, out=None):
        """pre-split pack of a conv weight [Co, Ci, k, k] in the operand order ``kind`` ('fwd' | 'dgrad')"""
        Co, Ci, k, _ = Wt.shape
        rowoff, koff, M, K = self.conv_pcm_tables(Co, Ci, k, kind)
        n = (K // 16) * ((M + 31) // 32) * 512
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.device)
        assert Wt.is_contiguous() and out.numel() == n
        _lib.check(self.L.rcot_conv_pcm_pack(Wt.data_ptr(), rowoff.data_ptr(), koff.data_ptr(), M, K, out.data_ptr(), self._st()),
                   "rcot_conv_pcm_pack")
        return out

    def _pcm_run(self, pack, M, K, buf, g, taps, bias, lrelu, cmap_g, Y, ldy):
        ldb = g["N"] + 2 * g["G"]
        arr = (C.c_int * len(taps))(*taps)
        _lib.check(self.L.rcot_conv_pcm(pack.data_ptr(), M, K, buf.data_ptr() + 4 * g["G"], ldb, g["N"], arr, len(taps), _ptr(bias),
                                        lrelu, cmap_g["colmap"].data_ptr(), Y.data_ptr(), ldy, self.ws.data_ptr(), self.ws_bytes,
                                        self._st()), "rcot_conv_pcm")

    def conv_pcm_fwd(self, X, pack, bias4, Y, k: int, lrelu: float = 1.0):
        """Y = lrelu(conv(X) + bias): k = 3 (s1 p1) or 4 (s2 p1); ``pack`` = conv_pcm_pack(W, 'fwd'); bias4: bias padded to a
        multiple of 4 entries (or None)."""
        B, Ci, H, W = X.shape
        Co, Ho, Wo = Y.shape[1], Y.shape[2], Y.shape[3]
        assert X.is_contiguous() and Y.is_contiguous()
        self._pcm_trim()
        g = self._pcm_geom(B, Ho, Wo, Co, Ho, Wo, "same")
        rows = Ci if k == 3 else 4 * Ci
        buf = self._pcm_buffer(rows, g)
        ldb = g["N"] + 2 * g["G"]
        _lib.check(self.L.rcot_conv_pcm_prep(X.data_ptr(), buf.data_ptr() + 4 * g["G"], ldb, B, Ci, H, W, 0 if k == 3 else 1, self._st()),
                   "rcot_conv_pcm_prep")
        Wp = g["Wp"]
        taps = [(ky - 1) * Wp + (kx - 1) for ky in range(3) for kx in range(3)] if k == 3 else [a * Wp + b for a in range(2) for b in range(2)]
        self._pcm_run(pack, Co, rows * len(taps), buf, g, taps, bias4, lrelu, g, Y, Ho * Wo)

    def conv_pcm_wgrad(self, dZ, X, dW, beta: float = 1.0):
        """dW = beta dW + 3x3 (s1 p1) weight gradient of dZ [B, Co, H, W] and X [B, Ci, H, W] as ONE pixel-reduction product over
        padded planes (rcot_conv_pcm_wgrad).  Leaves the padded copy of dZ in the buffer conv_pcm_dgrad(..., prepped=True)
        reads.  False (nothing launched) when the kernel does not take the shape."""
        B, Co, H, W = dZ.shape
        Ci = X.shape[1]
        assert dZ.is_contiguous() and X.is_contiguous() and dW.is_contiguous() and tuple(dW.shape) == (Co, Ci, 3, 3)
        self._pcm_trim()
        g = self._pcm_geom(B, H, W, Ci, H, W, "same")
        bz, bx = self._pcm_buffer(Co, g), self._pcm_buffer(Ci, g, "x")
        ldb = g["N"] + 2 * g["G"]
        _lib.check(self.L.rcot_conv_pcm_prep(dZ.data_ptr(), bz.data_ptr() + 4 * g["G"], ldb, B, Co, H, W, 0, self._st()), "rcot_conv_pcm_prep")
        _lib.check(self.L.rcot_conv_pcm_prep(X.data_ptr(), bx.data_ptr() + 4 * g["G"], ldb, B, Ci, H, W, 0, self._st()), "rcot_conv_pcm_prep")
        rc = self.L.rcot_conv_pcm_wgrad(bz.data_ptr() + 4 * g["G"], bx.data_ptr() + 4 * g["G"], ldb, g["N"], g["Wp"], Co, Ci, dW.data_ptr(),
                                        beta, self.ws.data_ptr(), self.ws_bytes, self.prec, self._st())
        if rc == _lib.EUNSUPPORTED:
            return False
        _lib.check(rc, "rcot_conv_pcm_wgrad")
        return True

    def conv_pcm_dgrad(self, dZ, pack, dX, k: int, prepped: bool = False):
        """dX = conv data gradient of dZ [B, Co, Ho, Wo]; ``pack`` = conv_pcm_pack(W, 'dgrad').  ``prepped`` (k = 3): the padded
        copy of dZ is already in its buffer (conv_pcm_wgrad of the same dZ ran just before)."""
        B, Co, Ho, Wo = dZ.shape
        Ci, H, W = dX.shape[1], dX.shape[2], dX.shape[3]
        assert dZ.is_contiguous() and dX.is_contiguous()
        if k == 3:
            g = self._pcm_geom(B, Ho, Wo, Ci, H, W, "same")
            buf = self._pcm_buffer(Co, g)
            ldb = g["N"] + 2 * g["G"]
            if not prepped:
                _lib.check(self.L.rcot_conv_pcm_prep(dZ.data_ptr(), buf.data_ptr() + 4 * g["G"], ldb, B, Co, Ho, Wo, 0, self._st()), "rcot_conv_pcm_prep")
            Wp = g["Wp"]
            taps = [-(ky - 1) * Wp - (kx - 1) for ky in range(3) for kx in range(3)]
            # the pack's tap order is flipped (t' = 8 - t reads W[..][8 - t']): tap slot t' carries the offset of kernel tap 8 - t'
            taps = taps[::-1]
            self._pcm_run(pack, Ci, Co * 9, buf, g, taps, None, 1.0, g, dX, H * W)
            return
        g = self._pcm_geom(B, Ho, Wo, Co, Ho, Wo, "same")              # geometry of dZ; results as parity planes in the same index space
        gp = self._pcm_geom(B, Ho, Wo, 0, 0, 0, "planes")
        buf = self._pcm_buffer(Co, g)
        ldb = g["N"] + 2 * g["G"]
        _lib.check(self.L.rcot_conv_pcm_prep(dZ.data_ptr(), buf.data_ptr() + 4 * g["G"], ldb, B, Co, Ho, Wo, 0, self._st()), "rcot_conv_pcm_prep")
        Wp = g["Wp"]
        taps = [-a * Wp - b for a in range(2) for b in range(2)]
        planes = self.empty(4 * Ci, g["N"])
        self._pcm_run(pack, 4 * Ci, 4 * Co, buf, g, taps, None, 1.0, gp, planes, g["N"])
        _lib.check(self.L.rcot_conv_pcm_merge(planes.data_ptr(), g["N"], dX.data_ptr(), B, Ci, H, W, self._st()), "rcot_conv_pcm_merge")

    def pixel_shuffle(self, inp, out, mode: int):
        """mode 1: PixelUnshuffle(2), mode 2: PixelShuffle(2); inp [B,C,H,W] contiguous."""
        B, Cc, H, W = inp.shape
        assert inp.is_contiguous() and out.is_contiguous()
        _lib.check(self.L.rcot_pixel_shuffle(inp.data_ptr(), out.data_ptr(), B * Cc, H, W, mode, self._st()),
                   "rcot_pixel_shuffle")

    # ------------------------------------------------------------------ LayerNorm
    def ln_stats(self, x, mu, rs):
        B, Cc, N, sx = self._bcn(x, "ln_stats x")
        assert sx == Cc * N
        _lib.check(self.L.rcot_ln_stats(x.data_ptr(), mu.data_ptr(), rs.data_ptr(), B, Cc, N, self._st()), "rcot_ln_stats")

    def ln_bwd(self, g, x, mu, rs, w, dres, dx, dw, db, slot=None):
        """``slot`` (0/1): leave the dw/db partial rows in the backend's LN scratch ``slot`` for block_param_reduce()."""
        B, Cc, N, sx = self._bcn(x, "ln_bwd x")
        assert sx == Cc * N and g.is_contiguous() and dx.is_contiguous() and (dres is None or dres.is_contiguous())
        if slot is None:
            ws, nb, dwp, dbp = self.ws, self.ws_bytes, dw.data_ptr(), db.data_ptr()
        else:
            gen = self._gen
            self._gen_acquire()
            sc = self._ln_scratch[gen][slot]
            ws, nb, dwp, dbp = sc, sc.numel() * 4, None, None
            self._ln_rows = int(self.L.rcot_ln_bwd_rows(B, Cc, N))
        _lib.check(self.L.rcot_ln_bwd(g.data_ptr(), x.data_ptr(), mu.data_ptr(), rs.data_ptr(), w.data_ptr(), _ptr(dres),
                                      dx.data_ptr(), dwp, dbp, B, Cc, N, ws.data_ptr(), nb, self._st()), "rcot_ln_bwd")

    @property
    def _ws_slabs(self):
        """the slab arena of the generation the block being swept writes"""
        return self._ws_slabs_gen[self._gen]

    def _gen_acquire(self):
        """before the calling stream writes the current generation of per-block scratch (LayerNorm partial rows, weight-gradient
        slabs): the deferred reduce that read this generation (two blocks ago, side stream) must have finished; what it held may be
        released — later allocations on this stream are ordered behind the wait"""
        gen = self._gen
        if self._gen_event[gen] is not None:
            if self._side is not None and torch.cuda.current_stream() == self._side:
                return                             # a writer ON the side stream is already ordered behind that reduce
            ev = self._gen_event[gen]
            if isinstance(ev, _Handover):
                dev = self._dev_index
                self._host(lambda: ev.wait(_raw_stream(dev)))
            else:
                self._host(lambda: torch.cuda.current_stream().wait_event(ev))
            self._gen_event[gen] = None
            self._held_gen[gen].clear()

    def slab_sets_reduce(self, slabs):
        """every descriptor of ``slabs`` (conv1x1_wgrad_slabs, at most 4): its weight gradient += the sum of its slabs, bit for bit what
        block_param_reduce() would add, on the current stream (rcot_slab_sets_reduce); nothing is launched for an empty list."""
        slabs = [d for d in slabs if d is not None]
        if not slabs:
            return
        rows = (ctypes_ll * (7 * len(slabs)))(*[v for d in slabs for v in d])
        _lib.check(self.L.rcot_slab_sets_reduce(rows, len(slabs), self._st()), "rcot_slab_sets_reduce")

    def block_param_reduce(self, C, gw1, gb1, gw2, gb2, dWo_part, gWo, dtemp_part, gtemp, slabs=(), close_block=False):
        """LN partials of scratch slot 0 -> (gw1, gb1), slot 1 -> (gw2, gb2); gWo += dWo_part.sum(0); gtemp += dtemp_part.sum(0);
        every descriptor of ``slabs`` (conv1x1_wgrad_slabs, at most 4): its weight gradient += the sum of its slabs.
        ``close_block``: this is the last launch of a transformer block's backward.  With the side stream on it is then enqueued
        THERE, behind the block's weight-gradient kernels (it only writes parameter gradients), and the calling stream goes on
        with the next block without waiting (side_join() before anything reads those gradients); otherwise the calling stream
        first waits for the side stream."""
        B, heads = dtemp_part.shape
        slabs = [d for d in slabs if d is not None]
        rows = (ctypes_ll * (7 * len(slabs)))(*[v for d in slabs for v in d]) if slabs else None
        g = self._gen
        sc0, sc1, ln_rows = self._ln_scratch[g][0], self._ln_scratch[g][1], self._ln_rows

        def launch():
            _lib.check(self.L.rcot_block_param_reduce(sc0.data_ptr(), sc1.data_ptr(), ln_rows, C,
                                                      gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(), gb2.data_ptr(),
                                                      dWo_part.data_ptr(), gWo.data_ptr(), dtemp_part.data_ptr(), gtemp.data_ptr(), B,
                                                      heads, rows, len(slabs), self._st()), "rcot_block_param_reduce")
        if close_block and self.overlap and self.defer_close:
            self._handover_to_side()
            with torch.cuda.stream(self._side):
                launch()
            if self._raw_events:
                ev, side = self._new_handover(), self._side.cuda_stream
                self._host(lambda: ev.record(side))
            else:
                ev = torch.cuda.Event()
                self._host(lambda: ev.record(self._side))
            self._gen_event[g] = ev
            self._held_gen[g] = self._held + [dWo_part, dtemp_part]
            self._held = []
            self._side_pending = True
            self._gen ^= 1
            return
        if close_block:
            self.side_join()
        launch()

    # ------------------------------------------------------------------ depthwise stencils
    def dwconv3x3(self, x, w, y, flip: bool = False):
        B, Cc, H, W = x.shape
        assert x.is_contiguous() and y.is_contiguous() and w.is_contiguous()
        _lib.check(self.L.rcot_dwconv3x3(x.data_ptr(), w.data_ptr(), y.data_ptr(), B, Cc, H, W, int(flip), self._st()),
                   "rcot_dwconv3x3")

    def gdfn_gate_fwd(self, p, w, g):
        B, c2, H, W = p.shape
        assert p.is_contiguous() and g.is_contiguous() and w.is_contiguous()
        _lib.check(self.L.rcot_gdfn_gate_fwd(p.data_ptr(), w.data_ptr(), g.data_ptr(), B, c2 // 2, H, W, self._st()),
                   "rcot_gdfn_gate_fwd")

    def gdfn_gate_bwd(self, p, w, dg, dd, dw=None):
        """dd from dg; with ``dw`` the depthwise weight gradient is accumulated in the same pass."""
        B, c2, H, W = p.shape
        assert p.is_contiguous() and dg.is_contiguous() and dd.is_contiguous() and (dw is None or dw.is_contiguous())
        _lib.check(self.L.rcot_gdfn_gate_bwd(p.data_ptr(), w.data_ptr(), dg.data_ptr(), dd.data_ptr(), _ptr(dw), B, c2 // 2,
                                             H, W, self._st()), "rcot_gdfn_gate_bwd")

    @staticmethod
    def gdfn_bwd_needs_scratch(H: int, W: int) -> bool:
        """True when rcot_gdfn_bwd cannot take its fused route for this plane size (mirrors the C dispatcher)."""
        wq = W // 4
        if wq > 64 or 64 % wq:
            return True
        for rs in (16, 8, 4):
            tpp = -(-H // rs) * wq
            if not (tpp % 256 == 0 or tpp % 64 == 0 or (tpp < 64 and tpp & (tpp - 1) == 0)):
                return True
        return False

    def gdfn_bwd(self, p, w, dg, dp, dw):
        """dp = dwconv3x3(gate backward of dg, w, flip) and dw += depthwise weight gradient, one pass (dd stays on chip)."""
        B, c2, H, W = p.shape
        assert p.is_contiguous() and dg.is_contiguous() and dp.is_contiguous() and dw.is_contiguous() and w.is_contiguous()
        scratch = self.empty(B, c2, H, W) if self.gdfn_bwd_needs_scratch(H, W) else None
        _lib.check(self.L.rcot_gdfn_bwd(p.data_ptr(), w.data_ptr(), dg.data_ptr(), dp.data_ptr(), dw.data_ptr(), _ptr(scratch), B,
                                        c2 // 2, H, W, self._st()), "rcot_gdfn_bwd")

    def dwconv3x3_bwd(self, dy, x, w, dx, dw):
        """dx = dwconv3x3(dy, w, flip) and dw += wgrad(dy, x) in one pass over dy."""
        B, Cc, H, W = x.shape
        assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and dw.is_contiguous() and w.is_contiguous()
        _lib.check(self.L.rcot_dwconv3x3_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), dw.data_ptr(), B, Cc, H, W,
                                             self._st()), "rcot_dwconv3x3_bwd")

    def dwconv3x3_wgrad(self, dy, x, dw):
        B, Cc, H, W = x.shape
        assert dy.is_contiguous() and x.is_contiguous() and dw.is_contiguous()
        _lib.check(self.L.rcot_dwconv3x3_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Cc, H, W, self._st()),
                   "rcot_dwconv3x3_wgrad")

    # ------------------------------------------------------------------ MDTA small-matrix core
    def row_sumsq(self, x, out):
        """x: [B,R,N] view (dense rows); out: [B,R] contiguous."""
        B, R, N, sx = self._bcn(x, "row_sumsq x")
        assert out.is_contiguous()
        _lib.check(self.L.rcot_row_sumsq(x.data_ptr(), out.data_ptr(), B, R, N, sx, self._st()), "rcot_row_sumsq")

    def attn_softmax(self, Graw, sq, temp, Gn, A):
        """``Graw``: the Gram tensor [B, heads, c, c], or the slab descriptor of bmm_nt_slabs()."""
        B, heads, c, _ = Gn.shape
        for t in (sq, temp, Gn, A):
            assert t.is_contiguous()
        if isinstance(Graw, tuple):
            gp, S, ld = Graw
        else:
            assert Graw.is_contiguous() and tuple(Graw.shape) == tuple(Gn.shape)
            gp, S, ld = Graw.data_ptr(), 0, c
        _lib.check(self.L.rcot_attn_softmax(gp, S, ld, sq.data_ptr(), temp.data_ptr(), Gn.data_ptr(), A.data_ptr(),
                                            B, heads, c, self._st()), "rcot_attn_softmax")

    def attn_core_fwd(self, u, temp, WoT, sq, Gn, A, MfT) -> bool:
        """sq, Gn, A and the folded operand MfT = (W_o blockdiag(A))^T straight from u = [q | k | v] (rcot_attn_core_fwd: the
        64x64 / 32x32 / 16x16 levels).  False when the shape has no such kernel: the caller runs the four separate launches."""
        B, heads, c, _ = Gn.shape
        N = u.shape[2] * u.shape[3]
        if N > self.attn_core_maxn:
            return False
        for t in (u, temp, sq, Gn, A, MfT):
            assert t.is_contiguous()
        assert WoT.stride(1) == 1 and tuple(MfT.shape) == (B, heads * c, heads * c) and u.shape[1] == 3 * heads * c
        rc = self.L.rcot_attn_core_fwd(u.data_ptr(), u.stride(0), temp.data_ptr(), WoT.data_ptr(), WoT.stride(0), sq.data_ptr(),
                                       Gn.data_ptr(), A.data_ptr(), MfT.data_ptr(), MfT.stride(1), MfT.stride(0), B, heads, c, N,
                                       self.ws.data_ptr(), self.ws_bytes, self._st())
        if rc == _lib.EUNSUPPORTED:
            return False
        _lib.check(rc, "rcot_attn_core_fwd")
        return True

    def attn_bwd_small(self, dA, A, Gn, sq, temp, dtemp_part, Eq, EqT, Dq, Dk):
        B, heads, c, _ = A.shape
        for t in (dA, A, Gn, sq, temp, dtemp_part, Eq, EqT, Dq, Dk):
            assert t.is_contiguous()
        _lib.check(self.L.rcot_attn_bwd_small(dA.data_ptr(), A.data_ptr(), Gn.data_ptr(), sq.data_ptr(), temp.data_ptr(),
                                              dtemp_part.data_ptr(), Eq.data_ptr(), EqT.data_ptr(), Dq.data_ptr(), Dk.data_ptr(), B, heads,
                                              c, self._st()), "rcot_attn_bwd_small")

    # "auto": the measured rule of attn_rows_route(); "on" / "off": every head width / none (tests and scripts/bench_attn_rows.py
    # compare the two forms through this wrapper)
    attn_rows = "auto"
    # planes up to this many pixels hand dM = dY V^T to the row-group form as the split-K slabs of the product (no reduce launch).
    # A wavefront adds the slabs of its 16 rows alone, four loads deep: fine for the 4 .. 16 slabs of a reduction over <= 1024 pixels
    # (rcot_bmm_nt_slabs splits at most K / 64 ways), not for the 64 of the 64x64 and 128x128 planes (attn_rows_kernel<6> 32.9 us with
    # 64 slabs at 128x128) — there the reduce launch (4.3 - 4.9 us on a thousand workgroups) stays
    attn_rows_slab_maxn = 1024

    def attn_rows_route(self, c: int, heads: int) -> bool:
        """Whether attn_core_bwd() takes the row-group form (rcot_attn_rows_bwd: row groups on many workgroups + a c x c tail) for
        this head width and count; TransformerBlockOp.backward then hands dM over as the slabs of bmm_nt_slabs."""
        if c not in (24, 48, 96) or (heads * c) % 16:                   # (what rcot_attn_rows_bwd refuses)
            return False
        if self.attn_rows != "auto":
            return self.attn_rows == "on"
        # Measured at B = 8, exact fp32 (profiles/attn_rows_bwd.txt; kernels behind their own dM product / one block backward from a
        # launch plan, us, old -> row groups):
        #   c = 96, 1 head,  128x128:  50.9 -> 30.2   /  998 -> 984      c = 96, 4 heads, 16x16:  92.4 -> 33.6   /  358 -> 300
        #   c = 48, 2 heads, 64x64:    20.6 -> 14.8   /  331 -> 327      c = 48, 4 heads, 32x32:  22.9 -> 12.3   /  294 -> 280
        #   c = 48, 8 heads, 16x16:    34.3 -> 18.4   /  301 -> 287      c = 48, 1 head,  128x128: 17.6 -> 14.1  /  452 -> 452
        # c = 96 always.  c = 48 from two heads on: with one head (C = 48, the 128x128 encoder / decoder level) the three row tiles
        # are ONE row group — the same 8 workgroups as the one-launch form plus a second launch, nothing in the block.  c = 24
        # (two block applications per step) was not measured: it stays on the one-launch form.
        return c == 96 or (c == 48 and heads >= 2)

    def attn_core_bwd(self, dM, Wo, A, Gn, sq, temp, Mf, dWo_part, dtemp_part, Eq, EqT, Dq, Dk) -> bool:
        """Mf = W_o blockdiag(A), the per-image dW_o and the outputs of attn_bwd_small, from rcot_attn_rows_bwd (two launches on
        many workgroups) where attn_rows_route() says so, else in ONE launch (rcot_attn_core_bwd).  ``dM``: the dense [B, C, C]
        tensor or the slab descriptor (pointer, S, ld) of bmm_nt_slabs (any S for the row-group form, S <= 8 for the one-launch
        form).  False when neither takes the shape: the caller runs the three products and attn_bwd_small."""
        B, heads, c, _ = A.shape
        for t in (Wo, A, Gn, sq, temp, Mf, dWo_part, dtemp_part, Eq, EqT, Dq, Dk):
            assert t.is_contiguous()
        if isinstance(dM, tuple):
            dp, S, ld = dM
        else:
            assert dM.is_contiguous()
            dp, S, ld = dM.data_ptr(), 0, heads * c
        if self.attn_rows_route(c, heads):
            # the row-group form (rcot_attn_rows_bwd): its partial dA blocks go into this stream's workspace BEHIND the slabs of dM
            # where those lie in it (both are dead once the call's second launch has run; the side stream has a workspace of its own)
            C_ = heads * c
            ws0, used = self.ws.data_ptr(), 0
            if S > 0 and ws0 <= dp < ws0 + self.ws_bytes:
                used = -(-(dp - ws0 + 4 * B * S * C_ * ld) // 256) * 256
            rc = self.L.rcot_attn_rows_bwd(dp, S, ld, Wo.data_ptr(), A.data_ptr(), Gn.data_ptr(), sq.data_ptr(), temp.data_ptr(),
                                           Mf.data_ptr(), dWo_part.data_ptr(), dtemp_part.data_ptr(), Eq.data_ptr(), EqT.data_ptr(),
                                           Dq.data_ptr(), Dk.data_ptr(), B, heads, c, 0, ws0 + used, max(self.ws_bytes - used, 0),
                                           self._st())
            if rc == _lib.EUNSUPPORTED:
                return False
            _lib.check(rc, "rcot_attn_rows_bwd")
            return True
        if S > 8:
            return False
        rc = self.L.rcot_attn_core_bwd(dp, S, ld, Wo.data_ptr(), A.data_ptr(), Gn.data_ptr(), sq.data_ptr(), temp.data_ptr(),
                                       Mf.data_ptr(), dWo_part.data_ptr(), dtemp_part.data_ptr(), Eq.data_ptr(), EqT.data_ptr(),
                                       Dq.data_ptr(), Dk.data_ptr(), B, heads, c, self._st())
        if rc == _lib.EUNSUPPORTED:
            return False
        _lib.check(rc, "rcot_attn_core_bwd")
        return True

    def batch_reduce(self, src, dst, beta: float = 1.0):
        """dst = beta*dst + src.sum(0); src: [B, ...] contiguous."""
        B = src.shape[0]
        assert src.is_contiguous() and dst.is_contiguous() and src.numel() == B * dst.numel()
        _lib.check(self.L.rcot_batch_reduce(src.data_ptr(), dst.data_ptr(), B, dst.numel(), beta, self._st()),
                   "rcot_batch_reduce")

    # ------------------------------------------------------------------ elementwise / critic pieces
    def lrelu_bwd(self, dy, a, dz, slope: float = 0.2):
        assert dy.is_contiguous() and a.is_contiguous() and dz.is_contiguous()
        _lib.check(self.L.rcot_lrelu_bwd(dy.data_ptr(), a.data_ptr(), dz.data_ptr(), dy.numel(), slope, self._st()),
                   "rcot_lrelu_bwd")

    def bias_grad(self, dz, db):
        """db[c] += sum over batch and pixels of dz [B,C,...]."""
        B, Cc = dz.shape[0], dz.shape[1]
        assert dz.is_contiguous()
        _lib.check(self.L.rcot_bias_grad(dz.data_ptr(), db.data_ptr(), B, Cc, dz.numel() // (B * Cc), self._st()),
                   "rcot_bias_grad")

    def axpby(self, x, y, out, a: float = 1.0, b: float = 1.0):
        """out = a*x + b*y on [rows, cols]-like tensors: dim 0 may be strided, the rest must be dense."""
        def rc(t):
            rows = t.shape[0]
            cols = t.numel() // rows
            assert t[0].is_contiguous()
            return rows, cols, (t.stride(0) if rows > 1 else cols)
        rows, cols, sx = rc(x)
        _, _, so = rc(out)
        sy = 0
        if y is not None:
            _, _, sy = rc(y)
            assert y.shape == x.shape
        assert out.shape == x.shape
        _lib.check(self.L.rcot_axpby2d(x.data_ptr(), sx, _ptr(y), sy, out.data_ptr(), so, rows, cols, a, b, self._st()),
                   "rcot_axpby2d")

    def fill(self, t, v: float = 0.0):
        """t[...] = v for a dense fp32 tensor / view (rcot_fill): loss seeds and gradient-buffer zeroing without a PyTorch launch"""
        assert t.is_contiguous() and t.dtype == torch.float32
        if t.numel():
            _lib.check(self.L.rcot_fill(t.data_ptr(), t.numel(), float(v), self._st()), "rcot_fill")

    # ------------------------------------------------------------------ MPRNet backbone pieces (csrc/mprnet_ops.hip; Net.py:19-176)
    def prelu_fwd(self, x, slope, y):
        """y = x > 0 ? x : slope x with the ONE device-resident slope of nn.PReLU() (Net.py:185)"""
        assert x.is_contiguous() and y.is_contiguous() and slope.numel() == 1
        _lib.check(self.L.rcot_prelu_fwd(x.data_ptr(), slope.data_ptr(), y.data_ptr(), x.numel(), self._st()), "rcot_prelu_fwd")

    def prelu_bwd(self, dy, x, slope, dx, dslope):
        """dx = x > 0 ? dy : slope dy (dx may alias dy); dslope[0] += sum_{x <= 0} x dy"""
        assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and slope.numel() == 1 and dslope.numel() == 1
        _lib.check(self.L.rcot_prelu_bwd(dy.data_ptr(), x.data_ptr(), slope.data_ptr(), dx.data_ptr(), dslope.data_ptr(), x.numel(),
                                         self.ws.data_ptr(), self.ws_bytes, self._st()), "rcot_prelu_bwd")

    def row_dot(self, a, b, out, scale: float = 1.0):
        """out[b, c] = scale * sum over the plane of a * (b or 1); a, b: [B, C, H, W] dense"""
        rows = a.shape[0] * a.shape[1]
        assert a.is_contiguous() and (b is None or (b.is_contiguous() and b.shape == a.shape)) and out.is_contiguous() and out.numel() == rows
        _lib.check(self.L.rcot_row_dot(a.data_ptr(), _ptr(b), out.data_ptr(), rows, a.numel() // rows, float(scale), self._st()),
                   "rcot_row_dot")

    def row_scale_add(self, a, s, x, t, tscale: float, out):
        """out = a * s[b, c] + (x or 0) + (t[b, c] * tscale or 0); out may alias a or x"""
        rows = a.shape[0] * a.shape[1]
        assert a.is_contiguous() and out.is_contiguous() and out.shape == a.shape and s.is_contiguous() and s.numel() == rows
        assert (x is None or (x.is_contiguous() and x.shape == a.shape)) and (t is None or (t.is_contiguous() and t.numel() == rows))
        _lib.check(self.L.rcot_row_scale_add(a.data_ptr(), s.data_ptr(), _ptr(x), _ptr(t), float(tscale), out.data_ptr(), rows,
                                             a.numel() // rows, self._st()), "rcot_row_scale_add")

    def ca_gate_fwd(self, mean, W1, W2, hid, gate):
        """CALayer.conv_du on pooled means [B, C]: hid = relu(W1 mean), gate = sigmoid(W2 hid) (Net.py:42-47)"""
        B, Cc = mean.shape
        Cr = W1.shape[0]
        assert all(t.is_contiguous() for t in (mean, W1, W2, hid, gate)) and W1.numel() == Cr * Cc == W2.numel()
        _lib.check(self.L.rcot_ca_gate_fwd(mean.data_ptr(), W1.data_ptr(), W2.data_ptr(), hid.data_ptr(), gate.data_ptr(), B, Cc, Cr,
                                           self._st()), "rcot_ca_gate_fwd")

    def ca_gate_bwd(self, dgate, gate, hid, mean, W1, W2, dW1, dW2, dmean):
        B, Cc = mean.shape
        Cr = W1.shape[0]
        assert all(t.is_contiguous() for t in (dgate, gate, hid, mean, W1, W2, dW1, dW2, dmean))
        _lib.check(self.L.rcot_ca_gate_bwd(dgate.data_ptr(), gate.data_ptr(), hid.data_ptr(), mean.data_ptr(), W1.data_ptr(),
                                           W2.data_ptr(), dW1.data_ptr(), dW2.data_ptr(), dmean.data_ptr(), B, Cc, Cr, self.ws.data_ptr(),
                                           self.ws_bytes, self._st()),
                   "rcot_ca_gate_bwd")

    def bilinear_down2(self, x, y):
        """nn.Upsample(scale_factor=0.5, bilinear, align_corners=False): [B, C, H, W] -> [B, C, H/2, W/2] (Net.py:149)"""
        B, Cc, H, W = x.shape
        assert x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (B, Cc, H // 2, W // 2)
        _lib.check(self.L.rcot_bilinear_down2(x.data_ptr(), y.data_ptr(), B * Cc, H, W, self._st()), "rcot_bilinear_down2")

    def bilinear_down2_bwd(self, dy, dx, beta: float = 0.0):
        B, Cc, H, W = dx.shape
        assert dy.is_contiguous() and dx.is_contiguous() and tuple(dy.shape) == (B, Cc, H // 2, W // 2)
        _lib.check(self.L.rcot_bilinear_down2_bwd(dy.data_ptr(), dx.data_ptr(), B * Cc, H, W, float(beta), self._st()),
                   "rcot_bilinear_down2_bwd")

    def bilinear_up2(self, x, skip, y):
        """y [B, C, 2H, 2W] = nn.Upsample(scale_factor=2, bilinear, align_corners=False)(x) + (skip or 0) (Net.py:167-176)"""
        B, Cc, H, W = x.shape
        assert x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (B, Cc, 2 * H, 2 * W)
        assert skip is None or (skip.is_contiguous() and skip.shape == y.shape)
        _lib.check(self.L.rcot_bilinear_up2(x.data_ptr(), _ptr(skip), y.data_ptr(), B * Cc, H, W, self._st()), "rcot_bilinear_up2")

    def bilinear_up2_bwd(self, dy, dx):
        B, Cc, H, W = dx.shape
        assert dy.is_contiguous() and dx.is_contiguous() and tuple(dy.shape) == (B, Cc, 2 * H, 2 * W)
        _lib.check(self.L.rcot_bilinear_up2_bwd(dy.data_ptr(), dx.data_ptr(), B * Cc, H, W, self._st()), "rcot_bilinear_up2_bwd")

    def conv_weight_flip(self, src, dst, table, n: int, Co: int, Ci: int, K: int):
        """dst[.. ci, co, K-1-ky, K-1-kx] = src[.. co, ci, ky, kx] for the n weights whose element offsets the DEVICE int64 table
        lists (pairs: in src, in dst): the operand with which rcot_conv2d_fwd computes a stride-1 data gradient"""
        assert src.is_contiguous() and dst.is_contiguous() and table.dtype == torch.int64 and table.numel() == 2 * n
        _lib.check(self.L.rcot_conv_weight_flip(src.data_ptr(), dst.data_ptr(), table.data_ptr(), n, Co, Ci, K, K, self._st()),
                   "rcot_conv_weight_flip")

    def lerp(self, t, f, alpha, out):
        B = t.shape[0]
        assert t.is_contiguous() and f.is_contiguous() and out.is_contiguous() and alpha.is_contiguous()
        _lib.check(self.L.rcot_lerp(t.data_ptr(), f.data_ptr(), alpha.data_ptr(), out.data_ptr(), B, t.numel() // B,
                                    self._st()), "rcot_lerp")

    def gp_penalty(self, g, norms, u0, gp_out, inv_global_batch: float):
        B = g.shape[0]
        assert g.is_contiguous() and u0.is_contiguous()
        _lib.check(self.L.rcot_gp_penalty(g.data_ptr(), norms.data_ptr(), u0.data_ptr(), gp_out.data_ptr(), B,
                                          g.numel() // B, inv_global_batch, self._st()), "rcot_gp_penalty")

    # ------------------------------------------------------------------ OT cost
    def ot_reduce(self, degraded, restored, target, sums):
        B = degraded.shape[0]
        assert degraded.is_contiguous() and restored.is_contiguous() and (target is None or target.is_contiguous())
        _lib.check(self.L.rcot_ot_reduce(degraded.data_ptr(), restored.data_ptr(), _ptr(target), sums.data_ptr(), B,
                                         degraded.numel() // B, self._st()), "rcot_ot_reduce")

    def ot_spectrum(self, degraded, restored, de_id, gF, spec):
        B, _, H, W = degraded.shape
        assert de_id.dtype == torch.int32 and de_id.is_cuda
        rc = self.L.rcot_ot_spectrum(degraded.data_ptr(), restored.data_ptr(), de_id.data_ptr(), gF.data_ptr(),
                                     spec.data_ptr(), self.ws.data_ptr(), self.ws_bytes, B, H, W, self._st())
        if rc == _lib.EUNSUPPORTED:
            raise _lib.RcotKernelError(f"rcot_ot_spectrum: H = {H}, W = {W}: the line FFT of the L1-spectrum OT cost takes "
                                       f"lengths up to 1024 per axis (rcot_fft_plan)")
        _lib.check(rc, "rcot_ot_spectrum")

    def ot_grad(self, degraded, restored, target, de_id, gF, sums, spec, dout, scal, sigma, Sigma, global_batch):
        B = degraded.shape[0]
        assert de_id.dtype == torch.int32 and dout.is_contiguous()
        _lib.check(self.L.rcot_ot_grad(degraded.data_ptr(), restored.data_ptr(), _ptr(target), de_id.data_ptr(),
                                       _ptr(gF), sums.data_ptr(), spec.data_ptr(), dout.data_ptr(), scal.data_ptr(), B,
                                       degraded.numel() // B, sigma, Sigma, global_batch, self._st()), "rcot_ot_grad")

    # ------------------------------------------------------------------ data contract
    def patch_prep(self, clean_img, deg_img, y0: int, x0: int, P: int, mode: int, sigma: float, seed: int, deg_out, clean_out):
        """clean_img / deg_img: uint8 [H, W, 3] on the device (deg_img None -> synthetic noise of ``sigma``); writes the
        [3, P, P] float slots of the batch tensors (rcot_patch_prep)."""
        H, W, _ = clean_img.shape
        assert clean_img.dtype == torch.uint8 and clean_img.is_contiguous() and clean_img.is_cuda
        assert deg_img is None or (deg_img.dtype == torch.uint8 and deg_img.is_contiguous() and tuple(deg_img.shape) == (H, W, 3))
        assert deg_out.is_contiguous() and clean_out.is_contiguous() and tuple(deg_out.shape) == (3, P, P)
        _lib.check(self.L.rcot_patch_prep(_ptr(deg_img), clean_img.data_ptr(), H, W, y0, x0, P, mode, float(sigma),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, deg_out.data_ptr(), clean_out.data_ptr(), self._st()),
                   "rcot_patch_prep")

    def patch_prep_batch(self, rows, P: int, deg_out, clean_out):
        """``rows``: one ``(clean_img, deg_img | None, y0, x0, mode, sigma, seed)`` per sample, the images uint8 [H, W, 3] resident on
        the device (any sizes; None -> synthetic noise of ``sigma``); writes ``deg_out`` / ``clean_out`` [len(rows), 3, P, P] in ONE
        launch, row b with the bits ``patch_prep`` gives (rcot_patch_prep_batch).  Every row is checked on the host first
        (``check_patch_rows``: ValueError, nothing launched); the table travels in one pinned host tensor, one copy on the current
        stream."""
        assert self._plan is None                                          # loader launches stay outside recorded launch plans
        check_patch_rows(rows, P, deg_out, clean_out)
        flat = []
        for clean_img, deg_img, y0, x0, mode, sigma, seed in rows:
            s = int(seed) & 0xFFFFFFFFFFFFFFFF
            flat += [clean_img.data_ptr(), 0 if deg_img is None else deg_img.data_ptr(), int(clean_img.shape[1]), int(y0), int(x0),
                     int(mode), struct.unpack("<I", struct.pack("<f", float(sigma)))[0], s - (1 << 64) if s >> 63 else s]
        # (pinned: the copy is asynchronous, and torch's host allocator keeps the block until the copy has run)
        table = torch.tensor(flat, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
        _lib.check(self.L.rcot_patch_prep_batch(table.data_ptr(), len(rows), int(P), deg_out.data_ptr(), clean_out.data_ptr(),
                                                self._st()), "rcot_patch_prep_batch")

    # ------------------------------------------------------------------ whole-image validation at any size (csrc/imageio.hip)
    PAD_MODES = {None: 0, "none": 0, "reflect": 1, "replicate": 2}

    def _u8_image(self, t, what: str, h: Optional[int] = None, w: Optional[int] = None):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[2] != 3:
            raise _lib.RcotKernelError(f"{what}: expected a contiguous uint8 [h, w, 3] image on the HIP device")
        if h is not None and tuple(t.shape[:2]) != (h, w):
            raise _lib.RcotKernelError(f"{what}: expected {h} x {w} pixels, got {t.shape[0]} x {t.shape[1]}")

    def _dense_planes(self, t, what: str):
        self._chk(t, what)
        if t.dim() < 2 or not t.is_contiguous():
            raise _lib.RcotKernelError(f"{what}: planes must be dense [..., H, W]")

    def image_ingest(self, img, Hp: int, Wp: int, mode, out=None):
        """img uint8 [h, w, 3] on the device -> float [1, 3, Hp, Wp] = img / 255 in CHW, padded bottom / right by ``mode``
        ("none" | "reflect" | "replicate"): the bits of F.pad(img.permute(2, 0, 1).float().div(255)[None], ...) (rcot_image_ingest)"""
        self._u8_image(img, "image_ingest")
        h, w, _ = img.shape
        if out is None:
            out = self.empty(1, 3, Hp, Wp)
        self._dense_planes(out, "image_ingest")
        if out.numel() != 3 * Hp * Wp:
            raise _lib.RcotKernelError("image_ingest: out must hold [3, Hp, Wp] floats")
        _lib.check(self.L.rcot_image_ingest(img.data_ptr(), h, w, out.data_ptr(), Hp, Wp, self.PAD_MODES[mode], self._st()),
                   "rcot_image_ingest")
        return out

    def pad2d(self, x, Hp: int, Wp: int, mode, out=None):
        """x float [..., h, w] (dense) -> [..., Hp, Wp], padded bottom / right by ``mode``: the bits of F.pad (rcot_pad2d)"""
        self._dense_planes(x, "pad2d")
        h, w = x.shape[-2:]
        planes = x.numel() // (h * w) if h * w else 0
        if out is None:
            out = self.empty(*x.shape[:-2], Hp, Wp)
        self._dense_planes(out, "pad2d")
        if tuple(out.shape) != (*x.shape[:-2], Hp, Wp):
            raise _lib.RcotKernelError("pad2d: out must be [..., Hp, Wp] with the leading dimensions of x")
        _lib.check(self.L.rcot_pad2d(x.data_ptr(), out.data_ptr(), planes, h, w, Hp, Wp, self.PAD_MODES[mode], self._st()), "rcot_pad2d")
        return out

    def image_egress(self, restored, h: int, w: int, degraded=None, target=None, res_scale: float = 2.0, want_out: bool = True,
                     want_res: bool = False, want_stats: bool = False, ws=None):
        """restored float [(1,) 3, Hp, Wp] -> (out_u8, res_u8, stats): the h x w crop quantised to uint8 [h, w, 3] as ``trainer.save_image``
        does, the same for (degraded - restored) * res_scale, and the float64 [4] statistics against ``target`` (uint8 [h, w, 3]) that
        ``wholeimage.image_metrics`` turns into PSNR / SSIM.  Whatever is not asked for is None.  One launch, two with statistics
        (per-workgroup partials in ``ws``, default the backend's workspace, then a fixed-order sum): rcot_image_egress."""
        self._dense_planes(restored, "image_egress")
        if restored.numel() != 3 * restored.shape[-2] * restored.shape[-1]:
            raise _lib.RcotKernelError("image_egress: restored must be one image, [3, Hp, Wp]")
        Hp, Wp = restored.shape[-2:]
        if want_res:
            if degraded is None:
                raise _lib.RcotKernelError("image_egress: the residual needs the degraded image")
            self._dense_planes(degraded, "image_egress")
            if degraded.numel() != restored.numel() or tuple(degraded.shape[-2:]) != (Hp, Wp):
                raise _lib.RcotKernelError("image_egress: degraded and restored differ in shape")
        if want_stats:
            if target is None:
                raise _lib.RcotKernelError("image_egress: the statistics need the target image")
            self._u8_image(target, "image_egress", h, w)
        ws = self.ws if ws is None else ws
        out_u8 = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device) if want_out else None
        res_u8 = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device) if want_res else None
        stats = torch.empty(4, dtype=torch.float64, device=self.device) if want_stats else None
        _lib.check(self.L.rcot_image_egress(restored.data_ptr(), _ptr(degraded if want_res else None), _ptr(target if want_stats else None),
                                            h, w, Hp, Wp, float(res_scale), _ptr(out_u8), _ptr(res_u8), _ptr(stats), ws.data_ptr(),
                                            ws.numel() * ws.element_size(), self._st()), "rcot_image_egress")
        return out_u8, res_u8, stats

    def _device_table(self, flat):
        # (pinned: the copy is asynchronous, and torch's host allocator keeps the block until the copy has run)
        return torch.tensor(flat, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)

    def image_ingest_batch(self, imgs, Hp: int, Wp: int, mode, out=None):
        """``imgs``: N uint8 [h, w, 3] images on the device (any byte address: views into an arena of packed images are fine), each of
        a size ``mode`` pads to Hp x Wp -> float [N, 3, Hp, Wp] in ONE launch, slot i with the bits ``image_ingest`` gives
        (rcot_image_ingest_batch).  Every row is checked on the host first (``check_ingest_rows``: ValueError, nothing launched); the
        table travels in one pinned host tensor, one copy on the current stream."""
        assert self._plan is None
        if out is None:
            check_ingest_rows(imgs, Hp, Wp, mode, None, self.device)
            out = self.empty(len(imgs), 3, Hp, Wp)
        check_ingest_rows(imgs, Hp, Wp, mode, out, self.device)
        flat = []
        for t in imgs:
            flat += [t.data_ptr(), int(t.shape[0]), int(t.shape[1]), 0]
        table = self._device_table(flat)
        _lib.check(self.L.rcot_image_ingest_batch(table.data_ptr(), len(imgs), int(Hp), int(Wp), self.PAD_MODES[mode], out.data_ptr(),
                                                  self._st()), "rcot_image_ingest_batch")
        return out

    EGRESS_TILE = (4, 256)                         # ROWS x TILE of csrc/imageio.hip: pixels of one workgroup

    @classmethod
    def image_egress_batch_ws_bytes(cls, N: int, Hp: int, Wp: int) -> int:
        """workspace bytes rcot_image_egress_batch needs for statistics (include/rcot_hip.h): 24 per workgroup of the Hp x Wp grid, per image"""
        th, tw = cls.EGRESS_TILE
        return 24 * int(N) * (-(-int(Hp) // th)) * (-(-int(Wp) // tw))

    def image_egress_batch(self, restored, sizes, targets=None, want_out=True, want_stats: bool = False, ws=None, outs=None, stats=None):
        """restored float [N, 3, Hp, Wp]; ``sizes``: N (h, w); ``targets``: N uint8 [h, w, 3] images (needed for statistics) ->
        (outs, stats): ``outs`` a list of N uint8 [h, w, 3] crops quantised as ``image_egress`` does (``want_out``: a bool, or one bool
        per image; None where not asked for) and ``stats`` float64 [N, 4] or None — row i bit for bit what ``image_egress`` gives for
        image i.  Two launches, one without statistics (rcot_image_egress_batch).  The rows are checked on the host first
        (``check_egress_rows``: ValueError, nothing launched).  ``outs`` (a list of uint8 [h, w, 3] tensors or None per image, at any
        byte address; replaces ``want_out``) and ``stats`` (float64 [N, 4]): the caller's own tensors instead of new ones."""
        assert self._plan is None
        N = len(sizes)
        if outs is not None:
            wants = [o is not None for o in outs]
        else:
            wants = [bool(want_out)] * N if isinstance(want_out, bool) else [bool(v) for v in want_out]
        want_stats = want_stats or stats is not None
        check_egress_rows(restored, sizes, targets, wants, want_stats, self.device)
        Hp, Wp = int(restored.shape[-2]), int(restored.shape[-1])
        if outs is None:
            outs = [torch.empty(h, w, 3, dtype=torch.uint8, device=self.device) if wo else None for (h, w), wo in zip(sizes, wants)]
        for i, ((h, w), o) in enumerate(zip(sizes, outs)):
            if o is not None:
                _check_u8_row("image_egress_batch", i, "8-bit output", o, self.device)
                if tuple(o.shape[:2]) != (int(h), int(w)):
                    raise ValueError(f"image_egress_batch: row {i}: the 8-bit output is {o.shape[0]} x {o.shape[1]}, the crop {h} x {w}")
        flat = []
        for i, (h, w) in enumerate(sizes):
            flat += [targets[i].data_ptr() if want_stats else 0, 0 if outs[i] is None else outs[i].data_ptr(), int(h), int(w)]
        table = self._device_table(flat)
        ws = self.ws if ws is None else ws
        if want_stats and stats is None:
            stats = torch.empty(N, 4, dtype=torch.float64, device=self.device)
        if stats is not None and (stats.dtype != torch.float64 or not stats.is_contiguous() or stats.numel() != 4 * N or stats.device != self.device):
            raise ValueError(f"image_egress_batch: stats must be a contiguous float64 [{N}, 4] tensor on {self.device}")
        _lib.check(self.L.rcot_image_egress_batch(restored.data_ptr(), table.data_ptr(), N, Hp, Wp, _ptr(stats), ws.data_ptr(),
                                                  ws.numel() * ws.element_size(), self._st()), "rcot_image_egress_batch")
        return outs, stats

    # ------------------------------------------------------------------ views and their blend: tiles, self-ensemble (csrc/views.hip)
    def _view_args(self, img, ys, xs, modes, Th: int, Tw: int, what: str):
        self._dense_planes(img, what)
        H, W = img.shape[-2:]
        planes = img.numel() // (H * W) if H * W else 0
        arr = lambda v: (C.c_int * len(v))(*[int(a) for a in v])
        return planes, H, W, arr(ys), len(ys), arr(xs), len(xs), arr(modes), len(modes), int(Th), int(Tw)

    def view_gather(self, img, ys, xs, modes, Th: int, Tw: int, out=None):
        """img float [..., H, W] (dense) -> float [len(modes) * len(ys) * len(xs), planes * Th * Tw]: view (k, iy, ix) is the Th x Tw
        window at (ys[iy], xs[ix]) under the dihedral map modes[k] (numpy's data_augmentation), [planes, Th, Tw] for modes 0, 1, 4, 5 and
        [planes, Tw, Th] for 2, 3, 6, 7 (rcot_view_gather)"""
        a = self._view_args(img, ys, xs, modes, Th, Tw, "view_gather")
        n, per = len(modes) * len(ys) * len(xs), a[0] * int(Th) * int(Tw)
        if out is None:
            out = self.empty(n, per)
        self._dense_planes(out, "view_gather")
        if out.numel() != n * per:
            raise _lib.RcotKernelError(f"view_gather: out must hold {n} views of {per} floats")
        _lib.check(self.L.rcot_view_gather(img.data_ptr(), *a, out.data_ptr(), self._st()), "rcot_view_gather")
        return out

    def view_blend(self, views, H: int, W: int, ys, xs, modes, Th: int, Tw: int, wy=None, wx=None, out=None):
        """views as ``view_gather`` lays them out (after the network) -> float [planes, H, W]: every pixel is the mean of the view
        elements mapped onto it, weighted by wy[i] * wx[j] at window position (i, j) (float [Th] / [Tw] on the device; both None: equal
        weights), summed in ascending view order (rcot_view_blend)"""
        self._dense_planes(views, "view_blend")
        n, vplane = len(modes) * len(ys) * len(xs), int(Th) * int(Tw)
        if out is None:
            if n < 1 or vplane < 1 or views.numel() % (n * vplane):
                raise _lib.RcotKernelError(f"view_blend: views must hold {n} views of whole {Th} x {Tw} planes")
            out = self.empty(views.numel() // (n * vplane), H, W)
        self._dense_planes(out, "view_blend")
        if tuple(out.shape[-2:]) != (H, W):
            raise _lib.RcotKernelError(f"view_blend: out must be [..., {H}, {W}]")
        a = self._view_args(out, ys, xs, modes, Th, Tw, "view_blend")
        if views.numel() != n * a[0] * vplane:
            raise _lib.RcotKernelError(f"view_blend: views must hold {n} views of {a[0]} planes of {Th} x {Tw}")
        for t, length in ((wy, Th), (wx, Tw)):
            if t is not None:
                self._chk(t, "view_blend")
                if not t.is_contiguous() or t.numel() != length:
                    raise _lib.RcotKernelError("view_blend: the taps must be dense float [Th] and [Tw]")
        _lib.check(self.L.rcot_view_blend(views.data_ptr(), *a, _ptr(wy), _ptr(wx), out.data_ptr(), self._st()), "rcot_view_blend")
        return out

    # ------------------------------------------------------------------ MATLAB-rule bicubic resize, one axis per launch (csrc/resize.hip)
    def resize_axis(self, src, axis: int, idx, taps, out=None):
        """src float [..., H, W] (dense) -> [..., out_len, W] (axis 0) or [..., H, out_len] (axis 1): out = sum_k taps[o, k] *
        src[idx[o, k]] along the axis, in fp32, k ascending (rcot_resize_axis).  idx int32 / taps float32 [out_len, K] on the device,
        as ``rcot_amd.resize.cubic_taps`` makes them."""
        self._dense_planes(src, "resize_axis")
        self._chk(taps, "resize_axis")
        if idx.dtype != torch.int32 or not idx.is_cuda or idx.dim() != 2 or tuple(idx.shape) != tuple(taps.shape) or \
                not idx.is_contiguous() or not taps.is_contiguous():
            raise _lib.RcotKernelError("resize_axis: idx (int32) and taps (float32) must be dense [out_len, K] tables on the HIP device")
        H, W = src.shape[-2:]
        planes = src.numel() // (H * W) if H * W else 0
        out_len, K = idx.shape
        shape = (*src.shape[:-2], out_len, W) if axis == 0 else (*src.shape[:-2], H, out_len)
        if out is None:
            out = self.empty(*shape)
        self._dense_planes(out, "resize_axis")
        if tuple(out.shape) != shape:
            raise _lib.RcotKernelError(f"resize_axis: out must be {shape}")
        _lib.check(self.L.rcot_resize_axis(src.data_ptr(), out.data_ptr(), planes, H, W, int(axis), out_len, idx.data_ptr(),
                                           taps.data_ptr(), K, self._st()), "rcot_resize_axis")
        return out

    # ------------------------------------------------------------------ baseline JPEG round trip (csrc/jpeg.hip)
    def jpeg_ws_bytes(self, h: int, w: int, subsampling: int) -> int:
        """workspace bytes rcot_jpeg_roundtrip needs (0 for 4:4:4); RcotKernelError for a geometry it refuses"""
        n = self.L.rcot_jpeg_ws_bytes(int(h), int(w), int(subsampling))
        _lib.check(min(n, 0), "rcot_jpeg_ws_bytes")
        return n

    def jpeg_roundtrip(self, img_u8, quality: int, subsampling: int = 2, out=None, ws=None):
        """img_u8 uint8 [h, w, 3] on the device -> uint8 [h, w, 3]: the image after a baseline JPEG round trip at ``quality`` (1 .. 100)
        with ``subsampling`` 0 (4:4:4, one launch) or 2 (4:2:0, two launches through ``ws``, default the backend's workspace) — the bytes
        Pillow on libjpeg-turbo holds after saving and loading it (rcot_jpeg_roundtrip)"""
        self._u8_image(img_u8, "jpeg_roundtrip")
        h, w, _ = img_u8.shape
        if out is None:
            out = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device)
        self._u8_image(out, "jpeg_roundtrip", h, w)
        ws = self.ws if ws is None else ws
        _lib.check(self.L.rcot_jpeg_roundtrip(img_u8.data_ptr(), out.data_ptr(), h, w, int(quality), int(subsampling), ws.data_ptr(),
                                              ws.numel() * ws.element_size(), self._st()), "rcot_jpeg_roundtrip")
        return out

    # ------------------------------------------------------------------ per-image PSF blur (csrc/blur.hip)
    def blur_u8(self, img_u8, psf_dev, border: int, step: int = 1, phase: int = 0, out=None):
        """img_u8 uint8 [h, w, 3] on the device -> uint8 [h / step, w / step, 3]: every channel correlated with ``psf_dev`` (int32 [K, K]
        on the device, K odd, weights >= 0 that sum to 2^22: rcot_amd.blur.device_psf) under the border rule ``border`` (0 replicate,
        1 mirror, 2 wrap), sampled at (oy step + phase, ox step + phase) (rcot_blur_u8: one launch, no workspace)"""
        self._u8_image(img_u8, "blur_u8")
        if psf_dev.dtype != torch.int32 or not psf_dev.is_cuda or not psf_dev.is_contiguous() or psf_dev.dim() != 2 \
                or psf_dev.shape[0] != psf_dev.shape[1]:
            raise _lib.RcotKernelError("blur_u8: the PSF must be a contiguous int32 [K, K] tensor on the HIP device")
        h, w, _ = img_u8.shape
        step, phase = int(step), int(phase)
        if step < 1 or h % step or w % step:
            raise _lib.RcotKernelError(f"blur_u8: invalid argument: {h} x {w} pixels are not multiples of the step {step}")
        if out is None:
            out = torch.empty(h // step, w // step, 3, dtype=torch.uint8, device=self.device)
        self._u8_image(out, "blur_u8", h // step, w // step)
        _lib.check(self.L.rcot_blur_u8(img_u8.data_ptr(), out.data_ptr(), h, w, psf_dev.data_ptr(), int(psf_dev.shape[0]), int(border),
                                       step, phase, self._st()), "rcot_blur_u8")
        return out

    # ------------------------------------------------------------------ whole-image noise (csrc/noise.hip)
    NOISE_MODELS = {"g": 0, "gray": 1, "pg": 2}

    def noise_u8(self, img_u8, model: str, p0: float, p1: float, seed: int, out=None):
        """img_u8 uint8 [h, w, 3] on the device -> uint8 [h, w, 3]: clip(v + s z, 0, 255) truncated, z a counter-based normal deviate of
        ``seed``; ``model`` "g" (s = p0, a deviate per byte), "gray" (s = p0, one deviate per pixel) or "pg" (s = sqrt(p0 v + p1^2)).
        ``out`` may be ``img_u8`` itself (rcot_noise_u8: one launch, no workspace)"""
        self._u8_image(img_u8, "noise_u8")
        if model not in self.NOISE_MODELS:
            raise _lib.RcotKernelError(f"noise_u8: invalid argument: model {model!r}, expected one of {tuple(self.NOISE_MODELS)}")
        h, w, _ = img_u8.shape
        if out is None:
            out = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device)
        self._u8_image(out, "noise_u8", h, w)
        _lib.check(self.L.rcot_noise_u8(img_u8.data_ptr(), out.data_ptr(), h, w, self.NOISE_MODELS[model], float(p0), float(p1),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, self._st()), "rcot_noise_u8")
        return out

    # ------------------------------------------------------------------ standard image-quality figures (csrc/quality.hip)
    WINDOWS ={"uniform7": 0, "gauss11": 1}
    SPACES = {"rgb": 0, "y": 1}
    QUALITY_TILE = (16, 32)                        # TH x TW of csrc/quality.hip: map positions of one workgroup

    @classmethod
    def image_quality_ws_bytes(cls, h: int, w: int, space: str) -> int:
        """workspace bytes rcot_image_quality needs (include/rcot_hip.h): 16 per workgroup, one workgroup per tile and plane"""
        th, tw = cls.QUALITY_TILE
        return 16 * (3 if space == "rgb" else 1) * (-(-h // th)) * (-(-w // tw))

    def image_quality(self, a_u8, b_u8, window: str, space: str, ws=None):
        """a_u8, b_u8 uint8 [h, w, 3] on the device -> float64 [4]: the exact squared-error sum over the planes of ``space`` ("rgb" | "y")
        and its element count, the sum of the SSIM map of ``window`` ("uniform7" | "gauss11") and its position count — what
        ``quality.quality_metrics`` turns into PSNR / SSIM.  Two launches (per-workgroup partials in ``ws``, default the backend's
        workspace, then a fixed-order sum): rcot_image_quality."""
        self._u8_image(a_u8, "image_quality")
        h, w, _ = a_u8.shape
        self._u8_image(b_u8, "image_quality", h, w)
        if window not in self.WINDOWS:
            raise _lib.RcotKernelError(f"image_quality: invalid argument: window {window!r}, expected one of {tuple(self.WINDOWS)}")
        if space not in self.SPACES:
            raise _lib.RcotKernelError(f"image_quality: invalid argument: color space {space!r}, expected one of {tuple(self.SPACES)}")
        ws = self.ws if ws is None else ws
        stats = torch.empty(4, dtype=torch.float64, device=self.device)
        _lib.check(self.L.rcot_image_quality(a_u8.data_ptr(), b_u8.data_ptr(), h, w, self.WINDOWS[window], self.SPACES[space],
                                             stats.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), self._st()),
                   "rcot_image_quality")
        return stats

    BLOCKINESS_TILE = (32, 63)                     # BTH x BTW of csrc/quality.hip: pixels of one workgroup

    @classmethod
    def image_blockiness_ws_bytes(cls, h: int, w: int, space: str) -> int:
        """workspace bytes rcot_image_blockiness needs (include/rcot_hip.h): 40 per workgroup and plane, one workgroup per tile"""
        th, tw = cls.BLOCKINESS_TILE
        return 40 * (3 if space == "rgb" else 1) * (-(-h // th)) * (-(-w // tw))

    def image_blockiness(self, a_u8, b_u8, space: str, oy: int = 0, ox: int = 0, ws=None):
        """a_u8 (the restored image), b_u8 uint8 [h, w, 3] on the device -> int64 [planes, 5]: per plane of ``space`` ("rgb" | "y") the
        squared-error sum between a and b and D_hb, D_hi, D_vb, D_vi, the squared steps of a across the borders of the 8 x 8 block grid
        with origin (oy, ox) and elsewhere — what ``quality.psnrb_from_sums`` turns into PSNR-B.  Two launches (per-workgroup partials
        in ``ws``, default the backend's workspace, then a fixed-order sum): rcot_image_blockiness."""
        self._u8_image(a_u8, "image_blockiness")
        h, w, _ = a_u8.shape
        self._u8_image(b_u8, "image_blockiness", h, w)
        if space not in self.SPACES:
            raise _lib.RcotKernelError(f"image_blockiness: invalid argument: color space {space!r}, expected one of {tuple(self.SPACES)}")
        ws = self.ws if ws is None else ws
        stats = torch.empty(3 if space == "rgb" else 1, 5, dtype=torch.int64, device=self.device)
        _lib.check(self.L.rcot_image_blockiness(a_u8.data_ptr(), b_u8.data_ptr(), h, w, self.SPACES[space], int(oy), int(ox),
                                                stats.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), self._st()),
                   "rcot_image_blockiness")
        return stats

    def crop_u8(self, img_u8, y0: int, x0: int, hc: int, wc: int, out=None):
        """img_u8 uint8 [h, w, 3] on the device -> uint8 [hc, wc, 3] (dense) = img_u8[y0:y0 + hc, x0:x0 + wc] in one launch (rcot_crop_u8):
        the border shave of the metrics"""
        self._u8_image(img_u8, "crop_u8")
        h, w, _ = img_u8.shape
        y0, x0, hc, wc = int(y0), int(x0), int(hc), int(wc)
        if y0 < 0 or x0 < 0 or hc < 1 or wc < 1 or y0 + hc > h or x0 + wc > w:
            raise _lib.RcotKernelError(f"crop_u8: invalid argument: {hc} x {wc} at ({y0}, {x0}) leaves the {h} x {w} image")
        if out is None:
            out = torch.empty(hc, wc, 3, dtype=torch.uint8, device=self.device)
        self._u8_image(out, "crop_u8", hc, wc)
        _lib.check(self.L.rcot_crop_u8(img_u8.data_ptr(), h, w, y0, x0, hc, wc, out.data_ptr(), self._st()), "rcot_crop_u8")
        return out

    # ------------------------------------------------------------------ optimizers
    def rmsprop_step(self, p, g, sq, n, lr, alpha=0.99, eps=1e-8, grad_scale=1.0):
        _lib.check(self.L.rcot_rmsprop_step(p.data_ptr(), g.data_ptr(), sq.data_ptr(), n, lr, alpha, eps, grad_scale,
                                            self._st()), "rcot_rmsprop_step")

    def adam_step(self, p, g, m, v, n, lr, step, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        _lib.check(self.L.rcot_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps,
                                         step, grad_scale, self._st()), "rcot_adam_step")

    def ema_step(self, ema, p, n, decay):
        """ema[0:n) += (1 - decay) (p[0:n) - ema[0:n)) in one launch (rcot_amd/ema.py); any n >= 1, any fp32 alignment"""
        _lib.check(self.L.rcot_ema_step(ema.data_ptr(), p.data_ptr(), n, decay, self._st()), "rcot_ema_step")

    # ---- gradient-norm clipping / non-finite skip decided on the device (control block: include/rcot_hip.h; trainer.FlatOptimizer)
    def grad_sumsq(self, g, n, partials):
        """partials[0:count) <- per-workgroup fp64 sums of g[0:n)^2; returns count (what grad_decide sums).  ``partials``: float64,
        at least lib.SUMSQ_MAX_PARTS elements."""
        if partials.dtype != torch.float64 or partials.numel() < _lib.SUMSQ_MAX_PARTS:
            raise _lib.RcotKernelError("grad_sumsq: invalid argument: the workspace must hold 4096 float64 values")
        _lib.check(self.L.rcot_grad_sumsq(g.data_ptr(), n, partials.data_ptr(), self._st()), "rcot_grad_sumsq")
        return self.L.rcot_grad_sumsq_parts(n)

    def grad_decide(self, partials, nparts, ctrl, adam_mask=0, b1=0.9, b2=0.999, inherit=False):
        """norm, clip scale, skip flag and counters of one step into the control block ``ctrl`` (float64 [lib.CB_WORDS]), on the device.
        ``inherit``: skip also when the block's previous decision skipped (a later step on the same batch; lib.DECIDE_INHERIT)"""
        if ctrl.dtype != torch.float64 or ctrl.numel() < _lib.CB_WORDS:
            raise _lib.RcotKernelError("grad_decide: invalid argument: the control block is float64 [16]")
        _lib.check(self.L.rcot_grad_decide(partials.data_ptr(), nparts, ctrl.data_ptr(), adam_mask | (_lib.DECIDE_INHERIT if inherit else 0), b1, b2,
                                           self._st()), "rcot_grad_decide")

    def rmsprop_step_guarded(self, p, g, sq, n, ctrl, alpha=0.99, eps=1e-8):
        _lib.check(self.L.rcot_rmsprop_step_guarded(p.data_ptr(), g.data_ptr(), sq.data_ptr(), n, alpha, eps, ctrl.data_ptr(), self._st()),
                   "rcot_rmsprop_step_guarded")

    def adam_step_guarded(self, p, g, m, v, n, ctrl, counter, b1=0.9, b2=0.999, eps=1e-8):
        _lib.check(self.L.rcot_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, b1, b2, eps, ctrl.data_ptr(),
                                                 counter, self._st()), "rcot_adam_step_guarded")

    # ---- AdamW, and the per-iteration schedule held on the device (schedule block: include/rcot_hip.h RCOT_SB_*; rcot_amd/schedule.py)
    def adamw_step(self, p, g, m, v, n, lr, step, weight_decay, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        """adam_step after the decoupled decay p <- p - (lr weight_decay) p (torch.optim.AdamW)"""
        _lib.check(self.L.rcot_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, step, grad_scale,
                                          weight_decay, self._st()), "rcot_adamw_step")

    def adamw_step_guarded(self, p, g, m, v, n, ctrl, counter, weight_decay, b1=0.9, b2=0.999, eps=1e-8):
        _lib.check(self.L.rcot_adamw_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, b1, b2, eps, ctrl.data_ptr(),
                                                  counter, weight_decay, self._st()), "rcot_adamw_step_guarded")

    def sched_advance(self, sched, table=None, lr_dst0=None, mult0=1.0, lr_dst1=None, mult1=1.0):
        """one iteration of the schedule block ``sched`` (float64 [lib.SB_WORDS]): this iteration's entry of ``table`` (float64, on the
        device; None = no rate) times mult0 / mult1 into the one-element float64 views lr_dst0 / lr_dst1 (None = skipped), the counter,
        and the EMA warm-up's 1 - D_u when the block's ema_decay word is set.  One launch, no host read."""
        if sched.dtype != torch.float64 or sched.numel() < _lib.SB_WORDS or (table is not None and table.dtype != torch.float64):
            raise _lib.RcotKernelError("sched_advance: invalid argument: the schedule block is float64 [8], the table float64")
        for d in (lr_dst0, lr_dst1):
            if d is not None and (d.dtype != torch.float64 or d.numel() < 1):
                raise _lib.RcotKernelError("sched_advance: invalid argument: a destination is a float64 word")
        _lib.check(self.L.rcot_sched_advance(sched.data_ptr(), 0 if table is None else table.data_ptr(), 0 if table is None else table.numel(),
                                             0 if lr_dst0 is None else lr_dst0.data_ptr(), mult0, 0 if lr_dst1 is None else lr_dst1.data_ptr(),
                                             mult1, self._st()), "rcot_sched_advance")

    def ema_step_dev(self, ema, p, n, omd_word):
        """ema_step with 1 - decay read from the device double ``omd_word`` (a one-element float64 view)"""
        if omd_word.dtype != torch.float64 or omd_word.numel() < 1:
            raise _lib.RcotKernelError("ema_step_dev: invalid argument: omd_word is a float64 word")
        _lib.check(self.L.rcot_ema_step_dev(ema.data_ptr(), p.data_ptr(), n, omd_word.data_ptr(), self._st()), "rcot_ema_step_dev")
