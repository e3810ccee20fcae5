"""Host restatement of the schedule launches (csrc/optim.hip: rcot_sched_advance, rcot_ema_step_dev, rcot_adamw_step,
rcot_adamw_step_guarded) in numpy / torch on the CPU, next to tests/clip_double.py, which it extends and does not edit.

    advance     v = table[min(t, n - 1)];  dst0 = v * mult0;  dst1 = v * mult1;  block.lr = v;  t += 1          (Python floats: doubles)
                D > 0:  omd = 1 - min(D, (1 + u) / (10 + u));  u += 1
    ema dev     tests/ema_double.py's ema_step with omd32 = float32(word)
    AdamW       p <- p - float32(lr * wd) p, then Adam's update (TorchDouble.adam_step); wd == 0: Adam alone.  On float64 tensors the
                product lr * wd stays a double: the rule of torch.optim.AdamW (p *= 1 - lr wd) up to rounding.

``ScheduleBackend`` is the backend double of the host tests: ClipBackend plus these methods and ema_step, with EVERY call of a launch
method noted by name in ``names`` (ClipBackend's own ``calls`` keeps the guarded ones with their sizes)."""
import numpy as np
import torch

from clip_double import ClipBackend
from ema_double import ulp  # noqa: F401  (re-exported for the GPU tests)
from rcot_amd import lib

_HOST = {"empty", "zeros", "stack_pack", "pack_weights", "device", "dtype", "name"}


def ema_omd(D: float, u: int) -> float:
    """1 - D_u of EMA update u, in double"""
    return 1.0 - min(D, (1.0 + u) / (10.0 + u))


def advance(block: torch.Tensor, table, dst0=None, mult0=1.0, dst1=None, mult1=1.0):
    """one rcot_sched_advance on a float64 [SB_WORDS] CPU tensor; table: a float64 numpy array or None; dst: one-element float64 views"""
    i = block.view(torch.int64)
    if table is not None:
        t = int(i[lib.SB_T])
        v = float(table[max(0, min(t, len(table) - 1))])
        if dst0 is not None:
            dst0[0] = v * mult0
        if dst1 is not None:
            dst1[0] = v * mult1
        block[lib.SB_LR] = v
        i[lib.SB_T] = t + 1
    D = float(block[lib.SB_EMA_DECAY])
    if D > 0.0:
        u = int(i[lib.SB_EMA_UPDATES])
        block[lib.SB_EMA_OMD] = ema_omd(D, u)
        i[lib.SB_EMA_UPDATES] = u + 1


def ema_step_omd(e: np.ndarray, p: np.ndarray, omd: float) -> np.ndarray:
    """tests/ema_double.py::ema_step with omd32 = float32(omd) given directly"""
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32
    d = (p.astype(np.float64) - e.astype(np.float64)).astype(np.float32)
    return (np.float64(np.float32(omd)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


class ScheduleBackend(ClipBackend):
    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        object.__setattr__(self, "names", [])

    def __getattribute__(self, name):
        v = object.__getattribute__(self, name)
        if name.startswith("_") or name in _HOST or name in ("names", "calls") or not callable(v):
            return v
        names = object.__getattribute__(self, "names")

        def noted(*a, **k):
            depth = object.__getattribute__(self, "__dict__").get("_depth", 0)
            if depth == 0:                                                 # a launch method that calls another one counts once
                names.append(name)
            object.__setattr__(self, "_depth", depth + 1)
            try:
                return v(*a, **k)
            finally:
                object.__setattr__(self, "_depth", depth)
        return noted

    def sched_advance(self, sched, table=None, lr_dst0=None, mult0=1.0, lr_dst1=None, mult1=1.0):
        advance(sched, None if table is None else table.numpy(), lr_dst0, mult0, lr_dst1, mult1)

    def ema_step(self, ema, p, n, decay):
        self.ema_step_dev(ema, p, n, torch.tensor([1.0 - decay], dtype=torch.float64))

    def ema_step_dev(self, ema, p, n, omd_word):
        e32, p32 = ema[:n].to(torch.float32).numpy(), p[:n].to(torch.float32).numpy()
        ema[:n].copy_(torch.from_numpy(ema_step_omd(e32, p32, float(omd_word[0]))).to(ema.dtype))

    def _decay(self, p, n, lr, wd):
        if wd != 0.0:
            f = lr * wd if p.dtype == torch.float64 else float(np.float32(lr * wd))     # the kernel hands the product on as fp32
            p[:n].sub_(p[:n] * f)                                          # fma(-f, p, p) up to one rounding of the product

    def adamw_step(self, p, g, m, v, n, lr, step, weight_decay, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
        self._decay(p, n, lr, weight_decay)
        self.adam_step(p, g, m, v, n, lr, step, b1, b2, eps, grad_scale)

    def adamw_step_guarded(self, p, g, m, v, n, ctrl, counter, weight_decay, b1=0.9, b2=0.999, eps=1e-8):
        i = ctrl.view(torch.int64)
        if not (int(i[lib.CB_SKIP]) or int(i[lib.CB_T + counter]) <= 0):
            self._decay(p, n, float(ctrl[lib.CB_LR]), weight_decay)
        self.adam_step_guarded(p, g, m, v, n, ctrl, counter, b1, b2, eps)
