"""Host restatement of the guarded optimizer step (csrc/optim.hip: rcot_grad_sumsq, rcot_grad_decide, rcot_rmsprop_step_guarded,
rcot_adam_step_guarded) in numpy / torch on the CPU.

    total = sum over i of float64(g[i])^2        every square of an fp32 value is exact in fp64 (48 significant bits); the sum of n
                                                 non-negative fp64 terms is within n 2^-53 relative of the exact one in any order
    skip  = not isfinite(total)                  squares of finite fp32 values stay below 2^256: no fp64 sum of them overflows, so skip
                                                 holds exactly when an element is Inf or NaN
    norm  = sqrt(total)
    scale = min(1, max_norm / (norm + 1e-6))     torch.nn.utils.clip_grad_norm_

The update itself is ``TorchDouble``'s (tests/host_double.py, imported, not edited): its rmsprop_step / adam_step with
``grad_scale = float32(scale)`` — the kernels hand the scale to the shared update expression as fp32 — or nothing at all on a skip.

Where torch differs and is NOT tested against: torch sums the squares of fp32 gradients in fp32, so a finite gradient with a value near
1e20 overflows its norm to Inf (clip_grad_norm_ then scales everything to 0, or raises with error_if_nonfinite); here the same gradient
has a finite fp64 norm and is clipped like any other.

``ClipBackend`` is the small backend double of the host tests: TorchDouble plus the four guarded methods of HipBackend on a control
block that is a float64 torch tensor laid out as include/rcot_hip.h documents (rcot_amd.lib.CB_*).
"""
import math

import numpy as np
import torch

from host_double import TorchDouble
from rcot_amd import lib

_T32 = TorchDouble(torch.float32)


def sumsq(g: np.ndarray) -> float:
    """the fp64 sum of squares of an fp32 array (numpy's pairwise fp64 sum: far inside n 2^-53)"""
    g = np.asarray(g)
    assert g.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(g.astype(np.float64) ** 2))


def decide(total: float, max_norm: float):
    """(norm, scale, skip) of one step; scale is 0 on a skip, as the control block holds it"""
    skip = not math.isfinite(total)
    norm = math.sqrt(total) if total == total else float("nan")
    scale = 0.0 if skip else min(1.0, max_norm / (norm + 1e-6))
    return norm, scale, skip


def rmsprop_guarded(p, g, sq, lr, max_norm, alpha=0.99, eps=1e-8, scale=None):
    """one guarded RMSprop step of the fp32 torch tensors p, sq (in place) with gradient g; ``scale``: use this clip coefficient
    instead of the restated one (the GPU tests pass the kernel's own).  Returns (norm, scale, skip)."""
    norm, s, skip = decide(sumsq(g.numpy()), max_norm)
    if not skip:
        s = s if scale is None else scale
        _T32.rmsprop_step(p, g, sq, p.numel(), lr, alpha, eps, grad_scale=float(np.float32(s)))
    return norm, s, skip


def adam_guarded(p, g, m, v, lr, step, max_norm, b1=0.9, b2=0.999, eps=1e-8, scale=None):
    """one guarded Adam step; ``step`` is the count this step would carry.  Returns (norm, scale, skip, the count afterwards)."""
    norm, s, skip = decide(sumsq(g.numpy()), max_norm)
    if skip:
        return norm, s, skip, step - 1
    s = s if scale is None else scale
    _T32.adam_step(p, g, m, v, p.numel(), lr, step, b1, b2, eps, grad_scale=float(np.float32(s)))
    return norm, s, skip, step


class ClipBackend(TorchDouble):
    """TorchDouble with the guarded-step methods of HipBackend (rcot_amd/ops.py), for the host tests of FlatOptimizer"""

    def __init__(self, dtype=torch.float32):
        super().__init__(dtype)
        self.calls = []                                                    # (method, n) in launch order

    def grad_sumsq(self, g, n, partials):
        self.calls.append(("grad_sumsq", n))
        partials.fill_(float("nan"))
        partials[0] = sumsq(g[:n].to(torch.float32).numpy())
        return 1

    def grad_decide(self, partials, nparts, ctrl, adam_mask=0, b1=0.9, b2=0.999, inherit=False):
        self.calls.append(("grad_decide", adam_mask | (lib.DECIDE_INHERIT if inherit else 0)))
        i = ctrl.view(torch.int64)
        inherited = inherit and int(i[lib.CB_SKIP]) != 0
        norm, scale, skip = decide(float(partials[:nparts].sum()), float(ctrl[lib.CB_MAX_NORM]))
        if inherited:                                                      # the previous decision of this block skipped: so does this one
            scale, skip = 0.0, True
        ctrl[lib.CB_NORM], ctrl[lib.CB_SCALE], i[lib.CB_SKIP] = norm, scale, int(skip)
        i[lib.CB_STEPS] += 1
        if skip:
            i[lib.CB_SKIPPED] += 1
            return
        if scale < 1.0:
            i[lib.CB_CLIPPED] += 1
        ctrl[lib.CB_MAX_SEEN] = max(float(ctrl[lib.CB_MAX_SEEN]), norm)
        for k in range(2):
            if adam_mask >> k & 1:
                i[lib.CB_T + k] += 1
                t = int(i[lib.CB_T + k])
                ctrl[lib.CB_BC1 + k], ctrl[lib.CB_BC2 + k] = 1 - b1 ** t, 1 - b2 ** t

    def rmsprop_step_guarded(self, p, g, sq, n, ctrl, alpha=0.99, eps=1e-8):
        self.calls.append(("rmsprop_step_guarded", n))
        if int(ctrl.view(torch.int64)[lib.CB_SKIP]):
            return
        self.rmsprop_step(p, g, sq, n, float(ctrl[lib.CB_LR]), alpha, eps, grad_scale=float(np.float32(float(ctrl[lib.CB_SCALE]))))

    def adam_step_guarded(self, p, g, m, v, n, ctrl, counter, b1=0.9, b2=0.999, eps=1e-8):
        self.calls.append(("adam_step_guarded", n))
        i = ctrl.view(torch.int64)
        if int(i[lib.CB_SKIP]) or int(i[lib.CB_T + counter]) <= 0:
            return
        self.adam_step(p, g, m, v, n, float(ctrl[lib.CB_LR]), int(i[lib.CB_T + counter]), b1, b2, eps,
                       grad_scale=float(np.float32(float(ctrl[lib.CB_SCALE]))))
