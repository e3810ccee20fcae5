"""Host restatement of rcot_ema_step (csrc/optim.hip) for two fp32 arrays, in numpy.

    omd32 = float32(1.0 - decay)                          (the subtraction in double, as the entry point forms it)
    d     = float32(float64(p) - float64(e))              == the fp32 subtraction: one rounding of the exact difference
    r     = float32(float64(omd32) * float64(d) + float64(e))

The product of two fp32 values is exact in fp64 (48 significant bits); the sum is rounded once to fp64 and once more to fp32, where the
kernel's fused multiply-add rounds the exact value once.  Double rounding can move the result by one fp32 ulp in rare cases and never
more, so the bar of ONE launch is |kernel - r| <= 1 ulp(r): derived, not measured.  It holds while no intermediate is subnormal: keep
the magnitudes of the inputs in [1e-4, 1].
"""
import numpy as np


def omd32(decay: float) -> np.float32:
    return np.float32(1.0 - float(decay))


def ema_step(e: np.ndarray, p: np.ndarray, decay: float) -> np.ndarray:
    """one update of the fp32 array ``e`` towards the fp32 array ``p``; returns a new fp32 array"""
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32 and e.shape == p.shape
    d = (p.astype(np.float64) - e.astype(np.float64)).astype(np.float32)
    return (np.float64(omd32(decay)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def ulp(r: np.ndarray) -> np.ndarray:
    """the fp32 unit in the last place at |r| (np.spacing: the distance to the next value away from zero), as float64"""
    return np.abs(np.spacing(np.asarray(r, dtype=np.float32))).astype(np.float64)
